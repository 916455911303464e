"""What tests/golden/make_golden_deit.py (the reference run) and the DeiT model tests share: the two small models, their
seed-defined state and inputs, the solver settings and the fixture files (pure torch / numpy, no GPU).

SMALL  12 x 12 input, 4-pixel patches: 9 patch tokens, 10 with the class token (no multiple of 16).  The dense
       attention kernels serve it.
LONG   30 x 30 input of FOUR channels, 2-pixel patches (a patch row of 4 x 2 x 2 = 16 elements: the GEMM of the patch
       projection takes 16-byte rows, which three channels would not give in bf16): 225 patch tokens, 226 with the
       class token and 227 with the distillation token too.  Both are beyond the dense kernels' 208 tokens, so these
       fixtures can only be met through the key-tiled kernels, backward included; 226 and 227 are no multiple of the key
       block (64) or of a query block (64 / 128).
Both: width 64 = 2 heads of dimension 32, depth 2, mlp_ratio 0.5, 8 classes, batch 2, epsilon 1e-6 (the factories').

To keep a file under the repository's size limit for a committed file, the parameters after two steps are recorded only
for tensors of at most ``FINAL_MAX`` elements (every vector, cls_token / dist_token, proj, the MLP and head weights, the
patch convolution; of the SMALL model pos_embed too); the gradient of EVERY parameter is recorded.

The state is a function of the parameter names and shapes, not a stored tensor (cait_model_util does the same)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = dict(in_chans=3, embed_dim=64, depth=2, num_heads=2, mlp_ratio=0.5, class_num=8, qkv_bias=True, epsilon=1e-6)
SMALL = dict(COMMON, img_size=12, patch_size=4)
LONG = dict(COMMON, img_size=30, patch_size=2, in_chans=4)
BATCH = 2
STEPS = 2
# the config's no_weight_decay_name (DeiT_base_patch16_224_in1k_1n8c_dp_fp16o2.yaml)
NO_DECAY = ['cls_token', 'pos_embed', 'norm', 'bias']
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.05)     # no clipping: the recipe has none
# fixture file -> {case: (class name, model arguments, drop_path_rate)}
CASES = {
    'deit_small': {'dp0': ('DeitVisionTransformer', SMALL, 0.0), 'dp5': ('DeitVisionTransformer', SMALL, 0.5)},
    'deit_long': {'plain': ('DeitVisionTransformer', LONG, 0.0), 'dist': ('DistilledVisionTransformer', LONG, 0.0)},
}
LAYERS = 'deit_layers'                                              # factory keys, position-table interpolation
FINAL_MAX = 4608
FACTORIES = ['DeiT_tiny_patch16_224', 'DeiT_small_patch16_224', 'DeiT_base_patch16_224',
             'DeiT_tiny_distilled_patch16_224', 'DeiT_small_distilled_patch16_224', 'DeiT_base_distilled_patch16_224',
             'DeiT_base_patch16_384', 'DeiT_base_distilled_patch16_384']
# load_pretrained(finetune=True): a 3 x 3 position grid (12-pixel model) into a 5 x 5 one (20 pixels), other head size
POS_FROM = dict(SMALL, class_num=5)
POS_TO = dict(SMALL, img_size=20)


def fixture_state(keys_shapes, seed=2012):
    """name -> fp32 tensor for every parameter, drawn in the order of the sorted names from manual_seed(seed)."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.split('.')[-1]
        if leaf in ('cls_token', 'dist_token', 'pos_embed'):
            t = torch.randn(shape, generator=gen) * 0.5
        elif leaf == 'bias':
            t = torch.randn(shape, generator=gen) * 0.1
        elif len(shape) == 1:                                   # LayerNorm weight
            t = 1.0 + torch.randn(shape, generator=gen) * 0.1
        else:                                                   # the patch convolution [out, in, k, k], Linears [in, out]
            fan_in = int(np.prod(shape[1:])) if len(shape) == 4 else shape[0]
            t = torch.randn(shape, generator=gen) * (1.0 / fan_in) ** 0.5
        out[name] = t
    return out


def batches(model_args):
    """[(x [B, in_chans, S, S] fp32, labels [B] int64)] for STEPS steps."""
    S, C = model_args['img_size'], model_args['in_chans']
    gen = torch.Generator().manual_seed(912 + S)
    return [(torch.randn(BATCH, C, S, S, generator=gen), torch.randint(0, model_args['class_num'], (BATCH,), generator=gen))
            for _ in range(STEPS)]


def block_rates(rate, depth):
    """dpr = np.linspace(0, drop_path_rate, depth) (deit.py:84)."""
    return [float(r) for r in np.linspace(0, rate, depth)]


def keep_table(draws, rate, depth):
    """The keep table [2 * depth, B] of the product from the reference's draws: a block with rate 0 is an Identity there
    (no draw) and owns two rows of ones here; the others floor(float32(1 - p) + u), two draws per block."""
    rows, it = [], iter(draws)
    for r in block_rates(rate, depth):
        for _ in range(2):
            if r > 0.:
                u = np.asarray(next(it), dtype=np.float32)
                rows.append(np.floor((np.float32(1.0 - r) + u).astype(np.float32)))
            else:
                rows.append(np.ones(BATCH, dtype=np.float32))
    assert next(it, None) is None
    return np.stack(rows).astype(np.float32)


def zero_grad_names(names):
    """Parameters whose gradient is analytically zero in part: the key third of a qkv.bias (a shift of the scores of a
    row by q . b_k, to which softmax is invariant)."""
    return [n for n in names if n.endswith('attn.qkv.bias')]


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
