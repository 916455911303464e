"""What tests/golden/make_golden_cait.py (the reference run) and the CaiT model tests share: the small model, its
seed-defined state and inputs, the solver settings and the fixture files (pure torch / numpy, no GPU).

The model: 8 x 20 input, 4-pixel patches, so a 2 x 5 grid (row and column strides differ) of 10 patch tokens, 11 with
the class token: neither is a multiple of 16.  Width 96 = 2 heads of dimension 48, 2 trunk blocks and 2 token-only
blocks, 8 classes.  To keep a file under the repository's size limit for a committed file, ``mlp_ratio`` is 0.5 (both
stages) and the parameters after two steps are recorded only for tensors of at most ``FINAL_MAX`` elements (every
vector, both head mixes, pos_embed, cls_token, the MLP and head weights); the gradient of EVERY parameter is recorded.

The state is a function of the parameter names and shapes, not a stored tensor (swin_model_util does the same):
gamma_1 / gamma_2 of order 1 (at the constructor's 1e-5 a wrong branch would vanish under the comparison's bound),
proj_l / proj_w weights = identity plus a dense deviation of order 0.5 / sqrt(H), their biases non-zero; biases and
LayerNorm parameters carry a signal too."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = dict(img_size=(8, 20), patch_size=4, embed_dim=96, depth=2, num_heads=2, mlp_ratio=0.5, num_classes=8,
             depth_token_only=2, mlp_ratio_token_only=0.5, init_values=1e-5)
BATCH = 2
STEPS = 2
NO_DECAY = ['cls_token', 'pos_embed', 'norm', 'bias']              # the config's no_weight_decay_name
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.05)     # no clipping: the recipe has none
CASES = {'cait_small': 0.0, 'cait_small_dp': 0.5}                  # file name -> drop_path_rate
LAYERS = 'cait_layers'                                              # single layers, factory keys
FINAL_MAX = 4608
FACTORIES = ['cait_xxs24_224', 'cait_xxs24_384', 'cait_xxs36_224', 'cait_xxs36_384', 'cait_xs24_384', 'cait_s24_224',
             'cait_s24_384', 'cait_s36_384', 'cait_m36_384', 'cait_m48_448']
RUNNING = ['cait_xxs24_224', 'cait_xxs36_224', 'cait_s24_224']      # the 224-pixel factories


def fixture_state(keys_shapes):
    """name -> fp32 tensor for every parameter, drawn in the order of the sorted names from manual_seed(2103)."""
    gen = torch.Generator().manual_seed(2103)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        parts = name.split('.')
        leaf, owner = parts[-1], (parts[-2] if len(parts) > 1 else '')
        if leaf in ('gamma_1', 'gamma_2'):
            t = 1.0 + torch.randn(shape, generator=gen) * 0.25
        elif owner in ('proj_l', 'proj_w') and leaf == 'weight':
            t = torch.eye(shape[0]) + torch.randn(shape, generator=gen) * (0.5 / shape[0] ** 0.5)
        elif owner in ('proj_l', 'proj_w'):
            t = torch.randn(shape, generator=gen) * 0.3
        elif leaf in ('cls_token', 'pos_embed'):
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


def batches():
    """[(x [B, 3, H, W] fp32, labels [B] int64)] for STEPS steps."""
    gen = torch.Generator().manual_seed(912)
    H, W = MODEL['img_size']
    return [(torch.randn(BATCH, 3, H, W, generator=gen), torch.randint(0, MODEL['num_classes'], (BATCH,), generator=gen))
            for _ in range(STEPS)]


def keep_probs(rate):
    """keep_prob = float32(1 - p) of the two DropPath calls of every trunk block (cait.py:282: the same rate for all)."""
    return [float(np.float32(1.0 - rate)) for _ in range(2 * MODEL['depth'])] if rate > 0. else []


def zero_grad_names(names):
    """Parameters whose gradient is analytically zero: every proj_l.bias (a shift of a softmax row), the key third of a
    trunk qkv.bias and ClassAttn's k.bias (a shift of the scores of a row by q . b_k)."""
    return [n for n in names if n.endswith('proj_l.bias') or n.endswith('attn.qkv.bias') or n.endswith('attn.k.bias')]


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
