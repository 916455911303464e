"""What tests/golden/make_golden_convmae.py (the reference run) and the ConvMAE model tests share: the small models, their
seed-defined state and inputs, the solver settings and the fixture files (pure torch / numpy, no GPU).

The reference hard-codes the 14 x 14 patch grid, the 56 x 56 and 28 x 28 maps and p = 16 (conv_mae.py:183, :240-245),
so the small models keep ``img_size [224, 56, 28]`` / ``patch_size [4, 2, 2]`` on a 2 x 3 x 224 x 224 input and are small
in width and depth only.  The state is a function of the parameter names and shapes, not a stored tensor
(convnext_model_util.py does the same): the fixture files then hold only what the reference COMPUTED.  Biases and
LayerNorm parameters carry a signal (the constructor's are 0 and 1)."""
import os
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = dict(img_size=[224, 56, 28], patch_size=[4, 2, 2], embed_dim=[16, 24, 64], depth=[1, 1, 2], num_heads=2,
              mlp_ratio=[4, 4, 4])
MAE_MODEL = dict(STAGES, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2, norm_pix_loss=True)
VIT_MODEL = dict(STAGES, num_classes=8, qkv_bias=True)
NORM_EPS = 1e-6                   # the factories' norm_layer = partial(nn.LayerNorm, epsilon=1e-6)
BATCH, IMG = 2, 224
L, K, P = 196, 49, 768            # patches, kept patches, pixels per patch
MASK_RATIO = 0.75
STEPS = 2
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.95, epsilon=1e-8, weight_decay=0.05)      # decay on every parameter
# file name -> drop_path_rate; each file holds both heads: keys 'tok/...' (global_pool False) and 'pool/...' (True)
VIT_CASES = {'convvit_small': 0.0, 'convvit_small_dp': 0.5}
POOLS = (('tok/', False), ('pool/', True))
PRED_ROWS = 8                     # rows (patches) of pred that the fixture records per image: the first PRED_ROWS
BIG = 1024                        # arrays with more elements are recorded as their first BIG elements (flat)


def norm_layer(nn_module):
    return partial(nn_module.LayerNorm, epsilon=NORM_EPS)


def fixture_state(keys_shapes, seed=2305):
    """name -> fp32 tensor, drawn in the order of the sorted names from Generator().manual_seed(seed).  pos_embed /
    decoder_pos_embed keep the constructor's values (not in the returned dict)."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.rsplit('.', 1)[-1]
        if name in ('decoder_pos_embed',):
            continue
        if name in ('pos_embed', 'mask_token'):
            t = torch.randn(shape, generator=gen) * 0.2
        elif leaf == 'bias':
            t = torch.randn(shape, generator=gen) * 0.1
        elif len(shape) == 1:                                   # LayerNorm weight
            t = 1.0 + torch.randn(shape, generator=gen) * 0.1
        else:                                                   # convolutions [out, in, k, k], Linears [in, out]
            fan_in = int(np.prod(shape[1:])) if len(shape) == 4 else shape[0]
            t = torch.randn(shape, generator=gen) * (1.0 / fan_in) ** 0.5
        out[name] = t
    return out


def batches():
    """[(imgs [B, 3, 224, 224] fp32, labels [B] int64, noise [B, 196] fp32)] for STEPS steps."""
    gen = torch.Generator().manual_seed(911)
    return [(torch.randn(BATCH, 3, IMG, IMG, generator=gen), torch.randint(0, VIT_MODEL['num_classes'], (BATCH,),
                                                                           generator=gen),
             torch.rand(BATCH, L, generator=gen)) for _ in range(STEPS)]


def ladder(rate):
    """The reference's dpr (conv_vit.py:229: np.linspace, float64) and keep_prob = float32(1 - p) of every residual with
    p > 0, two per block, in network order."""
    rates = [float(v) for v in np.linspace(0, rate, sum(STAGES['depth']))]
    keep_prob = [float(np.float32(1.0) - np.float32(p)) for p in rates if p > 0. for _ in range(2)]
    return rates, keep_prob


def clip(a):
    """What the fixture records of an array: all of it, or its first BIG elements."""
    a = np.asarray(a)
    return a.copy() if a.size <= BIG else a.reshape(-1)[:BIG].copy()


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
