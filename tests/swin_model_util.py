"""What tests/golden/make_golden_swin.py (the reference run) and the Swin model tests share: the small model, its
seed-defined state and inputs, the solver settings and the fixture files (pure torch / numpy, no GPU).

The model: 32 x 64 input, 4-pixel patches, so stage 1 is an 8 x 16 map with window 4 and a shifted second block; after the
merge stage 2 is a 4 x 8 map, where ``min(resolution) <= window`` switches the shift off.  Heads (1, 2) of dimension 32; ``mlp_ratio`` 2 keeps a file of every
gradient and every updated parameter under the repository's size limit for a committed file.

The state is a function of the parameter names and shapes, not a stored tensor (convnext_model_util does the same).
Bias tables are drawn at standard deviation 0.5: at the constructor's 0.02 a wrong bias index would move the logits by
less than the comparison's bound.  Biases and LayerNorm parameters carry a signal too."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = dict(img_size=(32, 64), patch_size=4, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=4, mlp_ratio=2.,
             num_classes=8)
BATCH = 2
STEPS = 2
NO_DECAY = ['absolute_pos_embed', 'relative_position_bias_table', 'norm', 'bias']    # the config's no_weight_decay_name
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.05, clip_norm=5.0)
CASES = {'swin_small': 0.0, 'swin_small_dp': 0.5}                                    # file name -> drop_path_rate
LAYERS = 'swin_layers'                                                                # single layers, factory keys
BUFFERS = ('relative_position_index', 'attn_mask')


def fixture_state(keys_shapes):
    """name -> fp32 tensor for every parameter, drawn in the order of the sorted names from manual_seed(2203)."""
    gen = torch.Generator().manual_seed(2203)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.rsplit('.', 1)[-1]
        if leaf in BUFFERS:
            continue
        if leaf == 'relative_position_bias_table':
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
    gen = torch.Generator().manual_seed(911)
    H, W = MODEL['img_size']
    return [(torch.randn(BATCH, 3, H, W, generator=gen), torch.randint(0, MODEL['num_classes'], (BATCH,), generator=gen))
            for _ in range(STEPS)]


def ladder(rate):
    """The reference's dpr (swin_transformer.py:537) and keep_prob = float32(1 - p), twice per block with p > 0 (one
    DropPath call per residual)."""
    rates = np.linspace(0, rate, sum(MODEL['depths'])).tolist()
    keep_prob = [float(np.float32(1.0 - p)) for p in rates if p > 0. for _ in range(2)]
    return rates, keep_prob


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
