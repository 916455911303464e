"""What tests/golden/make_golden_convnext.py (the reference run) and the ConvNeXt model tests share: the small model, its
seed-defined state and inputs, the solver settings and the fixture files (pure torch / numpy, no GPU).

The state is a function of the parameter names and shapes, not a stored tensor (oracle.mae.finetune_state does the same
for the fine-tuning fixtures): the two fixture files then hold only what the reference COMPUTED.  Every ``gamma`` is
uniform in [0.5, 1.5]: at the constructor's 1e-6 the whole branch (dwconv, both Linears) would contribute one part in a
million to the logits and a wrong depthwise kernel would pass a model-level comparison.  Biases and LayerNorm
parameters carry a signal too (the constructor's are 0 and 1)."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = dict(in_chans=3, class_num=8, depths=[1, 1, 2, 1], dims=[8, 16, 32, 64])
# feature maps 16x24, 8x12, 4x6, 2x3: the last two are smaller than the filter's reach
BATCH, HEIGHT, WIDTH = 2, 64, 96
STEPS = 2
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.05)      # decay on every parameter
CASES = {'convnext_small': 0.0, 'convnext_small_dp': 0.5}                           # file name -> drop_path_rate


def fixture_state(keys_shapes):
    """name -> fp32 tensor, drawn in the order of the sorted names from Generator().manual_seed(2201)."""
    gen = torch.Generator().manual_seed(2201)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.rsplit('.', 1)[-1]
        if leaf == 'gamma':
            t = torch.rand(shape, generator=gen) + 0.5
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
    """[(x [B, 3, H, W] fp32, labels [B] int64)] for STEPS steps."""
    gen = torch.Generator().manual_seed(909)
    return [(torch.randn(BATCH, 3, HEIGHT, WIDTH, generator=gen), torch.randint(0, MODEL['class_num'], (BATCH,),
                                                                                generator=gen)) for _ in range(STEPS)]


def ladder(rate):
    """The reference's dp_rates (convnext.py:145-147) and keep_prob = float32(1 - p) of the blocks with p > 0."""
    rates = [x.item() for x in torch.linspace(0, rate, sum(MODEL['depths']), dtype=torch.float32)]
    keep_prob = [float(np.float32(1.0) - np.float32(p)) for p in rates if p > 0.]
    return rates, keep_prob


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
