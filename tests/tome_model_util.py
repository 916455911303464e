"""What tests/golden/make_golden_tome.py (the reference run) and the token-merging model tests share: the small model,
its seed-defined state and inputs, the solver settings, how large tensors are sampled into the fixture, and the
conversion of the reference's index tensors into the kernels' ``dest`` (pure torch / numpy, no GPU).

The model: 96-pixel images, 16-pixel patches: 36 patch tokens, 37 with the class token (odd, no multiple of 16); width
128 = 2 heads of 64, depth 3, mlp_ratio 1, 8 classes, batch 2, ``r = [4, 3, 0]``: 37 -> 33 -> 30 -> 30 tokens.
To keep the fixture under the repository's size limit for a committed file, tensors above ``SAMPLE_ABOVE`` elements
are recorded as every ``SAMPLE_STRIDE``-th element of the flattened tensor (gradients and final parameters alike).

The state is a function of the parameter names, shapes and one seed.  The seed is chosen by the fixture maker (the first
for which the matching survives qkv rounded to bf16 with room to spare; the maker's docstring has the rule) and stored
in the fixture."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL = dict(img_size=96, patch_size=16, embed_dim=128, depth=3, num_heads=2, mlp_ratio=1, qkv_bias=True, class_num=8,
             epsilon=1e-6)
TOKENS = 37
R = [4, 3, 0]
BATCH = 2
STEPS = 2
NO_DECAY = ['cls_token', 'pos_embed', 'norm', 'bias']
# epsilon: with the recipes' 1e-8 AdamW's update lr m / (sqrt(v) + eps) is the sign of the gradient at these magnitudes,
# and an element whose gradient lies below the rounding noise of its fp32 computation (about 1e-6 of the tensor's
# largest; among the 10^5 elements of the large tensors there are such) moves by +lr on one side and -lr on the other:
# no bound on the updated parameters can hold for it, on any hardware.  With 1e-3 (times sqrt(1 - beta2^t) = 0.032 and
# 0.045 in the two steps) the update is Lipschitz in the gradient, lr / 3e-5 per unit, so fp32 noise of 1e-6 x 0.2 moves
# a parameter by less than 1e-2 lr, and bias correction, both moments and the decoupled decay are still exercised.
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-3, weight_decay=0.05)
SAMPLE_ABOVE = 4096
SAMPLE_STRIDE = 7
FIXTURE = 'tome_small'
LAYERS = 'tome_layers'
# single-layer cases of the reference's bipartite_soft_matching + merge_wavg: (B, T, H, DH, C, r, sizes from a merge before)
LAYER_CASES = [(2, 17, 2, 32, 32, 4, False), (2, 18, 1, 64, 24, 8, False), (2, 37, 2, 64, 16, 18, True),
               (1, 3, 1, 32, 8, 1, False)]


def fixture_state(keys_shapes, seed):
    """name -> fp32 tensor for every parameter, drawn in the order of the sorted names from manual_seed(seed)."""
    gen = torch.Generator().manual_seed(int(seed))
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.split('.')[-1]
        if leaf in ('cls_token', 'pos_embed'):
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
    """[(x [B, 3, 96, 96] fp32, labels [B] int64)] for STEPS steps."""
    gen = torch.Generator().manual_seed(416)
    S = MODEL['img_size']
    return [(torch.randn(BATCH, 3, S, S, generator=gen), torch.randint(0, MODEL['class_num'], (BATCH,), generator=gen))
            for _ in range(STEPS)]


def sample(t):
    """What the fixture keeps of a tensor: all of it, or every SAMPLE_STRIDE-th element of the flattened tensor."""
    t = torch.as_tensor(t).detach().reshape(-1)
    return t[::SAMPLE_STRIDE] if t.numel() > SAMPLE_ABOVE else t


def dest_from_indices(T, unm_idx, src_idx, dst_idx):
    """The reference's sorted ``unm_idx`` [B, NA - r], ``src_idx`` [B, r] (indices into the even tokens) and ``dst_idx``
    [B, r] (into the odd tokens) -> dest int64 [B, T]: ``concat([unm, dst])`` puts unmerged even token unm_idx[k] in row k
    and odd token j in row NA - r + j (tome.py:76-99)."""
    unm_idx, src_idx, dst_idx = [np.asarray(a).astype(np.int64) for a in (unm_idx, src_idx, dst_idx)]
    B, n_unm = unm_idx.shape
    dest = np.full((B, T), -1, dtype=np.int64)
    for b in range(B):
        dest[b, 2 * unm_idx[b]] = np.arange(n_unm)
        dest[b, 1::2] = n_unm + np.arange(T // 2)
        dest[b, 2 * src_idx[b]] = n_unm + dst_idx[b]
    assert dest.min() >= 0
    return dest


def zero_grad_part(name, t):
    """(the analytically-zero part of a gradient, the rest): the key third of attn.qkv.bias shifts every score of a row
    by q . b_k, which the softmax ignores, and the matching runs without gradient."""
    if name.endswith('attn.qkv.bias'):
        D = t.numel() // 3
        return t[D:2 * D], torch.cat([t[:D], t[2 * D:]])
    return None, t


def load(name):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
