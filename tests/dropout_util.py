"""A numpy restatement of element-wise dropout (include/passl_hip.h: passl_hip_dropout and its three relatives), shared
by tests/test_dropout_host.py (statistics and edge cases, no GPU), tests/test_dropout_gpu.py (the kernels, bit for bit)
and tests/test_vit_dropout_gpu.py (a float64 ViT fed these masks).  Philox4x32-10 is droppath_util's, whose
known-answer check stays the anchor."""
import math

import numpy as np

from droppath_util import MASK, philox4x32_10


def thr_factor(p):
    """(thr, factor) of rate p: thr = floor(p * 65536 + 0.5) in double; factor = float32(1 / (1 - float32(p)))."""
    thr = int(math.floor(float(p) * 65536.0 + 0.5))
    return thr, np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(n, seed, step, site, thr):
    """bool [n] (n a multiple of 8): chunk k = elements 8k .. 8k+7 draws x = Philox4x32-10((k, site, step_lo, step_hi),
    (seed_lo, seed_hi)); element e of the chunk owns r = (x[e >> 1] >> (16 * (e & 1))) & 0xFFFF and is kept iff
    r >= thr."""
    assert n % 8 == 0 and n // 8 <= 2 ** 32
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    k = np.arange(n // 8, dtype=np.uint64)
    x = philox4x32_10((k, np.full_like(k, site), np.full_like(k, step & MASK), np.full_like(k, step >> 32)),
                      (seed & MASK, seed >> 32))
    r = np.empty((n // 8, 8), dtype=np.uint64)
    for e in range(8):
        r[:, e] = (x[e >> 1] >> np.uint64(16 * (e & 1))) & np.uint64(0xFFFF)
    return (r >= np.uint64(thr)).reshape(n)


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite inputs."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def _finish(v, bf16):
    return bf16_round(v) if bf16 else v


# ---- the four kernels in float32: every product and sum below is ONE float32 operation, as the kernels perform it
def dropout(x, keep, factor, bf16=False):
    """mask * (x * factor); a dropped element is +0."""
    x = np.asarray(x, dtype=np.float32)
    return _finish(np.where(keep, x * np.float32(factor), np.float32(0.0)).astype(np.float32), bf16)


def dropout_add(branch, residual, keep, factor, bf16=False):
    """residual + mask * (branch * factor): the product rounded to float32, then the sum."""
    m = dropout(branch, keep, factor)
    return _finish((np.asarray(residual, dtype=np.float32) + m).astype(np.float32), bf16)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_dropout_fwd(x, keep, factor, bf16=False):
    """mask * (gelu(x) * factor), the GELU evaluated in float64 and rounded to float32 (the kernel's erff is within a
    few ulp of that: compare with a tolerance, the zero pattern exactly)."""
    return dropout(gelu64(x).astype(np.float32), keep, factor, bf16)


def gelu_dropout_bwd(dy, x, keep, factor, bf16=False):
    """(mask * (dy * factor)) * gelu'(x)."""
    m = dropout(dy, keep, factor)
    return _finish((m * gelu_grad64(x).astype(np.float32)).astype(np.float32), bf16)


# ---- ViTCELoss(type='sigmoid'): passl/loss/celoss.py:58-95
def vit_ce_targets(epsilon):
    """(t_on, t_off) in double: onehot * (1 - eps) + eps at the label / elsewhere."""
    if epsilon is None:
        return 1.0, 0.0
    return 1.0 * (1.0 - epsilon) + epsilon, 0.0 * (1.0 - epsilon) + epsilon


def vit_ce_targets_ref32(epsilon):
    """The two target values as the reference's own line forms them: in the float32 of F.one_hot's result."""
    if epsilon is None:
        return 1.0, 0.0
    f = np.float32
    return float(f(1.0) * f(1.0 - epsilon) + f(epsilon)), float(f(0.0) * f(1.0 - epsilon) + f(epsilon))


def vit_ce(x, labels, epsilon, dtype=np.float64, targets=None):
    """-> (terms [N, C], rows [N], loss, dx [N, C] for an incoming gradient of 1, sigmoid [N, C], target [N, C]), all
    evaluated in ``dtype``: term = max(x, 0) - x t + log1p(exp(-|x|)), rows = sum_c, loss = mean, dx = (sigmoid(x) -
    t) / N.  ``targets``: (t_on, t_off) in place of vit_ce_targets(epsilon)."""
    x = np.asarray(x, dtype=dtype)
    N, C = x.shape
    t_on, t_off = targets or vit_ce_targets(epsilon)
    t = np.full((N, C), t_off, dtype=dtype)
    t[np.arange(N), np.asarray(labels)] = t_on
    terms = np.maximum(x, dtype(0)) - x * t + np.log1p(np.exp(-np.abs(x)))
    rows = terms.sum(axis=1, dtype=dtype)
    with np.errstate(over='ignore'):
        sig = dtype(1) / (dtype(1) + np.exp(-x))
    return terms, rows, rows.sum(dtype=dtype) / dtype(N), (sig - t) / dtype(N), sig, t


# ---- a float64 ViT (passl/models/vision_transformer.py:339-363) with the dropout masks handed in
def vit_fp64(sd, x, depth, heads, patch, eps, drop=None):
    """``sd``: name -> float64 CPU tensor (state_dict names); ``drop``: None (evaluation) or a function
    (tensor [B, T, C], site) -> tensor that applies the mask of that site, e.g. ``site_dropper`` below.  Sites:
    pos_drop 0; block i: 1 + 3i after proj, 2 + 3i after the activation, 3 + 3i after fc2."""
    import torch
    import torch.nn.functional as F
    drop = drop or (lambda t, site: t)
    B = x.shape[0]
    t = F.conv2d(x.double(), sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'], stride=patch)
    t = t.flatten(2).transpose(1, 2)
    t = drop(torch.cat([sd['cls_token'].expand(B, -1, -1), t], 1) + sd['pos_embed'], 0)
    D = t.shape[-1]
    for i in range(depth):
        p = 'blocks.%d.' % i
        h = F.layer_norm(t, (D,), sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], eps)
        qkv = h @ sd[p + 'attn.qkv.weight'] + sd.get(p + 'attn.qkv.bias', 0.0)
        qkv = qkv.reshape(B, -1, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
        att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * (D // heads) ** -0.5, -1)
        a = (att @ qkv[2]).transpose(1, 2).reshape(B, -1, D)
        t = t + drop(a @ sd[p + 'attn.proj.weight'] + sd[p + 'attn.proj.bias'], 1 + 3 * i)
        h = F.layer_norm(t, (D,), sd[p + 'norm2.weight'], sd[p + 'norm2.bias'], eps)
        a = drop(F.gelu(h @ sd[p + 'mlp.fc1.weight'] + sd[p + 'mlp.fc1.bias']), 2 + 3 * i)
        t = t + drop(a @ sd[p + 'mlp.fc2.weight'] + sd[p + 'mlp.fc2.bias'], 3 + 3 * i)
    f = F.layer_norm(t, (D,), sd['norm.weight'], sd['norm.bias'], eps)[:, 0]
    return f @ sd['head.weight'] + sd['head.bias']


def site_dropper(p, seed, step, site_shift=0):
    """The ``drop`` of vit_fp64 for rate p: the host mask of (seed, step, site + site_shift) over the tensor's elements in
    row-major order, times factor."""
    import torch
    thr, factor = thr_factor(p)

    def drop(t, site):
        keep = keep_mask(t.numel(), seed, step, site + site_shift, thr).reshape(tuple(t.shape))
        return t * (torch.from_numpy(keep).double() * float(factor))
    return drop
