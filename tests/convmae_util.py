"""CPU helpers of the ConvMAE kernel tests (pure torch / numpy: no GPU, the native library is never loaded).

Cases, float64 references and element-wise bounds for csrc/convmae.hip, shared by test_convmae_kernels_host.py (a
float32 evaluation in a shuffled summation order meets every bound, planted defects break them) and
test_convmae_kernels_gpu.py (the kernels).

Every input is first rounded through the compute dtype, so the references see the kernels' inputs exactly; filter and
bias are fp32 parameters and stay fp32.  The mask is the 0 / 1 table [N, Hm * Wm] that passl_hip_mae_mask writes
(1 = removed); keep(n, h, w) = 1 - mask[n, (h // g) * Wm + w // g] with g = H / Hm = W / Wm.  A factor of 0 or 1 is
exact, so keep * x is a value of the compute dtype and adds no rounding.
E = 2^-24; u = 2^-8 for a bf16 store, 0 for fp32 (bn_pool_util.py has the reason for 2^-8); n = accumulated terms.

  y       |y - y64|   <= (n + 1) E (sum |keep x w| + |bias|) + u |y64|,  n = 26 (25 taps and the bias)
  dx      |dx - dx64| <= (n + 1) E keep sum |dy w| + u |dx64|,            n = 25
  dw      |dw - dw64| <= (n + 1) E sum |dy keep x|,  n = N H W            dbias  (n + 1) E sum |dy|, n = N H W

A sum of n terms evaluated in fp32 in ANY order, each term a correctly rounded product (or an fma), is within
(n + 1) E sum |terms| of the exact sum to first order (convnext_util.py), so the bounds constrain nothing about a
kernel's tiling or slab order.

The gather and token kernels move values or add two of them: they are compared bit for bit with the numpy restatements
below (one fp32 add, one rounding to the storage dtype).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bn_pool_util import DTNAME, DTYPES, E, rnd, unit, usage, verdict   # noqa: F401  (re-exported)

# (N, H, W, C, g): a single pixel; an image smaller than the halo; one mask cell over the whole map; C no multiple of
# the 32-channel chunk with a non-square grid; odd sizes that straddle tile edges; several workgroups and channel
# chunks; the stage-1 map (56 x 56 over a 14 x 14 grid); 520 weight-gradient tiles, more than the 512 slabs, so some
# workgroups of that launch visit a second tile
SHAPES = ((1, 1, 1, 8, 1), (2, 3, 5, 8, 1), (1, 4, 4, 8, 4), (3, 8, 12, 40, 2), (1, 17, 33, 24, 1),
          (2, 28, 28, 96, 2), (1, 56, 56, 32, 4), (52, 33, 17, 8, 1))
MASKS = ('null', 'kept', 'removed', 'checker', 'random')
CASES = tuple((s, m, d) for s in SHAPES for m in MASKS for d in DTYPES)
MASK_RATIO = 0.75


def case_id(case):
    shape, kind, dtype = case
    return '%s-g%d-%s-%s' % ('x'.join(str(v) for v in shape[:4]), shape[4], kind, DTNAME[dtype])


def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


def wgrad_ws_floats(N, H, W, C):
    """include/passl_hip.h: PASSL_DWCONV5_WGRAD_WS_FLOATS."""
    return min(N * -(-H // 8) * -(-W // 16), 512) * 26 * C


def make_mask(kind, N, Hm, Wm, gen):
    """fp32 [N, Hm * Wm], 1 = removed; None for 'null'.  random: int(L (1 - 0.75)) patches of every image are kept, as
    random_masking keeps them."""
    Lm = Hm * Wm
    if kind == 'null':
        return None
    if kind == 'kept':
        return torch.zeros(N, Lm)
    if kind == 'removed':
        return torch.ones(N, Lm)
    if kind == 'checker':
        i, j = torch.arange(Hm)[:, None], torch.arange(Wm)[None, :]
        m = ((i + j) % 2).float().reshape(1, Lm).repeat(N, 1)
        m[1::2] = 1 - m[1::2]                     # odd images carry the opposite board
        return m
    keep = int(Lm * (1 - MASK_RATIO))
    m = torch.ones(N, Lm)
    for n in range(N):
        m[n, torch.randperm(Lm, generator=gen)[:keep]] = 0.0
    return m


def keep_map(mask, N, H, W, g, shift=0):
    """[N, H, W, 1] float64 keep factors (ones without a mask), by indexing, not by the kernels' arithmetic.
    shift: the planted off-by-one, rows (h + shift) // g."""
    if mask is None:
        return torch.ones(N, H, W, 1, dtype=torch.float64)
    Hm, Wm = H // g, W // g
    hi = ((torch.arange(H) + shift) // g).clamp(max=Hm - 1)
    wi = torch.arange(W) // g
    idx = hi[:, None] * Wm + wi[None, :]
    return (1.0 - mask.double())[:, idx].unsqueeze(-1)


@functools.lru_cache(maxsize=None)
def conv_data(case):
    """x, dy [N, H, W, C] (fp32 tensors holding values of the compute dtype), w [C, 1, 5, 5], bias [C] (fp32), mask
    (fp32 [N, Hm * Wm] or None), keep [N, H, W, 1] float64, grid (Hm, Wm)."""
    (N, H, W, C, g), kind, dtype = case
    gen = torch.Generator().manual_seed(_seed(N, H, W, C, g, MASKS.index(kind)))
    shape = (N, H, W, C)
    x = torch.randn(shape, generator=gen) * 2 + 0.5
    dy = torch.randn(shape, generator=gen)
    w = torch.randn(C, 1, 5, 5, generator=gen) * 0.3
    bias = torch.randn(C, generator=gen)
    mask = make_mask(kind, N, H // g, W // g, gen)
    return dict(x=rnd(x, dtype), dy=rnd(dy, dtype), w=w, bias=bias, mask=mask, keep=keep_map(mask, N, H, W, g),
                grid=(H // g, W // g))


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_ref(case):
    """y64 and its bound [N, H, W, C]."""
    d, C, u = conv_data(case), case[0][3], unit(case[2])
    w, b = d['w'].double(), d['bias'].double()
    xk = d['x'].double() * d['keep']
    y = _nhwc(F.conv2d(_nchw(xk), w, b, padding=2, groups=C))
    mag = _nhwc(F.conv2d(_nchw(xk).abs(), w.abs(), b.abs(), padding=2, groups=C))
    return y, 27 * E * mag + u * y.abs()


@functools.lru_cache(maxsize=None)
def bwd_data_ref(case):
    """dx64 and its bound [N, H, W, C]."""
    d, C, u = conv_data(case), case[0][3], unit(case[2])
    w = d['w'].double()
    dx = d['keep'] * _nhwc(F.conv_transpose2d(_nchw(d['dy']), w, None, padding=2, groups=C))
    mag = d['keep'] * _nhwc(F.conv_transpose2d(_nchw(d['dy']).abs(), w.abs(), None, padding=2, groups=C))
    return dx, 26 * E * mag + u * dx.abs()


@functools.lru_cache(maxsize=None)
def bwd_weight_ref(case):
    """dw64 [C, 1, 5, 5], its bound, dbias64 [C], its bound."""
    d, (N, H, W, C, _) = conv_data(case), case[0]
    n = N * H * W
    x, dy = _nchw(d['x'].double() * d['keep']), _nchw(d['dy'])
    dw = torch.nn.grad.conv2d_weight(x, (C, 1, 5, 5), dy, padding=2, groups=C)
    mag = torch.nn.grad.conv2d_weight(x.abs(), (C, 1, 5, 5), dy.abs(), padding=2, groups=C)
    return dw, (n + 1) * E * mag, dy.sum((0, 2, 3)), (n + 1) * E * dy.abs().sum((0, 2, 3))


def shifted(v, r, s):
    """v [N, H, W, C] -> t with t[n, p, q] = v[n, p + r - 2, q + s - 2], zero outside (slicing only: independent of
    conv2d)."""
    N, H, W, C = v.shape
    t = torch.zeros_like(v)
    dp, dq = r - 2, s - 2
    p0, p1 = max(0, -dp), min(H, H - dp)
    q0, q1 = max(0, -dq), min(W, W - dq)
    if p0 < p1 and q0 < q1:
        t[:, p0:p1, q0:q1] = v[:, p0 + dp:p1 + dp, q0 + dq:q1 + dq]
    return t


def _ordered_sum(terms, gen):
    """fp32 sum of a list of tensors, one after the other in a shuffled order."""
    order = torch.randperm(len(terms), generator=gen).tolist()
    acc = terms[order[0]].clone()
    for i in order[1:]:
        acc += terms[i]
    return acc


TAPS = tuple((r, s) for r in range(5) for s in range(5))


def host_fp32(case, defect=None):
    """The three directions evaluated on the CPU in fp32 (products rounded, summed in a shuffled order) and rounded to
    the storage dtype: y, dx, dw, dbias.  defect plants one error:
      'mask_at_output'  y = keep * conv(x) + bias instead of conv(keep * x) + bias
      'unreversed'      dx reads the filter as the forward does
      'row_off_by_one'  the keep factor of row h is taken from mask row (h + 1) // g"""
    d, (N, H, W, C, g), dtype = conv_data(case), case[0], case[2]
    gen = torch.Generator().manual_seed(_seed(N, H, W, C, 99))
    w = d['w']
    keep = d['keep'] if defect != 'row_off_by_one' else keep_map(d['mask'], N, H, W, g, shift=1)
    keep = keep.float()
    xk = d['x'] if defect == 'mask_at_output' else d['x'] * keep
    y = _ordered_sum([shifted(xk, r, s) * w[:, 0, r, s] for r, s in TAPS], gen)
    if defect == 'mask_at_output':
        y = y * keep
    y = y + d['bias']
    if defect == 'unreversed':
        terms = [shifted(d['dy'], 4 - r, 4 - s) * w[:, 0, 4 - r, 4 - s] for r, s in TAPS]
    else:
        terms = [shifted(d['dy'], 4 - r, 4 - s) * w[:, 0, r, s] for r, s in TAPS]
    dx = _ordered_sum(terms, gen) * keep
    perm = torch.randperm(N * H * W, generator=gen)
    dyp = d['dy'].reshape(-1, C)[perm]
    xm = d['x'] * keep
    dw = torch.stack([(dyp * shifted(xm, r, s).reshape(-1, C)[perm]).sum(0) for r, s in TAPS], 1).view(C, 1, 5, 5)
    return rnd(y, dtype), rnd(dx, dtype), dw, dyp.sum(0)


# ------------------------------------------------------------------------------------------------ gather, tokens
# (B, Hm, Wm, p, C, K): one patch; the stage-2 form (2 x 2 patches) with C / 8 odd; the stage-1 form (4 x 4) on a
# non-square grid; 14 x 14 grid with K = 49 as the model has it
GATHER_SHAPES = ((1, 1, 1, 1, 8, 1), (2, 3, 4, 2, 24, 5), (3, 2, 3, 4, 40, 2), (2, 14, 14, 2, 16, 49))
GATHER_CASES = tuple((s, d) for s in GATHER_SHAPES for d in DTYPES)
# (B, L, K, D): one token; D / 8 odd; K == L (nothing removed); the model's 196 / 49 with several column blocks and
# position slabs (B * L > 128)
TOKEN_SHAPES = ((1, 1, 1, 8), (3, 7, 2, 24), (2, 5, 5, 40), (2, 196, 49, 264))
TOKEN_CASES = tuple((s, d) for s in TOKEN_SHAPES for d in DTYPES)


def pair_id(case):
    shape, dtype = case
    return '%s-%s' % ('x'.join(str(v) for v in shape), DTNAME[dtype])


def masking(B, L, K, gen):
    """ids_keep int32 [B, K], ids_restore int32 [B, L] as passl_hip_mae_mask writes them, from random noise."""
    noise = torch.rand(B, L, generator=gen)
    ids_shuffle = torch.argsort(noise, dim=1, stable=True)
    ids_restore = torch.argsort(ids_shuffle, dim=1, stable=True)
    return ids_shuffle[:, :K].to(torch.int32).contiguous(), ids_restore.to(torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def gather_data(case):
    (B, Hm, Wm, p, C, K), dtype = case
    gen = torch.Generator().manual_seed(_seed(B, Hm, Wm, p, C, K))
    x = rnd(torch.randn(B, Hm * p, Wm * p, C, generator=gen), dtype)
    dout = rnd(torch.randn(B * K, p * p * C, generator=gen), dtype)
    ids_keep, ids_restore = masking(B, Hm * Wm, K, gen)
    return dict(x=x, dout=dout, ids_keep=ids_keep, ids_restore=ids_restore)


def gather_restated(x, ids_keep, Hm, Wm, p):
    """[B * K, p * p * C] by slicing: row (b, k) is patch ids_keep[b, k] flattened (ph, pw, c)."""
    B, K = ids_keep.shape
    C = x.shape[3]
    out = torch.empty(B * K, p * p * C)
    for b in range(B):
        for k in range(K):
            ph, pw = divmod(int(ids_keep[b, k]), Wm)
            out[b * K + k] = x[b, ph * p:(ph + 1) * p, pw * p:(pw + 1) * p].reshape(-1)
    return out


def gather_bwd_restated(dout, ids_restore, K, Hm, Wm, p, C):
    B = ids_restore.shape[0]
    dx = torch.zeros(B, Hm * p, Wm * p, C)
    for b in range(B):
        for l in range(Hm * Wm):
            r = int(ids_restore[b, l])
            if r < K:
                ph, pw = divmod(l, Wm)
                dx[b, ph * p:(ph + 1) * p, pw * p:(pw + 1) * p] = dout[b * K + r].view(p, p, C)
    return dx


@functools.lru_cache(maxsize=None)
def token_data(case):
    (B, L, K, D), dtype = case
    gen = torch.Generator().manual_seed(_seed(B, L, K, D, 3))
    ids_keep, ids_restore = masking(B, L, K, gen)
    return dict(x=rnd(torch.randn(B, K, D, generator=gen), dtype), pos=torch.randn(L, D, generator=gen),
                mask_token=torch.randn(D, generator=gen), dout_k=rnd(torch.randn(B, K, D, generator=gen), dtype),
                dout_l=rnd(torch.randn(B, L, D, generator=gen), dtype), ids_keep=ids_keep, ids_restore=ids_restore)


def _add_f32(a, b, dtype):
    """One fp32 add of two fp32 arrays, one rounding to the storage dtype."""
    return torch.from_numpy((a.numpy().astype(np.float32) + b.numpy().astype(np.float32)).astype(np.float32)).to(dtype)


def pos_gather_add_restated(x, pos, ids_keep, dtype):
    return _add_f32(x, pos[ids_keep.long()], dtype)


def pos_gather_add_bwd_restated(dout, ids_restore, K, start=None):
    """dpos [L, D] fp32: the images added one after the other in ascending order from 0, in fp32, then that sum added
    to ``start`` (the gradient the kernel accumulates into)."""
    B, L = ids_restore.shape
    dpos = np.zeros((L, dout.shape[-1]), dtype=np.float32)
    for b in range(B):
        for l in range(L):
            r = int(ids_restore[b, l])
            if r < K:
                dpos[l] = (dpos[l] + dout[b, r].numpy().astype(np.float32)).astype(np.float32)
    if start is not None:
        dpos = (start.numpy().astype(np.float32) + dpos).astype(np.float32)
    return torch.from_numpy(dpos)


# (B, C, H, W, p): one patch; a 2 x 3 grid of 4 x 4 patches; the model's 14 x 14 grid of 16 x 16 patches
LOSS_SHAPES = ((1, 3, 2, 2, 2), (3, 3, 8, 12, 4), (2, 3, 224, 224, 16))
LOSS_CASES = tuple((s, n) for s in LOSS_SHAPES for n in (False, True))


def loss_id(case):
    shape, norm = case
    return '%s-%s' % ('x'.join(str(v) for v in shape), 'normpix' if norm else 'rawpix')


@functools.lru_cache(maxsize=None)
def loss_data(case):
    """img [B, C, H, W], pred [B, L, P], mask [B, L] (0.75 removed, at least one), all fp32."""
    (B, C, H, W, p), _ = case
    gen = torch.Generator().manual_seed(_seed(B, C, H, W, p, 13))
    L = (H // p) * (W // p)
    mask = make_mask('random', B, 1, L, gen)
    return dict(img=torch.randn(B, C, H, W, generator=gen), pred=torch.randn(B, L, p * p * C, generator=gen), mask=mask,
                denom=float(mask.sum()))


def unshuffle_restated(x, mask_token, pos, ids_restore, dtype):
    B, K, D = x.shape
    L = ids_restore.shape[1]
    full = torch.cat([x, mask_token.view(1, 1, D).expand(B, 1, D)], 1)            # row K = the mask token
    src = ids_restore.long().clamp(max=K)
    rows = torch.gather(full, 1, src.unsqueeze(-1).expand(B, L, D))
    return _add_f32(rows, pos.unsqueeze(0).expand(B, L, D), dtype)


def unshuffle_bwd_ref(dout, ids_keep, ids_restore):
    """dx [B, K, D] (a copy: exact) and the float64 sum over the removed positions with its bound
    (n + 1) E sum |dout|, n = B L."""
    B, L, D = dout.shape
    K = ids_keep.shape[1]
    dx = torch.gather(dout, 1, ids_keep.long().unsqueeze(-1).expand(B, K, D))
    removed = (ids_restore >= K).unsqueeze(-1).double()
    dm = (dout.double() * removed).sum((0, 1))
    return dx, dm, (B * L + 1) * E * (dout.double().abs() * removed).sum((0, 1))
