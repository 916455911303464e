"""CPU helpers of the ConvNeXt kernel tests (pure torch / numpy: no GPU, the native library is never loaded).

Cases, float64 references and element-wise bounds for csrc/dwconv.hip, shared by test_dwconv_host.py (a float32
evaluation in a shuffled summation order meets every bound) and test_dwconv_gpu.py (the kernels).

Every input is first rounded through the compute dtype, so the references see the kernels' inputs exactly; filter,
bias and gamma are fp32 parameters and stay fp32.  E = 2^-24; u = 2^-8 for a bf16 store, 0 for fp32 (bn_pool_util.py
has the reason for 2^-8); n is the number of accumulated terms.

  y       |y - y64|   <= (n + 1) E (sum |x w| + |bias|) + u |y64|,  n = 50 (49 taps and the bias)
  dx      the same with |add| in place of |bias|
  dw      |dw - dw64| <= (n + 1) E sum |dy x|,  n = N H W            dbias  (n + 1) E sum |dy|, n = N H W
  dgamma  (n + 1) E sum |branch g|, n = B T, g = keep (dy / keep_prob) formed in float64 from the fp32 keep_prob

A sum of n terms evaluated in fp32 in ANY order, each term a correctly rounded product (or an fma), is within
(n + 1) E sum |terms| of the exact sum to first order (n - 1 additions and one product rounding, each at most E of the
sum of the magnitudes), so the bounds constrain nothing about a kernel's tiling or slab order.

dbranch = gamma g has two roundings (the division, the product) and, with a table, the exact factor keep = 0 / 1:
|dbranch - dbranch64| <= 3 E |dbranch64| + u |dbranch64|.

layer_scale_add forward has no bound: it is compared bit for bit with `layer_scale_restated`, the numpy statement of
the reference's op sequence (`self.gamma * x` convnext.py:100, `x.divide(keep_prob) * random_tensor`
vision_transformer.py:68, `input + ...` convnext.py:102) in fp32, each operation rounded, then one rounding to `dtype`.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bn_pool_util import DTNAME, DTYPES, E, rnd, unit, usage, verdict   # noqa: F401  (re-exported)

# (N, H, W, C): images smaller than the halo, odd sizes that straddle tile edges, C / 8 odd, C no multiple of the
# 32-channel chunk, several workgroups, several weight-gradient slabs; the last has 520 weight-gradient tiles, more
# than the 512 slabs, so some workgroups of that launch visit a second tile
SHAPES = ((1, 1, 1, 8), (2, 3, 5, 8), (1, 7, 7, 96), (3, 9, 20, 40), (1, 17, 33, 24), (2, 14, 14, 192),
          (4, 28, 28, 96), (1, 56, 56, 96), (52, 33, 17, 8))
# the hard kinds probe the arithmetic, not the geometry: they run on three shapes (one chunk / a partial chunk / six)
HARD_SHAPES = ((2, 3, 5, 8), (3, 9, 20, 40), (2, 14, 14, 192))
KINDS = ('plain', 'cancel', 'bigbias')
CASES = tuple((s, 'plain', d) for s in SHAPES for d in DTYPES) + \
    tuple((s, k, d) for s in HARD_SHAPES for k in KINDS[1:] for d in DTYPES)

# (B, T, C): one chunk; C / 8 odd; several row lanes; three forward workgroups per sample; a slab of the backward that
# spans two samples (rows_per = 3, T = 700); more than 256 chunk columns (the column loop of the backward)
LS_SHAPES = ((1, 1, 8), (3, 7, 24), (2, 50, 40), (4, 196, 96), (3, 700, 16), (2, 3, 2056))
LS_CASES = tuple((s, t, d) for s in LS_SHAPES for t in (False, True) for d in DTYPES)
KEEP_PROB = float(np.float32(1) - np.float32(0.3))


def case_id(case):
    shape, kind, dtype = case
    return '%s-%s-%s' % ('x'.join(str(v) for v in shape), kind, DTNAME[dtype])


def ls_case_id(case):
    shape, table, dtype = case
    return '%s-%s-%s' % ('x'.join(str(v) for v in shape), 'table' if table else 'nokeep', DTNAME[dtype])


def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


def wgrad_ws_floats(N, H, W, C):
    """include/passl_hip.h: PASSL_DWCONV7_WGRAD_WS_FLOATS."""
    return min(N * -(-H // 8) * -(-W // 16), 512) * 50 * C


def ls_bwd_ws_floats(M, C):
    """include/passl_hip.h: PASSL_LAYER_SCALE_BWD_WS_FLOATS."""
    rows_per = -(-M // 1024)
    return -(-M // rows_per) * C


# ------------------------------------------------------------------------------------------------ depthwise 7x7
@functools.lru_cache(maxsize=None)
def conv_data(case):
    """x, dy, dyw (the dy of the weight gradient), add [N, H, W, C] (fp32 tensors holding values of the compute dtype),
    w [C, 1, 7, 7], bias [C] (fp32).

    cancel:  x and dy are a constant image (100) plus a sparse signal of +-0.5 (both bf16-representable) and the filter
             is a +-1 checkerboard with a zero centre, so in the interior sum |x w| = 4800 against |y| of order 0.5:
             10^4 times; dyw is a +-1 checkerboard over the pixels, so the weight gradient cancels the same way.
    bigbias: bias and add of magnitude 10^4 over operands of order 1."""
    (N, H, W, C), kind, dtype = case
    gen = torch.Generator().manual_seed(_seed(N, H, W, C, KINDS.index(kind)))
    shape = (N, H, W, C)
    x = torch.randn(shape, generator=gen) * 2 + 0.5
    dy = torch.randn(shape, generator=gen)
    add = torch.randn(shape, generator=gen)
    w = torch.randn(C, 1, 7, 7, generator=gen) * 0.3
    bias = torch.randn(C, generator=gen)
    dyw = dy
    if kind == 'cancel':
        def sparse():
            on = torch.rand(shape, generator=gen) < 0.125
            return 100.0 + 0.5 * on * torch.randint(-1, 2, shape, generator=gen).float()
        x, dy = sparse(), sparse()
        rs = torch.arange(7)
        sign = (1 - 2 * ((rs[:, None] + rs[None, :]) % 2)).float()
        sign[3, 3] = 0.0
        w = sign.expand(C, 1, 7, 7).contiguous() * (1 + torch.arange(C).float().view(C, 1, 1, 1) % 3)
        p, q = torch.arange(H), torch.arange(W)
        dyw = (1 - 2 * ((p[:, None] + q[None, :]) % 2)).float().view(1, H, W, 1).expand(shape).contiguous()
    elif kind == 'bigbias':
        bias = (1 - 2 * (torch.arange(C) % 2)).float() * 1e4 + bias
        add = torch.where(add > 0, 1e4, -1e4) + add
    return dict(x=rnd(x, dtype), dy=rnd(dy, dtype), dyw=rnd(dyw, dtype), add=rnd(add, dtype), w=w, bias=bias)


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fwd_ref(case):
    """y64 and its bound [N, H, W, C]."""
    d, C, u = conv_data(case), case[0][3], unit(case[2])
    w, b = d['w'].double(), d['bias'].double()
    y = _nhwc(F.conv2d(_nchw(d['x']), w, b, padding=3, groups=C))
    mag = _nhwc(F.conv2d(_nchw(d['x']).abs(), w.abs(), b.abs(), padding=3, groups=C))
    return y, 51 * E * mag + u * y.abs()


@functools.lru_cache(maxsize=None)
def bwd_data_ref(case, with_add):
    """dx64 and its bound [N, H, W, C]."""
    d, C, u = conv_data(case), case[0][3], unit(case[2])
    w = d['w'].double()
    dx = _nhwc(F.conv_transpose2d(_nchw(d['dy']), w, None, padding=3, groups=C))
    mag = _nhwc(F.conv_transpose2d(_nchw(d['dy']).abs(), w.abs(), None, padding=3, groups=C))
    if with_add:
        dx, mag = dx + d['add'].double(), mag + d['add'].double().abs()
    return dx, 51 * E * mag + u * dx.abs()


@functools.lru_cache(maxsize=None)
def bwd_weight_ref(case):
    """dw64 [C, 1, 7, 7], its bound, dbias64 [C], its bound."""
    d, (N, H, W, C) = conv_data(case), case[0]
    n = N * H * W
    x, dy = _nchw(d['x']), _nchw(d['dyw'])
    dw = torch.nn.grad.conv2d_weight(x, (C, 1, 7, 7), dy, padding=3, groups=C)
    mag = torch.nn.grad.conv2d_weight(x.abs(), (C, 1, 7, 7), dy.abs(), padding=3, groups=C)
    return dw, (n + 1) * E * mag, dy.sum((0, 2, 3)), (n + 1) * E * dy.abs().sum((0, 2, 3))


def shifted(v, r, s):
    """v [N, H, W, C] -> t with t[n, p, q] = v[n, p + r - 3, q + s - 3], zero outside (slicing only: independent of
    conv2d)."""
    N, H, W, C = v.shape
    t = torch.zeros_like(v)
    dp, dq = r - 3, s - 3
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


def host_fp32(case, with_add=True):
    """The three directions evaluated on the CPU in fp32 (products rounded, summed in a shuffled order) and rounded to
    the storage dtype: y, dx, dw, dbias."""
    d, (N, H, W, C), dtype = conv_data(case), case[0], case[2]
    gen = torch.Generator().manual_seed(_seed(N, H, W, C, 99))
    w = d['w']
    taps = [(r, s) for r in range(7) for s in range(7)]
    y = _ordered_sum([shifted(d['x'], r, s) * w[:, 0, r, s] for r, s in taps] + [d['bias'].expand(N, H, W, C)], gen)
    terms = [shifted(d['dy'], 6 - r, 6 - s) * w[:, 0, r, s] for r, s in taps]
    dx = _ordered_sum(terms + ([d['add']] if with_add else []), gen)
    perm = torch.randperm(N * H * W, generator=gen)
    dyw = d['dyw'].reshape(-1, C)[perm]
    dw = torch.stack([(dyw * shifted(d['x'], r, s).reshape(-1, C)[perm]).sum(0) for r, s in taps], 1).view(C, 1, 7, 7)
    return rnd(y, dtype), rnd(dx, dtype), dw, dyw.sum(0)


# ------------------------------------------------------------------------------------------------ layer scale
@functools.lru_cache(maxsize=None)
def ls_data(case):
    """branch, residual, dy [B*T, C] (values of the compute dtype), gamma [C], keep [B] (fp32 0 / 1, at least one of
    each when B > 1; None without a table)."""
    (B, T, C), table, dtype = case
    gen = torch.Generator().manual_seed(_seed(B, T, C, 5))
    branch = torch.randn(B * T, C, generator=gen) * 2
    residual = torch.randn(B * T, C, generator=gen)
    dy = torch.randn(B * T, C, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[1], gamma[2] = 1e-6, -1.0
    keep = None
    if table:
        keep = (torch.rand(B, generator=gen) < KEEP_PROB).float()
        keep[0] = 1.0
        if B > 1:
            keep[1] = 0.0
    return dict(branch=rnd(branch, dtype), residual=rnd(residual, dtype), dy=rnd(dy, dtype), gamma=gamma, keep=keep)


def layer_scale_restated(branch, residual, gamma, keep, keep_prob, T, dtype):
    """numpy, fp32, one rounding per operation; rows of a dropped sample are the residual's."""
    x, res, g = branch.numpy().astype(np.float32), residual.numpy().astype(np.float32), gamma.numpy()
    t = (g[None, :] * x).astype(np.float32)
    if keep is not None:
        k = np.repeat(keep.numpy().astype(np.float32), T)[:, None]
        with np.errstate(invalid='ignore'):
            t = (t / np.float32(keep_prob)).astype(np.float32)
            t = (t * k).astype(np.float32)
        out = np.where(k != 0, (res + t).astype(np.float32), res)
    else:
        out = (res + t).astype(np.float32)
    return torch.from_numpy(out).to(dtype)


def layer_scale_reference_ops(branch, residual, gamma, keep, keep_prob, T):
    """The reference's op sequence on fp32 torch tensors (convnext.py:100-102, vision_transformer.py:60-68)."""
    x = gamma * branch
    if keep is not None:
        kp = torch.tensor(keep_prob, dtype=x.dtype)
        random_tensor = keep.repeat_interleave(T).view(-1, 1)
        x = x.divide(kp) * random_tensor
    return residual + x


@functools.lru_cache(maxsize=None)
def ls_bwd_ref(case):
    """dbranch64 [B*T, C] and its bound, dgamma64 [C] and its bound."""
    d, (B, T, C), table, dtype = ls_data(case), case[0], case[1], case[2]
    g = d['dy'].double()
    if table:
        g = d['keep'].double().repeat_interleave(T).view(-1, 1) * (g / float(np.float32(KEEP_PROB)))
    db = d['gamma'].double() * g
    prod = d['branch'].double() * g
    return db, (3 * E + unit(dtype)) * db.abs(), prod.sum(0), (B * T + 1) * E * prod.abs().sum(0)


def ls_bwd_host_fp32(case):
    """dbranch (rounded to the storage dtype) and dgamma in fp32 on the CPU, the rows in a shuffled order."""
    d, (B, T, C), table, dtype = ls_data(case), case[0], case[1], case[2]
    g = d['dy']
    if table:
        g = d['keep'].repeat_interleave(T).view(-1, 1) * (g / torch.tensor(KEEP_PROB, dtype=torch.float32))
    perm = torch.randperm(B * T, generator=torch.Generator().manual_seed(_seed(B, T, C, 7)))
    return rnd(d['gamma'] * g, dtype), (d['branch'] * g)[perm].sum(0)
