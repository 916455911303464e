"""CPU helpers of the BatchNorm / pooling numerics tests (pure torch: no GPU, the native library is never loaded).

Cases, float64 references and element-wise bounds for csrc/bn.hip, layout_pool.hip (max / average pool) and
stem_pool.hip, shared by test_bn_pool_numerics_host.py (which shows that a float32 evaluation meets every bound and
that planted defects break them) and test_bn_pool_numerics_gpu.py (the kernels).

Every input is first rounded through the compute dtype, so the references see the kernels' inputs exactly.  A kernel
that consumes per-channel constants (scale, shift, mean, invstd, coef) is judged with the fp32 constants it was
handed: the reference takes them as float64.  e = 2^-24; u = 2^-8 for bf16 storage, 0 for fp32 storage.

  bn_apply        pre = x s + b (+ r), B_apply = 4 e (|x s| + |b| + |r|):  |z - z64| <= B_apply + u |z64|
                  three fp32 roundings, each at most e of the sum of the term magnitudes; the fourth e covers the
                  second order and the u B_apply of the store.  ReLU is 1-Lipschitz: the same bound with ReLU.
                  mask byte i, bit e == (z_got[8 i + e] > 0), exactly.
  bn_bwd_apply    |dx - dx64| <= 4 e (|A g| + |B x| + |Cc|) + u |dx64|, g the masked gradient; dres carries g's bits.
                  Mask source 2 (x scale + shift > 0, recomputed): an element with |pre64| <= B_apply may fall on
                  either side; it must meet the bound with g = dz or with g = 0.  At most AMBIGUOUS_CAP of a case.
  bn_stats        slab b of n rows, s = its first row: the stored shift is that row;
                  |S1 - sum (x - s)| <= (n + 1) e sum |x - s|,  |S2 - sum (x - s)^2| <= (n + 3) e sum (x - s)^2
                  (any-order fp32 summation, n - 1 additions, plus the rounding of the difference and the square).
  bn_bwd_reduce   |sum g| within (n + 1) e sum |g|, |sum g xhat| within (n + 4) e sum |g xhat|, xhat in float64 from
                  the fp32 mean and invstd.  Mask source 2: an ambiguous element may be in the sum or not, so its
                  |g| (|g xhat|) is added to the slab's allowance — the same either-side rule as in bn_bwd_apply,
                  which the issue states for the apply pass only.
  finalize        judged by tools/kbench fincheck, except what a wrong slab WEIGHT would move and fincheck (same slab
                  on both sides) cannot see: mean within sum_b bound(S1_b) / M + 2 e |mean|, and dbeta / dgamma within
                  the sum of their slabs' bounds + 2 e |value| (mean_usage, param_grad_usage).
  avgpool_fwd     |y - y64| <= (HW + 1) e sum |x| / HW + u |y64|       avgpool_bwd  |dx - dy / HW| <= (2 e + u) |dy| / HW
  maxpool_fwd     y and the index bytes exact: the first maximum in row-major window order
  maxpool_bwd     |dx - dx64| <= 3 e sum |dy terms| + u |dx64|  (an input is the maximum of up to four windows)
  bn_relu_maxpool fwd: y within the bn_apply bound at the position the index byte names, and that position must be
                  able to win: see stem_fwd_violations.  bwd: g = T(sum of dy over the windows that chose the pixel,
                  added in fp32 in ascending (p, q) as maxpool_bwd does), masked by source 2; then the bn_bwd_reduce
                  and bn_bwd_apply bounds with that g, a slab being the pixels of one workgroup.

Two corrections to the bounds as first written, both shown by the float32 evaluation of the host test.

u: bf16 keeps 8 significant bits, so round-to-nearest errs by up to 2^-8 of the value (1 + 2^-8 lies half-way between
the neighbours 1 and 1 + 2^-7), not 2^-9: a correctly rounded store of a correct fp32 result used up to 1.17 of the
bound written with 2^-9 (case 1x8-plain-bf16).  tests/attention_util.py uses the same 2^-8.

bn_relu_maxpool_fwd ("the named position's pre64 is within B_apply of
the window maximum of pre64"): that is right for fp32 storage only.  The kernel compares z ROUNDED TO THE STORAGE
TYPE (the z the separate bn_apply pass stores), so with bf16 two positions whose pre differ by less than a bf16 ulp
tie, and the first wins although its pre64 is u |pre| below the maximum.  The criterion used here is the one that
follows from rounding being monotone: with lo = T(relu(pre64 - B_apply)), hi = T(relu(pre64 + B_apply)), every value
the kernel can have compared lies in [lo, hi], so the winner k needs hi_k >= lo_j for every valid j of the window.
For fp32 storage this is the original statement (within B_apply of the maximum, from both sides); where a zero wins
it says that every other position is clamped too.  A float32 evaluation meets it; `zero padding` does not matter
here (ReLU clamps at the pad value), which is why the negative kind has teeth in maxpool3x3s2 only.
"""
import functools

import torch
import torch.nn.functional as F

from passl_amd.hip.ops import _bn_blocks

E = 2.0 ** -24
EPS = 1e-5
AMBIGUOUS_CAP = 1e-3
DTYPES = (torch.float32, torch.bfloat16)
DTNAME = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}
INF = float('inf')


def unit(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 0.0


def rnd(t, dtype):
    """round-trip through the compute dtype so the reference sees the kernel's inputs"""
    return t.to(dtype).float()


# ------------------------------------------------------------------------------------------------ cases
# (M, C, nblocks or None = ops._bn_blocks as ops.bn_train_fwd uses it)
BN_SHAPES = (
    (1, 8, None),         # one row, one 16-byte chunk; variance exactly 0
    (129, 64, None),      # 1032 chunks: for U = 2 / 4 / 8 the last workgroup holds 8 chunks of 512 / 1024 / 2048
    (515, 64, None),      # two reduce slabs of unequal height (258 + 257)
    (300, 256, None),     # 32 chunk columns, 8 row lanes
    (33, 2048, None),     # 256 chunk columns, one row lane, three slabs
    (37, 24, None),       # 3 chunk columns: grid-stride form, 255 of 256 threads active in the reduction
    (5, 4096, None),      # 512 chunk columns: column loop of the reduction, grid-stride apply
    (5, 8, 4),            # rows = 2: the fourth slab holds no row, the finalize must skip it
)
BN_KINDS = ('plain', 'mixed', 'const', 'ties')
BN_CASES = tuple((s, k, d) for s in BN_SHAPES for k in BN_KINDS for d in DTYPES)

MAXPOOL_SHAPES = ((1, 1, 1, 8), (2, 2, 3, 8), (1, 5, 5, 8), (3, 7, 9, 64), (2, 8, 8, 256))
AVGPOOL_SHAPES = ((1, 1, 8), (3, 7, 24), (2, 49, 2048))
STEM_SHAPES = ((2, 9, 8, 256), (3, 17, 21, 64), (1, 7, 9, 8), (4, 32, 32, 64))
POOL_KINDS = ('plain', 'negative', 'ties')
MAXPOOL_CASES = tuple((s, k, d) for s in MAXPOOL_SHAPES for k in POOL_KINDS for d in DTYPES)
AVGPOOL_CASES = tuple((s, k, d) for s in AVGPOOL_SHAPES for k in POOL_KINDS for d in DTYPES)
STEM_CASES = tuple((s, k, d) for s in STEM_SHAPES for k in POOL_KINDS for d in DTYPES)


def case_id(case):
    shape, kind, dtype = case
    if shape in BN_SHAPES:
        name = '%dx%d' % shape[:2] + ('n%d' % shape[2] if shape[2] else '')
    else:
        name = 'x'.join(str(v) for v in shape)
    return '%s-%s-%s' % (name, kind, DTNAME[dtype])


def tile_form(C):
    """bn_apply / bn_bwd_apply take the tile kernels (option bn_stream_unroll) for this C."""
    return 256 % (C // 8) == 0


def bn_slabs(M, C, nblocks=None):
    """(slab count, rows per slab) of a reduce launch."""
    if nblocks is None:
        nb = _bn_blocks(M, C)
        rows = -(-M // nb)
        return -(-M // rows), rows               # every slab holds rows
    return nblocks, -(-M // nblocks)


def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


def _values(kind, shape, gen):
    if kind == 'ties':
        return torch.randint(-8, 9, shape, generator=gen).float() * 0.25
    return torch.randn(shape, generator=gen) * 2 + 0.5


@functools.lru_cache(maxsize=None)
def bn_data(case):
    """x, dz, res, zsrc [M, C] (fp32 tensors holding values of the compute dtype), gamma, beta [C] and the bit mask of
    zsrc > 0.  zsrc / maskbits are the mask INPUTS of the backward kernels (sources 1 and 3)."""
    (M, C, nblocks), kind, dtype = case
    gen = torch.Generator().manual_seed(_seed(M, C, nblocks or 0, BN_KINDS.index(kind)))
    c = torch.arange(C)
    x = _values(kind, (M, C), gen)
    if kind == 'mixed':
        off = torch.tensor([0.0, 3.0, 200.0])[c % 3] * (1 - 2 * (c % 2)).float()
        x = torch.randn(M, C, generator=gen) * torch.tensor([1e-2, 1.0, 1e2])[(c // 3) % 3] + off
    elif kind == 'const':
        x[:, ::3] = x[0, ::3]
    dz = _values(kind, (M, C), gen) if kind == 'ties' else torch.randn(M, C, generator=gen)
    res = _values(kind, (M, C), gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[1], gamma[2] = 0.0, -1.0
    beta = torch.randn(C, generator=gen)
    if kind == 'mixed':
        # A channel at offset +-200 is constant next to its offset (in bf16 exactly: the spacing at 200 is 1), so its
        # pre = beta + rounding noise of size B_apply ~ 0.03: with |beta| below that, every element of the channel is
        # at the recomputed-mask boundary, 0.12 - 0.24 % of the elements of the wide bf16 cases, above AMBIGUOUS_CAP.
        # The case changes, not the cap: beta of these channels keeps its sign and moves 0.5 away from 0.
        far = c % 3 == 2
        beta[far] = beta[far] + torch.where(beta[far] < 0, -0.5, 0.5)
    x, dz, res = rnd(x, dtype), rnd(dz, dtype), rnd(res, dtype)
    zsrc = rnd(torch.relu(x - x.mean(0, keepdim=True)), dtype)
    return dict(x=x, dz=dz, res=res, zsrc=zsrc, gamma=gamma, beta=beta, maskbits=pack_mask(zsrc > 0))


@functools.lru_cache(maxsize=None)
def pool_data(case):
    """x [N, H, W, C] (avgpool: [N, HW, C]) and dy of the pooled shape, values of the compute dtype."""
    shape, kind, dtype = case
    gen = torch.Generator().manual_seed(_seed(*shape, POOL_KINDS.index(kind), 3))
    x = _values(kind, shape, gen)
    if kind == 'negative':
        x = -x.abs() - 0.125
    if len(shape) == 3:
        oshape = (shape[0], shape[2])
    else:
        P, Q = pool_dims(shape[1], shape[2])
        oshape = (shape[0], P, Q, shape[3])
    dy = _values('ties' if kind == 'ties' else 'plain', oshape, gen)
    return dict(x=rnd(x, dtype), dy=rnd(dy, dtype))


@functools.lru_cache(maxsize=None)
def stem_params(C):
    gen = torch.Generator().manual_seed(_seed(C, 11))
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[1], gamma[2] = 0.0, -1.0
    return gamma, torch.randn(C, generator=gen)


def pack_mask(bits):
    """bool [..] (a multiple of 8 elements) -> uint8 [numel / 8]: bit e of byte i <-> element 8 i + e."""
    b = bits.reshape(-1, 8).to(torch.int32)
    return (b * (1 << torch.arange(8, dtype=torch.int32))).sum(1).to(torch.uint8)


def unpack_mask(mask, shape):
    return ((mask.to(torch.int32).unsqueeze(1) >> torch.arange(8, dtype=torch.int32)) & 1).bool().reshape(shape)


# ------------------------------------------------------------------------------------------------ criteria
def _ratios(got, ref, bound):
    """|got - ref| / bound per element (flat).  A bound of 0 admits no error; NaN counts as inf."""
    err, bound = (got.double().flatten() - ref.flatten()).abs(), bound.flatten()
    r = err / bound.clamp_min(1e-300)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    return torch.where(torch.isnan(err) | ((bound == 0) & (err > 0)), torch.full_like(r, INF), r)


def usage(got, ref, bound):
    """(worst |got - ref| / bound, flat index of that element)."""
    ratio = _ratios(got, ref, bound)
    idx = int(ratio.argmax())
    return float(ratio[idx]), idx


def usage_either(got, ref_a, bound_a, ref_b, bound_b, either):
    """usage() where elements marked `either` may meet (ref_b, bound_b) instead of (ref_a, bound_a)."""
    ra, rb = _ratios(got, ref_a, bound_a), _ratios(got, ref_b, bound_b)
    ratio = torch.where(either.flatten(), torch.minimum(ra, rb), ra)
    idx = int(ratio.argmax())
    return float(ratio[idx]), idx


def verdict(what, tensor, ratio, idx):
    """None if the bound holds, else the message the tests raise."""
    if ratio <= 1:
        return None
    return '%s: %s exceeds its bound at flat index %d: error = %.4g x bound' % (what, tensor, idx, ratio)


def host_constants(x, gamma, beta, eps=EPS):
    """mean, invstd, scale, shift as bn_finalize forms them (fp64 statistics, results rounded to fp32), fp32 [C]."""
    xd = x.double()
    mu = xd.mean(0)
    var = ((xd - mu) ** 2).mean(0)
    mean = mu.float()
    invstd = (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    return mean, invstd, scale, shift


def host_coef(g, x, gamma, mean, invstd):
    """coef [3, C] (A, B, Cc) as bn_bwd_finalize forms them from float64 sums of the masked gradient g."""
    M = x.shape[0]
    gd, isd, mu = g.double(), invstd.double(), mean.double()
    sg = gd.sum(0)
    sgx = (gd * (x.double() - mu) * isd).sum(0)
    gi = gamma.double() * isd
    Bc = -gi * isd * sgx / M
    Cc = -gi * sg / M - Bc * mu
    return torch.stack([gi, Bc, Cc]).float()


def apply_ref(x, scale, shift, res=None, relu=False):
    """pre64, z64, B_apply of z = relu?(x scale + shift (+ res)); scale / shift fp32 [C]."""
    xs = x.double() * scale.double()
    b = shift.double().expand_as(xs)
    pre = xs + b
    mag = xs.abs() + b.abs()
    if res is not None:
        pre = pre + res.double()
        mag = mag + res.double().abs()
    return pre, (pre.clamp_min(0) if relu else pre), 4 * E * mag


def apply_usage(z_got, x, scale, shift, res, relu, dtype):
    _, z, B = apply_ref(x, scale, shift, res, relu)
    return usage(z_got, z, B + unit(dtype) * z.abs())


def mask_mismatch(mask_got, z_got):
    """(number of mask bytes that differ from pack(z_got > 0), first such byte or -1)."""
    bad = (mask_got != pack_mask(z_got > 0)).nonzero()
    return len(bad), int(bad[0]) if len(bad) else -1


def recomputed_mask(x, scale, shift):
    """Mask source 2: (pre64 > 0, ambiguous) with ambiguous = |pre64| <= B_apply."""
    pre, _, B = apply_ref(x, scale, shift)
    return pre > 0, pre.abs() <= B


def bwd_apply_ref(g, x, coef):
    """dx64 and the fp32 part of its bound; g the masked gradient, coef fp32 [3, C]."""
    a, b, c = coef.double()
    ag, bx = a * g.double(), b * x.double()
    return ag + bx + c, 4 * E * (ag.abs() + bx.abs() + c.abs())


def bwd_apply_usage(dx_got, dz, x, coef, mask, dtype, ambiguous=None):
    u = unit(dtype)
    g = torch.where(mask, dz, torch.zeros_like(dz)) if mask is not None else dz
    dx, B = bwd_apply_ref(g, x, coef)
    if ambiguous is None or not ambiguous.any():
        return usage(dx_got, dx, B + u * dx.abs())
    g2 = torch.where(mask, torch.zeros_like(dz), dz)            # the other side, used where ambiguous only
    dx2, B2 = bwd_apply_ref(g2, x, coef)
    return usage_either(dx_got, dx, B + u * dx.abs(), dx2, B2 + u * dx2.abs(), ambiguous)


def dres_mismatch(dres_got, dz, mask, ambiguous=None):
    """Elements of dres that are neither the masked dz (nor, where ambiguous, its other side), by value and sign."""
    g = torch.where(mask, dz, torch.zeros_like(dz)) if mask is not None else dz
    ok = dres_got.view(torch.int32) == g.view(torch.int32)
    if ambiguous is not None:
        g2 = torch.where(mask, torch.zeros_like(dz), dz)
        ok = ok | (ambiguous & (dres_got.view(torch.int32) == g2.view(torch.int32)))
    bad = (~ok).flatten().nonzero()
    return len(bad), int(bad[0]) if len(bad) else -1


def slab_rows(M, nb, rows):
    return [(min(b * rows, M), min((b + 1) * rows, M)) for b in range(nb)]


def stats_ref(x, nb, rows):
    """shift [nb, C] (fp32), sums [nb, C, 2] (float64) and their bounds, per slab of bn_stats."""
    M, C = x.shape
    shift = torch.zeros(nb, C)
    sums, bound = torch.zeros(nb, C, 2, dtype=torch.float64), torch.zeros(nb, C, 2, dtype=torch.float64)
    for b, (r0, r1) in enumerate(slab_rows(M, nb, rows)):
        if r1 <= r0:
            continue
        n = r1 - r0
        shift[b] = x[r0]
        d = x[r0:r1].double() - x[r0].double()
        sums[b, :, 0], sums[b, :, 1] = d.sum(0), (d * d).sum(0)
        bound[b, :, 0], bound[b, :, 1] = (n + 1) * E * d.abs().sum(0), (n + 3) * E * (d * d).sum(0)
    return shift, sums, bound


def split_stats_slab(partial, nb, C):
    """The slab bn_stats wrote: sums [nb, C, 2] followed by shifts [nb, C]."""
    return partial[:nb * C * 2].view(nb, C, 2), partial[nb * C * 2:nb * C * 3].view(nb, C)


def combine_mean(shift, sums, M, rows, skip_empty=True):
    """The mean bn_finalize forms from a slab: every slab re-centred on slab 0's shift in float64, rounded to fp32.
    skip_empty=False plants the defect the empty fourth slab of case 5x8n4 is there for."""
    g0 = shift[0].double()
    t1 = torch.zeros_like(g0)
    for b in range(shift.shape[0]):
        n = min(M - b * rows, rows)
        if n <= 0 and skip_empty:
            continue
        t1 += sums[b, :, 0].double() + n * (shift[b].double() - g0)
    return (g0 + t1 / M).float()


def mean_usage(mean_got, x, stats_bound):
    """The one constant judged here (tools/kbench fincheck judges the finalize kernels' arithmetic on a given slab):
    the mean, because a slab that is wrongly weighted or an empty slab that is not skipped moves it.  The combine is
    float64, so |mean - mean64| <= sum_b bound(S1_b) / M from the slab sums + e |mean64| from the fp32 result; 2 e."""
    mean = x.double().mean(0)
    return usage(mean_got, mean, stats_bound[:, :, 0].sum(0) / x.shape[0] + 2 * E * mean.abs())


def param_grad_usage(dbeta, dgamma, sums_ref, bound):
    """dbeta = fp32(sum_b slab sums of g), dgamma = fp32(sum_b slab sums of g xhat), accumulated into zeros: the
    float64 combine adds nothing to the slabs' own bounds but the e |value| of the result; 2 e."""
    ref = sums_ref.sum(0)
    return usage(torch.stack([dbeta, dgamma], 1), ref, bound.sum(0) + 2 * E * ref.abs())


def reduce_ref(g, x, mean, invstd, groups, ambiguous=None, gother=None):
    """(sum g, sum g xhat) [len(groups), C, 2] in float64 and the bounds.  groups: one (row index tensor or slice) per
    slab over the rows of g / x [rows, C].  Where `ambiguous`, the element may enter with gother instead of g."""
    C = x.shape[1]
    gx = g.double() * (x.double() - mean.double()) * invstd.double()
    sums = torch.zeros(len(groups), C, 2, dtype=torch.float64)
    bound = torch.zeros(len(groups), C, 2, dtype=torch.float64)
    if ambiguous is not None:
        dg = torch.where(ambiguous, (gother.double() - g.double()).abs(), torch.zeros_like(gx))
        dgx = dg * ((x.double() - mean.double()) * invstd.double()).abs()
    for b, rows in enumerate(groups):
        gb, gxb = g[rows].double(), gx[rows]
        n = gb.shape[0]
        if n == 0:
            continue
        sums[b, :, 0], sums[b, :, 1] = gb.sum(0), gxb.sum(0)
        bound[b, :, 0], bound[b, :, 1] = (n + 1) * E * gb.abs().sum(0), (n + 4) * E * gxb.abs().sum(0)
        if ambiguous is not None:
            bound[b, :, 0] += dg[rows].sum(0)
            bound[b, :, 1] += dgx[rows].sum(0)
    return sums, bound


def row_groups(M, nb, rows):
    return [slice(r0, r1) for r0, r1 in slab_rows(M, nb, rows)]


# ------------------------------------------------------------------------------------------------ pooling
def pool_dims(H, W):
    return (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1


def windows(v, pad):
    """v [N, H, W, C] -> [N, P, Q, 9, C]: tap r * 3 + s of window (p, q) is v[2 p - 1 + r, 2 q - 1 + s], else pad."""
    N, H, W, C = v.shape
    P, Q = pool_dims(H, W)
    vp = F.pad(v.permute(0, 3, 1, 2), (1, 1, 1, 1), value=pad).permute(0, 2, 3, 1)
    return torch.stack([vp[:, r:r + 2 * P - 1:2, s:s + 2 * Q - 1:2] for r in range(3) for s in range(3)], dim=3)


def argmax_tap(win, last=False):
    """The first (last) maximum of every window, by a score that has no ties."""
    eq = win == win.max(3, keepdim=True).values
    rank = (1 + torch.arange(9)) if last else (9 - torch.arange(9))
    return (eq * rank.view(1, 1, 1, 9, 1)).argmax(3)


def maxpool_ref(x, pad=-INF, last=False):
    """y (the values of x, exact) and idx uint8 [N, P, Q, C]."""
    win = windows(x.double(), pad)
    idx = argmax_tap(win, last)
    return win.gather(3, idx.unsqueeze(3)).squeeze(3).float(), idx.to(torch.uint8)


def maxpool_bwd_ref(dy, idx, H, W):
    """dx64 [N, H, W, C], the sum of |dy| terms per input, and the fp32 sum in the kernels' order: the windows that
    chose a pixel in ascending (p, q), i.e. taps in descending (r, s)."""
    N, P, Q, C = dy.shape
    acc = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    acc32 = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float32)
    for r in (2, 1, 0):
        for s in (2, 1, 0):
            t = torch.where(idx == r * 3 + s, dy, torch.zeros_like(dy))
            sl = (slice(None), slice(r, r + 2 * P - 1, 2), slice(s, s + 2 * Q - 1, 2))
            acc[sl] += t.double()
            mag[sl] += t.double().abs()
            acc32[sl] += t
    crop = (slice(None), slice(1, H + 1), slice(1, W + 1))
    return acc[crop], mag[crop], acc32[crop]


def maxpool_bwd_usage(dx_got, dy, idx, H, W, dtype):
    dx, mag, _ = maxpool_bwd_ref(dy, idx, H, W)
    return usage(dx_got, dx, 3 * E * mag + unit(dtype) * dx.abs())


def avgpool_fwd_usage(y_got, x, dtype):
    HW = x.shape[1]
    y = x.double().sum(1) / HW
    return usage(y_got, y, (HW + 1) * E * x.double().abs().sum(1) / HW + unit(dtype) * y.abs())


def avgpool_bwd_usage(dx_got, dy, HW, dtype):
    dx = (dy.double() / HW).unsqueeze(1).expand(-1, HW, -1)
    return usage(dx_got, dx, (2 * E + unit(dtype)) * dx.abs())


def stem_fwd_violations(what, y_got, idx_got, x, scale, shift, dtype):
    """Messages for bn_relu_maxpool_fwd (the module docstring has the criterion); [] if it holds.  Also returns the
    worst usage of the y bound."""
    pre, z, B = apply_ref(x, scale, shift, None, True)
    rt = (lambda t: t.float().to(dtype).double())
    whi, wlo = windows(rt((pre + B).clamp_min(0)), -INF), windows(rt((pre - B).clamp_min(0)), -INF)
    wz, wB = windows(z, 0.0), windows(B, 0.0)
    msgs = []
    k = idx_got.long().clamp_max(8).unsqueeze(3)
    hi_k = whi.gather(3, k).squeeze(3)
    bad = (idx_got > 8) | (hi_k == -INF)
    if bad.any():
        msgs.append('%s: idx names a tap outside the input at flat index %d (%d elements)' % (
            what, int(bad.flatten().nonzero()[0]), int(bad.sum())))
    lose = (hi_k < wlo.max(3).values) & ~bad
    if lose.any():
        msgs.append('%s: idx names a position that cannot hold the maximum at flat index %d (%d elements)' % (
            what, int(lose.flatten().nonzero()[0]), int(lose.sum())))
    z_k, B_k = wz.gather(3, k).squeeze(3), wB.gather(3, k).squeeze(3)
    ratio, at = usage(y_got, z_k, B_k + unit(dtype) * z_k.abs())
    msgs += [m for m in [verdict(what, 'y', ratio, at)] if m]
    return msgs, ratio


def stem_layout(N, H, W, C, form, wgs=1024):
    """(workgroups, 2 x 2 pixel blocks per workgroup) of bn_relu_maxpool_bwd_reduce: form 0 = 2048 items per
    workgroup, form 1 = ceil(chunks / wgs) chunks of 256 items (item = a 2 x 2 pixel block x 8 channels)."""
    cc = C // 8
    items = N * ((H + 1) // 2) * ((W + 1) // 2) * cc
    if form == 0:
        ipb = 2048
        nb = -(-items // ipb)
    else:
        chunks = -(-items // 256)
        per = -(-chunks // wgs)
        ipb, nb = per * 256, -(-chunks // per)
    return nb, ipb // cc


def stem_groups(N, H, W, nb, blocks_per_wg):
    """Row indices (into [N * H * W]) of the pixels each workgroup of the fused reduce pass owns."""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    n, p2, q2, dh, dw = torch.meshgrid(torch.arange(N), torch.arange(H2), torch.arange(W2), torch.arange(2),
                                       torch.arange(2), indexing='ij')
    h, w = 2 * p2 + dh, 2 * q2 + dw
    wg = ((n * H2 + p2) * W2 + q2) // blocks_per_wg
    ok = (h < H) & (w < W)
    row = (n * H + h) * W + w
    return [row[ok & (wg == b)] for b in range(nb)]


def stem_grad(dy, idx, x, scale, shift, dtype):
    """g of the fused backward and its other side: dz = T(fp32 sum of dy over the windows that chose the pixel),
    masked by x scale + shift > 0.  Returns g, gother, ambiguous, all [N * H * W, C]."""
    N, H, W, C = x.shape
    _, _, acc32 = maxpool_bwd_ref(dy, idx, H, W)
    dz = rnd(acc32, dtype)
    mask, amb = recomputed_mask(x, scale, shift)
    zero = torch.zeros_like(dz)
    return (torch.where(mask, dz, zero).reshape(-1, C), torch.where(mask, zero, dz).reshape(-1, C),
            amb.reshape(-1, C))
