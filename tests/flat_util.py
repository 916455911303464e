"""CPU helpers of the optimizer / flat-arena numerics tests (numpy + torch on the CPU: the native library is never loaded).

Case tables, seeded inputs, float64 references, element-wise bounds, a float32 evaluation ("twin") of every formula and
planted defects for the kernels of csrc/flat.hip (key-encoder EMA, momentum SGD, fp32 -> bf16 cast, LARS, LARC, the
fixed-order slab reduction, the BatchNorm fold, weight packing) and the flat AdamW walk of csrc/vit.hip.
test_flat_numerics_host.py shows that every twin uses at most HEADROOM = 0.5 of every bound and that each planted
defect breaks one (or, for the bit-exact kernels, a bit); test_flat_numerics_gpu.py judges the kernels by the same
bounds.  Adan and grad_sumsq / grad_clip_finalize have tests of this kind already (adan_util.py, grad_clip_util.py).

Every family has  X_data(case) -> the fp32 operands and scalars,  X_ref(case) -> {tensor: (float64 reference, bound)}
and  X_eval32(case, defect=None) -> {tensor: fp32 value}.  A reference restates the rule of the header comment of
include/passl_hip.h, end to end in float64, from the operands as the kernel receives them: every scalar is rounded to
float32 first (that is what crosses the ABI), so the EMA reference uses 1 - float32(0.999), not 0.001.  A comparison
is per element: usage = |got - ref64| / bound of that element.  A bound of 0 admits no error: an element the kernel
does not own (padding, the arena outside the listed blocks) has its initial value as reference and the bound 0.

Constants.  e = 2^-24 (one fp32 rounding, relative).  TINY = 2^-126: a product below the smallest normal fp32 may be
flushed or rounded as a denormal, an absolute error of at most TINY each.  F_RSQRT = 4 is the accuracy, in units of e
relative to the result, assumed for the hardware reciprocal square root behind rsqrtf (v_rsq_f32): the ONLY unmeasured
constant here, twice the 1 ulp = 2 e usually quoted and not tuned to any output (the GPU test's docstring records what
one run showed).  sqrtf and the division are correctly rounded (the build has no fast-math flag).

The rule for a bound:  R e M + (products) TINY.  R is the number of fp32 roundings on the element's path (those of
scalars the kernel derives in fp32 included, a squared factor counting twice).  M is the sum of the magnitudes of the
intermediate values of that path, every product, every partial sum and the result, each times the factors it is
still to be multiplied by (so that a learning rate above 1 scales the allowance of what it multiplies).  Every single
rounding errs by at most e times one of these magnitudes, so the true error is at most e M times the largest number
of roundings one term passes through; that number is at most R / 2 in every formula below but the two marked (*),
where a scalar's roundings pile on one term and a worst case of 0.6 R is possible in principle; the host test shows
what the twin reaches on the inputs used.  The compiler may contract a product and a sum into one FMA: that removes a
rounding and never adds one, so the same bound covers the kernel and the unfused twin.

  ema       om = 1 - m; k' = k m + q om.  R = 4 (om, two products, the sum), M = |k m| + |q om| + |k'|.  The bf16 copy
            is exact: round-to-nearest-even of the kernel's own fp32 k'.
  sgd       a = g gs, b = wd p, c = a + b, d = mu v, v' = d + c, f = lr v', p' = p - f.
            v': R = 5, M = |a| + |b| + |c| + |d| + |v'|.   p': R = 7, M = lr (|a| + |b| + |c| + |d|) + 2 |f| + |p'|
            (|f| stands for lr |v'| and for f itself).  momentum_sgd and momentum_sgd_dev give the same bits.
  adamw     derived in fp32 by the kernel, in float64 (from the float32 inputs) by the reference:
              c2 = sqrt(1 - b2p)          relative 2 e   (the subtraction, halved by the root, and the root: 1.5 e)
              decay = 1 - lr wd           absolute e (|lr wd| + |decay|)
              lr_t = lr c2 / (1 - b1p)    relative 5 e   (c2, the product, the subtraction, the division: 4.5 e)
              eps_t = eps c2              relative 3 e
            gg = g gs.  m' = b1 m + (1 - b1) gg: R = 5 (1 - b1, gg, two products, the sum) (*), M = |b1 m| +
            |(1 - b1) gg| + |m'|, + 2 TINY.  v' = b2 v + ((1 - b2) gg) gg: R = 7 (1 - b2, gg twice, three products,
            the sum) (*), M = |b2 v| + |(1 - b2) gg^2| + |v'|, + 3 TINY (gg^2 underflows for |g| ~ 1e-22: kind tiny_grad).
            p' = p decay - lr_t (m' / (sqrt(v') + eps_t)) is not linear in m', v': their bounds are propagated,
              sq = sqrt(v'):  B_sq = min(B_v / sq, sqrt(B_v)) + e sq
                             (|sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|)
              den = sq + eps_t:  B_den = B_sq + 3 e eps_t + e den
              r = m' / den:  B_r = (B_m + |r| B_den) / (den - B_den) + e |r|
              s = lr_t r:  B_s = lr_t B_r + 6 e |s|;    pd = p decay:  B_pd = |p| e (|lr wd| + |decay|) + e |pd|
              B_p = 2 (B_s + B_pd + e |p'|) + TINY     (twice the worst case: the twin is to stay within half).
            adamw and adamw_dev give the same bits.
  lars      per segment S_p = sum p^2, S_g = sum (g gs)^2 (norms[s][0 / 1]): every term is >= 0, so the relative
            error of the sum is at most depth e, depth = the longest chain of roundings one term passes through, read
            off lars_norm_kernel and lars_seg_reduce_kernel:
              1                     the square
              4 trips x 4           a lane's trips over a 4096-element chunk (256 lanes x float4): three additions
                                    inside the float4 and one onto the accumulator, each trip
              + 2 (S_g only)        the float4's sum times gs, times gs (the scalar tail: g g gs gs, no more)
              6 + 3                 block_sum: six shuffle steps, the four wave sums added in order
              ceil(blocks / 256)    a lane's trips in the segment reduce (two for the 258-block segment)
              6 + 3                 its block_sum
            depth_p = 35 + ceil(blocks / 256), depth_g = depth_p + 2; a block's partial sum: 26 and 28.  Not
            (N - 1) e: at a million elements that allows 6 % and proves nothing.  An all-zero operand gives S = 0
            exactly (bound 0): the branch conditions |p| > 0, |g| > 0 are tested with exact zeros only; a norm whose
            squares underflow in fp32 is out of scope.
            Propagation.  pn = sqrt(S_p): relative dpn = depth_p e / 2 + e, dgn likewise.  local_lr = ((lr coeff) pn) /
            ((gn + wd pn) + eps), all terms positive: relative dl = dpn + max(dgn, dpn + e) + 5 e (two products, two
            additions, the division); dl = 0 on the plain-lr branch.  Every element of the segment:
            a = g gs, b = wd p, c = a + b, d = llr c, f = mu v, v' = f + d, p' = p - v':
            v': R = 6, M = llr (|a| + |b|) + 2 |d| + |f| + |v'|, + dl |d|.   p': R = 7, M + |p'|, + dl |d|.
            lars_momentum and lars_momentum_dev give the same bits.
  larc      the same norms.  x = (trust pn) / ((gn + pn wd) + eps): relative dpn + max(dgn, dpn + e) + 4 e; clip:
            A = min(x / lr, 1), one more e, and no error at all once x / lr exceeds 1 by more than its allowance;
            A = 1, wd = 0 exactly on the zero-norm branch.  a = g gs, b = wd p, c = a + b, d = A c, f = mu v,
            v' = f + d, h = lr v', p' = p - h:  v': R = 6, M = A (|a| + |b|) + 2 |d| + |f| + |v'|, + dA |d|.
            p': R = 8, lr M + |h| + |p'|, + lr dA |d|.
  slab_reduce  exact against a twin that adds in the documented order (lane zl takes slabs zl, zl + ZL, ... ascending,
            from +0; the lanes are combined in lane order; the previous `out` comes last when accumulating; ZL = 1, 4,
            16 for slabs <= 4, <= 32, more).  Also slabs e sum |terms| against float64: the chain of roundings one term passes
            through, ceil(slabs / ZL) - 1 + ZL - 1 + accumulate, is never longer than `slabs` and exactly that up to 4
            slabs, so this twin alone may use its whole bound.
  bn_fold   scale = gamma rsqrt(var + eps): R = 2 + F_RSQRT, M = |scale|.  shift = beta - mean scale: R = 4 + F_RSQRT,
            M = |mean scale| + |shift|.
  cast, pack   exact: torch's own fp32 -> bf16 conversion on the CPU; emu_pack (tests/emu.py), and its bf16 rounding.

Which case catches which planted defect (test_planted_defect in the host test):
  the tail is skipped                       ema 7-plain (k), sgd 7-plain (p), adamw 7-plain (p), cast 9 (bits)
  wd multiplies g instead of p              sgd 1025-plain (v)
  velocity not scaled by mu                 sgd 1025-warm (v)
  grad_scale once in the gradient norm      lars b (norms)
  a segment takes its predecessor's norm    lars a (v)
  last block of a segment dropped           lars a (norms)
  segment reduce stops after 256 blocks     lars a (norms)
  LARC clip uses a instead of a / lr        larc a clip 1 (v)
  LARC weight decay on the zero-norm branch larc a clip 0 (v)
  b1p and b2p swapped                       adamw 1025-plain (p)
  eps instead of eps sqrt(1 - b2p)          adamw 1025-tiny_grad (p)
  decay after the step                      adamw 4099-mixed (p)
  EMA 1 - m with m rounded to bf16          ema 1025-plain (k)
  slab_reduce ignores accumulate            slab 64x5-plain accumulate (bits and bound)
  slab_reduce adds lanes in reverse order   slab 64x33-cancelling (bit equality only: the float64 bound holds for any order)
  bf16 truncated instead of rounded         cast patterns (bits), ema 1025-plain (k_lp bits)
  pack zero-fills one short of c_pad        pack job stem (bits)
  mode-2 tile transposed twice              pack job t33x65 (bits)
"""
import functools
import math
import zlib

import numpy as np
import torch

E = 2.0 ** -24
TINY = 2.0 ** -126
F_RSQRT = 4.0         # unmeasured: accuracy of the hardware reciprocal square root behind rsqrtf, in e relative to the result
HEADROOM = 0.5        # the float32 evaluation may use this share of a bound (as loss_util.HEADROOM)
F32 = np.float32


def f32(v):
    return float(F32(v))


def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def _ratios(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64).ravel() - ref.ravel())
    bound = np.broadcast_to(bound, ref.shape).ravel()
    with np.errstate(divide='ignore', invalid='ignore'):
        r = err / np.maximum(bound, 1e-300)
    r = np.where((err == 0) & (bound == 0), 0.0, r)
    return np.where(np.isnan(err) | ((bound == 0) & (err > 0)), np.inf, r)


def usage(got, ref, bound):
    """(worst |got - ref| / bound, flat index of that element).  A bound of 0 admits no error; NaN counts as inf."""
    ratio = _ratios(got, ref, bound)
    idx = int(ratio.argmax())
    return float(ratio[idx]), idx


def verdict(what, tensor, ratio, idx):
    if ratio <= 1:
        return None
    return '%s: %s exceeds its bound at flat index %d: error = %.4g x bound' % (what, tensor, idx, ratio)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def bf16_bits(x, truncate=False):
    """The bf16 bit patterns (uint16) of fp32 values: torch's CPU conversion (round to nearest even), or truncation."""
    x = np.ascontiguousarray(x, dtype=F32)
    if truncate:
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def bf16_value(b):
    return (b.astype(np.uint32) << 16).view(F32)


def rb(R, *terms):
    """R e M."""
    return R * E * sum(np.abs(t) for t in terms)


# ------------------------------------------------------------------------------------------------ streaming kernels
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4099)
# grid_for (flat.hip) and adamw_grid (vit.hip) cap the grid at 2048 blocks of 256 lanes, one float4 per lane and trip:
# 2^21 elements per trip.  One float4 more makes lane 0 of block 0 take a second trip; + 3 is the tail.
BIG = 2 ** 21 + 4 + 3
# the cast takes 8 elements per lane and trip: 2^22 per trip
BIG_CAST = 2 ** 22 + 8 + 5
KIND_SIZES = (7, 1025, 4099)
SGD_KINDS = ('mixed', 'warm', 'tiny_grad', 'zero_grad', 'gs3', 'gs16', 'wd0', 'mu0')
ADAMW_KINDS = ('mixed', 'warm', 'tiny_grad', 'zero_grad', 'gs3', 'gs16', 'wd0')
PLAIN_CASES = [(n, 'plain') for n in SIZES + (BIG,)]
EMA_CASES = PLAIN_CASES + [(n, 'mixed') for n in KIND_SIZES]
SGD_CASES = PLAIN_CASES + [(n, k) for k in SGD_KINDS for n in KIND_SIZES]
ADAMW_CASES = PLAIN_CASES + [(n, k) for k in ADAMW_KINDS for n in KIND_SIZES]
CAST_SIZES = SIZES + (BIG_CAST,)


def case_id(case):
    return '-'.join('%g' % c if isinstance(c, float) else str(c) for c in case)


def _mags(rng, n):
    """Magnitudes from 1e-12 to 1e6 within one buffer, random signs."""
    return (10.0 ** rng.uniform(-12, 6, n) * rng.choice([-1.0, 1.0], n)).astype(F32)


def _grad_scale(kind):
    return {'gs3': f32(1.0 / 3.0), 'mixed': f32(1.0 / 3.0), 'gs16': 2.0 ** -16}.get(kind, 1.0)


def _tail_keep(new, old, n, width=4):
    """Planted defect: the elements past the last whole vector keep their old value."""
    out = new.copy()
    out[n - n % width:] = old[n - n % width:]
    return out


# ---- EMA
EMA_M = f32(0.999)


@functools.lru_cache(maxsize=4)
def ema_data(case):
    n, kind = case
    rng = _rng('ema', n, kind)
    if kind == 'mixed':
        k, q = _mags(rng, n), _mags(rng, n)
        c = np.arange(n) % 3 == 0                                   # k m + q (1 - m) nearly cancels
        q[c] = (-k[c].astype(np.float64) * EMA_M / (1.0 - EMA_M) * (1 + 2.0 ** -10 * rng.standard_normal(int(c.sum())))
                ).astype(F32)
    else:
        k, q = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    return dict(k=k, q=q, m=EMA_M)


def ema_ref(case):
    d = ema_data(case)
    k, q, m = d['k'].astype(np.float64), d['q'].astype(np.float64), d['m']
    a, b = k * m, q * (1.0 - m)
    return {'k': (a + b, rb(4, a, b, a + b) + 2 * TINY)}


def ema_eval32(case, defect=None):
    d = ema_data(case)
    n = case[0]
    k, q, m = d['k'], d['q'], F32(d['m'])
    om = F32(1) - m
    if defect == 'om_bf16':
        om = F32(1) - bf16_value(bf16_bits(np.array([m])))[0]
    out = (k * m).astype(F32) + (q * om).astype(F32)
    if defect == 'skip_tail':
        out = _tail_keep(out, k, n)
    return {'k': out, 'k_lp': bf16_bits(out, truncate=defect == 'bf16_truncate')}


# ---- momentum SGD
def _sgd_scalars(kind):
    return dict(lr=f32(0.03), mu=0.0 if kind == 'mu0' else f32(0.9), wd=0.0 if kind == 'wd0' else f32(1e-4),
                gs=_grad_scale(kind))


@functools.lru_cache(maxsize=4)
def sgd_data(case):
    n, kind = case
    rng = _rng('sgd', n, kind)
    s = _sgd_scalars(kind)
    p, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    v = np.zeros(n, F32)
    if kind in ('warm', 'mu0', 'wd0', 'gs3', 'gs16'):
        v = (0.5 * rng.standard_normal(n)).astype(F32)
    elif kind == 'mixed':
        p, g, v = _mags(rng, n), _mags(rng, n), _mags(rng, n)
        i = np.arange(n)
        c = i % 3 == 0                                             # g gs + wd p nearly cancels
        g[c] = (-s['wd'] * p[c].astype(np.float64) / s['gs'] * (1 + 2.0 ** -10 * rng.standard_normal(int(c.sum())))
                ).astype(F32)
        c = i % 3 == 1                                             # mu v + (g gs + wd p) nearly cancels
        gp = g[c].astype(np.float64) * s['gs'] + s['wd'] * p[c].astype(np.float64)
        v[c] = (-gp / s['mu'] * (1 + 2.0 ** -10 * rng.standard_normal(int(c.sum())))).astype(F32)
    elif kind == 'tiny_grad':
        g = (1e-22 * rng.standard_normal(n)).astype(F32)
    elif kind == 'zero_grad':
        g = np.zeros(n, F32)
    return dict(p=p, g=g, v=v, **s)


def sgd_ref(case):
    d = sgd_data(case)
    p, g, v = (d[n].astype(np.float64) for n in 'pgv')
    lr, mu, wd, gs = d['lr'], d['mu'], d['wd'], d['gs']
    a, b = g * gs, wd * p
    c, dd = a + b, mu * v
    v1 = dd + c
    f = lr * v1
    p1 = p - f
    return {'v': (v1, rb(5, a, b, c, dd, v1) + 3 * TINY),
            'p': (p1, rb(7, lr * a, lr * b, lr * c, lr * dd, f, f, p1) + (3 * lr + 1) * TINY)}


def sgd_eval32(case, defect=None):
    d = sgd_data(case)
    n = case[0]
    p, g, v = d['p'], d['g'], d['v']
    lr, mu, wd, gs = (F32(d[k]) for k in ('lr', 'mu', 'wd', 'gs'))
    gp = (g * gs).astype(F32) + (wd * (g if defect == 'wd_on_g' else p)).astype(F32)
    v1 = ((v if defect == 'no_mu' else (mu * v).astype(F32)) + gp).astype(F32)
    p1 = (p - (lr * v1).astype(F32)).astype(F32)
    if defect == 'skip_tail':
        v1, p1 = _tail_keep(v1, v, n), _tail_keep(p1, p, n)
    return {'v': v1, 'p': p1}


# ---- AdamW
def _adamw_scalars(kind):
    t, b2 = {'warm': (1000, f32(0.999)), 'mixed': (10, f32(0.95))}.get(kind, (1, f32(0.95)))
    b1 = f32(0.9)
    return dict(lr=f32(1e-3), b1=b1, b2=b2, eps=f32(1e-8), wd=0.0 if kind == 'wd0' else f32(0.05),
                b1p=f32(b1 ** t), b2p=f32(b2 ** t), gs=_grad_scale(kind))


@functools.lru_cache(maxsize=4)
def adamw_data(case):
    n, kind = case
    rng = _rng('adamw', n, kind)
    p, g = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    m, v = np.zeros(n, F32), np.zeros(n, F32)
    if kind in ('warm', 'gs3', 'gs16', 'wd0'):
        m = (0.1 * rng.standard_normal(n)).astype(F32)
        v = (0.01 * rng.random(n)).astype(F32)
    elif kind == 'mixed':
        p, g, m, v = _mags(rng, n), _mags(rng, n), _mags(rng, n), np.abs(_mags(rng, n))
    elif kind == 'tiny_grad':                                   # g g underflows; sqrt(v) + eps_t is all epsilon
        g = (1e-22 * rng.standard_normal(n)).astype(F32)
        p[::2] = 0                                              # where the step is the whole result
    elif kind == 'zero_grad':
        g = np.zeros(n, F32)
    return dict(p=p, g=g, m=m, v=v, **_adamw_scalars(kind))


def adamw_ref(case):
    d = adamw_data(case)
    p, g, m, v = (d[n].astype(np.float64) for n in 'pgmv')
    lr, b1, b2, eps, wd, b1p, b2p, gs = (d[k] for k in ('lr', 'b1', 'b2', 'eps', 'wd', 'b1p', 'b2p', 'gs'))
    c2 = math.sqrt(1.0 - b2p)
    decay, lr_t, eps_t = 1.0 - lr * wd, lr * c2 / (1.0 - b1p), eps * c2
    gg = g * gs
    t1, t2 = b1 * m, (1.0 - b1) * gg
    m1 = t1 + t2
    u1, u2 = b2 * v, (1.0 - b2) * gg * gg
    v1 = u1 + u2
    Bm = rb(5, t1, t2, m1) + 2 * TINY
    Bv = rb(7, u1, u2, v1) + 3 * TINY
    sq = np.sqrt(v1)
    with np.errstate(divide='ignore'):
        Bsq = np.minimum(Bv / sq, np.sqrt(Bv)) + E * sq
    den = sq + eps_t
    Bden = Bsq + 3 * E * eps_t + E * den
    assert (den > 2 * Bden).all()
    r = m1 / den
    Br = (Bm + np.abs(r) * Bden) / (den - Bden) + E * np.abs(r)
    s = lr_t * r
    Bs = lr_t * Br + 6 * E * np.abs(s)
    pd = p * decay
    Bpd = np.abs(p) * E * (abs(lr * wd) + abs(decay)) + E * np.abs(pd)
    p1 = pd - s
    return {'m': (m1, Bm), 'v': (v1, Bv), 'p': (p1, 2 * (Bs + Bpd + E * np.abs(p1)) + TINY)}


def adamw_eval32(case, defect=None):
    d = adamw_data(case)
    n = case[0]
    p, g, m, v = d['p'], d['g'], d['m'], d['v']
    lr, b1, b2, eps, wd, b1p, b2p, gs = (F32(d[k]) for k in ('lr', 'b1', 'b2', 'eps', 'wd', 'b1p', 'b2p', 'gs'))
    one = F32(1)
    if defect == 'swap_pows':
        b1p, b2p = b2p, b1p
    c2 = np.sqrt(one - b2p)
    decay = one - lr * wd
    lr_t = lr * c2 / (one - b1p)
    eps_t = eps if defect == 'eps_raw' else eps * c2
    assert all(isinstance(x, F32) for x in (c2, decay, lr_t, eps_t))
    gg = (g * gs).astype(F32)
    m1 = ((b1 * m).astype(F32) + ((one - b1) * gg).astype(F32)).astype(F32)
    v1 = ((b2 * v).astype(F32) + (((one - b2) * gg).astype(F32) * gg).astype(F32)).astype(F32)
    step = (lr_t * (m1 / (np.sqrt(v1) + eps_t).astype(F32)).astype(F32)).astype(F32)
    if defect == 'decay_after':
        p1 = ((p - step).astype(F32) * decay).astype(F32)
    else:
        p1 = ((p * decay).astype(F32) - step).astype(F32)
    if defect == 'skip_tail':
        m1, v1, p1 = _tail_keep(m1, m, n), _tail_keep(v1, v, n), _tail_keep(p1, p, n)
    return {'m': m1, 'v': v1, 'p': p1}


# ---- cast
def cast_data(n):
    return _rng('cast', n).standard_normal(n).astype(F32)


# ties to even in both directions, the largest finite float (rounds to bf16 inf), +-inf, +-0, NaN; then fp32 denormals
CAST_PATTERNS = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001,
                          0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                          0x7FC00000, 0xFFC00001, 0x7F800001, 0x00800000, 0x80800000, 0x3F800000, 0x477FE000],
                         dtype=np.uint32)
CAST_DENORMALS = np.array([0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00400000,
                           0x80400000, 0x007F8000, 0x00010000], dtype=np.uint32)


def cast_expect(x, defect=None, width=8):
    """bf16 bits; defect 'bf16_truncate' or 'skip_tail' (the tail keeps 0xFFFF: never written)."""
    out = bf16_bits(x, truncate=defect == 'bf16_truncate')
    if defect == 'skip_tail':
        out[len(x) - len(x) % width:] = 0xFFFF
    return out


def bf16_equal(got, want):
    """Bit equality, but any NaN matches any NaN (the payload is not compared)."""
    nan = lambda b: ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)
    return bool(np.all((got == want) | (nan(got) & nan(want))))


# ------------------------------------------------------------------------------------------------ LARS / LARC
CHUNK = 4096
ALIGN = 8                 # the arena's slot alignment in elements (ParamArena.ALIGN)
# (elements, kind) in arena order; the 258-block segment is the only way into the second trip of the segment reduce
LARS_SEGS = ((1, 'plain'), (2, 'plain'), (3, 'plain'), (4, 'plain'), (5, 'plain'), (8, 'plain'), (64, 'plain'),
             (4095, 'plain'), (100, 'p_zero'), (4096, 'plain'), (257 * CHUNK + 5, 'plain'), (4097, 'plain'),
             (100, 'g_zero'), (3 * CHUNK + 40, 'plain'), (4097, 'wd0'), (1000, 'p_big'), (1000, 'p_small'))
LARS_TAIL = 24            # elements after the last segment that no block lists
LARS_SCALARS = {'a': dict(eps=0.0, gs=1.0, lr=f32(0.3)), 'b': dict(eps=f32(1e-8), gs=f32(1.0 / 3.0), lr=f32(4.8))}
LARC_SCALARS = {'a': dict(eps=0.0, gs=1.0, lr=f32(0.1)), 'b': dict(eps=f32(1e-8), gs=f32(1.0 / 3.0), lr=f32(0.02))}
LARS_MU, LARS_COEFF, LARS_WD = f32(0.9), f32(1e-3), f32(1e-4)
LARS_CASES = [('lars', s, 0) for s in 'ab'] + [('larc', s, c) for s in 'ab' for c in (0, 1)]


@functools.lru_cache(maxsize=1)
def lars_layout():
    """The arena and the block table, built as LarsMomentumOptimizer._build_table builds them: slots at multiples of
    ALIGN, chunks of 4096, blk_seg ascending."""
    slices, off = [], 0
    for n, _ in LARS_SEGS:
        slices.append((off, n))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    blk_off, blk_len, blk_seg = [], [], []
    for si, (o, n) in enumerate(slices):
        for c in range(0, n, CHUNK):
            blk_off.append(o + c)
            blk_len.append(min(CHUNK, n - c))
            blk_seg.append(si)
    total = off + LARS_TAIL
    elem_seg = np.full(total, -1, np.int32)
    for si, (o, n) in enumerate(slices):
        elem_seg[o:o + n] = si
    seg_wd = np.array([0.0 if k == 'wd0' else LARS_WD for _, k in LARS_SEGS], F32)
    return dict(slices=slices, total=total, elem_seg=elem_seg, seg_wd=seg_wd,
                blk_off=np.array(blk_off, np.int64), blk_len=np.array(blk_len, np.int32),
                blk_seg=np.array(blk_seg, np.int32))


@functools.lru_cache(maxsize=1)
def lars_arena():
    """p, g, v over the whole arena: padding and the tail hold values too, and must come back unchanged."""
    lay = lars_layout()
    rng = _rng('lars')
    p, g = rng.standard_normal(lay['total']).astype(F32), rng.standard_normal(lay['total']).astype(F32)
    v = (0.01 * rng.standard_normal(lay['total'])).astype(F32)
    for (o, n), (_, kind) in zip(lay['slices'], LARS_SEGS):
        if kind == 'p_zero':
            p[o:o + n] = 0
        elif kind == 'g_zero':
            g[o:o + n] = 0
        elif kind == 'p_big':                                      # |p| / |g| about 1e6
            p[o:o + n] *= F32(1e3)
            g[o:o + n] *= F32(1e-3)
        elif kind == 'p_small':                                    # about 1e-6
            p[o:o + n] *= F32(1e-3)
            g[o:o + n] *= F32(1e3)
    return dict(p=p, g=g, v=v)


def lars_scalars(case):
    rule, s, clip = case
    return dict((LARS_SCALARS if rule == 'lars' else LARC_SCALARS)[s], mu=LARS_MU, coeff=LARS_COEFF, clip=clip)


def _depths(n):
    blocks = -(-n // CHUNK)
    dp = 35 + -(-blocks // 256)
    return dp, dp + 2


def _seg_rates(case, Sp, Sg):
    """Per segment, in float64: (rate, relative allowance of the rate, wd in use).  The rate is LARS's local learning
    rate or LARC's coefficient."""
    rule, _, clip = case
    s, lay = lars_scalars(case), lars_layout()
    rate, drate, wds = [], [], []
    for si, (n, _) in enumerate(LARS_SEGS):
        wd = float(lay['seg_wd'][si])
        dp, dg = _depths(n)
        dpn, dgn = dp * E / 2 + E, dg * E / 2 + E
        pn, gn = math.sqrt(Sp[si]), math.sqrt(Sg[si])
        if rule == 'lars':
            if wd > 0 and pn > 0 and gn > 0:
                rate.append(s['lr'] * s['coeff'] * pn / (gn + wd * pn + s['eps']))
                drate.append(dpn + max(dgn, dpn + E) + 5 * E)
            else:
                rate.append(s['lr'])
                drate.append(0.0)
        elif pn != 0 and gn != 0:
            x = s['coeff'] * pn / (gn + pn * wd + s['eps'])
            dx = dpn + max(dgn, dpn + E) + 4 * E
            if clip:
                x, dx = x / s['lr'], dx + E
                if x * (1 - dx) >= 1:
                    x, dx = 1.0, 0.0
                elif x > 1:
                    x, dx = 1.0, dx * x                             # min(x~, 1) moves by no more than x~ does
            rate.append(x)
            drate.append(dx)
        else:
            rate.append(1.0)
            drate.append(0.0)
            wd = 0.0
        wds.append(wd)
    return np.array(rate), np.array(drate), np.array(wds)


@functools.lru_cache(maxsize=2)
def lars_ref(case):
    """{'norms': [n_seg + n_blocks][2] squared norms and block partials, 'v', 'p': the whole arena}; an element no
    block lists has its initial value and the bound 0."""
    rule = case[0]
    s, lay, d = lars_scalars(case), lars_layout(), lars_arena()
    p, g, v = (d[n].astype(np.float64) for n in 'pgv')
    gs, mu, lr = s['gs'], s['mu'], s['lr']
    sq = np.stack([p * p, (g * gs) * (g * gs)], 1)
    part = np.array([sq[o:o + n].sum(0) for o, n in zip(lay['blk_off'], lay['blk_len'])])
    segs = np.array([sq[o:o + n].sum(0) for o, n in lay['slices']])
    dep = np.array([_depths(n) for n, _ in LARS_SEGS], np.float64)
    norms = np.concatenate([segs, part])
    Bn = np.concatenate([segs * dep * E, part * np.array([26.0, 28.0]) * E])
    rate, drate, wds = _seg_rates(case, segs[:, 0], segs[:, 1])
    own = lay['elem_seg'] >= 0
    es = np.where(own, lay['elem_seg'], 0)
    R, dR, wd = rate[es], drate[es], wds[es]
    a, b = g * gs, wd * p
    c = a + b
    dd, f = R * c, mu * v
    v1 = f + dd
    M = R * (np.abs(a) + np.abs(b)) + 2 * np.abs(dd) + np.abs(f) + np.abs(v1)
    Bv = 6 * E * M + dR * np.abs(dd) + 3 * TINY
    if rule == 'lars':
        p1 = p - v1
        Bp = 7 * E * (M + np.abs(p1)) + dR * np.abs(dd) + 3 * TINY
    else:
        h = lr * v1
        p1 = p - h
        Bp = 8 * E * (lr * M + np.abs(h) + np.abs(p1)) + lr * dR * np.abs(dd) + (3 * lr + 1) * TINY
    return {'norms': (norms, Bn), 'v': (np.where(own, v1, v), np.where(own, Bv, 0.0)),
            'p': (np.where(own, p1, p), np.where(own, Bp, 0.0)), 'rate': rate}


def lars_eval32(case, defect=None):
    rule, _, clip = case
    s, lay, d = lars_scalars(case), lars_layout(), lars_arena()
    p, g, v = d['p'], d['g'], d['v']
    gs, mu, lr, coeff, eps = (F32(s[k]) for k in ('gs', 'mu', 'lr', 'coeff', 'eps'))
    pp = (p * p).astype(F32)
    gg = (g * g).astype(F32)
    n_seg, n_blk = len(LARS_SEGS), len(lay['blk_off'])
    part = np.zeros((n_blk, 2), F32)
    for b, (o, n) in enumerate(zip(lay['blk_off'], lay['blk_len'])):
        part[b, 0] = pp[o:o + n].sum(dtype=F32)
        sg = (gg[o:o + n].sum(dtype=F32) * gs).astype(F32)
        part[b, 1] = sg if defect == 'gs_once' else (sg * gs).astype(F32)
    norms = np.zeros((n_seg, 2), F32)
    for si in range(n_seg):
        blocks = np.nonzero(lay['blk_seg'] == si)[0]
        if defect == 'drop_last_block':
            blocks = blocks[:-1] if len(blocks) > 1 else blocks
        if defect == 'reduce_256':
            blocks = blocks[:256]
        norms[si] = part[blocks].sum(0, dtype=F32)
    used = norms.copy()
    if defect == 'prev_norm':
        used[1:] = norms[:-1]
    rate, wds = np.zeros(n_seg, F32), np.zeros(n_seg, F32)
    for si in range(n_seg):
        wd = lay['seg_wd'][si]
        pn, gn = np.sqrt(used[si, 0]), np.sqrt(used[si, 1])
        if rule == 'lars':
            r = lr
            if wd > 0 and pn > 0 and gn > 0:
                r = lr * coeff * pn / (gn + wd * pn + eps)
        else:
            r = F32(1)
            if pn != 0 and gn != 0:
                r = coeff * pn / (gn + pn * wd + eps)
                if clip:
                    r = min(r if defect == 'clip_a' else r / lr, F32(1))
            elif defect != 'wd_zero_branch':
                wd = F32(0)
        assert isinstance(r, F32)
        rate[si], wds[si] = r, wd
    own = lay['elem_seg'] >= 0
    es = np.where(own, lay['elem_seg'], 0)
    R, wd = rate[es], wds[es]
    c = ((g * gs).astype(F32) + (wd * p).astype(F32)).astype(F32)
    v1 = ((mu * v).astype(F32) + (R * c).astype(F32)).astype(F32)
    p1 = (p - v1).astype(F32) if rule == 'lars' else (p - (lr * v1).astype(F32)).astype(F32)
    return {'norms': np.concatenate([norms, part]), 'v': np.where(own, v1, v), 'p': np.where(own, p1, p)}


# ------------------------------------------------------------------------------------------------ slab_reduce
SLAB_N = (4, 8, 60, 64, 68, 1024, 4100)
SLAB_COUNTS = (1, 4, 5, 32, 33, 100)              # both sides of each ZL switch (slabs <= 4: 1, <= 32: 4, else 16)
SLAB_KINDS = ('plain', 'cancelling')
SLAB_CASES = [(n, s, a, k) for s in SLAB_COUNTS for a in (0, 1) for n in SLAB_N for k in SLAB_KINDS]


@functools.lru_cache(maxsize=4)
def slab_data(case):
    n, slabs, acc, kind = case
    rng = _rng('slab', n, slabs, kind)
    ws = rng.standard_normal((slabs, n)).astype(F32)
    if kind == 'cancelling':                                     # slab z + 1 nearly cancels slab z
        for z in range(1, slabs, 2):
            ws[z] = (-ws[z - 1].astype(np.float64) * (1 + 2.0 ** -12 * rng.standard_normal(n))).astype(F32)
    return dict(ws=ws, out=rng.standard_normal(n).astype(F32))


def slab_lanes(slabs):
    return 1 if slabs <= 4 else 4 if slabs <= 32 else 16


def slab_ref(case):
    n, slabs, acc, _ = case
    d = slab_data(case)
    ws, prev = d['ws'].astype(np.float64), d['out'].astype(np.float64) * (1 if acc else 0)
    return {'out': (ws.sum(0) + prev, slabs * E * (np.abs(ws).sum(0) + np.abs(prev)))}


def slab_eval32(case, defect=None):
    """The documented order, in fp32: bit for bit what the kernel must give."""
    n, slabs, acc, _ = case
    d = slab_data(case)
    ZL = slab_lanes(slabs)
    lanes = []
    for zl in range(ZL):
        a = np.zeros(n, F32)
        for z in range(zl, slabs, ZL):
            a = (a + d['ws'][z]).astype(F32)
        lanes.append(a)
    if defect == 'reverse_lanes':
        lanes = lanes[::-1]
    a = lanes[0]
    for l in lanes[1:]:
        a = (a + l).astype(F32)
    if acc and defect != 'ignore_accumulate':
        a = (a + d['out']).astype(F32)
    return {'out': a}


# ------------------------------------------------------------------------------------------------ bn_fold
BN_CASES = [(n, eps) for n in (1, 255, 256, 257) for eps in (f32(1e-5), f32(1e-3))]


@functools.lru_cache(maxsize=4)
def bn_data(case):
    """A flat buffer of 4 n + 37 floats; the four index lists point into it in scattered order."""
    n, eps = case
    rng = _rng('bn', n)
    slots = rng.permutation(4 * n + 37)[:4 * n].astype(np.int64)
    gi, bi, mi, vi = slots[:n], slots[n:2 * n], slots[2 * n:3 * n], slots[3 * n:]
    flat = rng.standard_normal(4 * n + 37).astype(F32)
    flat[vi] = (10.0 ** rng.uniform(-12, 6, n)).astype(F32)          # variances from 1e-12 to 1e6
    flat[mi] = (flat[mi] * np.sqrt(flat[vi])).astype(F32)
    return dict(flat=flat, gi=gi, bi=bi, mi=mi, vi=vi, eps=eps)


def bn_ref(case):
    d = bn_data(case)
    f = d['flat'].astype(np.float64)
    sc = f[d['gi']] / np.sqrt(f[d['vi']] + d['eps'])
    ms = f[d['mi']] * sc
    sh = f[d['bi']] - ms
    return {'scale': (sc, rb(2 + F_RSQRT, sc)), 'shift': (sh, rb(4 + F_RSQRT, ms, sh))}


def bn_eval32(case, defect=None):
    d = bn_data(case)
    f = d['flat']
    sc = (f[d['gi']] * (F32(1) / np.sqrt((f[d['vi']] + F32(d['eps'])).astype(F32))).astype(F32)).astype(F32)
    return {'scale': sc, 'shift': (f[d['bi']] - (f[d['mi']] * sc).astype(F32)).astype(F32)}


# ------------------------------------------------------------------------------------------------ pack_weights
# name, K, R, S, C, (TR, TS, r_base, r_step, s_base, s_step, transpose, c_pad), source offset skew, mode the packer picks
PACK_JOBS = (
    ('subset', 5, 3, 3, 6, (1, 3, 1, 2, 0, 1, 0, 0), 0, 0),          # taps kept: a strided subset of a 3x3
    ('stem', 4, 3, 3, 3, (3, 3, 0, 1, 0, 1, 0, 8), 0, 0),            # c_pad > C
    ('dgrad', 6, 3, 3, 5, (2, 2, -1, 2, 2, 2, 1, 0), 0, 1),          # residue class: r = -1 and s = 4 are zero filled
    ('partial', 40, 3, 3, 30, (3, 3, 0, 1, 0, 1, 1, 0), 0, 1),       # 10800 elements: the last block is partial
    ('t32x32', 32, 1, 1, 32, (1, 1, 0, 1, 0, 1, 1, 0), 0, 2),
    ('t33x65', 33, 1, 1, 65, (1, 1, 0, 1, 0, 1, 1, 0), 0, 2),
    ('t1x40', 1, 1, 1, 40, (1, 1, 0, 1, 0, 1, 1, 0), 0, 2),
    ('t100x7', 100, 1, 1, 7, (1, 1, 0, 1, 0, 1, 1, 0), 0, 2),
    ('c4', 1, 1, 1, 4, (1, 1, 0, 1, 0, 1, 0, 0), 0, 3),
    ('c1020', 10, 1, 1, 102, (1, 1, 0, 1, 0, 1, 0, 0), 0, 3),
    ('c1024', 4, 2, 2, 64, (2, 2, 0, 1, 0, 1, 0, 0), 0, 3),
    ('c1027', 13, 1, 1, 79, (1, 1, 0, 1, 0, 1, 0, 0), 0, 3),
    ('c_misaligned', 3, 1, 1, 10, (1, 1, 0, 1, 0, 1, 0, 0), 2, 0),   # eligible for the cast, but src_off % 4 = 2
)


@functools.lru_cache(maxsize=1)
def pack_case():
    """The jobs through WeightPacker (one launch), its tables as CPU tensors, the source buffer and, per job, emu_pack's
    result.  -> dict(src, size, jobs [(name, Pack, src_off, K, R, S, C, emu)], jobs_raw, block_job, block_start,
    n_blocks, modes)."""
    from emu import emu_pack
    from passl_amd.hip import lib as L
    from passl_amd.hip.packer import WeightPacker
    from passl_amd.hip.plan import Pack
    packer, jobs, off = WeightPacker(), [], 0
    for name, K, R, S, C, f, skew, _ in PACK_JOBS:
        TR, TS, rb_, rs, sb, ss, tr, cp = f
        inner = cp if cp > 0 else (K if tr else C)
        pk = Pack(TR, TS, rb_, rs, sb, ss, tr, cp, size=(C if tr else K) * TR * TS * inner)
        off = (off + 3) // 4 * 4 + skew
        packer.add(off, K, R, S, C, pk)
        jobs.append([name, pk, off, K, R, S, C])
        off += K * R * S * C
    src = _rng('pack').standard_normal(off + 5).astype(F32)
    for j in jobs:
        name, pk, o, K, R, S, C = j
        w = torch.from_numpy(src[o:o + K * R * S * C].copy()).view(K, R, S, C)
        j.append(emu_pack(pk, w).numpy().ravel())
        assert j[-1].size == pk.size
    packer.build('cpu', torch.float32)
    raw = packer.jobs_dev.numpy().copy()
    arr = (L.PackJob * len(jobs)).from_buffer_copy(raw.tobytes())
    return dict(src=src, size=packer.size, jobs=jobs, jobs_raw=raw, block_job=packer.block_job.numpy().copy(),
                block_start=packer.block_start.numpy().copy(), n_blocks=packer.n_blocks,
                modes=[int(a.transpose) for a in arr], structs=arr)


def pack_expect(dtype_bf16):
    """The destination buffer: NaN (fp32) / 0xFFFF (bf16 bits) where no job writes, emu_pack elsewhere.
    -> (values or bits, written mask)."""
    c = pack_case()
    out = np.full(c['size'], np.nan, F32)
    mask = np.zeros(c['size'], bool)
    for name, pk, o, K, R, S, C, emu in c['jobs']:
        out[pk.dst_off:pk.dst_off + pk.size] = emu
        mask[pk.dst_off:pk.dst_off + pk.size] = True
    if dtype_bf16:
        return np.where(mask, bf16_bits(out), 0xFFFF).astype(np.uint16), mask
    return out, mask


def pack_eval32(defect=None):
    """The kernel's addressing restated per mode from the job table the packer built (fp32 destination)."""
    c = pack_case()
    src, out = c['src'], np.full(c['size'], np.nan, F32)
    for j in c['structs']:
        s = src[j.src_off:]
        K, R, S, C = j.K, j.R, j.S, j.C
        if j.transpose == 2:
            w = s[:K * C].reshape(K, C)
            out[j.dst_off:j.dst_off + K * C] = (w if defect == 'double_transpose' else w.T).ravel()
            continue
        if j.transpose == 3:
            out[j.dst_off:j.dst_off + K * R * S * C] = s[:K * R * S * C]
            continue
        inner_src = K if j.transpose else C
        inner = j.c_pad if j.c_pad > 0 else inner_src
        outer = C if j.transpose else K
        e = np.arange(outer * j.TR * j.TS * inner)
        i_in, t = e % inner, e // inner
        ts, t = t % j.TS, t // j.TS
        tr, o = t % j.TR, t // j.TR
        k, ch = (i_in, o) if j.transpose else (o, i_in)
        r, sx = j.r_base + tr * j.r_step, j.s_base + ts * j.s_step
        lim = inner_src - 1 if (defect == 'cpad_off_by_one' and j.c_pad > 0) else inner_src
        ok = (i_in < lim) & (r >= 0) & (r < R) & (sx >= 0) & (sx < S)
        idx = np.where(ok, ((k * R + r) * S + sx) * C + ch, 0)
        out[j.dst_off + e] = np.where(ok, s[idx], F32(0))
    return out


def same_bits_or_nan(a, b):
    """fp32 arrays: equal bit for bit, a NaN matching any NaN."""
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
