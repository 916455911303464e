"""CPU helpers of the token, index and layout numerics tests (numpy + torch on the CPU: the native library is never loaded).

Case tables, seeded inputs, numpy references, element-wise bounds, a float32 or bit-exact evaluation ("twin") of every
kernel and planted defects for
  csrc/vit.hip          mae_mask, mae_gather(_bwd) with cls_grad_kernel, mae_unshuffle(_bwd), patchify
  csrc/deit_tokens.hip  prefix_tokens_fwd / _bwd, mean2
  csrc/clip.hip         embed_fwd / _bwd, gather_rows, scatter_rows, eot_index
  csrc/layout_pool.hip  nchw_to_nhwc_pad, colsum / colsum_acc, relu_bwd
test_token_numerics_host.py shows that every reference is the project's own statement of the operation, that every
float32 twin uses at most HEADROOM = 0.5 of every bound and that each planted defect breaks a bound or a bit on a named
case; test_token_numerics_gpu.py judges the kernels by the same references and bounds.

Every family has  X_data(case, lp) -> the operands as the kernel receives them (`lp`: the compute dtype is bf16; such
operands are float32 arrays that hold bf16 values),  X_eval32(case, lp, defect=None) -> {tensor: value} restated from
the kernel's own index arithmetic and order of additions, and for the summed tensors  X_ref(case, lp) -> {tensor:
(float64 reference, bound)}.

What is exact.  Pure data movement is compared bit for bit: wbits(value, lp) are the bits an output of the compute
dtype must hold, the float32 value itself or its round-to-nearest-even bf16 (flat_util.bf16_bits: torch's CPU
conversion).  With one addition (x + pos) the value is the float32 sum, whose rounding to bf16 is the bf16 result.
The exact tensors have a second, independent statement (X_expect: numpy's stable argsort, fancy indexing, transposes)
that the host test compares the twin with.

What is bounded.  An fp32 sum of n terms onto an initial value (0 where the kernel does not accumulate) is compared
element by element with the float64 sum of the same operands:
    bound = n * 2 E * (sum |terms| + |initial|),   E = 2^-24.
Derivation: n additions, each with a relative error of at most E of a partial sum that never exceeds sum |terms| +
|initial|, in any order, to first order: n E (sum |terms| + |initial|); the factor 2 is room, so that the float32 twin
in the kernel's documented order stays within HEADROOM = 0.5 (the host test asserts it on every case, and that the
formula itself holds for the adversarial orders: largest first, all of one sign).  n = 0 gives the bound 0: the
element comes back bit-identical.

dtable of embed_bwd is accumulated in 64-bit fixed point: s = min(61 - e, 120) with frexp(float32(amax) *
float32(B T)) = (., e), formed in float32 as the kernel forms it; every addend is truncated to a multiple of 2^-s
(error < 2^-s each), the integer total is exact, is rounded to fp32 once (E |S|) and added to dtable (E (|S| +
|initial|) and the propagated first rounding):
    bound(tok, c) = count(tok) 2^-s + 4 E (|S| + |initial|),   S the float64 sum of the addends of row tok.
The first term is a hard limit that a sound kernel may use in full (truncation is one-sided), the second has the room
of the sum bound.  The twin stays within HEADROOM of the whole on `normal`, `decades` (one magnitude per token row, as
gradients have) and `zero`; on `scattered` (12 decades element by element: an addend 2^40 times smaller than the largest
keeps a dozen bits, and where the accumulated-into value is small too the truncation is most of the bound) it is held
to the bound itself, and to the truncation term plus HEADROOM of the rest.

The slab formulas (read off the entry points, restated here so that a change of either shows):
  mae_unshuffle_bwd   ntok = B (L + 1); slabs = min(ceil(ntok / 128), 1024); tpb = ceil(ntok / slabs);
                      slabs = ceil(ntok / tpb); ws needs slabs * D floats
  colsum              per = 256 if M >= 32768 else 64; slabs = min(ceil(M / per), 1024); rows = ceil(M / slabs);
                      slabs = ceil(M / rows); several slabs need ws of slabs * C floats
  embed_bwd           rows_par = 256 // (C / 8); slabs = clamp(ceil(B / (32 rows_par)), 1, 64); ws: slabs T C floats
and the slab sum itself is slab_reduce's documented order (flat_util.slab_eval32, restated by slab_reduce32).

Which case catches which planted defect (test_planted_defect in the host test):
  mae_mask ties resolved to the higher index          mask 49-quant4 (ids_restore bits)
  mae_mask rank > K in place of >=                    mask 49-uniform, K = 12 (mask bits)
  mae_gather pos[src] for pos[src + 1]                gather 3-5-2-8-mask (out bits)
  patchify h / w swapped                              patchify 2-3-8-12-4 (bits)
  patchify column order (pw, ph, c)                   patchify 2-3-8-12-4 (bits)
  mae_unshuffle_bwd last token slab dropped           unshuffle 3-42-10-32 (dmask_token, and dx bits)
  mae_unshuffle_bwd columns >= 256 dropped            unshuffle 4-196-1-264 (dmask_token, and dx bits)
  cls_grad images >= 8 dropped                        gather 9-17-17-264-mask (dcls)
  prefix_tokens dprefix1 summed from row 0            prefix 3-5-2-8 (dprefix1)
  embed out-of-range id clamped to V - 1              embed 3-12-24-7 oob (out bits, dtable)
  embed final run never flushed                       embed 40-9-64-50 text normal (dtable)
  eot_index takes the last maximum                    eot 4-77 (bits)
  eot_index compares ids in 32 bits                   eot 4-77 (bits)
  nchw_to_nhwc_pad columns beyond W + 2 pad unwritten pad lp C3 Cp4 pad3 extra3 (bits)
  colsum rows past a multiple of 8 dropped            colsum 40-9 (out)
  relu_bwd >= in place of >                           relu 8 (bits)
"""
import functools
import zlib

import numpy as np
import torch

from flat_util import E, HEADROOM, F32, bf16_bits, bf16_value, bits, case_id, slab_lanes, usage, verdict  # noqa: F401

I32, I64 = np.int32, np.int64
LPS = (False, True)                      # the compute dtypes: fp32, bf16


def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def q(x, lp):
    """The float32 array x as an operand of the compute dtype: rounded to bf16 values when lp."""
    x = np.ascontiguousarray(x, dtype=F32)
    return bf16_value(bf16_bits(x)).reshape(x.shape) if lp else x


def wbits(v, lp):
    """The bits an output of the compute dtype holds for the float32 value v (uint32, or uint16 of the bf16 rounding)."""
    v = np.ascontiguousarray(v, dtype=F32)
    return (bf16_bits(v) if lp else bits(v)).reshape(v.shape)


def _normal(rng, shape, lp=False):
    return q(rng.standard_normal(shape), lp)


def _decades(rng, shape, lp=False):
    """Normal values times 10^-9 .. 10^2, one power for each row of the last axis (a token's gradient has one
    magnitude): the spread of test_embedding_scatter_is_exact_and_order_independent (tests/test_clip_gpu.py)."""
    return q(rng.standard_normal(shape) * 10.0 ** rng.integers(-9, 3, shape[:-1] + (1,)), lp)


def _scattered(rng, shape, lp=False):
    """Magnitudes spread over 12 decades element by element, random signs."""
    return q(10.0 ** rng.uniform(-6, 6, shape) * rng.choice([-1.0, 1.0], shape), lp)


def sum_ref(terms, initial=0.0):
    """(float64 sum over axis 0 + initial, n 2 E (sum |terms| + |initial|))."""
    t = np.asarray(terms, dtype=np.float64)
    init = np.asarray(initial, dtype=np.float64)
    return t.sum(0) + init, len(t) * 2 * E * (np.abs(t).sum(0) + np.abs(init))


def lane_sum32(terms, lanes=8):
    """The float32 sum over axis 0 in the order of the 8-lane column reductions (cls_grad_kernel, colsum_kernel,
    mae_unshuffle_bwd_kernel): lane z adds terms z, z + lanes, ... ascending from +0; the lanes are combined in lane
    order."""
    t = np.asarray(terms, dtype=F32)
    pad = -len(t) % lanes
    if pad:
        t = np.concatenate([t, np.zeros((pad,) + t.shape[1:], F32)])
    t = t.reshape((-1, lanes) + t.shape[1:])
    acc = np.zeros(t.shape[1:], F32)
    for it in range(len(t)):
        acc = (acc + t[it]).astype(F32)
    s = acc[0]
    for z in range(1, lanes):
        s = (s + acc[z]).astype(F32)
    return s


def slab_reduce32(ws, prev=None):
    """slab_reduce's documented order over ws [slabs][n] (flat_util.slab_eval32): lane zl takes slabs zl, zl + ZL, ...
    ascending from +0, the lanes are combined in lane order, the previous `out` comes last when accumulating."""
    ZL = slab_lanes(len(ws))
    lanes = []
    for zl in range(ZL):
        a = np.zeros(ws.shape[1:], F32)
        for z in range(zl, len(ws), ZL):
            a = (a + ws[z]).astype(F32)
        lanes.append(a)
    a = lanes[0]
    for l in lanes[1:]:
        a = (a + l).astype(F32)
    return a if prev is None else (a + prev).astype(F32)


# ------------------------------------------------------------------------------------------------ mae_mask
MASK_B = 3
MASK_L = (1, 2, 49, 196, 256, 257, 513, 4096)       # 256 = the block: 257 and more take the i += 256 loop
MASK_KINDS = ('uniform', 'quant4', 'equal', 'tie256', 'negzero', 'denormal')
MASK_CASES = [(L, k) for L in MASK_L for k in MASK_KINDS]
MASK_REFUSED = ((4097, 5), (49, 0), (49, 50))       # (L, K)


def mask_keeps(L):
    return sorted({k for k in (1, L // 4, L - 1, L) if 1 <= k <= L})


@functools.lru_cache(maxsize=8)
def mask_data(case):
    L, kind = case
    rng = _rng('mask', L, kind)
    n = rng.random((MASK_B, L)).astype(F32)
    if kind == 'quant4':
        n = (np.floor(n * 4) / 4).astype(F32)
    elif kind == 'equal':
        n[:] = F32(0.5)
    elif kind == 'tie256':                                  # i and i + 256: the same thread's two trips
        i = 0 if L <= 256 else (L - 257) // 2
        j = i + 256 if L > 256 else L - 1
        n[:, j] = n[:, i]
    elif kind == 'negzero':                                 # -0.0 == +0.0: ordered by index
        z = rng.random((MASK_B, L)) < 0.6
        n = np.where(z, np.where(rng.random((MASK_B, L)) < 0.5, F32(-0.0), F32(0.0)), n - F32(0.5)).astype(F32)
    elif kind == 'denormal':                                # multiples of 2^-149 from -8 to 8: ordered, with ties
        n = (rng.integers(-8, 9, (MASK_B, L)) * 2.0 ** -149).astype(F32)
    return n


def mask_expect(noise, K):
    """numpy's stable argsort: ids_keep int32 [B][K], ids_restore int32 [B][L], mask fp32 [B][L] (1 = removed)."""
    order = np.argsort(noise, axis=1, kind='stable')
    restore = np.argsort(order, axis=1, kind='stable')
    return {'ids_keep': order[:, :K].astype(I32), 'ids_restore': restore.astype(I32),
            'mask': (restore >= K).astype(F32)}


@functools.lru_cache(maxsize=4)
def _mask_rank(case, tie_high):
    """The kernel's counting rank: rank[i] = #{j: n[j] < n[i] or (n[j] == n[i] and j < i)}."""
    noise = mask_data(case)
    j = np.arange(noise.shape[1])
    first = (j[None, :] > j[:, None]) if tie_high else (j[None, :] < j[:, None])
    return np.stack([((n[None, :] < n[:, None]) | ((n[None, :] == n[:, None]) & first)).sum(1) for n in noise]).astype(I32)


def mask_eval(case, K, defect=None):
    """mae_mask_kernel: ids_restore = rank, ids_keep[rank] = i for rank < K (-1: never written), mask = rank >= K."""
    rank = _mask_rank(case, defect == 'tie_high')
    B, L = rank.shape
    keep = np.full((B, K), -1, I32)
    for b in range(B):
        kept = rank[b] < K
        keep[b, rank[b][kept]] = np.arange(L)[kept]
    mask = (rank > K) if defect == 'rank_gt' else (rank >= K)
    return {'ids_keep': keep, 'ids_restore': rank, 'mask': mask.astype(F32)}


def _ids(B, L, K, kind, *key):
    """ids_keep [B][K], ids_restore [B][L]: from the mask reference on uniform noise, or ('subset') an arbitrary
    unsorted subset: the first K of a permutation whose head is in descending order."""
    rng = _rng('ids', B, L, K, kind, *key)
    if kind == 'subset':
        perm = np.stack([rng.permutation(L) for _ in range(B)])
        perm[:, :K] = -np.sort(-perm[:, :K], axis=1)
        return perm[:, :K].astype(I32), np.argsort(perm, axis=1).astype(I32)
    m = mask_expect(rng.random((B, L)).astype(F32), K)
    return m['ids_keep'], m['ids_restore']


# ------------------------------------------------------------------------------------------------ mae_gather(_bwd)
# B, L, K, D.  The last: 4098 tokens of 256 chunks, 1024 chunks more than the 4096 x 256 threads at which vit.hip caps a
# grid, the only way into the grid-stride loops of mae_gather_kernel and mae_gather_bwd_kernel (and the reason for its size)
GATHER_LOOP = (2, 2049, 2048, 2048)
GATHER_SHAPES = ((1, 1, 1, 8), (3, 5, 2, 8), (2, 49, 12, 40), (9, 17, 17, 264), (17, 196, 49, 64), GATHER_LOOP)
GATHER_CASES = [s + (k,) for s in GATHER_SHAPES for k in ('mask', 'subset')]


@functools.lru_cache(maxsize=4)
def gather_data(case, lp):
    B, L, K, D, kind = case
    rng = _rng('gather', case)
    keep, restore = _ids(B, L, K, kind)
    return dict(x=_normal(rng, (B, L, D), lp), cls=_normal(rng, D), pos=_normal(rng, (L + 1, D)), ids_keep=keep,
                ids_restore=restore, dout=_normal(rng, (B, K + 1, D), lp), dcls=_normal(rng, D))


def gather_expect(case, lp):
    d = gather_data(case, lp)
    B, L, K, D, _ = case
    keep = d['ids_keep'].astype(I64)
    out = np.empty((B, K + 1, D), F32)
    out[:, 0] = d['cls'] + d['pos'][0]
    out[:, 1:] = np.take_along_axis(d['x'], keep[:, :, None], 1) + d['pos'][1:][keep]
    dx = np.zeros((B, L, D), F32)
    np.put_along_axis(dx, keep[:, :, None], d['dout'][:, 1:], 1)
    return {'out': out, 'dx': dx}


def gather_eval32(case, lp, defect=None):
    """mae_gather_kernel, mae_gather_bwd_kernel and cls_grad_kernel by their own index arithmetic."""
    d = gather_data(case, lp)
    B, L, K, D, _ = case
    out = np.empty((B, K + 1, D), F32)
    dx = np.empty((B, L, D), F32)
    for b in range(B):
        for t in range(K + 1):
            if t == 0:
                v, src = d['cls'], 0
            else:
                src = int(d['ids_keep'][b, t - 1])
                v, src = d['x'][b, src], src + 1
            out[b, t] = v + d['pos'][src - 1 if (defect == 'pos_src' and t) else src]
        for l in range(L):
            rank = int(d['ids_restore'][b, l])
            dx[b, l] = d['dout'][b, 1 + rank] if rank < K else 0
    rows = d['dout'][:, 0]
    dcls = (d['dcls'] + lane_sum32(rows[:8] if defect == 'cls_first_8' else rows)).astype(F32)
    return {'out': out, 'dx': dx, 'dcls': dcls}


def gather_ref(case, lp):
    d = gather_data(case, lp)
    return {'dcls': sum_ref(d['dout'][:, 0], d['dcls'])}


# ------------------------------------------------------------------------------------------------ mae_unshuffle(_bwd)
# B, L, K, D: 128 tokens = one slab; 129 = two; K = L: nothing is masked; D = 264: a second, partly filled column block;
# the last: 4098 x 256 chunks, the grid-stride loop of mae_unshuffle_kernel (as GATHER_LOOP)
UNSHUFFLE_LOOP = (2, 2048, 512, 2048)
UNSHUFFLE_CASES = ((1, 1, 1, 8), (2, 63, 16, 8), (3, 42, 10, 32), (2, 49, 49, 40), (4, 196, 1, 264), (2, 196, 49, 512),
                   UNSHUFFLE_LOOP)
UNSHUFFLE_WS = 1024                      # the workspace the entry documents: 1024 * D floats


def unshuffle_slabs(B, L):
    """(slabs, tokens per slab) as passl_hip_mae_unshuffle_bwd forms them."""
    ntok = B * (L + 1)
    slabs = min(-(-ntok // 128), 1024)
    tpb = -(-ntok // slabs)
    return -(-ntok // tpb), tpb


@functools.lru_cache(maxsize=4)
def unshuffle_data(case, lp):
    B, L, K, D = case
    rng = _rng('unshuffle', case)
    keep, restore = _ids(B, L, K, 'mask', 'unshuffle')
    return dict(x=_normal(rng, (B, K + 1, D), lp), mask_token=_normal(rng, D), pos=_normal(rng, (L + 1, D)),
                ids_keep=keep, ids_restore=restore, dout=_normal(rng, (B, L + 1, D), lp), dmask_token=_normal(rng, D))


def unshuffle_expect(case, lp):
    d = unshuffle_data(case, lp)
    B, L, K, D = case
    r = d['ids_restore'].astype(I64)
    full = np.concatenate([d['x'][:, 1:], np.broadcast_to(d['mask_token'], (B, L - K, D))], 1)
    out = np.concatenate([d['x'][:, :1], np.take_along_axis(full, r[:, :, None], 1)], 1) + d['pos']
    dx = np.concatenate([d['dout'][:, :1],
                         np.take_along_axis(d['dout'][:, 1:], d['ids_keep'].astype(I64)[:, :, None], 1)], 1)
    return {'out': out.astype(F32), 'dx': dx}


def _masked_rows(case, lp):
    d = unshuffle_data(case, lp)
    return d['dout'][:, 1:][d['ids_restore'] >= case[2]]           # [B (L - K)][D], (b, l) ascending


def unshuffle_eval32(case, lp, defect=None):
    d = unshuffle_data(case, lp)
    B, L, K, D = case
    out = np.empty((B, L + 1, D), F32)
    dx = np.full((B, K + 1, D), np.nan, F32)
    slabs, tpb = unshuffle_slabs(B, L)
    ws = np.zeros((slabs, D), F32)
    cols = min(D, 256) if defect == 'cols_256' else D
    flat = d['dout'].reshape(B * (L + 1), D)
    for b in range(B):
        for t in range(L + 1):
            r = 0 if t == 0 else int(d['ids_restore'][b, t - 1]) + 1
            out[b, t] = (d['x'][b, r] if r <= K else d['mask_token']) + d['pos'][t]
    for y in range(slabs - 1 if defect == 'last_slab' else slabs):
        toks = np.arange(y * tpb, min((y + 1) * tpb, B * (L + 1)))
        terms = np.zeros((len(toks), D), F32)                     # a kept token adds nothing: +0 keeps a lane's sum
        for i, tok in enumerate(toks):
            b, t = divmod(int(tok), L + 1)
            if t <= K:
                src = 0 if t == 0 else 1 + int(d['ids_keep'][b, t - 1])
                dx[b, t, :cols] = d['dout'][b, src, :cols]
            if t > 0 and d['ids_restore'][b, t - 1] >= K:
                terms[i] = flat[tok]
        ws[y, :cols] = lane_sum32(terms)[:cols]
    return {'out': out, 'dx': dx, 'dmask_token': slab_reduce32(ws, d['dmask_token'])}


def unshuffle_ref(case, lp):
    return {'dmask_token': sum_ref(_masked_rows(case, lp), unshuffle_data(case, lp)['dmask_token'])}


# ------------------------------------------------------------------------------------------------ patchify
PATCHIFY_CASES = ((1, 1, 1, 1, 1), (2, 3, 8, 12, 4), (1, 3, 14, 28, 7), (2, 4, 32, 16, 16), (1, 1, 64, 32, 32))
PATCHIFY_INPUTS = ('coded', 'random')
# 1075200 pixels, one thread each: past the 4096 x 256 threads of the capped grid, into patchify_kernel's grid-stride
# loop (random input only: 'coded' has 50000 distinct values at the most)
PATCHIFY_LOOP = (2, 3, 448, 400, 16)
PATCHIFY_REFUSED = (1, 3, 9, 12, 4)      # H % p != 0


@functools.lru_cache(maxsize=4)
def patchify_data(case, which):
    """'coded': pixel (b, c, h, w) holds its own flat index as a bf16 bit pattern from 0x3C00 up: every pixel a
    distinct value that bf16 holds exactly (consecutive integers stop being exact at 256, the largest case has 4096
    pixels), so any permutation shows in either dtype.  'random': for the rounding."""
    B, C, H, W, p = case
    if which == 'coded':
        return bf16_value((0x3C00 + np.arange(B * C * H * W)).astype(np.uint16)).reshape(B, C, H, W)
    return _rng('patchify', case).standard_normal((B, C, H, W)).astype(F32)


def patchify_expect(img, p):
    B, C, H, W = img.shape
    return img.reshape(B, C, H // p, p, W // p, p).transpose(0, 2, 4, 3, 5, 1).reshape(-1, p * p * C)


def patchify_eval(img, p, defect=None):
    """patchify_kernel's index arithmetic."""
    B, C, H, W = img.shape
    gh, gw, P = H // p, W // p, p * p * C
    i = np.arange(B * gh * gw * P)
    col, patch = i % P, i // P
    c, pw, ph = col % C, (col // C) % p, col // (C * p)
    if defect == 'col_order':
        c, ph, pw = col % C, (col // C) % p, col // (C * p)
    w_, h_, b = patch % gw, (patch // gw) % gh, patch // (gw * gh)
    if defect == 'swap_hw':
        h_, w_ = patch % gh, (patch // gh) % gw
    return img.ravel()[((b * C + c) * H + h_ * p + ph) * W + w_ * p + pw].reshape(-1, P)


# ------------------------------------------------------------------------------------------------ prefix tokens, mean2
# B, L, NP, C; the last two: 257 chunks of 8 in the forward, and in the backward's copy: one past a 256-thread block
PREFIX_CASES = ((1, 1, 1, 8), (3, 5, 2, 8), (2, 49, 2, 40), (9, 16, 1, 264), (1, 255, 2, 8), (1, 257, 1, 8))
MEAN2_N = (1, 255, 257)


@functools.lru_cache(maxsize=4)
def prefix_data(case, lp):
    B, L, NP, C = case
    rng = _rng('prefix', case)
    return dict(x=_normal(rng, (B, L, C), lp), prefix=_normal(rng, (2, C)), pos=_normal(rng, (L + NP, C)),
                dout=_normal(rng, (B, L + NP, C), lp), dprefix=_normal(rng, (2, C)))


def prefix_expect(case, lp):
    d = prefix_data(case, lp)
    B, L, NP, C = case
    out = np.concatenate([np.broadcast_to(d['prefix'][:NP], (B, NP, C)), d['x']], 1) + d['pos']
    return {'out': out.astype(F32), 'dx': d['dout'][:, NP:]}


def prefix_eval32(case, lp, defect=None):
    d = prefix_data(case, lp)
    B, L, NP, C = case
    out = np.empty((B, L + NP, C), F32)
    for t in range(L + NP):
        out[:, t] = (d['prefix'][t] if t < NP else d['x'][:, t - NP]) + d['pos'][t]
    res = {'out': out, 'dx': np.stack([d['dout'][b, NP:] for b in range(B)])}
    for t in range(NP):
        s = d['dprefix'][t]
        for b in range(B):                                        # images in order, onto the previous value
            s = (s + d['dout'][b, 0 if defect == 'dprefix1_row0' else t]).astype(F32)
        res['dprefix%d' % t] = s
    return res


def prefix_ref(case, lp):
    d = prefix_data(case, lp)
    return {'dprefix%d' % t: sum_ref(d['dout'][:, t], d['dprefix'][t]) for t in range(case[2])}


def mean2_data(n):
    rng = _rng('mean2', n)
    return rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)


def mean2_eval32(a, b=None):
    """One rounding (of the sum); the halving is exact."""
    return ((a + b).astype(F32) if b is not None else a) * F32(0.5)


# ------------------------------------------------------------------------------------------------ embed_fwd / embed_bwd
# B, T, C, V: C / 8 = 3 does not divide 256; (70, 5, 2048, 3): rows_par = 1, three image slabs
EMBED_SHAPES = ((1, 1, 8, 1), (3, 12, 24, 7), (40, 9, 64, 50), (70, 5, 2048, 3), (2, 77, 512, 300))
EMBED_TEXTS = ('text', 'equal', 'pad', 'oob')
EMBED_DOUTS = ('normal', 'decades', 'scattered', 'zero')
EMBED_CASES = [s + (t,) for s in EMBED_SHAPES for t in EMBED_TEXTS]
EMBED_NAN = ((3, 12, 24, 7, 'text'), (1, 4, 13))       # the case and (b, t, c) of the single NaN in dout
OOB_IDS = (-1, None, 2 ** 40)                          # None: V itself


@functools.lru_cache(maxsize=32)
def embed_text(case):
    B, T, C, V, kind = case
    rng = _rng('text', B, T, C, V)
    if kind in ('text', 'oob'):
        if T >= 3 and V >= 4:                                       # what OC.make_text can build
            from oracle import clip as OC
            text = OC.make_text(torch.Generator().manual_seed(B * T), B, T, V).numpy().copy()
        else:
            text = rng.integers(0, V, (B, T))
        if kind == 'oob':                                           # -1, V and 2^40 at the first and every fifth position
            flat = text.reshape(-1)
            for n, i in enumerate(sorted(set(range(min(3, B * T))) | set(range(4, B * T, 5)))):
                flat[i] = V if OOB_IDS[n % 3] is None else OOB_IDS[n % 3]
    elif kind == 'equal':
        text = np.full((B, T), V // 2)
    else:                                                           # the pad id 0 at most positions
        text = np.where(rng.random((B, T)) < 0.85, 0, rng.integers(0, V, (B, T)))
    return text.astype(I64)


@functools.lru_cache(maxsize=4)
def embed_data(case, dkind, lp, nan_at=None):
    B, T, C, V, _ = case
    rng = _rng('embed', B, T, C, V)
    table, pos, dtable, dpos = (_normal(rng, s) for s in ((V, C), (T, C), (V, C), (T, C)))
    dout = {'normal': _normal, 'decades': _decades, 'scattered': _scattered, 'zero': lambda r, s, l: np.zeros(s, F32)}[dkind](rng, (B, T, C), lp)
    if nan_at is not None:
        dout[nan_at] = np.nan
    return dict(text=embed_text(case), table=table, pos=pos, dout=dout, dtable=dtable, dpos=dpos)


def embed_bwd_slabs(B, C):
    rows_par = 256 // (C // 8)
    return max(1, min(64, -(-B // (rows_par * 32)))), rows_par


def embed_scale_exp(dout, rows):
    """s, formed in float32 as embed_scale_exp (clip.hip) forms it; amax skips a NaN as fmaxf does."""
    amax = F32(np.nanmax(np.abs(dout), initial=0.0))
    return min(61 - int(np.frexp(F32(amax * F32(rows)))[1]), 120), amax


def _valid(text, V):
    return (text >= 0) & (text < V)


def _unflushed(text, B, T, C):
    """[B][T] rows of the final run of each thread's image sequence (the planted defect drops them)."""
    slabs, rows_par = embed_bwd_slabs(B, C)
    drop = np.zeros((B, T), bool)
    for t in range(T):
        for b0 in range(min(slabs * rows_par, B)):
            seq = list(range(b0, B, slabs * rows_par))
            for b in reversed(seq):
                if text[b, t] != text[seq[-1], t]:
                    break
                drop[b, t] = True
    return drop


def embed_eval32(case, dkind, lp, defect=None, nan_at=None):
    """embed_fwd_kernel's gather, the fixed-point path of embed_scatter_kernel / embed_flush_kernel in integers, and
    the position gradient in the order of embed_scatter_kernel and slab_reduce."""
    B, T, C, V, _ = case
    d = embed_data(case, dkind, lp, nan_at)
    text = d['text']
    ok = _valid(text, V)
    tok = np.where(ok, text, 0)
    if defect == 'clamp_oob':
        ok, tok = np.ones_like(ok), np.clip(text, 0, V - 1)
    out = (np.where(ok[:, :, None], d['table'][tok], F32(0)) + d['pos']).astype(F32)
    s, amax = embed_scale_exp(d['dout'], B * T)
    scale = np.ldexp(F32(1), s) if amax > 0 else F32(0)
    with np.errstate(invalid='ignore'):
        fixed = np.trunc(np.nan_to_num((d['dout'] * scale).astype(F32), nan=0.0)).astype(np.int64)
    add = ok & ~_unflushed(text, B, T, C) if defect == 'no_final_flush' else ok
    acc = np.zeros((V, C), np.int64)
    np.add.at(acc, tok[add], fixed[add])
    touched = np.zeros(V, bool)
    touched[tok[add]] = True
    total = (acc.astype(np.float64) * 2.0 ** -s).astype(F32)
    dtable = np.where(touched[:, None], (d['dtable'] + total).astype(F32), d['dtable'])
    slabs, rows_par = embed_bwd_slabs(B, C)
    stride = slabs * rows_par
    g = np.concatenate([d['dout'], np.zeros((-B % stride, T, C), F32)]).reshape(-1, slabs, rows_par, T, C)
    lane = np.zeros(g.shape[1:], F32)
    for it in range(len(g)):                                     # a thread's images, ascending
        lane = (lane + g[it]).astype(F32)
    ws = np.zeros((slabs, T, C), F32)
    for r in range(rows_par):                                    # the block's row lanes, in order
        ws = (ws + lane[:, r]).astype(F32)
    return {'out': out, 'dtable': dtable, 'dpos': slab_reduce32(ws, d['dpos'])}


def embed_ref(case, dkind, lp, nan_at=None):
    """dtable and dpos: (float64 reference, bound).  With nan_at the NaN counts as 0 here: the caller leaves
    dpos[t, c] and row text[b, t] of dtable out."""
    B, T, C, V, _ = case
    d = embed_data(case, dkind, lp, nan_at)
    ok = _valid(d['text'], V)
    g = np.nan_to_num(d['dout'].astype(np.float64), nan=0.0)
    S, A = np.zeros((V, C)), np.zeros((V, C))
    np.add.at(S, d['text'][ok], g[ok])
    np.add.at(A, d['text'][ok], np.abs(g[ok]))
    count = np.bincount(d['text'][ok], minlength=V).astype(np.float64)
    s, _ = embed_scale_exp(d['dout'], B * T)
    init = d['dtable'].astype(np.float64)
    return {'dtable': (S + init, count[:, None] * 2.0 ** -s + 4 * E * (np.abs(S) + np.abs(init))),
            'dpos': sum_ref(g, d['dpos'])}


# ------------------------------------------------------------------------------------------------ eot_index, rows
EOT_CASES = [(B, T) for B in (1, 4, 5, 9) for T in (1, 63, 64, 65, 77, 129)]
# (5, 9): two lanes; (3, 67): one lane's two trips (t and t + 64); (10, 70)
EOT_ROWS = ('first', 'last', 'tie-5-9', 'tie-3-67', 'tie-10-70', 'negative', 'big')


@functools.lru_cache(maxsize=8)
def eot_text(case, shift):
    """[B][T] int64; row b holds the pattern EOT_ROWS[(b + shift) % 7] where T has room for it (else a plain row)."""
    B, T = case
    rng = _rng('eot', B, T, shift)
    text = rng.integers(2, 1000, (B, T)).astype(I64)
    for b in range(B):
        kind = EOT_ROWS[(b + shift) % len(EOT_ROWS)]
        if kind == 'first':
            text[b, 0] = 5000
        elif kind == 'last':
            text[b, T - 1] = 5000
        elif kind.startswith('tie'):
            i, j = (int(v) for v in kind.split('-')[1:])
            if j < T:
                text[b, i] = text[b, j] = 5000
        elif kind == 'negative':
            text[b] = -text[b] - (1 << 33)
        elif T >= 2:                                                 # 2^40 + 1 wins; in 32 bits both are below every other id
            i, j = sorted(rng.choice(T, 2, replace=False))
            text[b, j], text[b, i] = 2 ** 40, 2 ** 40 + 1
    return text


def eot_eval(text, defect=None):
    """eot_index_kernel: lane l takes t = l, l + 64, ... (a strictly greater id replaces), the lanes are combined by
    (greater id, then lower t)."""
    B, T = text.shape
    key = text.astype(np.uint32).astype(np.int32).astype(I64) if defect == 'ids_32bit' else text
    idx = np.zeros(B, I32)
    for b in range(B):
        best = None
        for lane in range(min(64, T)):
            lb = None
            for t in range(lane, T, 64):
                if lb is None or key[b, t] > lb[0] or (defect == 'last_max' and key[b, t] == lb[0]):
                    lb = (key[b, t], t)
            if best is None or lb[0] > best[0] or (lb[0] == best[0] and (lb[1] > best[1]) == (defect == 'last_max')):
                best = lb
        idx[b] = b * T + best[1]
    return idx


ROWS_TOTAL = 13
ROWS_CASES = [(n, C) for n in (1, 9) for C in (8, 24, 512)]


@functools.lru_cache(maxsize=4)
def rows_data(case, lp):
    """x [13][C]; gather idx with duplicates (n = 9), scatter idx unique."""
    n, C = case
    rng = _rng('rows', case)
    gidx = rng.integers(0, ROWS_TOTAL, n)
    if n > 2:
        gidx[n - 1] = gidx[0]
        gidx[n // 2] = gidx[1]
    return dict(x=_normal(rng, (ROWS_TOTAL, C), lp), gidx=gidx.astype(I32), dout=_normal(rng, (n, C), lp),
                sidx=rng.permutation(ROWS_TOTAL)[:n].astype(I32))


def rows_eval(case, lp):
    d = rows_data(case, lp)
    dx = np.zeros_like(d['x'])
    for r, i in enumerate(d['sidx']):
        dx[i] = d['dout'][r]
    return {'out': np.stack([d['x'][i] for i in d['gidx']]), 'dx': dx}


# ------------------------------------------------------------------------------------------------ nchw_to_nhwc_pad
PAD_N, PAD_H, PAD_W = 2, 5, 7
# lp, C, Cp, pad, extra columns (Wp = W + 2 pad + extra), skew of y in elements.  bf16 with Cp = 4 is the stem's kernel
# unless y is off 8 bytes (skew 1), which takes the generic kernel and must give the same values.
PAD_CASES = ([(True, C, 4, pad, ex, skew) for C in (1, 2, 3, 4) for pad in (0, 3) for ex in (0, 3) for skew in (0, 1)] +
             [(lp, min(Cp, 3), Cp, pad, ex, 0) for lp in LPS for Cp in (1, 3, 8) for pad in (0, 3) for ex in (0, 3)])
PAD_REFUSED = {'Cp < C': dict(C=3, Cp=2, short=0), 'Cp = 9': dict(C=3, Cp=9, short=0),
               'Wp one short': dict(C=3, Cp=4, short=1)}


@functools.lru_cache(maxsize=4)
def pad_data(C):
    return _rng('pad', C).standard_normal((PAD_N, C, PAD_H, PAD_W)).astype(F32)


def pad_expect(case):
    _, C, Cp, pad, ex, _ = case
    y = np.zeros((PAD_N, PAD_H + 2 * pad, PAD_W + 2 * pad + ex, Cp), F32)
    y[:, pad:pad + PAD_H, pad:pad + PAD_W, :C] = pad_data(C).transpose(0, 2, 3, 1)
    return y


def pad_eval(case, defect=None):
    """The kernels' index arithmetic, one output pixel at a time; NaN where nothing is written."""
    _, C, Cp, pad, ex, _ = case
    x = pad_data(C)
    Hp, Wp = PAD_H + 2 * pad, PAD_W + 2 * pad + ex
    i = np.arange(PAD_N * Hp * Wp)
    wp, hp, n = i % Wp, (i // Wp) % Hp, i // (Wp * Hp)
    h, w = hp - pad, wp - pad
    inside = (h >= 0) & (h < PAD_H) & (w >= 0) & (w < PAD_W)
    y = np.zeros((len(i), Cp), F32)
    for c in range(C):
        y[:, c] = np.where(inside, x[n, c, np.clip(h, 0, PAD_H - 1), np.clip(w, 0, PAD_W - 1)], F32(0))
    if defect == 'beyond_unwritten':
        y[wp >= PAD_W + 2 * pad] = np.nan
    return y.reshape(PAD_N, Hp, Wp, Cp)


# ------------------------------------------------------------------------------------------------ colsum, colsum_acc
# C, M.  (8, 32767) and (8, 32768) are the two sides of the slab-size switch, the only reason for their size.
COLSUM_CASES = [(C, M) for C in (8, 40, 264) for M in (1, 7, 8, 9, 64, 65, 129)] + [(8, 32767), (8, 32768)]
COLSUM_REFUSED = (40, 65)                # two slabs: needs the workspace


def colsum_slabs(M):
    """(slabs, rows per slab) as colsum_impl forms them."""
    per = 256 if M >= 32768 else 64
    slabs = min(-(-M // per), 1024)
    rows = -(-M // slabs)
    return -(-M // rows), rows


@functools.lru_cache(maxsize=4)
def colsum_data(case, lp):
    C, M = case
    rng = _rng('colsum', case)
    return dict(x=_normal(rng, (M, C), lp), out=_normal(rng, C))


def colsum_eval32(case, lp, acc, defect=None):
    C, M = case
    d = colsum_data(case, lp)
    slabs, rows = colsum_slabs(M)
    x = np.concatenate([d['x'], np.zeros((slabs * rows - M, C), F32)]).reshape(slabs, rows, C).copy()
    if defect == 'tail_rows':                                        # a slab's rows past a multiple of 8 are dropped
        for y in range(slabs):
            n = min(rows, M - y * rows)
            x[y, n - n % 8:] = 0
    ws = lane_sum32(x.transpose(1, 0, 2))                            # [slabs][C]: every slab in the 8-lane order
    if slabs == 1:
        return {'out': (d['out'] + ws[0]).astype(F32) if acc else ws[0]}
    return {'out': slab_reduce32(ws, d['out'] if acc else None)}


def colsum_ref(case, lp, acc):
    d = colsum_data(case, lp)
    return {'out': sum_ref(d['x'], d['out'] if acc else 0.0)}


# ------------------------------------------------------------------------------------------------ relu_bwd
# the grid is capped at 4096 blocks of 256 lanes, 8 elements a lane: only one chunk more reaches the grid-stride loop
RELU_N = (8, 2056, 8 * 4096 * 256 + 8)
RELU_REFUSED = 12
# +0, -0, a positive and a negative denormal (bf16 holds both), negatives, +inf, NaN, -inf, positives
RELU_Y = np.array([0x00000000, 0x80000000, 0x00010000, 0x80400000, 0xBFC00000, 0x7F800000, 0x7FC00000, 0xFF800000,
                   0x40000000, 0x00400000, 0xBA000000, 0x3F000000, 0x80010000], dtype=np.uint32)


@functools.lru_cache(maxsize=2)
def relu_data(n, lp):
    """y cycles through RELU_Y (13 values against chunks of 8: every value meets every lane slot); dy holds NaN and
    -3 in turn where y <= 0 or y is NaN, normal values elsewhere."""
    y = np.resize(RELU_Y, n).view(F32)
    dy = q(_rng('relu', n).standard_normal(n), lp)
    off = ~(y > 0)
    dy[off] = np.where(np.arange(n)[off] % 2 == 0, F32(np.nan), F32(-3))
    return dict(y=y, dy=dy)


def relu_eval(n, lp, defect=None):
    d = relu_data(n, lp)
    on = (d['y'] >= 0) if defect == 'ge' else (d['y'] > 0)
    return np.where(on, d['dy'], F32(0))
