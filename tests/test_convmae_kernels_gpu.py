"""The ConvMAE kernels (csrc/convmae.hip) against float64 references, element by element, over the case tables of
convmae_util.py (which has the derivation of every bound), and bit for bit where a kernel only moves values or adds two.

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must
survive; outputs start as NaN (slabs: as 0xA5 bytes) and every element must have been written; every input must come
back bit-identical; a second run of every launch must give the same bits (dw, dbias, dpos and the mask token's gradient
included: no atomics).
"""
import pytest
import torch

import convmae_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32 = torch.float32
I32 = torch.int32
WORST = {}


def fig(kernel, what, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print('FIG %s %s %.4f of the bound (largest so far for this kernel: %.4f)' % (kernel, what, ratio, WORST[kernel]))


def gin(t, dtype):
    return Guarded(t.numel(), dtype, fill=t)


def ptr(g):
    return None if g is None else g.view.data_ptr()


def run(what, fn, ins, outs):
    """Launches fn() twice on the guarded operands.  Asserts: status 0, the same output bits both times, every guard
    intact, every input unchanged, every output element written."""
    before = {n: g.raw() for n, g in ins.items()}
    assert fn() == 0, what
    torch.cuda.synchronize()
    first = {n: g.raw() for n, g in outs.items()}
    for g in outs.values():
        g.reset()
    assert fn() == 0, what
    torch.cuda.synchronize()
    for n, g in outs.items():
        assert torch.equal(g.raw(), first[n]), '%s: %s differs between two runs of the same launch' % (what, n)
    for n, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), '%s: a guard region of %s was written' % (what, n)
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), '%s: the input %s was modified' % (what, n)
    for n, g in outs.items():
        left = g.unwritten()
        assert left == 0, '%s: %d elements of %s were not written' % (what, left, n)


def check(what, tensor, kernel, ratio_idx):
    fig(kernel, what, ratio_idx[0])
    msg = U.verdict(what, tensor, *ratio_idx)
    assert msg is None, msg


def host(g, shape):
    return g.view.float().cpu().view(shape)


def bits_equal(got, want, dtype):
    """Number of elements whose bits differ after `want` is rounded to the storage dtype."""
    b = torch.int32 if dtype == F32 else torch.int16
    return int((got.to(dtype).view(b) != want.to(dtype).view(b)).sum())


def mask_ins(ins, mask):
    if mask is not None:
        ins['mask'] = gin(mask, F32)
    return ins


def conv_fwd(x, w, bias, mask, grid, shape, dtype, what='dwconv5_masked_fwd'):
    N, H, W, C = shape
    ins = mask_ins(dict(x=gin(x, dtype), w=gin(w, F32), bias=gin(bias, F32)), mask)
    y = Guarded(x.numel(), dtype)
    run(what, lambda: L.load().passl_hip_dwconv5_masked_fwd(
        ptr(ins['x']), ptr(ins['w']), ptr(ins['bias']), ptr(ins.get('mask')), ptr(y), N, H, W, C, grid[0], grid[1],
        L.dt(dtype), L.stream()), ins, dict(y=y))
    return host(y, shape)


def conv_bwd_data(dy, w, mask, grid, shape, dtype, what='dwconv5_masked_bwd_data'):
    N, H, W, C = shape
    ins = mask_ins(dict(dy=gin(dy, dtype), w=gin(w, F32)), mask)
    dx = Guarded(dy.numel(), dtype)
    run(what, lambda: L.load().passl_hip_dwconv5_masked_bwd_data(
        ptr(ins['dy']), ptr(ins['w']), ptr(ins.get('mask')), ptr(dx), N, H, W, C, grid[0], grid[1], L.dt(dtype),
        L.stream()), ins, dict(dx=dx))
    return host(dx, shape)


def conv_bwd_weight(x, dy, mask, grid, shape, dtype, what='dwconv5_masked_bwd_weight'):
    N, H, W, C = shape
    ins = mask_ins(dict(x=gin(x, dtype), dy=gin(dy, dtype)), mask)
    outs = dict(dw=Guarded(25 * C, F32), dbias=Guarded(C, F32),
                ws=Guarded(U.wgrad_ws_floats(N, H, W, C), F32, prefill='a5'))
    run(what, lambda: L.load().passl_hip_dwconv5_masked_bwd_weight(
        ptr(ins['x']), ptr(ins['dy']), ptr(ins.get('mask')), ptr(outs['dw']), ptr(outs['dbias']), ptr(outs['ws']),
        outs['ws'].view.numel(), N, H, W, C, grid[0], grid[1], L.dt(dtype), L.stream()), ins, outs)
    return host(outs['dw'], (C, 1, 5, 5)), host(outs['dbias'], (C,))


def poisoned(t, keep):
    """t with NaN at the removed pixels: the kernels must not let a removed pixel of x reach any result."""
    return torch.where(keep.float().expand_as(t) == 0, torch.full_like(t, float('nan')), t)


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv5_masked_fwd(case):
    d, (shape, kind, dtype) = U.conv_data(case), case
    y = conv_fwd(poisoned(d['x'], d['keep']), d['w'], d['bias'], d['mask'], d['grid'], shape[:4], dtype)
    check(U.case_id(case), 'y', 'dwconv5_masked_fwd', U.usage(y, *U.fwd_ref(case)))
    if kind == 'removed':
        assert bits_equal(y, d['bias'].expand_as(y), dtype) == 0, 'all patches removed: y is not the bias bit for bit'


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv5_masked_bwd_data(case):
    d, (shape, kind, dtype) = U.conv_data(case), case
    dx = conv_bwd_data(d['dy'], d['w'], d['mask'], d['grid'], shape[:4], dtype)
    check(U.case_id(case), 'dx', 'dwconv5_masked_bwd_data', U.usage(dx, *U.bwd_data_ref(case)))
    removed = (d['keep'].float().expand_as(dx) == 0)
    assert bits_equal(torch.where(removed, dx, torch.zeros_like(dx)), torch.zeros_like(dx), dtype) == 0, \
        'dx at a removed pixel is not +0 bit for bit'


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv5_masked_bwd_weight(case):
    d, (shape, kind, dtype) = U.conv_data(case), case
    dw, db = conv_bwd_weight(poisoned(d['x'], d['keep']), d['dy'], d['mask'], d['grid'], shape[:4], dtype)
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    check(U.case_id(case), 'dw', 'dwconv5_masked_bwd_weight', U.usage(dw, dw64, dw_bound))
    check(U.case_id(case), 'dbias', 'dwconv5_masked_bwd_weight', U.usage(db, db64, db_bound))
    if kind == 'removed':
        assert bits_equal(dw, torch.zeros_like(dw), F32) == 0, 'all patches removed: dw is not +0 bit for bit'


# ------------------------------------------------------------------------------------------------ exact cases
EXACT_SHAPE = (2, 18, 20, 8)          # crosses the 16-column tile edge and the 8- and 16-row tile edges
EXACT_G = 2


def exact_mask(kind):
    N, H, W, C = EXACT_SHAPE
    grid = (H // EXACT_G, W // EXACT_G)
    mask = U.make_mask(kind, N, grid[0], grid[1], torch.Generator().manual_seed(29))
    return mask, grid, U.keep_map(mask, N, H, W, EXACT_G).float()


@pytest.mark.parametrize('dtype', U.DTYPES, ids=lambda d: U.DTNAME[d])
@pytest.mark.parametrize('kind', ('null', 'checker'))
def test_delta_filters_shift_exactly(kind, dtype):
    """For each of the 25 taps a delta filter makes y the zero-filled shift of keep * x and dx keep times the opposite
    shift of dy, bit for bit.  Channel c of launch k carries tap (k + c) % 25, so a launch mixes eight taps."""
    N, H, W, C = EXACT_SHAPE
    mask, grid, keep = exact_mask(kind)
    gen = torch.Generator().manual_seed(17)
    x = U.rnd(torch.randn(EXACT_SHAPE, generator=gen), dtype)
    dy = U.rnd(torch.randn(EXACT_SHAPE, generator=gen), dtype)
    zero = torch.zeros(C)
    for k in range(25):
        w = torch.zeros(C, 25)
        taps = [(k + c) % 25 for c in range(C)]
        w[torch.arange(C), torch.tensor(taps)] = 1.0
        y = conv_fwd(x, w, zero, mask, grid, EXACT_SHAPE, dtype)
        dx = conv_bwd_data(dy, w, mask, grid, EXACT_SHAPE, dtype)
        for c, t in enumerate(taps):
            r, s = divmod(t, 5)
            assert torch.equal(y[..., c], U.shifted(x * keep, r, s)[..., c]), 'y, tap (%d, %d)' % (r, s)
            assert torch.equal(dx[..., c], (U.shifted(dy, 4 - r, 4 - s) * keep)[..., c]), 'dx, tap (%d, %d)' % (r, s)


@pytest.mark.parametrize('dtype', U.DTYPES, ids=lambda d: U.DTNAME[d])
@pytest.mark.parametrize('kind', ('null', 'checker'))
@pytest.mark.parametrize('pixel', ((0, 0, 0), (1, 17, 19), (0, 0, 7), (1, 9, 0), (0, 8, 16), (1, 4, 10)),
                         ids=lambda p: 'n%d-p%d-q%d' % p)
def test_one_hot_dy_picks_x_exactly(pixel, kind, dtype):
    """dy = 1 at one pixel (corners, edges, tile edges, interior): dw[c, 0, r, s] is the matching keep * x value or
    zero, and dbias is 1, bit for bit."""
    N, H, W, C = EXACT_SHAPE
    n, p, q = pixel
    mask, grid, keep = exact_mask(kind)
    x = U.rnd(torch.randn(EXACT_SHAPE, generator=torch.Generator().manual_seed(23)), dtype)
    dy = torch.zeros(EXACT_SHAPE)
    dy[n, p, q] = 1.0
    dw, db = conv_bwd_weight(x, dy, mask, grid, EXACT_SHAPE, dtype)
    xk = x * keep
    want = torch.zeros(C, 1, 5, 5)
    for r in range(5):
        for s in range(5):
            h, w = p + r - 2, q + s - 2
            if 0 <= h < H and 0 <= w < W:
                want[:, 0, r, s] = xk[n, h, w]
    assert torch.equal(dw, want)
    assert torch.equal(db, torch.ones(C))


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize('case', U.GATHER_CASES, ids=U.pair_id)
def test_patch_gather_is_the_restatement(case):
    (B, Hm, Wm, p, C, K), dtype = case
    d = U.gather_data(case)
    ins = dict(x=gin(d['x'], dtype), ids_keep=gin(d['ids_keep'], I32))
    out = Guarded(B * K * p * p * C, dtype)
    run(U.pair_id(case), lambda: L.load().passl_hip_patch_gather_fwd(
        ptr(ins['x']), ptr(ins['ids_keep']), ptr(out), B, K, Hm, Wm, p, C, L.dt(dtype), L.stream()), ins, dict(out=out))
    want = U.gather_restated(d['x'], d['ids_keep'], Hm, Wm, p)
    assert bits_equal(host(out, want.shape), want, dtype) == 0

    ins = dict(dout=gin(d['dout'], dtype), ids_restore=gin(d['ids_restore'], I32))
    dx = Guarded(d['x'].numel(), dtype)
    run(U.pair_id(case), lambda: L.load().passl_hip_patch_gather_bwd(
        ptr(ins['dout']), ptr(ins['ids_restore']), ptr(dx), B, K, Hm, Wm, p, C, L.dt(dtype), L.stream()), ins,
        dict(dx=dx))
    want = U.gather_bwd_restated(d['dout'], d['ids_restore'], K, Hm, Wm, p, C)
    assert bits_equal(host(dx, want.shape), want, dtype) == 0


# ------------------------------------------------------------------------------------------------ tokens
@pytest.mark.parametrize('case', U.TOKEN_CASES, ids=U.pair_id)
def test_pos_gather_add_is_the_restatement(case):
    (B, Ln, K, D), dtype = case
    d = U.token_data(case)
    ins = dict(x=gin(d['x'], dtype), pos=gin(d['pos'], F32), ids_keep=gin(d['ids_keep'], I32))
    out = Guarded(B * K * D, dtype)
    run(U.pair_id(case), lambda: L.load().passl_hip_tokens_pos_gather_add(
        ptr(ins['x']), ptr(ins['pos']), ptr(ins['ids_keep']), ptr(out), B, Ln, K, D, L.dt(dtype), L.stream()), ins,
        dict(out=out))
    want = U.pos_gather_add_restated(d['x'], d['pos'], d['ids_keep'], dtype)
    assert bits_equal(host(out, want.shape), want.float(), dtype) == 0

    # the backward ADDS to the table's gradient: it starts from a known value
    start = torch.randn(Ln, D, generator=torch.Generator().manual_seed(41))
    ins = dict(dout=gin(d['dout_k'], dtype), ids_restore=gin(d['ids_restore'], I32))
    dpos = Guarded(Ln * D, F32, fill=start)
    run(U.pair_id(case), lambda: L.load().passl_hip_tokens_pos_gather_add_bwd(
        ptr(ins['dout']), ptr(ins['ids_restore']), ptr(dpos), B, Ln, K, D, L.dt(dtype), L.stream()), ins,
        dict(dpos=dpos))
    want = U.pos_gather_add_bwd_restated(d['dout_k'], d['ids_restore'], K, start)
    assert bits_equal(host(dpos, want.shape), want, F32) == 0


@pytest.mark.parametrize('case', U.TOKEN_CASES, ids=U.pair_id)
def test_unshuffle_is_the_restatement(case):
    (B, Ln, K, D), dtype = case
    d = U.token_data(case)
    ins = dict(x=gin(d['x'], dtype), mask_token=gin(d['mask_token'], F32), pos=gin(d['pos'], F32),
               ids_restore=gin(d['ids_restore'], I32))
    out = Guarded(B * Ln * D, dtype)
    run(U.pair_id(case), lambda: L.load().passl_hip_tokens_unshuffle(
        ptr(ins['x']), ptr(ins['mask_token']), ptr(ins['pos']), ptr(ins['ids_restore']), ptr(out), B, Ln, K, D,
        L.dt(dtype), L.stream()), ins, dict(out=out))
    want = U.unshuffle_restated(d['x'], d['mask_token'], d['pos'], d['ids_restore'], dtype)
    assert bits_equal(host(out, want.shape), want.float(), dtype) == 0

    # the backward ADDS to the mask token's gradient: it starts from a known value
    start = torch.arange(D, dtype=F32) * 0.25 - 3
    ins = dict(dout=gin(d['dout_l'], dtype), ids_keep=gin(d['ids_keep'], I32), ids_restore=gin(d['ids_restore'], I32))
    outs = dict(dx=Guarded(B * K * D, dtype), dmask=Guarded(D, F32, fill=start),
                ws=Guarded(1024 * D, F32, prefill='a5'))
    before = {n: g.raw() for n, g in ins.items()}
    fn = lambda: L.load().passl_hip_tokens_unshuffle_bwd(                                               # noqa: E731
        ptr(ins['dout']), ptr(ins['ids_keep']), ptr(ins['ids_restore']), ptr(outs['dx']), ptr(outs['dmask']), B, Ln, K,
        D, L.dt(dtype), ptr(outs['ws']), outs['ws'].view.numel(), L.stream())
    assert fn() == 0
    torch.cuda.synchronize()
    first = {n: outs[n].raw() for n in ('dx', 'dmask')}
    outs['dx'].reset()
    outs['dmask'].reset()
    assert fn() == 0
    torch.cuda.synchronize()
    for n in ('dx', 'dmask'):
        assert torch.equal(outs[n].raw(), first[n]), '%s differs between two runs of the same launch' % n
    for n, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), 'a guard region of %s was written' % n
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), 'the input %s was modified' % n
    assert outs['dx'].unwritten() == 0
    dx, dm64, dm_bound = U.unshuffle_bwd_ref(d['dout_l'], d['ids_keep'], d['ids_restore'])
    assert bits_equal(host(outs['dx'], dx.shape), dx, dtype) == 0
    # one more fp32 addition (onto the start value) than the sum the bound covers: its rounding is at most E times
    # the magnitude of its result, which is at most |start| + |sum| + the sum's own error
    got = host(outs['dmask'], (D,)).double() - start.double()
    bound = dm_bound + U.E * (dm64.abs() + start.double().abs() + dm_bound)
    check(U.pair_id(case), 'dmask_token', 'tokens_unshuffle_bwd', U.usage(got, dm64, bound))


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize('case', U.LOSS_CASES, ids=U.loss_id)
def test_loss_without_a_class_row_is_the_loss_with_one(case):
    """passl_hip_tokens_mae_loss_* on pred [B, L, P] against passl_hip_mae_loss_* on the same rows behind a class row
    (tested by the MAE suites): dpred bit for bit; the loss is the fp32 sum of the same per-patch terms in another
    order, and two such sums of n non-negative terms differ by at most 2 (n + 1) E times their value."""
    (B, C, H, W, p), norm = case
    d = U.loss_data(case)
    Ln, P = d['mask'].shape[1], p * p * C
    with_cls = torch.cat([torch.full((B, 1, P), 7.0), d['pred']], 1)
    lib = L.load()
    ins = dict(img=gin(d['img'], F32), pred=gin(d['pred'], F32), mask=gin(d['mask'], F32), gscale=gin(torch.tensor([1.7]), F32))
    outs = dict(loss=Guarded(1, F32), ws=Guarded(B * Ln, F32, prefill='a5'))
    run(U.loss_id(case), lambda: lib.passl_hip_tokens_mae_loss_fwd(
        ptr(ins['img']), ptr(ins['pred']), ptr(ins['mask']), ptr(outs['loss']), B, C, H, W, p, int(norm), d['denom'],
        ptr(outs['ws']), B * Ln, L.stream()), ins, outs)
    dpred = Guarded(B * Ln * P, F32)
    run(U.loss_id(case), lambda: lib.passl_hip_tokens_mae_loss_bwd(
        ptr(ins['img']), ptr(ins['pred']), ptr(ins['mask']), ptr(ins['gscale']), ptr(dpred), B, C, H, W, p, int(norm),
        d['denom'], L.stream()), ins, dict(dpred=dpred))
    ref_in = dict(pred=gin(with_cls, F32))
    ref_loss, ref_ws, ref_d = Guarded(1, F32), Guarded(B * (Ln + 1), F32, prefill='a5'), Guarded(B * (Ln + 1) * P, F32)
    assert lib.passl_hip_mae_loss_fwd(ptr(ins['img']), ptr(ref_in['pred']), ptr(ins['mask']), ptr(ref_loss), B, C, H, W,
                                      p, int(norm), d['denom'], ptr(ref_ws), B * (Ln + 1), L.stream()) == 0
    assert lib.passl_hip_mae_loss_bwd(ptr(ins['img']), ptr(ref_in['pred']), ptr(ins['mask']), ptr(ins['gscale']),
                                      ptr(ref_d), B, C, H, W, p, int(norm), d['denom'], L.stream()) == 0
    torch.cuda.synchronize()
    want = host(ref_d, (B, Ln + 1, P))[:, 1:]
    assert bits_equal(host(dpred, (B, Ln, P)), want, F32) == 0
    terms, ref_terms = host(outs['ws'], (B, Ln)), host(ref_ws, (B, Ln + 1))[:, 1:]
    assert bits_equal(terms, ref_terms, F32) == 0, 'the per-patch terms differ'
    a, b = float(host(outs['loss'], (1,))), float(host(ref_loss, (1,)))
    bound = 2 * (B * (Ln + 1) + 1) * U.E * max(a, b)
    fig('tokens_mae_loss_fwd', U.loss_id(case), abs(a - b) / bound if bound else 0.0)
    assert abs(a - b) <= bound and a > 0
    # and against the definition in float64 (a coarse guard against both being wrong together)
    tgt = d['img'].double().view(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, Ln, P)
    if norm:
        tgt = (tgt - tgt.mean(-1, keepdim=True)) / (tgt.var(-1, keepdim=True) + 1e-6) ** .5
    l64 = float(((((d['pred'].double() - tgt) ** 2).mean(-1)) * d['mask'].double()).sum() / d['denom'])
    assert abs(a - l64) <= 1e-4 * abs(l64)


def test_zzz_report_the_largest_share_of_an_allowance():
    """Runs last in this file: the largest share of its bound that any element of each kernel used."""
    for kernel, ratio in sorted(WORST.items()):
        print('FIG largest share of the bound: %s %.4f' % (kernel, ratio))
    assert all(r <= 1 for r in WORST.values())
