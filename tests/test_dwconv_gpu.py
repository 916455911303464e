"""The ConvNeXt block kernels (csrc/dwconv.hip) against float64 references, element by element, over the case tables of
convnext_util.py (which has the derivation of every bound).

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must
survive; outputs start as NaN (slabs: as 0xA5 bytes) and every element must have been written; every input must come
back bit-identical; a second run of every launch must give the same bits (dw, dbias, dgamma included: no atomics).
"""
import pytest
import torch

import convnext_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32 = torch.float32


def fig(kernel, what, ratio):
    print('FIG %s %s %.4f of the bound' % (kernel, what, ratio))


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


def conv_fwd(x, w, bias, shape, dtype, what='dwconv7_fwd'):
    N, H, W, C = shape
    ins = dict(x=gin(x, dtype), w=gin(w, F32), bias=gin(bias, F32))
    y = Guarded(x.numel(), dtype)
    run(what, lambda: L.load().passl_hip_dwconv7_fwd(ptr(ins['x']), ptr(ins['w']), ptr(ins['bias']), ptr(y), N, H, W, C,
                                                    L.dt(dtype), L.stream()), ins, dict(y=y))
    return host(y, shape)


def conv_bwd_data(dy, w, add, shape, dtype, what='dwconv7_bwd_data'):
    N, H, W, C = shape
    ins = dict(dy=gin(dy, dtype), w=gin(w, F32))
    if add is not None:
        ins['add'] = gin(add, dtype)
    dx = Guarded(dy.numel(), dtype)
    run(what, lambda: L.load().passl_hip_dwconv7_bwd_data(ptr(ins['dy']), ptr(ins['w']), ptr(ins.get('add')), ptr(dx),
                                                         N, H, W, C, L.dt(dtype), L.stream()), ins, dict(dx=dx))
    return host(dx, shape)


def conv_bwd_weight(x, dy, shape, dtype, what='dwconv7_bwd_weight'):
    N, H, W, C = shape
    ins = dict(x=gin(x, dtype), dy=gin(dy, dtype))
    outs = dict(dw=Guarded(49 * C, F32), dbias=Guarded(C, F32),
                ws=Guarded(U.wgrad_ws_floats(N, H, W, C), F32, prefill='a5'))
    run(what, lambda: L.load().passl_hip_dwconv7_bwd_weight(
        ptr(ins['x']), ptr(ins['dy']), ptr(outs['dw']), ptr(outs['dbias']), ptr(outs['ws']), outs['ws'].view.numel(),
        N, H, W, C, L.dt(dtype), L.stream()), ins, outs)
    return host(outs['dw'], (C, 1, 7, 7)), host(outs['dbias'], (C,))


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv7_fwd(case):
    d, (shape, _, dtype) = U.conv_data(case), case
    y = conv_fwd(d['x'], d['w'], d['bias'], shape, dtype)
    check(U.case_id(case), 'y', 'dwconv7_fwd', U.usage(y, *U.fwd_ref(case)))


@pytest.mark.parametrize('with_add', (False, True), ids=('noadd', 'add'))
@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv7_bwd_data(case, with_add):
    d, (shape, _, dtype) = U.conv_data(case), case
    dx = conv_bwd_data(d['dy'], d['w'], d['add'] if with_add else None, shape, dtype)
    check(U.case_id(case), 'dx', 'dwconv7_bwd_data', U.usage(dx, *U.bwd_data_ref(case, with_add)))


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_dwconv7_bwd_weight(case):
    d, (shape, _, dtype) = U.conv_data(case), case
    dw, db = conv_bwd_weight(d['x'], d['dyw'], shape, dtype)
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    check(U.case_id(case), 'dw', 'dwconv7_bwd_weight', U.usage(dw, dw64, dw_bound))
    check(U.case_id(case), 'dbias', 'dwconv7_bwd_weight', U.usage(db, db64, db_bound))


# ------------------------------------------------------------------------------------------------ exact cases
EXACT_SHAPE = (2, 18, 20, 8)          # crosses the 16-column tile edge and the 8- and 16-row tile edges


@pytest.mark.parametrize('dtype', U.DTYPES, ids=lambda d: U.DTNAME[d])
def test_delta_filters_shift_exactly(dtype):
    """For each of the 49 taps a delta filter makes y the zero-filled shift of x and dx the opposite shift of dy, bit
    for bit.  Channel c of launch k carries tap (k + c) % 49, so a launch mixes eight taps."""
    N, H, W, C = EXACT_SHAPE
    gen = torch.Generator().manual_seed(17)
    x = U.rnd(torch.randn(EXACT_SHAPE, generator=gen), dtype)
    dy = U.rnd(torch.randn(EXACT_SHAPE, generator=gen), dtype)
    zero = torch.zeros(C)
    for k in range(49):
        w = torch.zeros(C, 49)
        taps = [(k + c) % 49 for c in range(C)]
        w[torch.arange(C), torch.tensor(taps)] = 1.0
        y = conv_fwd(x, w, zero, EXACT_SHAPE, dtype)
        dx = conv_bwd_data(dy, w, None, EXACT_SHAPE, dtype)
        for c, t in enumerate(taps):
            r, s = divmod(t, 7)
            assert torch.equal(y[..., c], U.shifted(x, r, s)[..., c]), 'y, tap (%d, %d)' % (r, s)
            assert torch.equal(dx[..., c], U.shifted(dy, 6 - r, 6 - s)[..., c]), 'dx, tap (%d, %d)' % (r, s)


@pytest.mark.parametrize('dtype', U.DTYPES, ids=lambda d: U.DTNAME[d])
@pytest.mark.parametrize('pixel', ((0, 0, 0), (1, 17, 19), (0, 0, 7), (1, 9, 0), (0, 8, 16), (1, 4, 10)),
                         ids=lambda p: 'n%d-p%d-q%d' % p)
def test_one_hot_dy_picks_x_exactly(pixel, dtype):
    """dy = 1 at one pixel (corners, edges, tile edges, interior): dw[c, 0, r, s] is the matching x value or zero, and
    dbias is 1, bit for bit."""
    N, H, W, C = EXACT_SHAPE
    n, p, q = pixel
    x = U.rnd(torch.randn(EXACT_SHAPE, generator=torch.Generator().manual_seed(23)), dtype)
    dy = torch.zeros(EXACT_SHAPE)
    dy[n, p, q] = 1.0
    dw, db = conv_bwd_weight(x, dy, EXACT_SHAPE, dtype)
    want = torch.zeros(C, 1, 7, 7)
    for r in range(7):
        for s in range(7):
            h, w = p + r - 3, q + s - 3
            if 0 <= h < H and 0 <= w < W:
                want[:, 0, r, s] = x[n, h, w]
    assert torch.equal(dw, want)
    assert torch.equal(db, torch.ones(C))


# ------------------------------------------------------------------------------------------------ layer scale
def ls_operands(case):
    """The case's operands with NaN in the rows a dropped sample must not read."""
    (B, T, C), table, dtype = case
    d = U.ls_data(case)
    branch, dy = d['branch'].clone(), d['dy'].clone()
    if table:
        dropped = (d['keep'] == 0).repeat_interleave(T)
        branch[dropped] = float('nan')
        dy[dropped] = float('nan')
    return d, branch, dy


@pytest.mark.parametrize('case', U.LS_CASES, ids=U.ls_case_id)
def test_layer_scale_add_fwd_is_the_restatement(case):
    (B, T, C), table, dtype = case
    d, branch, _ = ls_operands(case)
    ins = dict(branch=gin(branch, dtype), residual=gin(d['residual'], dtype), gamma=gin(d['gamma'], F32))
    if table:
        ins['keep'] = gin(d['keep'], F32)
    out = Guarded(B * T * C, dtype)
    run(U.ls_case_id(case), lambda: L.load().passl_hip_layer_scale_add_fwd(
        ptr(ins['branch']), ptr(ins['residual']), ptr(ins['gamma']), ptr(ins.get('keep')), U.KEEP_PROB, ptr(out),
        B, T, C, L.dt(dtype), L.stream()), ins, dict(out=out))
    want = U.layer_scale_restated(d['branch'], d['residual'], d['gamma'], d['keep'], U.KEEP_PROB, T, dtype)
    got = out.view.cpu().view(B * T, C)
    bits = torch.int32 if dtype == F32 else torch.int16
    diff = int((got.view(bits) != want.view(bits)).sum())
    assert diff == 0, '%d of %d elements differ from the restatement' % (diff, got.numel())


@pytest.mark.parametrize('case', U.LS_CASES, ids=U.ls_case_id)
def test_layer_scale_add_bwd(case):
    (B, T, C), table, dtype = case
    d, branch, dy = ls_operands(case)
    ins = dict(dy=gin(dy, dtype), branch=gin(branch, dtype), gamma=gin(d['gamma'], F32))
    if table:
        ins['keep'] = gin(d['keep'], F32)
    outs = dict(dbranch=Guarded(B * T * C, dtype), dgamma=Guarded(C, F32),
                ws=Guarded(U.ls_bwd_ws_floats(B * T, C), F32, prefill='a5'))
    run(U.ls_case_id(case), lambda: L.load().passl_hip_layer_scale_add_bwd(
        ptr(ins['dy']), ptr(ins['branch']), ptr(ins['gamma']), ptr(ins.get('keep')), U.KEEP_PROB, ptr(outs['dbranch']),
        ptr(outs['dgamma']), ptr(outs['ws']), outs['ws'].view.numel(), B, T, C, L.dt(dtype), L.stream()), ins, outs)
    db64, db_bound, dg64, dg_bound = U.ls_bwd_ref(case)
    check(U.ls_case_id(case), 'dbranch', 'layer_scale_add_bwd', U.usage(host(outs['dbranch'], (B * T, C)), db64, db_bound))
    check(U.ls_case_id(case), 'dgamma', 'layer_scale_add_bwd', U.usage(host(outs['dgamma'], (C,)), dg64, dg_bound))
