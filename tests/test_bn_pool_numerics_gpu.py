"""BatchNorm and pooling kernels (csrc/bn.hip, layout_pool.hip, stem_pool.hip) against float64 references, element by
element, over the shape / kind tables of bn_pool_util.py (which has the derivation of every bound).

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must
survive; outputs start as NaN (index bytes, mask bytes and slabs: as 0xA5 bytes) and every element must have been
written; every input must come back bit-identical; a second run of every launch must give the same bits.  The
streaming kernels run under bn_stream_unroll = 0, 2, 4, 8 and the fused stem backward under stem_pool_form = 0, 1:
every form meets the bounds on its own and all forms of a launch give the same bits.

Worst error on an MI355X in units of the element's own bound, over all cases and flags (a record of one run, not a
pass criterion; bf16 figures near 1 are the store rounding, which the u |value| term of the bound is there for):
  kernel                       fp32    bf16   worst case (fp32 / bf16)
  bn_stats slab                0.455   0.417  5x4096-const / 33x2048-const
  bn_finalize mean             0.323   0.319  5x4096-plain / 33x2048-mixed
  bn_apply                     0.466   0.996  300x256-plain, residual / 33x2048-mixed
  bn_bwd_reduce slab           0.430   0.362  5x8n4-plain / 5x8n4-plain
  bn_bwd_finalize dbeta,dgamma 0.316   0.300  5x4096-const / 5x8n4-const
  bn_bwd_apply                 0.550   0.996  5x4096-plain, mask 3 / 300x256-const, mask 3
  maxpool3x3s2_fwd             exact   exact
  maxpool3x3s2_bwd             0.562   0.996  3x7x9x64-negative / 2x8x8x256-negative
  avgpool_fwd                  0.351   0.983  3x7x24-negative / 2x49x2048-negative
  avgpool_bwd                  0.835   0.919  3x7x24-plain / 2x49x2048-negative
  bn_relu_maxpool_fwd y        0.250   0.996  2x9x8x256-ties / 2x9x8x256-negative
  bn_relu_maxpool_bwd_reduce   0.089   0.089  3x17x21x64-ties, second form (both)
  bn_relu_maxpool_bwd_apply    0.484   0.996  3x17x21x64-ties / 4x32x32x64-negative
All forms of a launch (bn_stream_unroll 0 / 2 / 4 / 8, stem_pool_form 0 / 1 for dx) gave the same bits in every case.
Elements at the recomputed-mask boundary (mask source 2, |pre64| <= B_apply; cap 0.1 %): 0 in 84 of the 88 cases
that have the mask (64 BatchNorm, 24 stem), else 33x2048-mixed-fp32 0.036 %, 5x4096-mixed-fp32 0.034 %,
300x256-mixed-fp32 0.022 %, 515x64-mixed-fp32 0.018 %.  The file's 201 tests take 6 s.
"""
import functools

import pytest
import torch

import bn_pool_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32, U8 = torch.float32, torch.uint8
DEFAULTS = {'bn_stream_unroll': 4, 'stem_pool_form': 1}
APPLY_FLAGS = [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]        # relu, mask, residual
BWD_FLAGS = [(0, 1), (1, 1), (2, 1), (3, 1), (0, 0), (2, 0)]                            # mask source, dres


@pytest.fixture
def options():
    """Sets bn_stream_unroll / stem_pool_form through the option table; both are back at their defaults afterwards."""
    def select(**opts):
        for name, default in DEFAULTS.items():
            L.set_option(name, opts.get(name, default))
    yield select
    select()
    for name, default in DEFAULTS.items():
        assert L.get_option(name) == default


def fig(kernel, what, ratio, unit='of the bound'):
    print('FIG %s %s %.4f %s' % (kernel, what, ratio, unit))


def gin(t, dtype):
    return Guarded(t.numel(), dtype, fill=t)


def run(what, fn, ins, outs, written=None, unchecked=()):
    """Launches fn() twice on the guarded operands.  Asserts: the same output bits both times, every guard intact,
    every input unchanged, every output element written (`written`: only that many leading elements of an output;
    `unchecked`: outputs whose every bit pattern is a valid result)."""
    before = {n: g.raw() for n, g in ins.items()}
    fn()
    torch.cuda.synchronize()
    first = {n: g.raw() for n, g in outs.items()}
    for g in outs.values():
        g.reset()
    fn()
    torch.cuda.synchronize()
    for n, g in outs.items():
        assert torch.equal(g.raw(), first[n]), '%s: %s differs between two runs of the same launch' % (what, n)
    for n, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), '%s: a guard region of %s was written' % (what, n)
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), '%s: the input %s was modified' % (what, n)
    for n, g in outs.items():
        if n not in unchecked:
            left = g.unwritten((written or {}).get(n))
            assert left == 0, '%s: %d elements of %s were not written' % (what, left, n)


def check(what, tensor, kernel, ratio_idx):
    fig(kernel, what, ratio_idx[0])
    msg = U.verdict(what, tensor, *ratio_idx)
    assert msg is None, msg


def partial_floats(nb, C, shifted):
    return int(L.load().passl_hip_bn_partial_floats(nb, C, shifted))


def stats_and_finalize(what, x, gamma, beta, dtype, nblocks=None):
    """passl_hip_bn_stats (slab judged) and passl_hip_bn_finalize (finite, guards) -> the device's mean, invstd,
    scale, shift as CPU fp32 tensors."""
    lib = L.load()
    M, C = x.shape
    nb, rows = U.bn_slabs(M, C, nblocks)
    gx = gin(x, dtype)
    part = Guarded(partial_floats(nb, C, 1), F32, prefill='a5')
    run(what + ' bn_stats', lambda: L.check(lib.passl_hip_bn_stats(
        L.ptr(gx.view), L.ptr(part.view), M, C, nb, L.dt(dtype), L.stream()), 'bn_stats'),
        {'x': gx}, {'partial': part}, written={'partial': nb * C * 3})
    sums, shift = U.split_stats_slab(part.view.cpu(), nb, C)
    shift_ref, sums_ref, bound = U.stats_ref(x, nb, rows)
    assert torch.equal(shift.view(torch.int32), shift_ref.view(torch.int32)), \
        '%s: a slab shift of bn_stats is not the first row of its slab' % what
    check(what, 'bn_stats slab [slab, channel, (S1, S2)]', 'bn_stats-' + U.DTNAME[dtype], U.usage(sums, sums_ref, bound))
    ggamma, gbeta = gin(gamma, F32), gin(beta, F32)
    outs = {n: Guarded(C, F32) for n in ('mean', 'invstd', 'scale', 'shift')}
    run(what + ' bn_finalize', lambda: L.check(lib.passl_hip_bn_finalize(
        L.ptr(part.view), nb, M, C, rows, L.ptr(ggamma.view), L.ptr(gbeta.view), None, None, 0.9, U.EPS,
        L.ptr(outs['mean'].view), L.ptr(outs['invstd'].view), L.ptr(outs['scale'].view), L.ptr(outs['shift'].view),
        L.stream()), 'bn_finalize'), {'partial': part, 'gamma': ggamma, 'beta': gbeta}, outs)
    k = {n: g.view.cpu() for n, g in outs.items()}
    check(what + ' bn_finalize', 'mean', 'bn_finalize_mean-' + U.DTNAME[dtype], U.mean_usage(k['mean'], x, bound))
    return k


@functools.lru_cache(maxsize=None)
def bn_constants(case):
    (M, C, nblocks), kind, dtype = case
    d = U.bn_data(case)
    return stats_and_finalize(U.case_id(case), d['x'], d['gamma'], d['beta'], dtype, nblocks)


def stream_forms(C):
    """bn_stream_unroll values to run: all four where the tile kernels are eligible, else the default alone (such a C
    takes the grid-stride kernels whatever the option says)."""
    return (0, 2, 4, 8) if U.tile_form(C) else (DEFAULTS['bn_stream_unroll'],)


BN_IDS = [U.case_id(c) for c in U.BN_CASES]


@pytest.mark.parametrize('case', U.BN_CASES, ids=BN_IDS)
def test_bn_stats_finalize_apply(case, options):
    (M, C, _), kind, dtype = case
    d = U.bn_data(case)
    what, dn = U.case_id(case), U.DTNAME[dtype]
    k = bn_constants(case)
    lib = L.load()
    gx, gres, gsc, gsh = gin(d['x'], dtype), gin(d['res'], dtype), gin(k['scale'], F32), gin(k['shift'], F32)
    for relu, want_mask, with_res in APPLY_FLAGS:
        base = None
        res = d['res'] if with_res else None
        for form in stream_forms(C):
            options(bn_stream_unroll=form)
            tag = '%s bn_apply (U %d, relu %d, mask %d, res %d)' % (what, form, relu, want_mask, with_res)
            ins = {'x': gx, 'scale': gsc, 'shift': gsh}
            if with_res:
                ins['res'] = gres
            outs = {'z': Guarded(M * C, dtype)}
            if want_mask:
                outs['mask'] = Guarded(M * C // 8, U8)
            run(tag, lambda: L.check(lib.passl_hip_bn_apply(
                L.ptr(gx.view), L.ptr(gsc.view), L.ptr(gsh.view), L.ptr(gres.view) if with_res else None,
                L.ptr(outs['z'].view), L.ptr(outs['mask'].view) if want_mask else None, M, C, relu, L.dt(dtype),
                L.stream()), 'bn_apply'), ins, outs, unchecked=('mask',))
            raw = [g.raw() for g in outs.values()]
            if base is None or not all(torch.equal(a, b) for a, b in zip(raw, base)):
                z = outs['z'].view.float().cpu().view(M, C)
                check(tag, 'z', 'bn_apply-' + dn, U.apply_usage(z, d['x'], k['scale'], k['shift'], res, relu, dtype))
                if want_mask:
                    n, at = U.mask_mismatch(outs['mask'].view.cpu(), z)
                    assert n == 0, '%s: %d mask bytes differ from (z > 0), first at byte %d' % (tag, n, at)
            assert base is None or all(torch.equal(a, b) for a, b in zip(raw, base)), \
                '%s: the bits differ from those of U %d' % (tag, stream_forms(C)[0])
            base = base or raw


@pytest.mark.parametrize('case', U.BN_CASES, ids=BN_IDS)
def test_bn_bwd_reduce_finalize_apply(case, options):
    (M, C, nblocks), kind, dtype = case
    d = U.bn_data(case)
    x, dz = d['x'], d['dz']
    what, dn = U.case_id(case), U.DTNAME[dtype]
    k = bn_constants(case)
    lib = L.load()
    nb, rows = U.bn_slabs(M, C, nblocks)
    gx, gdz = gin(x, dtype), gin(dz, dtype)
    gk = {n: gin(t, F32) for n, t in k.items()}
    ggamma = gin(d['gamma'], F32)
    m2, amb2 = U.recomputed_mask(x, k['scale'], k['shift'])
    share = float(amb2.double().mean())
    fig('mode2-share', what, 100 * share, '% of the elements')
    assert share <= U.AMBIGUOUS_CAP, '%s: %.3f %% of the elements are at the recomputed-mask boundary' % (what, 100 * share)
    source = {0: (None, None, None), 1: (d['zsrc'] > 0, None, gin(d['zsrc'], dtype)), 2: (m2, amb2, None),
              3: (U.unpack_mask(d['maskbits'], x.shape), None, gin(d['maskbits'], U8))}
    zero = torch.zeros_like(dz)
    coefs = {}
    for relu, (mask, amb, gz) in source.items():
        tag = '%s bn_bwd_reduce (relu %d)' % (what, relu)
        ins = {'dz': gdz, 'x': gx, 'mean': gk['mean'], 'invstd': gk['invstd']}
        if gz is not None:
            ins['z'] = gz
        if relu == 2:
            ins.update(scale=gk['scale'], shift=gk['shift'])
        part = Guarded(partial_floats(nb, C, 0), F32, prefill='a5')
        run(tag, lambda: L.check(lib.passl_hip_bn_bwd_reduce(
            L.ptr(gdz.view), L.ptr(gz.view) if gz is not None else None, L.ptr(gx.view), L.ptr(gk['mean'].view),
            L.ptr(gk['invstd'].view), L.ptr(gk['scale'].view) if relu == 2 else None,
            L.ptr(gk['shift'].view) if relu == 2 else None, L.ptr(part.view), M, C, nb, relu, L.dt(dtype), L.stream()),
            'bn_bwd_reduce'), ins, {'partial': part}, written={'partial': nb * C * 2})
        g = dz if mask is None else torch.where(mask, dz, zero)
        gother = None if amb is None else torch.where(mask, zero, dz)
        sums_ref, bound = U.reduce_ref(g, x, k['mean'], k['invstd'], U.row_groups(M, nb, rows), amb, gother)
        check(tag, 'slab [slab, channel, (sum g, sum g xhat)]', 'bn_bwd_reduce-' + dn,
              U.usage(part.view.cpu()[:nb * C * 2].view(nb, C, 2), sums_ref, bound))
        outs = {'dgamma': gin(torch.zeros(C), F32), 'dbeta': gin(torch.zeros(C), F32), 'coef': Guarded(3 * C, F32)}
        run('%s bn_bwd_finalize (relu %d)' % (what, relu), lambda: L.check(lib.passl_hip_bn_bwd_finalize(
            L.ptr(part.view), nb, M, C, L.ptr(ggamma.view), L.ptr(gk['mean'].view), L.ptr(gk['invstd'].view),
            L.ptr(outs['dgamma'].view), L.ptr(outs['dbeta'].view), L.ptr(outs['coef'].view), L.stream()),
            'bn_bwd_finalize'), {'partial': part, 'gamma': ggamma, 'mean': gk['mean'], 'invstd': gk['invstd']}, outs)
        check('%s bn_bwd_finalize (relu %d)' % (what, relu), '(dbeta, dgamma)', 'bn_bwd_finalize_grads-' + dn,
              U.param_grad_usage(outs['dbeta'].view.cpu(), outs['dgamma'].view.cpu(), sums_ref, bound))
        coefs[relu] = (outs['coef'], outs['coef'].view.cpu().view(3, C))
    for relu, want_dres in BWD_FLAGS:
        mask, amb, gz = source[relu]
        gcoef, coef = coefs[relu]
        base = None
        for form in stream_forms(C):
            options(bn_stream_unroll=form)
            tag = '%s bn_bwd_apply (U %d, relu %d, dres %d)' % (what, form, relu, want_dres)
            ins = {'dz': gdz, 'x': gx, 'coef': gcoef}
            if gz is not None:
                ins['z'] = gz
            if relu == 2:
                ins.update(scale=gk['scale'], shift=gk['shift'])
            outs = {'dx': Guarded(M * C, dtype)}
            if want_dres:
                outs['dres'] = Guarded(M * C, dtype)
            run(tag, lambda: L.check(lib.passl_hip_bn_bwd_apply(
                L.ptr(gdz.view), L.ptr(gz.view) if gz is not None else None, L.ptr(gx.view), L.ptr(gcoef.view),
                L.ptr(gk['scale'].view) if relu == 2 else None, L.ptr(gk['shift'].view) if relu == 2 else None,
                L.ptr(outs['dx'].view), L.ptr(outs['dres'].view) if want_dres else None, M, C, relu, L.dt(dtype),
                L.stream()), 'bn_bwd_apply'), ins, outs)
            raw = [g.raw() for g in outs.values()]
            if base is None or not all(torch.equal(a, b) for a, b in zip(raw, base)):
                dx = outs['dx'].view.float().cpu().view(M, C)
                check(tag, 'dx', 'bn_bwd_apply-' + dn, U.bwd_apply_usage(dx, dz, x, coef, mask, dtype, amb))
                if want_dres:
                    n, at = U.dres_mismatch(outs['dres'].view.float().cpu().view(M, C), dz, mask, amb)
                    assert n == 0, '%s: %d elements of dres are not the masked dz, first at flat index %d' % (tag, n, at)
            assert base is None or all(torch.equal(a, b) for a, b in zip(raw, base)), \
                '%s: the bits differ from those of U %d' % (tag, stream_forms(C)[0])
            base = base or raw


@pytest.mark.parametrize('case', U.MAXPOOL_CASES, ids=[U.case_id(c) for c in U.MAXPOOL_CASES])
def test_maxpool(case):
    (N, H, W, C), kind, dtype = case
    d = U.pool_data(case)
    what, dn = U.case_id(case), U.DTNAME[dtype]
    P, Q = U.pool_dims(H, W)
    lib = L.load()
    gx, gdy = gin(d['x'], dtype), gin(d['dy'], dtype)
    outs = {'y': Guarded(N * P * Q * C, dtype), 'idx': Guarded(N * P * Q * C, U8)}
    run(what + ' maxpool_fwd', lambda: L.check(lib.passl_hip_maxpool3x3s2_fwd(
        L.ptr(gx.view), L.ptr(outs['y'].view), L.ptr(outs['idx'].view), N, H, W, C, L.dt(dtype), L.stream()),
        'maxpool_fwd'), {'x': gx}, outs)
    y_ref, idx_ref = U.maxpool_ref(d['x'])
    y, idx = outs['y'].view.float().cpu().view(N, P, Q, C), outs['idx'].view.cpu().view(N, P, Q, C)
    bad = (y != y_ref).flatten().nonzero()
    assert len(bad) == 0, '%s: %d elements of y are not the window maximum, first at flat index %d' % (
        what, len(bad), int(bad[0]))
    bad = (idx != idx_ref).flatten().nonzero()
    assert len(bad) == 0, '%s: %d index bytes do not name the first maximum, first at flat index %d (%d, expected %d)' % (
        what, len(bad), int(bad[0]), int(idx.flatten()[bad[0]]), int(idx_ref.flatten()[bad[0]]))
    gidx = gin(idx_ref, U8)
    dx = Guarded(N * H * W * C, dtype)
    run(what + ' maxpool_bwd', lambda: L.check(lib.passl_hip_maxpool3x3s2_bwd(
        L.ptr(gdy.view), L.ptr(gidx.view), L.ptr(dx.view), N, H, W, C, L.dt(dtype), L.stream()), 'maxpool_bwd'),
        {'dy': gdy, 'idx': gidx}, {'dx': dx})
    check(what + ' maxpool_bwd', 'dx', 'maxpool_bwd-' + dn,
          U.maxpool_bwd_usage(dx.view.float().cpu().view(N, H, W, C), d['dy'], idx_ref, H, W, dtype))


@pytest.mark.parametrize('case', U.AVGPOOL_CASES, ids=[U.case_id(c) for c in U.AVGPOOL_CASES])
def test_avgpool(case):
    (N, HW, C), kind, dtype = case
    d = U.pool_data(case)
    what, dn = U.case_id(case), U.DTNAME[dtype]
    lib = L.load()
    gx, gdy = gin(d['x'], dtype), gin(d['dy'], dtype)
    y, dx = Guarded(N * C, dtype), Guarded(N * HW * C, dtype)
    run(what + ' avgpool_fwd', lambda: L.check(lib.passl_hip_avgpool_fwd(
        L.ptr(gx.view), L.ptr(y.view), N, HW, C, L.dt(dtype), L.stream()), 'avgpool_fwd'), {'x': gx}, {'y': y})
    check(what + ' avgpool_fwd', 'y', 'avgpool_fwd-' + dn, U.avgpool_fwd_usage(y.view.float().cpu().view(N, C), d['x'], dtype))
    run(what + ' avgpool_bwd', lambda: L.check(lib.passl_hip_avgpool_bwd(
        L.ptr(gdy.view), L.ptr(dx.view), N, HW, C, L.dt(dtype), L.stream()), 'avgpool_bwd'), {'dy': gdy}, {'dx': dx})
    check(what + ' avgpool_bwd', 'dx', 'avgpool_bwd-' + dn,
          U.avgpool_bwd_usage(dx.view.float().cpu().view(N, HW, C), d['dy'], HW, dtype))


def test_each_stem_pool_form_is_taken(options):
    """The library's slab count of every accepted shape is the one of the selected form, and the forms differ."""
    lib = L.load()
    differ = 0
    for shape in U.STEM_SHAPES:
        counts = []
        for form in (0, 1):
            options(stem_pool_form=form)
            counts.append(lib.passl_hip_bn_relu_maxpool_blocks(*shape))
            assert counts[-1] == U.stem_layout(*shape, form)[0] > 0, (shape, form, counts)
        differ += counts[0] != counts[1]
    assert differ > 0


@pytest.mark.parametrize('case', U.STEM_CASES, ids=[U.case_id(c) for c in U.STEM_CASES])
def test_bn_relu_maxpool(case, options):
    (N, H, W, C), kind, dtype = case
    d = U.pool_data(case)
    x, dy = d['x'], d['dy']
    x2 = x.reshape(-1, C)
    what, dn = U.case_id(case), U.DTNAME[dtype]
    P, Q = U.pool_dims(H, W)
    lib = L.load()
    gamma, beta = U.stem_params(C)
    k = stats_and_finalize(what, x2, gamma, beta, dtype)
    gx, gdy, ggamma = gin(x, dtype), gin(dy, dtype), gin(gamma, F32)
    gk = {n: gin(t, F32) for n, t in k.items()}
    outs = {'y': Guarded(N * P * Q * C, dtype), 'idx': Guarded(N * P * Q * C, U8)}
    run(what + ' bn_relu_maxpool_fwd', lambda: L.check(lib.passl_hip_bn_relu_maxpool_fwd(
        L.ptr(gx.view), L.ptr(gk['scale'].view), L.ptr(gk['shift'].view), L.ptr(outs['y'].view), L.ptr(outs['idx'].view),
        N, H, W, C, L.dt(dtype), L.stream()), 'bn_relu_maxpool_fwd'),
        {'x': gx, 'scale': gk['scale'], 'shift': gk['shift']}, outs)
    y, idx = outs['y'].view.float().cpu().view(N, P, Q, C), outs['idx'].view.cpu().view(N, P, Q, C)
    msgs, ratio = U.stem_fwd_violations(what + ' bn_relu_maxpool_fwd', y, idx, x, k['scale'], k['shift'], dtype)
    fig('bn_relu_maxpool_fwd-' + dn, what, ratio)
    assert not msgs, '\n'.join(msgs)
    # backward, from the device's own index bytes
    gidx = outs['idx']
    g, gother, amb = U.stem_grad(dy, idx, x, k['scale'], k['shift'], dtype)
    share = float(amb.double().mean())
    fig('mode2-share', what, 100 * share, '% of the elements')
    assert share <= U.AMBIGUOUS_CAP, '%s: %.3f %% of the elements are at the recomputed-mask boundary' % (what, 100 * share)
    ins = {'dy': gdy, 'idx': gidx, 'x': gx, 'mean': gk['mean'], 'invstd': gk['invstd'], 'scale': gk['scale'],
           'shift': gk['shift']}
    parts = {}
    for form in (0, 1):
        options(stem_pool_form=form)
        tag = '%s bn_relu_maxpool_bwd_reduce (form %d)' % (what, form)
        nb, per = U.stem_layout(N, H, W, C, form)
        assert lib.passl_hip_bn_relu_maxpool_blocks(N, H, W, C) == nb
        part = Guarded(partial_floats(nb, C, 0), F32, prefill='a5')
        run(tag, lambda: L.check(lib.passl_hip_bn_relu_maxpool_bwd_reduce(
            L.ptr(gdy.view), L.ptr(gidx.view), L.ptr(gx.view), L.ptr(gk['mean'].view), L.ptr(gk['invstd'].view),
            L.ptr(gk['scale'].view), L.ptr(gk['shift'].view), L.ptr(part.view), nb, N, H, W, C, L.dt(dtype), L.stream()),
            'bn_relu_maxpool_bwd_reduce'), ins, {'partial': part}, written={'partial': nb * C * 2})
        sums_ref, bound = U.reduce_ref(g, x2, k['mean'], k['invstd'], U.stem_groups(N, H, W, nb, per), amb, gother)
        check(tag, 'slab [workgroup, channel, (sum g, sum g xhat)]', 'bn_relu_maxpool_bwd_reduce-' + dn,
              U.usage(part.view.cpu()[:nb * C * 2].view(nb, C, 2), sums_ref, bound))
        parts[form] = (part, nb)
    part, nb = parts[1]
    fin = {'dgamma': gin(torch.zeros(C), F32), 'dbeta': gin(torch.zeros(C), F32), 'coef': Guarded(3 * C, F32)}
    run(what + ' bn_bwd_finalize', lambda: L.check(lib.passl_hip_bn_bwd_finalize(
        L.ptr(part.view), nb, N * H * W, C, L.ptr(ggamma.view), L.ptr(gk['mean'].view), L.ptr(gk['invstd'].view),
        L.ptr(fin['dgamma'].view), L.ptr(fin['dbeta'].view), L.ptr(fin['coef'].view), L.stream()), 'bn_bwd_finalize'),
        {'partial': part, 'gamma': ggamma, 'mean': gk['mean'], 'invstd': gk['invstd']}, fin)
    check(what + ' bn_bwd_finalize', '(dbeta, dgamma)', 'bn_bwd_finalize_grads-' + dn,
          U.param_grad_usage(fin['dbeta'].view.cpu(), fin['dgamma'].view.cpu(), sums_ref, bound))
    gcoef, coef = fin['coef'], fin['coef'].view.cpu().view(3, C)
    a, b, c = coef.double()
    refs = []
    for t in (g, gother):
        ag, bx = a * t.double(), b * x2.double()
        dx64 = ag + bx + c
        refs += [dx64, 4 * U.E * (ag.abs() + bx.abs() + c.abs()) + U.unit(dtype) * dx64.abs()]
    base = None
    for form in (0, 1):
        options(stem_pool_form=form)
        tag = '%s bn_relu_maxpool_bwd_apply (form %d)' % (what, form)
        dx = Guarded(N * H * W * C, dtype)
        run(tag, lambda: L.check(lib.passl_hip_bn_relu_maxpool_bwd_apply(
            L.ptr(gdy.view), L.ptr(gidx.view), L.ptr(gx.view), L.ptr(gcoef.view), L.ptr(gk['scale'].view),
            L.ptr(gk['shift'].view), L.ptr(dx.view), N, H, W, C, L.dt(dtype), L.stream()), 'bn_relu_maxpool_bwd_apply'),
            {'dy': gdy, 'idx': gidx, 'x': gx, 'coef': gcoef, 'scale': gk['scale'], 'shift': gk['shift']}, {'dx': dx})
        check(tag, 'dx', 'bn_relu_maxpool_bwd_apply-' + dn,
              U.usage_either(dx.view.float().cpu().view(-1, C), *refs, amb))
        assert base is None or torch.equal(dx.raw(), base), '%s: dx differs from form 0 given the same coefficients' % tag
        base = dx.raw()
