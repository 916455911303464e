"""The optimizer and flat-arena kernels (csrc/flat.hip, the flat AdamW walk of csrc/vit.hip) against float64 references,
element by element, over the case tables of flat_util.py (which has the derivation of every bound).

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must survive;
pure outputs (k_lp, dst, norms, scale, shift, out without accumulate) start as NaN and every element must have been
written; every read-only operand must come back bit-identical; of an in-place operand everything the kernel does not
own must (the references carry the initial value and the bound 0 there); every launch runs twice from the same initial
state and must give the same bits.  A device error after a launch ends the session.

Worst error on an MI355X in units of the element's own bound, over all cases (a record of one run, not a pass
criterion):
  kernel          tensor   worst   case
  ema_update      k        0.220   4099-mixed
  ema_update      k_lp     exact   (the rounding of the kernel's own k)
  momentum_sgd    v        0.136   4099-gs3
  momentum_sgd    p        0.142   2097159-plain
  adamw           m        0.188   4099-mixed
  adamw           v        0.196   4099-mixed
  adamw           p        0.207   7-gs16
  lars            norms    0.096   lars-a-0
  lars            v        0.157   lars-a-0
  lars            p        0.142   lars-a-0
  larc            norms    0.096   larc-a-0
  larc            v        0.161   larc-a-0
  larc            p        0.125   larc-b-0
  slab_reduce     out      0.998   4100-1-1-plain (one slab onto `out`: a single addition, whose rounding is the bound);
                                   bit for bit the documented order in all 168 cases
  bn_fold         scale    0.367   257-1e-05
  bn_fold         shift    0.176   255-1e-05
  cast, pack_weights       exact
The _dev forms gave the bits of the by-value forms in every case.  bn_fold's scale at 0.367 of (2 + F_RSQRT) e is a
relative error of 2.2 e, the addition and the product included: the reciprocal square root stayed within about 1 ulp
where F_RSQRT allows 2.  The cast of fp32 denormals: all 10 recorded patterns came back correctly rounded (to a bf16
denormal or to the smallest normal), none flushed to zero.  No kernel needed a change to meet its bounds.
The file's 133 tests take 4 s.
"""
import numpy as np
import pytest
import torch

import flat_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32, BF16, I64, I32, U8 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8


def gin(a, dtype=F32, skew=0):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return Guarded(t.numel(), dtype, skew=skew, fill=t)


def gvec(*v):
    return gin(np.array(v, np.float32))


def sync(what):
    """A device fault ends the whole session: nothing more is launched on a GPU that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit('%s: the device reported %s' % (what, err), returncode=3)


def run(what, fn, ins, outs, unchecked=()):
    """Launches fn() twice on the guarded operands, from the same initial state (an in-place operand is an output
    with a fill).  Asserts: the same bits both times, every guard intact, every input unchanged, every element of a
    pure output written (`unchecked`: outputs whose unwritten or non-finite elements the caller judges)."""
    before = {n: g.raw() for n, g in ins.items()}
    fn()
    sync(what)
    first = {n: g.raw() for n, g in outs.items()}
    for g in outs.values():
        g.reset()
    fn()
    sync(what)
    for n, g in outs.items():
        assert torch.equal(g.raw(), first[n]), '%s: %s differs between two runs of the same launch' % (what, n)
    for n, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), '%s: a guard region of %s was written' % (what, n)
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), '%s: the input %s was modified' % (what, n)
    for n, g in outs.items():
        if n not in unchecked and g.fill is None:
            left = g.unwritten()
            assert left == 0, '%s: %d elements of %s were not written' % (what, left, n)
    return first


def refused(what, fn, operands):
    """fn() returns PASSL_EINVAL and leaves every guarded byte as it was."""
    before = {n: g.buf.view(torch.uint8).clone() for n, g in operands.items()}
    rc = fn()
    sync(what)
    assert rc == L.EINVAL, '%s: status %d, not PASSL_EINVAL' % (what, rc)
    for n, g in operands.items():
        assert torch.equal(g.buf.view(torch.uint8), before[n]), '%s: %s was written by a refused call' % (what, n)


def cpu(g):
    return g.view.float().cpu().numpy()


def bf_bits(g):
    return g.view.view(torch.int16).cpu().numpy().view(np.uint16)


def check(kernel, what, ref, got):
    """Every tensor of `got` against ref[name] = (float64 reference, bound)."""
    failures = []
    for name, value in got.items():
        ratio, idx = U.usage(value, *ref[name])
        print('FIG %s %s %s %.4f of the bound' % (kernel, name, what, ratio))
        msg = U.verdict('%s %s' % (kernel, what), name, ratio, idx)
        if msg:
            failures.append(msg)
    assert not failures, '\n'.join(failures)


def same(what, a, b):
    for n in a:
        assert torch.equal(a[n], b[n]), '%s: %s differs' % (what, n)


# ------------------------------------------------------------------------------------------------ streaming kernels
@pytest.mark.parametrize('case', U.EMA_CASES, ids=U.case_id)
def test_ema_update(case):
    n = case[0]
    d, what, lib = U.ema_data(case), U.case_id(case), L.load()
    ins = {'q': gin(d['q'])}
    k = gin(d['k'])
    plain = run(what + ' ema', lambda: L.check(lib.passl_hip_ema_update(
        L.ptr(k.view), L.ptr(ins['q'].view), None, n, d['m'], L.stream()), 'ema_update'), ins, {'k': k})
    k.reset()
    outs = {'k': k, 'k_lp': Guarded(n, BF16)}
    both = run(what + ' ema + bf16 copy', lambda: L.check(lib.passl_hip_ema_update(
        L.ptr(k.view), L.ptr(ins['q'].view), L.ptr(outs['k_lp'].view), n, d['m'], L.stream()), 'ema_update'), ins, outs)
    assert torch.equal(plain['k'], both['k']), '%s: the bf16 copy changes the fp32 result' % what
    got = cpu(k)
    check('ema_update', what, U.ema_ref(case), dict(k=got))
    assert np.array_equal(bf_bits(outs['k_lp']), U.bf16_bits(got)), '%s: k_lp is not the rounding of k' % what


def sgd_launch(what, d, n, dev, skew=0):
    lib = L.load()
    ins = {'g': gin(d['g'], skew=skew)}
    outs = {'p': gin(d['p'], skew=skew), 'v': gin(d['v'], skew=skew)}
    a = [L.ptr(outs['p'].view), L.ptr(ins['g'].view), L.ptr(outs['v'].view), n]
    if dev:
        ins['hyper'] = gvec(d['lr'])
        fn = lambda: L.check(lib.passl_hip_momentum_sgd_dev(*a, L.ptr(ins['hyper'].view), d['mu'], d['wd'], d['gs'],
                                                            L.stream()), 'momentum_sgd_dev')
    else:
        fn = lambda: L.check(lib.passl_hip_momentum_sgd(*a, d['lr'], d['mu'], d['wd'], d['gs'], L.stream()),
                             'momentum_sgd')
    return run('%s sgd%s' % (what, ' dev' if dev else ''), fn, ins, outs), outs


@pytest.mark.parametrize('case', U.SGD_CASES, ids=U.case_id)
def test_momentum_sgd(case):
    d, what = U.sgd_data(case), U.case_id(case)
    bits, outs = sgd_launch(what, d, case[0], False)
    check('momentum_sgd', what, U.sgd_ref(case), dict(v=cpu(outs['v']), p=cpu(outs['p'])))
    same(what + ': momentum_sgd and momentum_sgd_dev', bits, sgd_launch(what, d, case[0], True)[0])


def adamw_launch(what, d, n, dev):
    lib = L.load()
    ins = {'g': gin(d['g'])}
    outs = {x: gin(d[x]) for x in 'pmv'}
    a = [L.ptr(outs['p'].view), L.ptr(ins['g'].view), L.ptr(outs['m'].view), L.ptr(outs['v'].view), n]
    if dev:
        ins['hyper'] = gvec(d['lr'], d['b1p'], d['b2p'])
        fn = lambda: L.check(lib.passl_hip_adamw_dev(*a, L.ptr(ins['hyper'].view), d['b1'], d['b2'], d['eps'], d['wd'],
                                                     d['gs'], L.stream()), 'adamw_dev')
    else:
        fn = lambda: L.check(lib.passl_hip_adamw(*a, d['lr'], d['b1'], d['b2'], d['eps'], d['wd'], d['b1p'], d['b2p'],
                                                 d['gs'], L.stream()), 'adamw')
    return run('%s adamw%s' % (what, ' dev' if dev else ''), fn, ins, outs), outs


@pytest.mark.parametrize('case', U.ADAMW_CASES, ids=U.case_id)
def test_adamw(case):
    d, what = U.adamw_data(case), U.case_id(case)
    bits, outs = adamw_launch(what, d, case[0], False)
    got = {x: cpu(outs[x]) for x in 'mvp'}
    assert all(np.isfinite(t).all() for t in got.values()), what
    check('adamw', what, U.adamw_ref(case), got)
    same(what + ': adamw and adamw_dev', bits, adamw_launch(what, d, case[0], True)[0])


@pytest.mark.parametrize('n', U.CAST_SIZES)
def test_cast_f32_to_bf16(n):
    x, lib = U.cast_data(n), L.load()
    ins, dst = {'src': gin(x)}, Guarded(n, BF16, prefill='a5')
    run('cast %d' % n, lambda: L.check(lib.passl_hip_cast_f32_to_bf16(L.ptr(ins['src'].view), L.ptr(dst.view), n,
                                                                       L.stream()), 'cast'), ins, {'dst': dst})
    assert np.array_equal(bf_bits(dst), U.cast_expect(x)), 'cast %d: not the round-to-nearest-even bits' % n


def test_cast_bit_patterns_and_denormals():
    lib = L.load()
    x = U.CAST_PATTERNS.view(np.float32)
    ins, dst = {'src': gin(x)}, Guarded(len(x), BF16, prefill='a5')
    run('cast patterns', lambda: L.check(lib.passl_hip_cast_f32_to_bf16(
        L.ptr(ins['src'].view), L.ptr(dst.view), len(x), L.stream()), 'cast'), ins, {'dst': dst})
    got, want = bf_bits(dst), U.cast_expect(x)
    assert U.bf16_equal(got, want), ['%08x: %04x, not %04x' % t for t in zip(U.CAST_PATTERNS, got, want) if t[1] != t[2]]
    x = U.CAST_DENORMALS.view(np.float32)                       # recorded: correctly rounded, or a zero of the same sign
    ins, dst = {'src': gin(x)}, Guarded(len(x), BF16, prefill='a5')
    run('cast denormals', lambda: L.check(lib.passl_hip_cast_f32_to_bf16(
        L.ptr(ins['src'].view), L.ptr(dst.view), len(x), L.stream()), 'cast'), ins, {'dst': dst})
    got, want = bf_bits(dst), U.cast_expect(x)
    zero = (U.CAST_DENORMALS >> 16).astype(np.uint16) & 0x8000
    print('FIG cast denormals: %d of %d correctly rounded, %d flushed to a signed zero' % (
        (got == want).sum(), len(x), ((got == zero) & (got != want)).sum()))
    assert ((got == want) | (got == zero)).all(), ['%08x: %04x' % t for t in zip(U.CAST_DENORMALS, got)]


def test_streaming_kernels_with_n_0_write_nothing():
    lib, z = L.load(), np.zeros(8, np.float32)
    g = {n: gin(z + i) for i, n in enumerate('pgmvh')}
    g['lp'] = Guarded(8, BF16)
    before = {n: t.raw() for n, t in g.items()}
    P = lambda n: L.ptr(g[n].view)
    s = L.stream()
    for what, rc in (('ema', lib.passl_hip_ema_update(P('p'), P('g'), P('lp'), 0, 0.9, s)),
                     ('sgd', lib.passl_hip_momentum_sgd(P('p'), P('g'), P('v'), 0, 0.1, 0.9, 0.1, 1.0, s)),
                     ('sgd_dev', lib.passl_hip_momentum_sgd_dev(P('p'), P('g'), P('v'), 0, P('h'), 0.9, 0.1, 1.0, s)),
                     ('cast', lib.passl_hip_cast_f32_to_bf16(P('p'), P('lp'), 0, s)),
                     ('adamw', lib.passl_hip_adamw(P('p'), P('g'), P('m'), P('v'), 0, 0.1, 0.9, 0.9, 1e-8, 0.1, 0.9,
                                                   0.9, 1.0, s)),
                     ('adamw_dev', lib.passl_hip_adamw_dev(P('p'), P('g'), P('m'), P('v'), 0, P('h'), 0.9, 0.9, 1e-8,
                                                           0.1, 1.0, s))):
        assert rc == L.OK, what
    sync('n = 0')
    assert all(torch.equal(t.raw(), before[n]) and t.intact() for n, t in g.items())


def test_streaming_kernels_refuse_misaligned_pointers_negative_n_and_a_null_hyper():
    lib, z = L.load(), np.ones(16, np.float32)
    g = {n: gin(z) for n in 'pgmvh'}
    g.update({n + '1': gin(z, skew=1) for n in 'pg'}, lp=Guarded(16, BF16), lp1=Guarded(16, BF16, skew=2))
    P = lambda n: L.ptr(g[n].view) if n else None
    s = L.stream()
    calls = {
        'ema k off': lambda: lib.passl_hip_ema_update(P('p1'), P('g'), None, 16, 0.9, s),
        'ema q off': lambda: lib.passl_hip_ema_update(P('p'), P('g1'), None, 16, 0.9, s),
        'ema k_lp off': lambda: lib.passl_hip_ema_update(P('p'), P('g'), P('lp1'), 16, 0.9, s),
        'ema n < 0': lambda: lib.passl_hip_ema_update(P('p'), P('g'), P('lp'), -1, 0.9, s),
        'sgd p off': lambda: lib.passl_hip_momentum_sgd(P('p1'), P('g'), P('v'), 16, 0.1, 0.9, 0.1, 1.0, s),
        'sgd g off': lambda: lib.passl_hip_momentum_sgd(P('p'), P('g1'), P('v'), 16, 0.1, 0.9, 0.1, 1.0, s),
        'sgd n < 0': lambda: lib.passl_hip_momentum_sgd(P('p'), P('g'), P('v'), -4, 0.1, 0.9, 0.1, 1.0, s),
        'sgd_dev null hyper': lambda: lib.passl_hip_momentum_sgd_dev(P('p'), P('g'), P('v'), 16, None, 0.9, 0.1, 1.0, s),
        'sgd_dev p off': lambda: lib.passl_hip_momentum_sgd_dev(P('p1'), P('g'), P('v'), 16, P('h'), 0.9, 0.1, 1.0, s),
        'cast src off': lambda: lib.passl_hip_cast_f32_to_bf16(P('p1'), P('lp'), 16, s),
        'cast dst off': lambda: lib.passl_hip_cast_f32_to_bf16(P('p'), P('lp1'), 16, s),
        'cast n < 0': lambda: lib.passl_hip_cast_f32_to_bf16(P('p'), P('lp'), -1, s),
        'adamw p off': lambda: lib.passl_hip_adamw(P('p1'), P('g'), P('m'), P('v'), 16, 0.1, 0.9, 0.9, 1e-8, 0.1, 0.9,
                                                   0.9, 1.0, s),
        'adamw n < 0': lambda: lib.passl_hip_adamw(P('p'), P('g'), P('m'), P('v'), -1, 0.1, 0.9, 0.9, 1e-8, 0.1, 0.9,
                                                   0.9, 1.0, s),
        'adamw_dev null hyper': lambda: lib.passl_hip_adamw_dev(P('p'), P('g'), P('m'), P('v'), 16, None, 0.9, 0.9,
                                                                1e-8, 0.1, 1.0, s),
        'adamw_dev g off': lambda: lib.passl_hip_adamw_dev(P('p'), P('g1'), P('m'), P('v'), 16, P('h'), 0.9, 0.9, 1e-8,
                                                           0.1, 1.0, s),
    }
    for what, fn in calls.items():
        refused(what, fn, g)


# ------------------------------------------------------------------------------------------------ LARS / LARC
def lars_operands(skew=0):
    lay, d = U.lars_layout(), U.lars_arena()
    ins = {'g': gin(d['g'], skew=skew), 'blk_off': gin(lay['blk_off'], I64), 'blk_len': gin(lay['blk_len'], I32),
           'blk_seg': gin(lay['blk_seg'], I32), 'seg_wd': gin(lay['seg_wd'])}
    n_seg, n_blk = len(U.LARS_SEGS), len(lay['blk_off'])
    outs = {'p': gin(d['p'], skew=skew), 'v': gin(d['v'], skew=skew), 'norms': Guarded(2 * (n_seg + n_blk), F32)}
    return ins, outs, n_seg, n_blk


def lars_call(case, ins, outs, n_seg, n_blk, dev, hyper='hyper'):
    rule, _, clip = case
    s, lib = U.lars_scalars(case), L.load()
    P = lambda g: L.ptr(g.view) if g is not None else None
    a = [P(outs['p']), P(ins['g']), P(outs['v']), P(ins['blk_off']), P(ins['blk_len']), P(ins['blk_seg']), n_blk,
         P(ins['seg_wd']), n_seg, P(outs['norms'])]
    if rule == 'larc':
        return lambda: lib.passl_hip_larc_momentum_dev(*a, P(ins.get(hyper)), s['mu'], s['coeff'], s['eps'], clip,
                                                       s['gs'], L.stream())
    if dev:
        return lambda: lib.passl_hip_lars_momentum_dev(*a, P(ins.get(hyper)), s['mu'], s['coeff'], s['eps'], s['gs'],
                                                       L.stream())
    return lambda: lib.passl_hip_lars_momentum(*a, s['lr'], s['mu'], s['coeff'], s['eps'], s['gs'], L.stream())


@pytest.mark.parametrize('case', U.LARS_CASES, ids=U.case_id)
def test_lars_and_larc(case):
    what, ref = U.case_id(case), U.lars_ref(case)
    ins, outs, n_seg, n_blk = lars_operands()
    ins['hyper'] = gvec(U.lars_scalars(case)['lr'])
    fn = lars_call(case, ins, outs, n_seg, n_blk, dev=case[0] == 'larc')
    bits = run(what, lambda: L.check(fn(), what), ins, outs)
    got = dict(norms=cpu(outs['norms']).reshape(-1, 2), v=cpu(outs['v']), p=cpu(outs['p']))
    check(case[0], what, ref, got)
    own = U.lars_layout()['elem_seg'] >= 0                        # (the bound 0 says it already: stated once more)
    d = U.lars_arena()
    assert np.array_equal(U.bits(got['p'][~own]), U.bits(d['p'][~own])), what + ': p outside the listed blocks'
    assert np.array_equal(U.bits(got['v'][~own]), U.bits(d['v'][~own])), what + ': v outside the listed blocks'
    if case[0] == 'lars':
        for g in outs.values():
            g.reset()
        fn = lars_call(case, ins, outs, n_seg, n_blk, dev=True)
        same(what + ': lars_momentum and lars_momentum_dev', bits, run(what + ' dev', lambda: L.check(fn(), what), ins, outs))


def test_lars_and_larc_refusals():
    lay = U.lars_layout()
    ins, outs, n_seg, n_blk = lars_operands()
    ins['hyper'] = gvec(0.1)
    ins1, outs1, _, _ = lars_operands(skew=1)
    ins1 = dict(ins, g=ins1['g'])
    everything = dict(ins, **{'o_' + n: g for n, g in outs.items()}, g1=ins1['g'], p1=outs1['p'], v1=outs1['v'])
    for case, dev in ((('lars', 'a', 0), False), (('lars', 'a', 0), True), (('larc', 'a', 1), True)):
        what = '%s dev=%d' % (case[0], dev)
        refused(what + ' p off', lars_call(case, ins, dict(outs, p=outs1['p']), n_seg, n_blk, dev), everything)
        refused(what + ' g off', lars_call(case, ins1, outs, n_seg, n_blk, dev), everything)
        refused(what + ' v off', lars_call(case, ins, dict(outs, v=outs1['v']), n_seg, n_blk, dev), everything)
        refused(what + ' n_seg = 0', lars_call(case, ins, outs, 0, n_blk, dev), everything)
        refused(what + ' n_seg < 0', lars_call(case, ins, outs, -1, n_blk, dev), everything)
        refused(what + ' n_blocks < 0', lars_call(case, ins, outs, n_seg, -1, dev), everything)
        if dev:
            refused(what + ' null hyper', lars_call(case, ins, outs, n_seg, n_blk, dev, hyper='none'), everything)


# ------------------------------------------------------------------------------------------------ slab_reduce
@pytest.mark.parametrize('slabs,acc', [(s, a) for s in U.SLAB_COUNTS for a in (0, 1)])
def test_slab_reduce(slabs, acc):
    lib = L.load()
    for case in (c for c in U.SLAB_CASES if c[1] == slabs and c[2] == acc):
        n, what, d = case[0], U.case_id(case), U.slab_data(case)
        ins = {'ws': gin(d['ws'])}
        out = gin(d['out']) if acc else Guarded(n, F32)
        run('slab ' + what, lambda: L.check(lib.passl_hip_slab_reduce(L.ptr(ins['ws'].view), L.ptr(out.view), n, slabs,
                                                                      acc, L.stream()), 'slab_reduce'), ins, {'out': out})
        got = cpu(out)
        check('slab_reduce', what, U.slab_ref(case), dict(out=got))
        twin = U.slab_eval32(case)['out']
        diff = np.nonzero(U.bits(got) != U.bits(twin))[0]
        assert not len(diff), 'slab %s: not the documented order at %s' % (what, diff[:8])


def test_slab_reduce_refusals():
    lib, s = L.load(), L.stream()
    g = dict(ws=gin(np.ones(64, np.float32)), out=gin(np.ones(16, np.float32)), ws1=gin(np.ones(64, np.float32), skew=1),
             out1=gin(np.ones(16, np.float32), skew=1))
    P = lambda n: L.ptr(g[n].view)
    for what, fn in {'n % 4': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out'), 14, 4, 0, s),
                     'n = 0': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out'), 0, 4, 0, s),
                     'n < 0': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out'), -4, 4, 0, s),
                     'slabs = 0': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out'), 16, 0, 0, s),
                     'slabs < 0': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out'), 16, -1, 1, s),
                     'ws off': lambda: lib.passl_hip_slab_reduce(P('ws1'), P('out'), 16, 4, 0, s),
                     'out off': lambda: lib.passl_hip_slab_reduce(P('ws'), P('out1'), 12, 4, 1, s)}.items():
        refused('slab ' + what, fn, g)


# ------------------------------------------------------------------------------------------------ bn_fold
@pytest.mark.parametrize('case', U.BN_CASES, ids=U.case_id)
def test_bn_fold(case):
    n, eps = case
    d, what, lib = U.bn_data(case), U.case_id(case), L.load()
    ins = {'flat': gin(d['flat'])}
    ins.update({x: gin(d[x], I64) for x in ('gi', 'bi', 'mi', 'vi')})
    outs = {'scale': Guarded(n, F32), 'shift': Guarded(n, F32)}
    P = lambda g: L.ptr(g.view)
    run('bn_fold ' + what, lambda: L.check(lib.passl_hip_bn_fold(
        P(ins['flat']), P(ins['gi']), P(ins['bi']), P(ins['mi']), P(ins['vi']), n, eps, P(outs['scale']),
        P(outs['shift']), L.stream()), 'bn_fold'), ins, outs)
    check('bn_fold', what, U.bn_ref(case), dict(scale=cpu(outs['scale']), shift=cpu(outs['shift'])))
    refused('bn_fold n = 0', lambda: lib.passl_hip_bn_fold(
        P(ins['flat']), P(ins['gi']), P(ins['bi']), P(ins['mi']), P(ins['vi']), 0, eps, P(outs['scale']),
        P(outs['shift']), L.stream()), dict(ins, **outs))


# ------------------------------------------------------------------------------------------------ pack_weights
@pytest.mark.parametrize('dtype', (F32, BF16), ids=('fp32', 'bf16'))
def test_pack_weights(dtype):
    c, lib = U.pack_case(), L.load()
    assert c['modes'] == [j[-1] for j in U.PACK_JOBS]              # the packer chose the modes the jobs are named for
    ins = {'src': gin(c['src']), 'jobs': gin(c['jobs_raw'], U8), 'block_job': gin(c['block_job'], I32),
           'block_start': gin(c['block_start'], I32)}
    dst = Guarded(c['size'], dtype)                                # in place of packer.buffer; NaN where no job writes
    P = lambda g: L.ptr(g.view)
    run('pack', lambda: L.check(lib.passl_hip_pack_weights(
        P(ins['src']), P(dst), L.dt(dtype), P(ins['jobs']), P(ins['block_job']), P(ins['block_start']), c['n_blocks'],
        L.stream()), 'pack_weights'), ins, {'dst': dst}, unchecked=('dst',))
    want, mask = U.pack_expect(dtype == BF16)
    got = cpu(dst)
    assert np.array_equal(np.isnan(got), ~mask), 'pack: %d elements of a job unwritten, %d bytes between jobs written' % (
        (np.isnan(got) & mask).sum(), (~np.isnan(got) & ~mask).sum())
    for name, pk, *_ in c['jobs']:
        sl = slice(pk.dst_off, pk.dst_off + pk.size)
        g = bf_bits(dst)[sl] if dtype == BF16 else U.bits(got[sl])
        w = want[sl] if dtype == BF16 else U.bits(want[sl])
        bad = np.nonzero(g != w)[0]
        assert not len(bad), 'pack job %s: %d elements differ from emu_pack, first at %s' % (name, len(bad), bad[:8])
