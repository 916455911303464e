"""The criteria of flat_util.py, tested on the CPU before any kernel is judged by them.

For every case of the tables the float32 twin of each formula stays within HEADROOM = 0.5 of every element's bound
against the float64 reference (the condition the inputs were chosen to meet); the bit-exact twins agree with their
statements; the float64 references agree, to float64 rounding, with the project's own statements of the same rules
(the LARS rule of oracle/simclr.py, the LARC update of oracle/linprobe_v2.py, the AdamW rule of oracle/mae.py;
emu_pack is the pack reference itself).  Then the planted defects: each, applied to the twin, must exceed 1.0 on the
named tensor of the named case, or change a bit where the kernel is held to bits, or the GPU test could not see it
either.  Every figure is printed as a `FIG host ...` line.

One twin is exempt from the 0.5 (not from the bound): slab_reduce's, which is the kernel's contract bit for bit and
whose bound is slabs e sum |terms| by its contract: with one slab and `accumulate` the single addition may
use all of e sum |terms| by definition (up to 4 slabs the chain has exactly `slabs` roundings).
"""
import types

import numpy as np
import pytest
import torch

import flat_util as U


def judge(what, ref, got, limit=U.HEADROOM):
    worst = {}
    for name, r in ref.items():
        if name not in got:
            continue
        ratio, idx = U.usage(got[name], r[0], r[1])
        worst[name] = ratio
        print('FIG host %s %s %.4f of the bound' % (what, name, ratio))
        assert ratio <= limit, '%s: float32 %s uses %.3f of its bound at flat index %d (limit %.2f)' % (
            what, name, ratio, idx, limit)
    return worst


@pytest.mark.parametrize('case', U.EMA_CASES, ids=U.case_id)
def test_float32_ema_meets_the_bounds(case):
    judge('ema ' + U.case_id(case), U.ema_ref(case), U.ema_eval32(case))


@pytest.mark.parametrize('case', U.SGD_CASES, ids=U.case_id)
def test_float32_sgd_meets_the_bounds(case):
    judge('sgd ' + U.case_id(case), U.sgd_ref(case), U.sgd_eval32(case))


@pytest.mark.parametrize('case', U.ADAMW_CASES, ids=U.case_id)
def test_float32_adamw_meets_the_bounds(case):
    ev = U.adamw_eval32(case)
    judge('adamw ' + U.case_id(case), U.adamw_ref(case), ev)
    assert all(np.isfinite(t).all() for t in ev.values())
    if case[1] == 'zero_grad':                                     # m / (0 + eps_t) = 0: the decay alone
        d = U.adamw_data(case)
        assert not ev['m'].any() and not ev['v'].any()
        assert np.array_equal(ev['p'], (d['p'] * (np.float32(1) - np.float32(d['lr']) * np.float32(d['wd']))))


def test_the_streaming_kinds_are_what_they_are_named_for():
    d = U.adamw_data((1025, 'warm'))
    assert d['b1p'] == 0.0 and 0.3 < d['b2p'] < 0.4              # 1 - b1^t rounds to 1 at t = 1000
    d = U.adamw_data((1025, 'tiny_grad'))
    assert not (d['g'] * d['g']).astype(np.float32).all() and (U.adamw_ref((1025, 'tiny_grad'))['v'][0] < U.TINY).all()
    for fam, case in ((U.sgd_data, (4099, 'mixed')), (U.adamw_data, (4099, 'mixed')), (U.ema_data, (4099, 'mixed'))):
        mag = np.abs(fam(case)['p' if 'p' in fam(case) else 'k'])
        assert mag.min() < 1e-10 and mag.max() > 1e4
    d = U.sgd_data((4099, 'mixed'))                                # the planted cancellations cancel
    gp = d['g'].astype(np.float64) * d['gs'] + d['wd'] * d['p'].astype(np.float64)
    assert (np.abs(gp[::3]) < 1e-2 * np.abs(d['wd'] * d['p'][::3])).all()
    assert (np.abs(d['mu'] * d['v'][1::3] + gp[1::3]) < 1e-2 * np.abs(gp[1::3])).all()


@pytest.mark.parametrize('case', U.LARS_CASES, ids=U.case_id)
def test_float32_lars_and_larc_meet_the_bounds(case):
    ref = U.lars_ref(case)
    judge(U.case_id(case), {k: ref[k] for k in ('norms', 'v', 'p')}, U.lars_eval32(case))


def test_the_lars_arena_is_what_the_cases_are_named_for():
    lay, d = U.lars_layout(), U.lars_arena()
    assert all(o % U.ALIGN == 0 for o, _ in lay['slices']) and (np.diff(lay['blk_seg']) >= 0).all()
    assert (lay['blk_off'] % 4 == 0).all() and lay['blk_len'].max() == U.CHUNK
    assert max(np.bincount(lay['blk_seg'])) == 258                # the second trip of the segment reduce
    assert (lay['elem_seg'] < 0).sum() > U.LARS_TAIL              # padding between segments and the unlisted tail
    ratio = {}
    for (o, n), (_, kind) in zip(lay['slices'], U.LARS_SEGS):
        pn, gn = np.linalg.norm(d['p'][o:o + n].astype(np.float64)), np.linalg.norm(d['g'][o:o + n].astype(np.float64))
        ratio[kind] = pn / gn if gn else np.inf
    assert ratio['p_zero'] == 0 and ratio['g_zero'] == np.inf and 5e5 < ratio['p_big'] < 2e6
    assert 5e-7 < ratio['p_small'] < 2e-6
    for s in 'ab':                                                 # clip on: both sides of min(a / lr, 1)
        on, off = U.lars_ref(('larc', s, 1))['rate'], U.lars_ref(('larc', s, 0))['rate']
        lr = U.LARC_SCALARS[s]['lr']
        assert ((off / lr > 2) & (on == 1)).any() and ((off / lr < 0.5) & (on < 1)).any()


@pytest.mark.parametrize('slabs', U.SLAB_COUNTS)
def test_float32_slab_reduce_in_the_documented_order_meets_the_float64_bound(slabs):
    for case in (c for c in U.SLAB_CASES if c[1] == slabs):
        judge('slab ' + U.case_id(case), U.slab_ref(case), U.slab_eval32(case), limit=1.0)


@pytest.mark.parametrize('case', U.BN_CASES, ids=U.case_id)
def test_float32_bn_fold_meets_the_bounds(case):
    judge('bn_fold ' + U.case_id(case), U.bn_ref(case), U.bn_eval32(case))
    v = U.bn_data(case)['flat'][U.bn_data(case)['vi']]
    assert case[0] == 1 or (v.min() < 1e-9 and v.max() > 1e3)             # variances from 1e-12 to 1e6


def test_the_pack_restatement_is_emu_pack_and_the_packer_chose_the_modes():
    c = U.pack_case()
    assert c['modes'] == [j[-1] for j in U.PACK_JOBS], c['modes']
    want, mask = U.pack_expect(False)
    assert U.same_bits_or_nan(U.pack_eval32(), want)
    assert mask.sum() == sum(j[1].size for j in c['jobs']) and (~mask).any()     # gaps between jobs stay unwritten
    assert any(j[1].size % 1024 for j in c['jobs'] if j[0] == 'partial')
    dgrad = [j for j in c['jobs'] if j[0] == 'dgrad'][0]
    assert (dgrad[-1].reshape(5, 2, 2, 6)[:, 0] == 0).all() and (dgrad[-1].reshape(5, 2, 2, 6)[:, 1, 0] != 0).all()


def test_cast_patterns_round_as_named():
    got = U.cast_expect(U.CAST_PATTERNS.view(np.float32))
    assert list(got[:4]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82]      # ties go to even, down and up
    assert got[8] == 0x7F80 and got[9] == 0xFF80                  # the largest finite float rounds to inf
    assert list(got[11:15]) == [0x7F80, 0xFF80, 0x0000, 0x8000]
    assert U.bf16_equal(got[15:18], np.array([0x7FC0, 0xFFC0, 0x7FC1], np.uint16))


# ------------------------------------------------------------------------------------------------ the project's own rules
def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1e-300)


def test_the_lars_reference_is_the_rule_of_the_simclr_oracle():
    from oracle.simclr import SimCLROracle
    case = ('lars', 'a', 0)                                        # grad_scale 1: the oracle has none
    s, lay, d, ref = U.lars_scalars(case), U.lars_layout(), U.lars_arena(), U.lars_ref(case)
    names = ['s%d' % i for i in range(len(U.LARS_SEGS))]
    cut = lambda t: {n: torch.from_numpy(t[o:o + m].astype(np.float64)) for n, (o, m) in zip(names, lay['slices'])}
    me = types.SimpleNamespace(st=cut(d['p']), velocity=cut(d['v']), mu=s['mu'], coeff=s['coeff'], eps=s['eps'],
                               wd=U.LARS_WD, excluded={n for n, (_, k) in zip(names, U.LARS_SEGS) if k == 'wd0'},
                               lr=lambda: s['lr'], step_count=0)
    SimCLROracle.apply_lars(me, cut(d['g']))
    for n, (o, m) in zip(names, lay['slices']):
        assert _close(ref['p'][0][o:o + m], me.st[n].numpy()) and _close(ref['v'][0][o:o + m], me.velocity[n].numpy()), n


@pytest.mark.parametrize('clip', (0, 1))
def test_the_larc_reference_is_the_update_of_the_linear_probe_oracle(clip):
    from oracle.linprobe_v2 import LinearProbeOracle
    case = ('larc', 'a', clip)
    s, lay, d, ref = U.lars_scalars(case), U.lars_layout(), U.lars_arena(), U.lars_ref(case)
    names = ['s%d' % i for i in range(len(U.LARS_SEGS))]
    cut = lambda t: {n: torch.from_numpy(t[o:o + m].astype(np.float64)) for n, (o, m) in zip(names, lay['slices'])}
    decayed = [n for n, (_, k) in zip(names, U.LARS_SEGS) if k != 'wd0']
    for group, wd in ((decayed, U.LARS_WD), ([n for n in names if n not in decayed], 0.0)):
        me = types.SimpleNamespace(st=cut(d['p']), exp_avg=cut(d['v']), optimizer='MomentumLARC', mu=s['mu'], wd=wd,
                                   tc=s['coeff'], clip=bool(clip), eps=s['eps'], lr=lambda: s['lr'], step_count=0)
        g = cut(d['g'])
        LinearProbeOracle.update(me, {n: g[n] for n in group})
        for n in group:
            o, m = lay['slices'][names.index(n)]
            assert _close(ref['p'][0][o:o + m], me.st[n].numpy()), n
            assert _close(ref['v'][0][o:o + m], me.exp_avg[n].numpy()), n


def test_the_adamw_reference_is_the_rule_of_the_mae_oracle():
    from oracle.mae import MAEOracle
    # the oracle forms b^t in double, the kernel is handed float32(b^t): the whole rule is compared at t = 1, where
    # b^t = b (grad_scale 1: the oracle has none), the moments also from a warm state
    case = (1025, 'warm')
    d, ref = U.adamw_data(case), U.adamw_ref(case)
    t64 = lambda n: torch.from_numpy(d[n].astype(np.float64))
    me = types.SimpleNamespace(st={'w': t64('p')}, m={'w': t64('m')}, v={'w': t64('v')}, b1=d['b1'], b2=d['b2'],
                               eps=d['eps'], wd=d['wd'], lr=lambda: d['lr'], step_count=999)
    MAEOracle.apply_adamw(me, {'w': t64('g')})
    assert _close(ref['m'][0], me.m['w'].numpy()) and _close(ref['v'][0], me.v['w'].numpy())
    case = (1025, 'plain')
    d, ref = U.adamw_data(case), U.adamw_ref(case)
    me = types.SimpleNamespace(st={'w': t64('p')}, m={}, v={}, b1=d['b1'], b2=d['b2'], eps=d['eps'], wd=d['wd'],
                               lr=lambda: d['lr'], step_count=0)
    MAEOracle.apply_adamw(me, {'w': t64('g')})
    for n, got in (('p', me.st['w']), ('m', me.m['w']), ('v', me.v['w'])):
        assert _close(ref[n][0], got.numpy()), n


# ------------------------------------------------------------------------------------------------ planted defects
EMA = (U.ema_ref, U.ema_eval32)
SGD = (U.sgd_ref, U.sgd_eval32)
ADAMW = (U.adamw_ref, U.adamw_eval32)
LARS = (U.lars_ref, U.lars_eval32)
SLAB = (U.slab_ref, U.slab_eval32)
DEFECTS = [          # what is planted, the twin's switch, family, the case that must catch it, the tensor
    ('the tail is skipped', 'skip_tail', EMA, (7, 'plain'), 'k'),
    ('the tail is skipped', 'skip_tail', SGD, (7, 'plain'), 'p'),
    ('the tail is skipped', 'skip_tail', ADAMW, (7, 'plain'), 'p'),
    ('wd multiplies g instead of p', 'wd_on_g', SGD, (1025, 'plain'), 'v'),
    ('the velocity is not scaled by mu', 'no_mu', SGD, (1025, 'warm'), 'v'),
    ('grad_scale once instead of squared in the gradient norm', 'gs_once', LARS, ('lars', 'b', 0), 'norms'),
    ("a segment takes its predecessor's norm", 'prev_norm', LARS, ('lars', 'a', 0), 'v'),
    ('the last block of a segment is dropped from the norm', 'drop_last_block', LARS, ('lars', 'a', 0), 'norms'),
    ('the segment reduce stops after 256 blocks', 'reduce_256', LARS, ('lars', 'a', 0), 'norms'),
    ('LARC clip uses a instead of a / lr', 'clip_a', LARS, ('larc', 'a', 1), 'v'),
    ('LARC applies weight decay on the zero-norm branch', 'wd_zero_branch', LARS, ('larc', 'a', 0), 'v'),
    ('b1p and b2p are swapped', 'swap_pows', ADAMW, (1025, 'plain'), 'p'),
    ('eps instead of eps sqrt(1 - b2p)', 'eps_raw', ADAMW, (1025, 'tiny_grad'), 'p'),
    ('the decay is applied after the step', 'decay_after', ADAMW, (4099, 'mixed'), 'p'),
    ('EMA uses 1 - m with m rounded to bf16', 'om_bf16', EMA, (1025, 'plain'), 'k'),
    ('slab_reduce ignores accumulate', 'ignore_accumulate', SLAB, (64, 5, 1, 'plain'), 'out'),
]


@pytest.mark.parametrize('what,defect,family,case,tensor', DEFECTS, ids=['%s-%d' % (d[1], i) for i, d in enumerate(DEFECTS)])
def test_planted_defect(what, defect, family, case, tensor):
    ref_fn, eval_fn = family
    ref = ref_fn(case)[tensor]
    sound, _ = U.usage(eval_fn(case)[tensor], *ref)
    broken, idx = U.usage(eval_fn(case, defect)[tensor], *ref)
    print('FIG host defect %s: %s %.3g of the bound (sound: %.3f)' % (defect, tensor, broken, sound))
    assert sound <= U.HEADROOM
    assert broken > 1.0, '%s goes unnoticed: %s stays at %.3f of its bound' % (what, tensor, broken)


def test_planted_defect_in_the_bit_exact_kernels():
    """Each changes a bit of what the GPU test compares bit for bit."""
    case = (64, 33, 0, 'cancelling')                              # bit equality only: the float64 bound holds for any order
    sound, rev = U.slab_eval32(case)['out'], U.slab_eval32(case, 'reverse_lanes')['out']
    assert not np.array_equal(U.bits(sound), U.bits(rev))
    assert U.usage(rev, *U.slab_ref(case)['out'])[0] <= 1.0
    case = (64, 5, 1, 'plain')
    assert not np.array_equal(U.bits(U.slab_eval32(case)['out']), U.bits(U.slab_eval32(case, 'ignore_accumulate')['out']))
    x = U.CAST_PATTERNS.view(np.float32)
    assert not U.bf16_equal(U.cast_expect(x, 'bf16_truncate'), U.cast_expect(x))
    x = U.cast_data(9)
    assert not U.bf16_equal(U.cast_expect(x, 'skip_tail'), U.cast_expect(x))
    case = (1025, 'plain')
    assert not np.array_equal(U.ema_eval32(case, 'bf16_truncate')['k_lp'], U.ema_eval32(case)['k_lp'])
    want, mask = U.pack_expect(False)
    for defect, job in (('cpad_off_by_one', 'stem'), ('double_transpose', 't33x65')):
        got = U.pack_eval32(defect)
        pk = [j[1] for j in U.pack_case()['jobs'] if j[0] == job][0]
        sl = slice(pk.dst_off, pk.dst_off + pk.size)
        assert not U.same_bits_or_nan(got[sl], want[sl]), defect
