"""Adan on the MI355X.  Kernel level: the four launches against the float64 statement of the rule on the reference's
vectors (tests/golden/adan_vectors.npz) at 4 x max(the reference's own error, one fp32 ulp), sizes up to a second sweep
of the capped grid with guard bands, the grouped kernel bit for bit against the flat one, the clip coefficient, the
first-step flag read from device memory, refused arguments.  Optimizer level: parity with the reference's Adan on the
fine-tuning model (tests/golden/adan_mae_ft_small.npz, plain and clipped), replay from a step plan recorded at t == 2
and at t == 1 while the schedule moves, state_dict round trip, the YAML through the Engine."""
import math
import os

import numpy as np
import pytest
import torch

import adan_util as U
import grad_clip_util

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, 'tests', 'golden', 'adan_vectors.npz')
MODEL = os.path.join(ROOT, 'tests', 'golden', 'adan_mae_ft_small.npz')
B1, B2, B3 = U.BETAS
EPS = U.EPS
CFG = (B1, B2, B3, EPS)
LR = 1e-2
FT_TOL_F32 = dict(loss=1e-3, param=1e-4)              # tests/test_adamw_groups_gpu.py, unchanged
FT_TOL_BF16 = dict(loss=3e-2, param=1e-2)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _hyper(t, lr, first=None):
    first = (t == 1) if first is None else first
    return torch.tensor([lr, B1 ** t, B2 ** t, B3 ** t, 1.0 if first else 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)


def _zeros(n, k=4):
    return [torch.zeros(n, device=DEV) for _ in range(k)]


def _buffers(n, seed, steps=2):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10 ** torch.empty(n).uniform_(-4, 0, generator=gen) for _ in range(steps)]
    return p, grads


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize('run', ['prox', 'noprox'])
def test_kernel_against_the_float64_rule_on_the_reference_vectors(run):
    """The fixture's five tensors side by side in one buffer, one segment each with its group's (lr_scale, decay), four
    steps through ops.adan_groups_dev: after every step every buffer of every tensor lies within 4 x max(ref_err, one
    fp32 ulp of the tensor's largest magnitude) of the float64 statement.  Elements whose gradient is zero throughout
    keep m = d = s = pre = 0 exactly and move by the decay only."""
    from passl_amd.hip import ops
    z = np.load(VECTORS)
    no_prox = dict(U.vector_runs(z))[run]
    names = U.vector_names(z)
    sizes = [z['p0/' + n].size for n in names]
    ends = np.cumsum(sizes).tolist()
    n_all = ends[-1]
    cfgs = [U.vector_config(z, n) for n in names]
    table = ops.adamw_groups_table(ends, [s for s, _w in cfgs], [w for _s, w in cfgs], n_all, DEV)
    p = torch.from_numpy(np.concatenate([z['p0/' + n] for n in names])).to(DEV)
    p0 = p.clone()
    m, d, s, pre = _zeros(n_all)
    want = {n: U.trajectory(z, n, no_prox) for n in names}
    zero_g = torch.from_numpy(np.concatenate([np.stack([z['g_s%d/%s' % (t, n)] for t in range(1, 5)]) for n in names], 1)
                              == 0).all(0).to(DEV)
    assert int(zero_g.sum()) >= 300                                          # an eighth of every tensor but the tiny one
    worst, worst_at, prev = 0.0, None, p0.clone()
    for t in range(1, int(z['steps']) + 1):
        g = torch.from_numpy(np.concatenate([z['g_s%d/%s' % (t, n)] for n in names])).to(DEV)
        ops.adan_groups_dev(p, g, m, d, s, pre, table, _hyper(t, float(z['lr'][t - 1])), *CFG, no_prox, 1.0)
        got = dict(p=p, m=m, d=d, s=s, pre=pre)
        off = 0
        for n, end in zip(names, ends):
            errs = z['%s_s%d_ref_err/%s' % (run, t, n)]
            for bi, b in enumerate(U.BUFFERS):
                ref = z['%s_s%d_%s/%s' % (run, t, b, n)]
                bd = U.bound(errs[bi], ref)
                err = float(np.max(np.abs(got[b][off:end].double().cpu().numpy() - want[n][t - 1][b])))
                if err / bd > worst:
                    worst, worst_at = err / bd, (n, t, b, err, bd)
            off = end
        for buf in (m, d, s, pre):
            assert not buf[zero_g].any()                                      # exactly zero
        decayed = torch.from_numpy(np.repeat([w > 0 for _s, w in cfgs], sizes)).to(DEV) & zero_g
        assert torch.equal(_bits(p[zero_g & ~decayed]), _bits(p0[zero_g & ~decayed]))       # no decay: untouched
        moved = p[decayed].abs() < prev[decayed].abs()
        assert bool(moved.all()) and torch.equal(torch.sign(p[decayed]), torch.sign(p0[decayed]))   # shrunk, nothing else
        prev = p.clone()
    print('adan kernel against float64, run %s: largest err / bound = %.3f at %r' % (run, worst, worst_at))
    assert worst <= 1.0, worst_at


# ---------------------------------------------------------------------------------------------- 2. sizes
@pytest.mark.parametrize('n', [4, 4100, 2 ** 20 + 24, 2 ** 21 + 2 ** 19 + 24])
def test_flat_kernel_sizes_against_the_twin_with_guard_bands(n):
    """One float4 (4), a partial workgroup after 4 full ones (4100), more than one grid round of whole workgroups
    (2**20 + 24) and a second sweep of the capped grid (2**21 + 2**19 + 24 = 655366 float4 > 2048 * 256).  Two steps
    (the second takes the difference branch).  Bound: that of test 1 with the twin's own distance to float64 in the
    place of the reference's; the kernel is held to it against float64 AND against the twin.  A guard band behind every
    buffer keeps its sentinel."""
    from passl_amd.hip import ops
    GUARD, SENT = 64, -7.25
    p0, grads = _buffers(n, 17 + n % 1000)
    bufs = []
    for src in (p0, None, None, None, None):
        b = torch.full((n + GUARD,), SENT, device=DEV)
        b[:n] = src.to(DEV) if src is not None else 0.0
        bufs.append(b)
    gbuf = torch.full((n + GUARD,), SENT, device=DEV)
    f64, f32 = U.zero_state(p0.numpy()), U.zero_state(p0.numpy(), np.float32)
    worst = 0.0
    for t, g in enumerate(grads, 1):
        gbuf[:n] = g.to(DEV)
        lr = LR * (1.0 - 0.1 * t)
        ops.adan_dev(bufs[0][:n], gbuf[:n], bufs[1][:n], bufs[2][:n], bufs[3][:n], bufs[4][:n], _hyper(t, lr), *CFG, 0.02,
                     False, 0.5)
        lr32 = float(np.float32(lr))
        f64 = U.adan_rule(f64, g.numpy(), t, lr32, 0.02, grad_scale=0.5)
        f32 = U.adan_rule_f32(f32, g.numpy(), t, lr32, 0.02, grad_scale=0.5)
        for bi, b in enumerate(U.BUFFERS):
            got = bufs[bi][:n].double().cpu().numpy()
            twin_err = float(np.max(np.abs(f32[b].astype(np.float64) - f64[b])))
            bd = U.bound(twin_err, f64[b])
            e64 = float(np.max(np.abs(got - f64[b])))
            e32 = float(np.max(np.abs(got - f32[b].astype(np.float64))))
            worst = max(worst, e64 / bd, e32 / bd)
            assert e64 <= bd and e32 <= bd, (n, t, b, e64, e32, bd)
    print('adan flat kernel, n = %d: largest err / bound = %.3f' % (n, worst))
    torch.cuda.synchronize()
    for b in bufs + [gbuf]:
        assert bool((b[n:] == SENT).all())
    assert not torch.equal(bufs[0][:n].cpu(), p0)


# ---------------------------------------------------------------------------------------------- 3. segments = flat
def _cuts(n, n_seg, gen):
    inner = torch.randperm(n // 4 - 1, generator=gen)[:n_seg - 1] + 1
    return sorted((inner * 4).tolist()) + [n]


@pytest.mark.parametrize('no_prox', [False, True])
@pytest.mark.parametrize('n_seg', [1, 3, 300])
def test_uniform_table_equals_the_flat_kernel_bit_for_bit(n_seg, no_prox):
    from passl_amd.hip import ops
    n = 2 ** 20 + 24
    gen = torch.Generator().manual_seed(n_seg)
    table = ops.adamw_groups_table(_cuts(n, n_seg, gen), [1.0] * n_seg, [0.02] * n_seg, n, DEV)
    p0, grads = _buffers(n, 11, steps=3)
    pa, pb = p0.to(DEV), p0.to(DEV)
    sa, sb = _zeros(n), _zeros(n)
    for t, g in enumerate(grads, 1):
        g = g.to(DEV)
        lr = LR * (1.0 - 0.1 * t)
        ops.adan_dev(pa, g, *sa, _hyper(t, lr), *CFG, 0.02, no_prox, 0.5)
        ops.adan_groups_dev(pb, g, *sb, table, _hyper(t, lr), *CFG, no_prox, 0.5)
        assert _same([pa] + sa, [pb] + sb), t
    assert not torch.equal(pa.cpu(), p0)


LENGTHS = [4, 8, 12, 1000, 4096, 4100, 65540]


@pytest.mark.parametrize('n_seg', [2, 7, 300, 5000])
def test_groups_equal_the_flat_kernel_per_slice_bit_for_bit(n_seg):
    """Segment s of the grouped launch = the flat launch on that slice alone with lr = fp32(lr) * fp32(scale_s), handed
    over in a second hyper block, and wd_s: no tolerance.  Lengths of 4, 8 and 12 elements put boundaries inside one
    wave of a workgroup tile; the 65540s keep whole tiles apart; there is no segment limit."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(n_seg)
    if n_seg == 2:
        lens = [4100, 65540]
    elif n_seg == 7:
        lens = [LENGTHS[i] for i in torch.randperm(7, generator=gen).tolist()]
    else:
        w = torch.tensor([0.3, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05])
        lens = LENGTHS + [LENGTHS[i] for i in torch.multinomial(w, n_seg - 7, replacement=True, generator=gen).tolist()]
        lens = [lens[i] for i in torch.randperm(n_seg, generator=gen).tolist()]
    ends = np.cumsum(lens).tolist()
    n = ends[-1]
    scales = torch.empty(n_seg).uniform_(0.01, 1.0, generator=gen).tolist()
    scales[0] = 1.0
    wds = [[0.0, 0.02, 0.3][i] for i in torch.randint(0, 3, (n_seg,), generator=gen).tolist()]
    table = ops.adamw_groups_table(ends, scales, wds, n, DEV)
    p0, grads = _buffers(n, 5 + n_seg)
    pa, pb = p0.to(DEV), p0.to(DEV)
    sa, sb = _zeros(n), _zeros(n)
    for t, g in enumerate(grads, 1):
        g = g.to(DEV)
        lr = LR * (1.0 - 0.1 * t)
        rows = np.zeros((n_seg, 8), dtype=np.float32)
        rows[:, 0] = np.float32(lr) * np.asarray(scales, dtype=np.float32)
        rows[:, 1:5] = [B1 ** t, B2 ** t, B3 ** t, 1.0 if t == 1 else 0.0]
        hyp = torch.from_numpy(rows).to(DEV)
        off = 0
        for i, (end, wd) in enumerate(zip(ends, wds)):
            ops.adan_dev(pa[off:end], g[off:end], *[x[off:end] for x in sa], hyp[i], *CFG, wd, False, 1.0 / 3.0)
            off = end
        ops.adan_groups_dev(pb, g, *sb, table, _hyper(t, lr), *CFG, False, 1.0 / 3.0)
        assert torch.equal(_bits(pa), _bits(pb)), 'step %d: %d elements differ' % (t, int((pa != pb).sum()))
        assert _same(sa, sb)
    assert not torch.equal(pa.cpu(), p0)


# ---------------------------------------------------------------------------------------------- 4. clip
def test_flat_clip_coefficient_from_device_memory():
    """Coefficient 1.0 = the unclipped bits.  Coefficient 0.25 on grad_scale 0.5 = the unclipped kernel on grad_scale
    0.125: (g * 0.5) * 0.25 and g * 0.125 are the same float, powers of two being exact.  pre holds that product."""
    from passl_amd.hip import ops
    n = 4100
    p0, grads = _buffers(n, 23, steps=3)
    pa, pb, pc, pd = (p0.to(DEV) for _ in range(4))
    sa, sb, sc, sd = (_zeros(n) for _ in range(4))
    one = torch.tensor([9.0, 1.0], device=DEV)[1:]                   # views into a {norm, coef} row
    quarter = torch.tensor([4.0, 0.25], device=DEV)[1:]
    for t, g in enumerate(grads, 1):
        g = g.to(DEV)
        h = _hyper(t, LR)
        ops.adan_dev(pa, g, *sa, h, *CFG, 0.02, False, 0.5)
        ops.adan_clip_dev(pb, g, *sb, h, one, *CFG, 0.02, False, 0.5)
        assert _same([pa] + sa, [pb] + sb), t
        ops.adan_dev(pc, g, *sc, h, *CFG, 0.02, False, 0.125)
        ops.adan_clip_dev(pd, g, *sd, h, quarter, *CFG, 0.02, False, 0.5)
        assert _same([pc] + sc, [pd] + sd), t
        assert torch.equal(_bits(sd[3]), _bits(g * 0.125)) and not torch.equal(sd[3], sb[3])
    assert not torch.equal(pa, pc)


def test_grouped_clip_reads_the_coefficient_of_each_segments_set():
    """Per-segment coefficients through seg_set from the {norm, coef} table; a set outside [0, n_sets) — the table's -1 and
    an index beyond the table alike — takes coefficient 1.  The bits are those of ops.adan_groups_dev fed (g * gs) * coef."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(4)
    lens = [LENGTHS[i] for i in torch.randperm(7, generator=gen).tolist()]
    ends = np.cumsum(lens).tolist()
    n, n_sets = ends[-1], 3
    scales, wds = [1.0, 0.5, 0.25, 1.0, 0.7, 0.3, 0.9], [0.02, 0.0, 0.02, 0.3, 0.0, 0.02, 0.02]
    sets = [0, -1, 2, 1, 0, -1, 2]
    table = ops.adamw_groups_clip_table(ends, scales, wds, sets, n, n_sets, DEV)
    plain = ops.adamw_groups_table(ends, scales, wds, n, DEV)
    table['seg_set'][5] = n_sets + 4                                  # beyond the table: the kernel reads nothing there
    clip = torch.tensor([[3.0, 0.3], [1.5, 1.0], [40.0, 0.025]], device=DEV)
    coefs = [0.3, 1.0, 0.025, 1.0, 0.3, 1.0, 0.025]
    coef = torch.from_numpy(np.repeat(np.asarray(coefs, dtype=np.float32), lens)).to(DEV)
    p0, grads = _buffers(n, 29, steps=3)
    pa, pb = p0.to(DEV), p0.to(DEV)
    sa, sb = _zeros(n), _zeros(n)
    gs = torch.tensor(1.0 / 3.0, dtype=torch.float32, device=DEV)
    for t, g in enumerate(grads, 1):
        g = g.to(DEV)
        h = _hyper(t, LR)
        ops.adan_groups_clip_dev(pa, g, *sa, table, h, clip, *CFG, True, 1.0 / 3.0)
        clipped = (g * gs) * coef
        ops.adan_groups_dev(pb, clipped, *sb, plain, h, *CFG, True, 1.0)
        assert _same([pa] + sa, [pb] + sb), t
        assert torch.equal(_bits(sa[3]), _bits(clipped))              # pre holds the clipped gradient
    assert not torch.equal(pa.cpu(), p0)


# ---------------------------------------------------------------------------------------------- 5. first, from device memory
def test_first_step_flag_is_read_from_device_memory():
    """Two launches that differ in hyper[4] alone.  first = 1: whatever pre holds (NaN, huge, anything) reaches no output.
    first = 0: it does."""
    from passl_amd.hip import ops
    n = 4100
    p0, grads = _buffers(n, 31, steps=1)
    g = grads[0].to(DEV)
    garbage = torch.randn(n, device=DEV) * 1e3
    garbage[::3] = float('nan')
    garbage[1::3] = 3e38
    outs = {}
    for name, pre0, first in (('clean', torch.zeros(n, device=DEV), True), ('garbage', garbage.clone(), True),
                              ('clean0', torch.zeros(n, device=DEV), False), ('garbage0', garbage.clone(), False)):
        p = p0.to(DEV)
        m, d, s = _zeros(n, 3)
        ops.adan_dev(p, g, m, d, s, pre0, _hyper(2, LR, first=first), *CFG, 0.02, False, 1.0)
        outs[name] = [p, m, d, s, pre0]
    assert _same(outs['clean'], outs['garbage'])
    assert not outs['clean'][2].any() and torch.equal(_bits(outs['clean'][4]), _bits(g))
    assert not _same(outs['clean0'][:4], outs['garbage0'][:4])
    assert bool(torch.isnan(outs['garbage0'][2][::3]).all()) and torch.isfinite(outs['clean0'][0]).all()
    assert not torch.equal(outs['clean0'][2], outs['clean'][2])       # first = 0 on a zero pre: diff = gg, not 0


# ---------------------------------------------------------------------------------------------- 6. model parity
def _run_model_golden(run, dtype, tol, parity):
    from test_adamw_groups_gpu import _build_finetune
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import Adan
    z = np.load(MODEL)
    N, hw, steps, classes = [int(v) for v in z['meta']]
    torch.manual_seed(0)
    model, keys_shapes = _build_finetune(dtype, classes)
    assert ['%s:%s' % (k, 'x'.join(map(str, s))) for k, s in keys_shapes] == [str(k) for k in z['keys']]
    model.train()
    gc = C(clip_norm=float(z['clip_norm'])) if run == 'clip' else None
    opt = Adan(float(z['lr']), betas=tuple(float(b) for b in z['betas']), eps=float(z['eps']),
               weight_decay=float(z['weight_decay']), parameters=list(model.parameters()), grad_clip=gc)
    assert opt._tables == [None] and (opt._clip is not None) == (run == 'clip')
    watch, elem = [str(n) for n in z['watch']], [str(n) for n in z['elementwise']]
    ps = dict(model.named_parameters())
    arena = model.arena_q

    def state(buf, name):
        # a state vector has the arena's layout: read it through the parameter's own strided view of its slot
        p = ps[name]
        return torch.as_strided(buf[0], p.shape, p.stride(), p.storage_offset()).detach().double().cpu().numpy().reshape(-1)

    gen = torch.Generator().manual_seed(909)
    report, bad = [], []

    def check(what, err, bound):
        line = '%-64s err %.3e  bound %.3e' % (what, err, bound)
        report.append(line)
        if not err <= bound:
            bad.append(line)

    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        out = model(x.to(DEV), y.to(DEV), mode='train')
        opt.clear_grad()
        out['loss'].backward()
        unclipped = arena.grads.clone()
        opt.step()
        assert torch.equal(_bits(arena.grads), _bits(unclipped))           # param.grad keeps the unclipped gradient
        pre = '%s_s%d_' % (run, s)
        ref_loss = float(z[pre + 'loss'])
        check(pre + 'loss', abs(float(out['loss'].detach()) - ref_loss) / abs(ref_loss), tol['loss'] * (1.0 if s == 0 else 20.0))
        if s == 0:
            for n in watch:
                ref = float(z[pre + 'pnorm/' + n])
                check(pre + 'pnorm/' + n, abs(ps[n].detach().double().norm().item() - ref) / ref, tol['param'])
        if run == 'clip':
            got = opt.grad_norms().detach().double().cpu().numpy()
            assert got.shape == (1, 2) and np.isfinite(got).all()
            if parity:
                ref_norm, ref_coef = float(z[pre + 'set_norm'][0]), float(z[pre + 'set_coef'][0])
                check(pre + 'set norm', abs(got[0, 0] - ref_norm) / ref_norm, grad_clip_util.NORM_BOUND)
                check(pre + 'set coefficient', abs(got[0, 1] - ref_coef) / ref_coef, grad_clip_util.NORM_BOUND)
                assert (got[0, 1] == 1.0) == (ref_coef == 1.0)
        if parity and s == 0:
            for n in elem:
                ref = z[pre + 'p/' + n].astype(np.float64).reshape(-1)
                got = ps[n].detach().double().cpu().numpy().reshape(-1)
                check(pre + 'p/' + n, float(np.max(np.abs(got - ref))), tol['param'] * float(np.max(np.abs(ref))))
                ref = z[pre + 'pre/' + n].astype(np.float64).reshape(-1)
                check(pre + 'pre_grad/' + n, float(np.linalg.norm(state(opt._pre, n) - ref) / np.linalg.norm(ref)),
                      grad_clip_util.M_BOUND)
    print('\n'.join(report))                                  # every figure, before the assertion
    assert not bad, 'parity violations:\n' + '\n'.join(bad)


@pytest.mark.parametrize('run', list(U.MODEL_RUNS))
def test_finetune_adan_golden_fp32(run):
    """fp32 is the parity claim: loss and pnorm at the bounds of test_finetune_layer_decay_golden_fp32, the clipped run's
    set norm and coefficient at those of tests/test_grad_clip_gpu.py; the element-wise tensors after the first update at
    the pnorm bound times their largest magnitude, pre_grad (the clipped gradient) at the exp_avg bound."""
    _run_model_golden(run, torch.float32, FT_TOL_F32, True)


def test_finetune_adan_golden_bf16():
    """The bf16 path runs the same update within the project's bf16 bounds (loss, pnorm); no parity claim."""
    _run_model_golden('plain', torch.bfloat16, FT_TOL_BF16, False)


# ---------------------------------------------------------------------------------------------- 7. replay
@pytest.mark.parametrize('warmup', [1, 0])
def test_step_plan_replays_grouped_clipped_adan_while_the_schedule_moves(warmup):
    """Adan on groups with clipping through a step plan: the replayed steps read the rate, the beta powers and the
    first-step flag of THEIR step from device memory.  warmup = 0 records the plan at t == 1 (first = 1 while recording)
    and replays it at t >= 2: losses and the whole arena equal the eager twin's, bit for bit, at every step.  (With
    warmup = 0 one forward / backward without an update runs first, in both twins alike, so that nothing of the model
    is set up while the step is recorded.)"""
    from test_adamw_groups_gpu import _tiny_groups, _tiny_step_model
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.lr_scheduler import CosineAnnealingDecay
    from passl_amd.solver.optimizer import Adan
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    B, T, dim, classes, steps = 16, 17, 128, 16, 4
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(B * T, dim, generator=gen).to(DEV), torch.randint(0, classes, (B,), generator=gen).to(DEV))
               for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        torch.manual_seed(9)
        model = _tiny_step_model(dim, 4, classes, B, T)
        model.train()
        sched = CosineAnnealingDecay(1e-3, T_max=6)
        opt = Adan(sched, weight_decay=0.02, parameters=_tiny_groups(model), grad_clip=C(0.05))
        assert 'seg_set' in opt._tables[0] and opt._tables[0]['n_seg'] >= 4 and opt._clip['n_sets'] == len(_tiny_groups(model))

        def full_step(x, y):
            out = model(x, y)
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            opt.step()
            return out
        if warmup == 0:
            out = model(*batches[0])
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            torch.cuda.synchronize()
            opt.clear_grad()
        sp = StepPlan(full_step, optimizers=[opt], warmup=warmup, enabled=(mode == 'plan'), strict=True)
        losses, lrs, flats, firsts = [], [], [], []
        for x, y in batches:
            lrs.append(opt.get_lr())
            out = sp.run(x, y)
            sched.step()
            losses.append(out['loss'].detach().clone().reshape(1))
            flats.append(model.arena_q.flat[:model.arena_q.n_train].clone())
            firsts.append(opt._hyper_dev[4:5].clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= steps - 1 - warmup
            print('step plan:', sp.info)
        assert len(set(lrs)) == steps and opt.state_dict()['t'] == steps
        assert torch.cat(firsts).tolist() == [1.0] + [0.0] * (steps - 1)
        results[mode] = (torch.cat(losses).cpu(), torch.stack(flats).cpu(), opt._pre[0].cpu(), opt.grad_norms().cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, fa, qa, na), (lb, fb, qb, nb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(qa), _bits(qb)) and torch.equal(_bits(na), _bits(nb))
    for s in range(steps):
        assert torch.equal(_bits(fa[s]), _bits(fb[s])), 'parameters differ after step %d' % s
    assert not torch.equal(fa[steps - 1], fa[steps - 2]) and (na[:, 1] < 1.0).any()


# ---------------------------------------------------------------------------------------------- 8. state_dict
def test_state_dict_round_trip_gives_identical_bits():
    from test_adamw_groups_gpu import _build_finetune
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.lr_decay import param_groups_lrd
    from passl_amd.solver.optimizer import Adan
    gen = torch.Generator().manual_seed(21)
    data = [(torch.randn(8, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 16, (8,), generator=gen).to(DEV))
            for _ in range(3)]

    def make():
        torch.manual_seed(0)
        model, _ = _build_finetune(torch.float32)
        model.train()
        return model, Adan(1e-3, weight_decay=0.02, grad_clip=C(1.0),
                           parameters=param_groups_lrd(model, 0.02, {'pos_embed', 'cls_token'}, 0.65))

    def step(model, opt, x, y):
        out = model(x, y, mode='train')
        opt.clear_grad()
        out['loss'].backward()
        opt.step()

    m1, o1 = make()
    for x, y in data[:2]:
        step(m1, o1, x, y)
    sd, weights = o1.state_dict(), {k: v.detach().clone() for k, v in m1.state_dict().items()}
    assert sorted(sd) == ['exp_avg_0', 'exp_avg_diff_0', 'exp_avg_sq_0', 'pre_grad_0', 't'] and sd['t'] == 2
    assert all(bool(sd[k].any()) for k in sd if k != 't')
    step(m1, o1, *data[2])
    m2, o2 = make()
    m2.load_state_dict(weights)
    o2.set_state_dict(sd)
    step(m2, o2, *data[2])
    assert o2._hyper_dev[4].item() == 0.0 and o2.state_dict()['t'] == 3       # resumed: never the first-step branch
    a, b = m1.arena_q, m2.arena_q
    assert torch.equal(_bits(a.flat[:a.n_train]), _bits(b.flat[:b.n_train]))
    for x, y in zip((o1._m, o1._d, o1._s, o1._pre), (o2._m, o2._d, o2._s, o2._pre)):
        assert torch.equal(_bits(x[0]), _bits(y[0]))


# ---------------------------------------------------------------------------------------------- 9. bad arguments
def test_bad_arguments_are_refused_before_any_launch():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib = L.load()
    n = 4104
    p0, grads = _buffers(n + 4, 3, steps=1)
    p, g = p0.to(DEV), grads[0].to(DEV)
    m, d, s, pre = _zeros(n + 4)
    t = ops.adamw_groups_clip_table([8, 4104], [1.0, 0.5], [0.02, 0.0], [0, 1], n, 2, DEV)
    hyper, coef, clip = _hyper(1, LR), torch.tensor([0.5], device=DEV), torch.ones(2, 2, device=DEV)
    six = [x.data_ptr() for x in (p, g, m, d, s, pre)]
    tail = [B1, B2, B3, EPS, 0, 1.0, L.stream()]
    tab = [t['seg_end'].data_ptr(), t['seg_lr_scale'].data_ptr(), t['seg_wd'].data_ptr()]

    def flat(bufs=six, n_=n, h=hyper.data_ptr()):
        return lib.passl_hip_adan_dev(*bufs, n_, h, B1, B2, B3, EPS, 0.02, 0, 1.0, L.stream())

    def groups(bufs=six, n_=n, tb=tab, n_seg=2, h=hyper.data_ptr()):
        return lib.passl_hip_adan_groups_dev(*bufs, n_, *tb, n_seg, h, *tail)

    def groups_clip(n_sets=2, st=t['seg_set'].data_ptr(), cl=clip.data_ptr()):
        return lib.passl_hip_adan_groups_clip_dev(*six, n, *tab, st, 2, hyper.data_ptr(), cl, n_sets, *tail)
    for i in range(6):
        for bad in (None, six[i] + 4):                                               # NULL, not 16-byte aligned
            b = list(six)
            b[i] = bad
            assert flat(bufs=b) == L.EINVAL and groups(bufs=b) == L.EINVAL, (i, bad)
    assert flat(n_=4102) == L.EINVAL and flat(n_=-4) == L.EINVAL and flat(h=None) == L.EINVAL
    assert groups(n_=4102) == L.EINVAL and groups(n_seg=0) == L.EINVAL and groups(h=None) == L.EINVAL
    for i in range(3):
        tb = list(tab)
        tb[i] = None
        assert groups(tb=tb) == L.EINVAL
    assert groups(tb=[tab[0] + 4, tab[1], tab[2]]) == L.EINVAL                       # int64 table not 8-byte aligned
    assert lib.passl_hip_adan_clip_dev(*six, n, hyper.data_ptr(), None, B1, B2, B3, EPS, 0.02, 0, 1.0, L.stream()) == L.EINVAL
    assert groups_clip(n_sets=0) == L.EINVAL and groups_clip(st=None) == L.EINVAL and groups_clip(cl=None) == L.EINVAL
    assert flat(n_=0) == L.OK and groups(n_=0) == L.OK                               # nothing to do
    # the wrappers: a host tensor, a table covering another n, a table naming more sets than the clip table holds
    args = (p[:n], g[:n], m[:n], d[:n], s[:n], pre[:n])
    with pytest.raises(L.PasslHipError):
        ops.adan_dev(p[:n].cpu(), *args[1:], hyper, *CFG, 0.02)
    with pytest.raises(L.PasslHipError):
        ops.adan_clip_dev(*args, hyper, coef.cpu(), *CFG, 0.02)
    with pytest.raises(ValueError):
        ops.adan_groups_dev(p, g, m, d, s, pre, t, hyper, *CFG)
    with pytest.raises(ValueError):
        ops.adan_groups_clip_dev(p, g, m, d, s, pre, t, hyper, clip, *CFG)
    with pytest.raises(ValueError):
        ops.adan_groups_clip_dev(*args, t, hyper, torch.ones(1, 2, device=DEV), *CFG)
    with pytest.raises(ValueError):
        ops.adan_dev(*args, torch.zeros(4, device=DEV), *CFG, 0.02)                   # a 4-wide hyper block
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(p0.to(DEV))) and not any(bool(x.any()) for x in (m, d, s, pre))   # nothing ran
    assert groups_clip() == L.OK
    torch.cuda.synchronize()
    assert not torch.equal(p[:n], p0[:n].to(DEV)) and torch.equal(_bits(p[n:]), _bits(p0[n:].to(DEV)))   # bounded by n
    assert not any(bool(x[n:].any()) for x in (m, d, s, pre))


# ---------------------------------------------------------------------------------------------- 10. the YAML
def test_engine_trains_the_adan_vit_yaml(tmp_path):
    """configs/v2/vit_base_adan_synthetic.yaml at a reduced size through the Engine, exactly as
    test_engine_trains_the_supervised_vit_yaml runs its twin: two steps, two accumulated micro-batches each, bf16."""
    from test_vit_dropout_gpu import ARCH
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N, steps = 8, 2
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_adan_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'Global.eval_during_train=False', 'LRScheduler.warmup_steps=3',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 4), 'DataLoader.Train.dataset.image_size=64',
                      'DataLoader.Train.dataset.num_classes=16', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=64',
                      'DataLoader.Eval.dataset.num_classes=16', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'ViT_base_patch16_224' and cfg['Optimizer']['name'] == 'Adan'
    cfg['Model'] = dict(name='VisionTransformer', drop_rate=cfg['Model']['drop_rate'], qkv_bias=True, epsilon=1e-6,
                        representation_size=64, **ARCH)
    cfg['Global']['max_train_step'] = steps
    eng = Engine(cfg, mode='train')
    opt = eng.optimizer
    assert type(opt).__name__ == 'Adan' and opt._wd == 0.02 and opt._clip is None and eng.accum_steps == 2
    assert type(eng.lr_scheduler).__name__ == 'ViTLRScheduler'
    arena = opt._arenas[0]
    before = arena.flat[:arena.n_train].clone()
    lrs, losses, pre_after = [], [], []
    inner = eng.train_loop.train_one_step

    def spy(batch):
        lrs.append(opt.get_lr())
        out, ld = inner(batch)
        losses.append(float(ld['loss'].detach().float().reshape(())))
        pre_after.append(bool(opt._pre[0].any()))
        return out, ld
    eng.train_loop.train_one_step = spy
    eng.train()
    print('lr', lrs, 'loss', losses)
    assert eng.global_step == steps and len(losses) == steps
    assert all(math.isfinite(v) and v > 0 for v in losses)
    assert lrs[0] == 0.0 and abs(lrs[1] - 1.5e-2 / 3) < 1e-15
    assert pre_after == [True, True]                                       # pre_grad is non-zero after step 1
    assert not torch.equal(arena.flat[:arena.n_train], before)             # the arena changed
    assert opt.state_dict()['t'] == steps and bool(torch.isfinite(arena.flat[:arena.n_train]).all())
