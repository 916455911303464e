"""Global-norm gradient clipping on the MI355X.  Kernel level: the chunk sums against float64 at a bound that follows from
the length of the addition chains, bit-identical repeats, the finalize kernel bit for bit against the numpy-float32
evaluation of the rule, the clip variants of the AdamW update bit for bit against the existing kernels fed the clipped
gradient, refused arguments.  Model level: the reference's runs with clipping (tests/golden/mae_ft_clip_small.npz: per
group through AdamW(grad_clip=ClipGradByGlobalNorm), over all parameters through clip_grad_norm_), replay from a step
plan, state_dict round trip, the v2 Engine with ``Optimizer.grad_clip``."""
import math
import os

import numpy as np
import pytest
import torch

import grad_clip_util
from test_adamw_groups_gpu import (B1, B2, EPS, FT_TOL_BF16, FT_TOL_F32, LR, _bits, _build_finetune, _hyper, _tiny_groups,
                                   _tiny_step_model)

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mae_ft_clip_small.npz')
LRD_GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mae_ft_lrd_small.npz')
CHUNK = 16384
SIZES = [8, CHUNK - 4, CHUNK, CHUNK + 4, 4104, 2 ** 20 + 24]
U = 2.0 ** -24
f32 = np.float32


def _grad(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=gen) * 10 ** torch.empty(n).uniform_(-4, 0, generator=gen)).to(DEV)


def _block_sum(lanes):
    """The workgroup reduction of the kernels in numpy float32: per wave the xor butterfly (offsets 32 ... 1), then the
    four wave sums left to right."""
    v = lanes.astype(f32).reshape(4, 64)
    idx = np.arange(64)
    with np.errstate(all='ignore'):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, idx ^ o]
        return f32(f32(f32(v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


def _set_sum(values):
    """The finalize kernel's fixed order over one set's partials: lane t adds the entries t, t + 256, ... in order."""
    values = np.asarray(values, dtype=f32)
    lanes = np.zeros(256, dtype=f32)
    for start in range(0, len(values), 256):
        part = np.asarray(values[start:start + 256], dtype=f32)
        lanes[:len(part)] = lanes[:len(part)] + part
    return _block_sum(lanes)


def _rule(sq, clip_norm, clip_max, always):
    """ClipGradByGlobalNorm in numpy float32 (tests/test_grad_clip_host.py pins this evaluation to the statement)."""
    with np.errstate(all='ignore'):
        return _rule_f32(f32(sq), clip_norm, clip_max, always)


def _rule_f32(sq, clip_norm, clip_max, always):
    norm = np.sqrt(sq)
    if not always and norm <= f32(clip_norm):
        return norm, f32(1.0)
    coef = f32(clip_norm) / f32(norm + f32(1e-6))
    return norm, (f32(clip_max) if clip_max is not None and coef > f32(clip_max) else coef)


def _chains(n_chunks):
    """Longest addition chains: a chunk = CHUNK / 1024 float4 per lane over four accumulators, four additions each
    (three inside the float4, one into the accumulator) = CHUNK / 1024, + 2 to merge the accumulators, + 6 shuffle steps,
    + 3 wave sums; a set = ceil(n_chunks / 256) per lane + 6 + 3."""
    return CHUNK // 1024 + 2 + 6 + 3, -(-n_chunks // 256) + 6 + 3


# ---------------------------------------------------------------------------------------------- 1. sum of squares
@pytest.mark.parametrize('grad_scale', [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize('n', SIZES)
def test_sum_of_squares_against_float64(n, grad_scale):
    """Relative error of every chunk's partial <= (K1 + 2) u and of the set's sum <= (K1 + K2 + 2) u, u = 2^-24, K = the
    addition chains: every term is >= 0, so the error of a chain of K additions is at most K u relative, the squaring adds
    one u, second-order terms the rest.  The reference squares fp32(g * grad_scale) in float64.  Two launches: the same
    bits."""
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    assert ops.GRAD_CLIP_CHUNK == CHUNK == L.load().passl_hip_grad_clip_chunk(L.ABI_VERSION)
    g = _grad(n, n)
    plan = ops.grad_clip_plan([[(0, n, 0)]], [n], 1, DEV)
    n_chunks = -(-n // CHUNK)
    assert plan['total'] == n_chunks
    ops.grad_sumsq(g, plan, 0, grad_scale)
    first = plan['partial'].clone()
    plan['partial'].zero_()
    ops.grad_sumsq(g, plan, 0, grad_scale)
    assert torch.equal(_bits(first), _bits(plan['partial']))
    scaled = (g * torch.tensor(grad_scale, dtype=torch.float32, device=DEV)).double()
    want = torch.stack([(scaled[c:c + CHUNK] ** 2).sum() for c in range(0, n, CHUNK)]).cpu().numpy()
    got = first.cpu().numpy()
    k1, k2 = _chains(n_chunks)
    err = np.max(np.abs(got.astype(np.float64) - want) / want)
    print('n %d gs %.3f: chunk error %.2e (bound %.2e)' % (n, grad_scale, err, (k1 + 2) * U))
    assert err <= (k1 + 2) * U
    out = ops.grad_clip_finalize(plan, 1.0).cpu().numpy()
    total = _set_sum(got)
    assert out[0, 0] == np.sqrt(total)                                       # the emulated order IS the kernel's
    err = abs(float(total) - want.sum()) / want.sum()
    print('            set error   %.2e (bound %.2e)' % (err, (k1 + k2 + 2) * U))
    assert err <= (k1 + k2 + 2) * U


def test_chunks_of_several_sets_and_excluded_ranges():
    """Runs of three sets with a gap (an excluded parameter) between them, one of them longer than a chunk: every partial
    is the sum over its own chunk only, what no run covers reaches no norm — poisoned with NaN here."""
    from passl_amd.hip import ops
    n = 3 * CHUNK
    g = _grad(n, 5)
    runs = [(0, 8, 2), (8, 4104, 0), (8200, 8200 + CHUNK + 4, 1), (8200 + CHUNK + 4, n - 4, 0)]
    g[4104:8200] = float('nan')
    g[n - 4:] = float('inf')
    plan = ops.grad_clip_plan([runs], [n], 3, DEV)
    ops.grad_sumsq(g, plan, 0, 1.0)
    host = plan['host']
    got = plan['partial'].cpu().numpy().astype(np.float64)
    want = np.array([float((g[o:o + l].double() ** 2).sum()) for o, l in zip(host['chunk_off'][0], host['chunk_len'][0])])
    assert np.isfinite(got).all() and np.max(np.abs(got - want) / want) <= (_chains(1)[0] + 2) * U
    out = ops.grad_clip_finalize(plan, 1.0).cpu().numpy()
    part = plan['partial'].cpu().numpy()
    for s in range(3):
        mine = host['set_chunks'][host['set_ptr'][s]:host['set_ptr'][s + 1]]
        norm, coef = _rule(_set_sum(part[mine]), 1.0, None, False)
        assert out[s, 0] == norm and out[s, 1] == coef


# ---------------------------------------------------------------------------------------------- 2. finalize
@pytest.mark.parametrize('clip_norm,clip_max,always', [(1.0, None, False), (1.0, 1.0, True), (0.3, None, False),
                                                        (3.0, 2.0, True), (3.0, None, True)])
def test_finalize_is_the_float32_rule_bit_for_bit(clip_norm, clip_max, always):
    """{norm, coef} of every set = the numpy-float32 evaluation of the rule from the partials read back from the device,
    summed in the kernel's order.  Sets interleave chunk by chunk; their norms lie below, exactly at and above clip_norm;
    one set has more than 256 chunks (the strided loop), one is non-finite."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(17)
    n_sets = 8
    sets = torch.randint(4, n_sets - 1, (900,), generator=gen).tolist()     # sets 4 .. 6: random, interleaved; 7: empty
    sets += [0, 1, 1, 2, 3, 3, 3]
    order = torch.randperm(len(sets), generator=gen).tolist()
    sets = [sets[i] for i in order]
    plan = ops.grad_clip_plan([[(4 * i, 4 * i + 4, s) for i, s in enumerate(sets)]], [4 * len(sets)], n_sets, DEV)
    assert plan['total'] == len(sets)
    part = (torch.rand(len(sets), generator=gen) * 0.01).numpy().astype(f32)
    fixed = {0: [clip_norm ** 2], 1: [clip_norm ** 2 / 2, clip_norm ** 2 / 2], 2: [clip_norm ** 2 / 4],
             3: [4.0 * clip_norm ** 2, 1e-3, float('inf' if always else 'nan')]}
    seen = {s: 0 for s in fixed}
    for c, s in enumerate(sets):
        if s in fixed:
            part[c] = fixed[s][seen[s]]
            seen[s] += 1
    plan['partial'].copy_(torch.from_numpy(part))
    out = ops.grad_clip_finalize(plan, clip_norm, clip_max, always).cpu().numpy()
    back = plan['partial'].cpu().numpy()
    host = plan['host']
    counts = []
    for s in range(n_sets):
        mine = host['set_chunks'][host['set_ptr'][s]:host['set_ptr'][s + 1]]
        counts.append(len(mine))
        norm, coef = _rule(_set_sum(back[mine]), clip_norm, clip_max, always)
        assert out[s, 0].tobytes() == norm.tobytes() or (np.isnan(out[s, 0]) and np.isnan(norm)), (s, out[s], norm)
        assert out[s, 1].tobytes() == coef.tobytes() or (np.isnan(out[s, 1]) and np.isnan(coef)), (s, out[s], coef)
    assert max(counts) > 256 and counts[7] == 0
    if clip_norm == 1.0:
        assert out[0, 0] == 1.0 and out[1, 0] == 1.0 and out[2, 0] == 0.5     # at, at (two halves) and below clip_norm
        if not always:
            assert out[0, 1] == 1.0 and out[2, 1] == 1.0                      # norm == clip_norm is not clipped
            assert np.isnan(out[3, 0]) and np.isnan(out[3, 1])                # a NaN norm propagates
        else:
            assert out[0, 1] == f32(1.0) / f32(f32(1.0) + f32(1e-6)) and out[2, 1] == 1.0      # held by clip_norm_max
            assert np.isinf(out[3, 0]) and out[3, 1] == 0.0
    if clip_max is None and always:
        assert out[2, 1] > 1.0                                                # always_clip without a limit scales up


# ---------------------------------------------------------------------------------------------- 3. update
def _clipped(g, gs, coef):
    """torch fp32 (g * gs) * coef: what the clip variants feed the shared update."""
    return (g * torch.tensor(gs, dtype=torch.float32, device=DEV)) * coef


@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 3.0])
@pytest.mark.parametrize('n', SIZES)
def test_flat_clip_variant_equals_the_flat_kernel_on_the_clipped_gradient(n, grad_scale):
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen).to(DEV)
    pa, pb, pc, pd = (p0.clone() for _ in range(4))
    ma, va, mb, vb, mc, vc, md, vd = (torch.zeros(n, device=DEV) for _ in range(8))
    one = torch.ones(1, device=DEV)
    for t, coef in enumerate([0.173, 1.0 / 3.0, 2.5], 1):
        g = _grad(n, 100 * t + 1)
        c = torch.tensor([7.0, coef], dtype=torch.float32, device=DEV)[1:]   # a view into a {norm, coef} row
        ops.adamw_clip_dev(pa, g, ma, va, _hyper(t, LR), c, B1, B2, EPS, 0.05, grad_scale)
        ops.adamw_dev(pb, _clipped(g, grad_scale, c), mb, vb, _hyper(t, LR), B1, B2, EPS, 0.05, 1.0)
        assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
        # coefficient exactly 1: the existing kernel on the raw inputs
        ops.adamw_clip_dev(pc, g, mc, vc, _hyper(t, LR), one, B1, B2, EPS, 0.05, grad_scale)
        ops.adamw_dev(pd, g, md, vd, _hyper(t, LR), B1, B2, EPS, 0.05, grad_scale)
        assert torch.equal(_bits(pc), _bits(pd)) and torch.equal(_bits(mc), _bits(md)) and torch.equal(_bits(vc), _bits(vd))
    assert not torch.equal(pa, p0) and not torch.equal(ma, mc)


@pytest.mark.parametrize('n_seg', [1, 7, 300])
def test_grouped_clip_variant_equals_the_grouped_kernel_per_segment(n_seg):
    """Per-segment coefficients read through seg_set from the {norm, coef} table, -1 = coefficient 1: p / m / v over 3 steps
    carry the bits of ops.adamw_groups_dev fed (g * gs) * coef[segment] with grad_scale 1."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(n_seg)
    lens = [4, 8, 12, 1000, 4096, 4100, 65540]
    lens = [lens[i] for i in torch.randint(0, 7, (n_seg,), generator=gen).tolist()] if n_seg != 7 else lens
    ends = np.cumsum(lens).tolist()
    n, n_sets, gs = ends[-1], 5, 1.0 / 3.0
    scales = torch.empty(n_seg).uniform_(0.01, 1.0, generator=gen).tolist()
    wds = [[0.0, 0.05][i] for i in torch.randint(0, 2, (n_seg,), generator=gen).tolist()]
    seg_set = (torch.randint(0, n_sets + 1, (n_seg,), generator=gen) - 1).tolist()          # -1 .. n_sets - 1
    if n_seg > 1:
        seg_set[0], seg_set[-1] = -1, n_sets - 1
    table = ops.adamw_groups_clip_table(ends, scales, wds, seg_set, n, n_sets, DEV)
    plain = ops.adamw_groups_table(ends, scales, wds, n, DEV)
    p0 = torch.randn(n, generator=gen).to(DEV)
    pa, pb, pc, pd = (p0.clone() for _ in range(4))
    ma, va, mb, vb, mc, vc, md, vd = (torch.zeros(n, device=DEV) for _ in range(8))
    ones = torch.tensor([[3.0, 1.0]] * n_sets, device=DEV)
    seg_of = torch.repeat_interleave(torch.arange(n_seg), torch.tensor(lens)).to(DEV)
    set_of = torch.tensor(seg_set, device=DEV)[seg_of]
    for t in range(1, 4):
        g = _grad(n, 7 * t + n_seg)
        clip = torch.stack([torch.full((n_sets,), 9.0), torch.empty(n_sets).uniform_(0.1, 1.5, generator=gen)], 1).to(DEV)
        coef = torch.where(set_of >= 0, clip[:, 1][set_of.clamp(min=0)], torch.ones((), device=DEV))
        ops.adamw_groups_clip_dev(pa, g, ma, va, table, _hyper(t, LR), clip, B1, B2, EPS, gs)
        ops.adamw_groups_dev(pb, _clipped(g, gs, coef), mb, vb, plain, _hyper(t, LR), B1, B2, EPS, 1.0)
        assert torch.equal(_bits(pa), _bits(pb)), 'step %d: %d elements differ' % (t, int((pa != pb).sum()))
        assert torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
        ops.adamw_groups_clip_dev(pc, g, mc, vc, table, _hyper(t, LR), ones, B1, B2, EPS, gs)
        ops.adamw_groups_dev(pd, g, md, vd, plain, _hyper(t, LR), B1, B2, EPS, gs)
        assert torch.equal(_bits(pc), _bits(pd)) and torch.equal(_bits(mc), _bits(md)) and torch.equal(_bits(vc), _bits(vd))
    assert not torch.equal(pa, p0)


# ---------------------------------------------------------------------------------------------- 4. bad arguments
def test_refused_arguments_launch_nothing():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib = L.load()
    n = 4104
    g = _grad(n + 4, 1)
    plan = ops.grad_clip_plan([[(0, n, 0)]], [n], 1, DEV)
    plan['partial'].fill_(-7.0)
    plan['out'].fill_(-7.0)
    st = L.stream()
    good = [g.data_ptr(), n, plan['chunk_off'][0].data_ptr(), plan['chunk_len'][0].data_ptr(), 1, 1.0,
            plan['partial'].data_ptr(), st]

    def call(fn, good, **kw):
        a = list(good)
        for i, val in kw.items():
            a[int(i[1:])] = val
        return fn(*a)
    fn = lib.passl_hip_grad_sumsq
    for i in (0, 2, 3, 6):
        assert call(fn, good, **{'a%d' % i: None}) == L.EINVAL, i
    for kw in (dict(a1=0), dict(a1=-4), dict(a1=4102), dict(a4=0), dict(a4=-1), dict(a0=good[0] + 4), dict(a2=good[2] + 4)):
        assert call(fn, good, **kw) == L.EINVAL, kw
    fin = [plan['partial'].data_ptr(), 1, plan['set_ptr'].data_ptr(), plan['set_chunks'].data_ptr(), 1, 1, 1.0,
           float('inf'), 0, plan['out'].data_ptr(), st]
    fn = lib.passl_hip_grad_clip_finalize
    for i in (0, 2, 3, 9):
        assert call(fn, fin, **{'a%d' % i: None}) == L.EINVAL, i
    for kw in (dict(a1=0), dict(a4=0), dict(a5=0), dict(a6=0.0), dict(a6=-1.0), dict(a6=float('nan')), dict(a6=float('inf')),
               dict(a7=0.0), dict(a7=float('nan'))):
        assert call(fn, fin, **kw) == L.EINVAL, kw
    torch.cuda.synchronize()
    assert (plan['partial'] == -7.0).all() and (plan['out'] == -7.0).all()       # nothing was launched
    assert lib.passl_hip_grad_clip_chunk(0) == L.EINVAL and lib.passl_hip_grad_clip_chunk(L.ABI_VERSION) == CHUNK
    # the update variants
    p0 = torch.randn(n + 4, device=DEV)
    p, m, v = p0.clone(), torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    hyper, coef = _hyper(1, LR), torch.tensor([0.5], device=DEV)
    flat = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, hyper.data_ptr(), coef.data_ptr(), B1, B2, EPS, 0.05,
            1.0, st]
    fn = lib.passl_hip_adamw_clip_dev
    for i in (0, 1, 2, 3, 5, 6):
        assert call(fn, flat, **{'a%d' % i: None}) == L.EINVAL, i
    for kw in (dict(a4=-4), dict(a4=4102), dict(a0=flat[0] + 4), dict(a3=flat[3] + 4)):
        assert call(fn, flat, **kw) == L.EINVAL, kw
    assert call(fn, flat, a4=0) == L.OK
    t = ops.adamw_groups_clip_table([8, n], [1.0, 0.5], [0.05, 0.0], [0, -1], n, 1, DEV)
    clip = torch.tensor([[2.0, 0.5]], device=DEV)
    grp = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, t['seg_end'].data_ptr(), t['seg_lr_scale'].data_ptr(),
           t['seg_wd'].data_ptr(), t['seg_set'].data_ptr(), 2, hyper.data_ptr(), clip.data_ptr(), 1, B1, B2, EPS, 1.0, st]
    fn = lib.passl_hip_adamw_groups_clip_dev
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 10, 11):
        assert call(fn, grp, **{'a%d' % i: None}) == L.EINVAL, i
    for kw in (dict(a4=-4), dict(a4=4102), dict(a9=0), dict(a12=0), dict(a5=grp[5] + 4), dict(a2=grp[2] + 4)):
        assert call(fn, grp, **kw) == L.EINVAL, kw
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(p0)) and not m.any() and not v.any()      # nothing was launched
    with pytest.raises(L.PasslHipError):
        ops.adamw_clip_dev(p[:n].cpu(), g[:n], m[:n], v[:n], hyper, coef, B1, B2, EPS, 0.05)      # no host fall-back
    with pytest.raises(ValueError):
        ops.adamw_groups_clip_dev(p, g, m, v, t, hyper, clip, B1, B2, EPS)       # the table of another buffer
    with pytest.raises(ValueError):
        ops.grad_sumsq(g, plan, 0)                                               # the plan of another buffer
    assert call(fn, grp) == L.OK and call(lib.passl_hip_adamw_clip_dev, flat) == L.OK
    torch.cuda.synchronize()
    assert not torch.equal(p[:n], p0[:n]) and torch.equal(_bits(p[n:]), _bits(p0[n:]))   # ... and bounded by n


# ---------------------------------------------------------------------------------------------- 5. reference parity
def _reference_groups(model, wd, ld):
    """The 13 groups of the fixture: the v2 rule on the backbone + the head as two groups (run A of the lrd fixture)."""
    from passl_amd.solver.lr_decay import param_groups_lrd
    groups = param_groups_lrd(model.backbone, wd, {'pos_embed', 'cls_token', 'dist_token'}, ld)
    head = list(model.head.parameters())
    groups.append({'lr_scale': 1.0, 'weight_decay': wd, 'params': [p for p in head if p.ndim != 1]})
    groups.append({'lr_scale': 1.0, 'weight_decay': 0., 'params': [p for p in head if p.ndim == 1]})
    return groups


def _run_clip_golden(run, dtype, tol, parity):
    """Runs P (per group) and T (over all parameters) of the fixture through AdamW(groups, grad_clip=...).  Loss at the
    project's bounds (x 20 after the first update, as tests/test_adamw_groups_gpu.py).  parity (fp32): every set's norm and
    coefficient within 2e-3 relative; exp_avg of every stored tensor within 2e-3 and exp_avg_sq within 4e-3, relative in
    norm, element by element for the ELEMENTWISE tensors and norm against norm for the WATCH list.  The fixture guarantees
    (grad_clip_util.check_golden) that the unclipped run and the other scope are >= 10 bounds further away; the product's own
    distance to the unclipped fixture is asserted to exceed the bound for every tensor its run clips."""
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    z = np.load(GOLDEN)
    N, hw, steps, classes = [int(v) for v in z['meta']]
    torch.manual_seed(0)
    model, keys_shapes = _build_finetune(dtype, classes)
    assert ['%s:%s' % (k, 'x'.join(map(str, s))) for k, s in keys_shapes] == [str(k) for k in z['keys']]
    model.train()
    lr, wd, ld, clip_norm = float(z['lr']), float(z['weight_decay']), float(z['layer_decay']), float(z['clip_norm'])
    gc = C(clip_norm=clip_norm) if run == 'P' else C.like_clip_grad_norm_(clip_norm)
    opt = AdamW(lr, beta1=B1, beta2=B2, weight_decay=wd, parameters=_reference_groups(model, wd, ld), grad_clip=gc)
    named = list(model.named_parameters())
    assert [n for n, _p in named] == [str(n) for n in z['table_names']]
    if run == 'P':
        assert [s for _n, s in opt.clip_sets()] == z['group_of'].tolist()
    else:
        assert {s for _n, s in opt.clip_sets()} == {0}
    watch, elem = [str(n) for n in z['watch']], [str(n) for n in z['elementwise']]
    ps = dict(named)
    arena = model.arena_q

    def moment(buf, name):
        # the moment of a parameter in the parameter's own element order: the arena stores a Linear weight transposed
        # (and a convolution filter channels-last), the parameter is a strided view of its slot — the same view of the
        # moment buffer, which has the arena's layout
        p = ps[name]
        off, n = arena.param_slices[p._passl_index]
        assert off <= p.storage_offset() < off + n
        return torch.as_strided(buf[0], p.shape, p.stride(), p.storage_offset()).detach().double().cpu().numpy().reshape(-1)

    gen = torch.Generator().manual_seed(909)
    report, bad = [], []

    def check(what, err, bound, at_least=False):
        line = '%-64s %s %.3e  bound %.3e' % (what, 'dist' if at_least else 'err', err, bound)
        report.append(line)
        if not (err > bound if at_least else err <= bound):
            bad.append(line)

    lrd = np.load(LRD_GOLDEN)
    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        out = model(x.to(DEV), y.to(DEV), mode='train')
        opt.clear_grad()
        out['loss'].backward()
        opt.step()
        pre = '%s_s%d_' % (run, s)
        ref_loss = float(z[pre + 'loss'])
        check(pre + 'loss', abs(float(out['loss'].detach()) - ref_loss) / abs(ref_loss), tol['loss'] * (1.0 if s == 0 else 20.0))
        got = opt.grad_norms().detach().double().cpu().numpy()
        assert np.isfinite(got).all()
        ref_norm = z[pre + 'group_norm'] if run == 'P' else np.array([float(z[pre + 'global_norm'])])
        ref_coef = z[pre + 'group_coef'] if run == 'P' else np.array([float(z[pre + 'global_coef'])])
        assert got.shape == (len(ref_norm), 2)
        if not parity:
            if s == 0:
                # Adam is invariant to the gradient's scale: after the first update the clipped parameters are those of
                # the unclipped run A of the lrd fixture (up to eps) — its pnorm at the project's bf16 bound
                for n in watch:
                    ref = float(lrd['A_s0_pnorm/' + n])
                    check(pre + 'pnorm/' + n, abs(ps[n].detach().double().norm().item() - ref) / ref, tol['param'])
            continue
        check(pre + 'set norms', float(np.max(np.abs(got[:, 0] - ref_norm) / ref_norm)), grad_clip_util.NORM_BOUND)
        check(pre + 'set coefficients', float(np.max(np.abs(got[:, 1] - ref_coef) / ref_coef)), grad_clip_util.NORM_BOUND)
        assert ((got[:, 1] == 1.0) == (ref_coef == 1.0)).all()               # the same sets are clipped
        for n in watch:
            for what, buf, bound in (('mnorm', opt._m, grad_clip_util.M_BOUND), ('vnorm', opt._v, grad_clip_util.V_BOUND)):
                ref = float(z[pre + what + '/' + n])
                check(pre + what + '/' + n, abs(np.linalg.norm(moment(buf, n)) - ref) / ref, bound)
        for n in elem:
            for what, buf, bound in (('m', opt._m, grad_clip_util.M_BOUND), ('v', opt._v, grad_clip_util.V_BOUND)):
                ref = z[pre + what + '/' + n].astype(np.float64).reshape(-1)
                check(pre + what + '/' + n, float(np.linalg.norm(moment(buf, n) - ref) / np.linalg.norm(ref)), bound)
            if run == 'T' or grad_clip_util.clipped_so_far(z, s, n):
                unclipped = z['N_s%d_m/%s' % (s, n)].astype(np.float64).reshape(-1)
                check(pre + 'm/' + n + ' vs unclipped', float(np.linalg.norm(moment(opt._m, n) - unclipped)
                                                              / np.linalg.norm(unclipped)), grad_clip_util.M_BOUND, at_least=True)
    print('\n'.join(report))                                  # every figure, before the assertion
    assert not bad, 'parity violations:\n' + '\n'.join(bad)


@pytest.mark.parametrize('run', ['P', 'T'])
def test_finetune_clip_golden_fp32(run):
    """fp32 is the parity claim: the bounds are those of DESIGN.md §24.4 (every figure is printed before the assertion)."""
    _run_clip_golden(run, torch.float32, FT_TOL_F32, True)


def test_finetune_clip_golden_bf16():
    """The bf16 path runs the same clipped update within the project's bf16 bounds (loss, pnorm); no parity claim."""
    _run_clip_golden('P', torch.bfloat16, FT_TOL_BF16, False)


# ---------------------------------------------------------------------------------------------- 6. replay
@pytest.mark.parametrize('scope', ['group', 'global'])
def test_step_plan_replays_clipped_adamw_while_the_schedule_moves(scope):
    """The chunk sums, the finalize and the clip update are recorded like their neighbours; the coefficient is read from
    device memory when the replayed kernels run: parameters, losses and {norm, coef} equal the eager twin's bit for bit."""
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.lr_scheduler import CosineAnnealingDecay
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    B, T, dim, classes, steps = 16, 17, 128, 16, 4              # one warm-up step, then 3 steps through the plan
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(B * T, dim, generator=gen).to(DEV), torch.randint(0, classes, (B,), generator=gen).to(DEV))
               for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        torch.manual_seed(9)
        model = _tiny_step_model(dim, 4, classes, B, T)
        model.train()
        sched = CosineAnnealingDecay(1e-3, T_max=6)
        opt = AdamW(sched, weight_decay=0.05, parameters=_tiny_groups(model), grad_clip=C(0.05, scope=scope))
        assert 'seg_set' in opt._tables[0] and opt._clip['n_sets'] == (1 if scope == 'global' else len(_tiny_groups(model)))

        def full_step(x, y):
            out = model(x, y)
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            opt.step()
            return out
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, lrs, flats, norms = [], [], [], []
        for x, y in batches:
            lrs.append(opt.get_lr())
            out = sp.run(x, y)
            sched.step()
            losses.append(out['loss'].detach().clone().reshape(1))
            flats.append(model.arena_q.flat[:model.arena_q.n_train].clone())
            norms.append(opt.grad_norms().clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
        assert len(set(lrs)) == steps
        results[mode] = (torch.cat(losses).cpu(), torch.stack(flats).cpu(), torch.stack(norms).cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, fa, na), (lb, fb, nb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(na), _bits(nb))
    for s in range(steps):
        assert torch.equal(_bits(fa[s]), _bits(fb[s])), 'parameters differ after step %d' % s
    assert not torch.equal(fa[steps - 1], fa[steps - 2])
    assert (na[:, :, 1] < 1.0).any() and not torch.equal(na[1], na[2])       # something was clipped; the norms moved


# ---------------------------------------------------------------------------------------------- 7. state_dict
def test_state_dict_round_trip_gives_identical_bits():
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    gen = torch.Generator().manual_seed(21)
    data = [(torch.randn(8, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 16, (8,), generator=gen).to(DEV))
            for _ in range(3)]

    def make():
        torch.manual_seed(0)
        model, _ = _build_finetune(torch.float32)
        model.train()
        return model, AdamW(LR, weight_decay=0.05, parameters=_reference_groups(model, 0.05, 0.65), grad_clip=C(1.0))

    def step(model, opt, x, y):
        out = model(x, y, mode='train')
        opt.clear_grad()
        out['loss'].backward()
        opt.step()

    m1, o1 = make()
    for x, y in data[:2]:
        step(m1, o1, x, y)
    sd, weights = o1.state_dict(), {k: v.detach().clone() for k, v in m1.state_dict().items()}
    assert sorted(sd) == ['moment1_0', 'moment2_0', 't'] and sd['t'] == 2        # clipping is not state
    step(m1, o1, *data[2])
    m2, o2 = make()
    m2.load_state_dict(weights)
    o2.set_state_dict(sd)
    step(m2, o2, *data[2])
    a, b = m1.arena_q, m2.arena_q
    assert torch.equal(_bits(a.flat[:a.n_train]), _bits(b.flat[:b.n_train]))
    assert torch.equal(_bits(o1._m[0]), _bits(o2._m[0])) and torch.equal(_bits(o1._v[0]), _bits(o2._v[0]))
    assert torch.equal(_bits(o1.grad_norms()), _bits(o2.grad_norms())) and (o1.grad_norms()[:, 1] < 1.0).any()
    # param.grad is NOT rewritten: the gradient buffer still holds the unclipped gradient
    g = a.grads.double()
    assert abs(math.sqrt(float((g * g).sum())) - math.sqrt(float((o1.grad_norms()[:, 0].double() ** 2).sum()))) \
        <= 1e-5 * math.sqrt(float((g * g).sum()))


# ---------------------------------------------------------------------------------------------- 8. Engine
def test_v2_engine_trains_with_grad_clip_override(tmp_path, monkeypatch):
    """configs/v2/mocov3_vit_base_pt_synthetic.yaml with ``Optimizer.grad_clip`` set: the Engine builds the object, every
    step runs the chunk sums over the ViT-B arena, one finalize and the flat clip update."""
    from passl_amd.engine.engine import Engine
    from passl_amd.hip import ops
    from passl_amd.utils.config import AttrDict, get_config
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'DataLoader.Train.dataset.num_samples=40', 'DataLoader.Train.sampler.batch_size=4'])
    cfg['Global']['max_train_step'] = 3
    cfg.LRScheduler.warmup_start_lr = 1e-4                      # the yaml's first step has lr 0: nothing would move
    cfg.Optimizer.grad_clip = AttrDict(name='ClipGradByGlobalNorm', clip_norm=0.5)
    eng = Engine(cfg, mode='train')
    opt = eng.optimizer
    assert type(opt).__name__ == 'AdamW' and opt._grad_clip.clip_norm == 0.5 and opt._clip['n_sets'] == 1
    calls = []
    for name in ('grad_sumsq', 'grad_clip_finalize', 'adamw_clip_dev', 'adamw_dev'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    a = eng.model.arena_q
    w0 = a.flat[:a.n_train].clone()
    eng.train()
    # (steps replayed from a recorded plan do not pass through Python again)
    assert calls[:3] == ['grad_sumsq', 'grad_clip_finalize', 'adamw_clip_dev'] and 'adamw_dev' not in calls
    norm, coef = opt.grad_norms()[0].tolist()
    assert math.isfinite(norm) and norm > 0 and 0 < coef <= 1.0
    assert coef == 1.0 or abs(coef - 0.5 / (norm + 1e-6)) <= 1e-6 * coef
    assert not torch.equal(a.flat[:a.n_train], w0)
