"""Adan (passl/optimizer/adan.py:117-148, is_vanilla=False) restated in numpy, and what the two fixtures
tests/golden/adan_vectors.npz and tests/golden/adan_mae_ft_small.npz (tests/golden/make_golden_adan.py) must satisfy.

    gg   = g*gs;  if clip: gg *= coef
    diff = first ? 0 : gg - pre
    m    = b1*m + (1-b1)*gg
    d    = b2*d + (1-b2)*diff
    u    = gg + b2*diff
    s    = b3*s + (1-b3)*(u*u)
    den  = sqrt(s)/sqrt(1-b3^t) + eps
    upd  = (m/(1-b1^t) + b2*d/(1-b2^t)) / den
    prox (default): p = (p - lr*upd) / (1 + lr*wd)        no_prox: p = p*(1 - lr*wd) - lr*upd
    pre  = gg

``adan_rule`` is that statement in float64 (the yardstick), ``adan_rule_f32`` its float32 twin: every operation rounded
to fp32 in the order the kernel (csrc/adan.hip) performs it, the powers b^t rounded to fp32 first as the hyper block
holds them.  ``lr``, ``wd`` and ``coef`` may be arrays (one value per element): groups are a per-element multiplier and
decay, a clip set a per-element coefficient."""
import numpy as np

BUFFERS = ('p', 'm', 'd', 's', 'pre')
BETAS = (0.98, 0.92, 0.99)
EPS = 1e-8
MARGIN = 4.0                    # the bound is MARGIN x max(ref_err, one fp32 ulp of the tensor's largest magnitude)
WRONG = ('pre_never_updated', 'pre_starts_at_zero', 'prox_swapped', 'u_without_b2')
PNORM_BOUND = 1e-4              # what tests/test_adamw_groups_gpu.py::test_finetune_layer_decay_golden_fp32 applies to pnorm


def zero_state(p, dtype=np.float64):
    p = np.asarray(p, dtype=dtype)
    z = np.zeros_like(p)
    return dict(p=p.copy(), m=z.copy(), d=z.copy(), s=z.copy(), pre=z.copy())


def adan_rule(state, g, t, lr, wd, betas=BETAS, eps=EPS, no_prox=False, coef=1.0, grad_scale=1.0, wrong=None):
    """One step (t = 1, 2, ...) in float64 -> the new state.  ``wrong``: one of WRONG, a deliberately wrong rule that the
    fixture must tell from the right one."""
    b1, b2, b3 = (float(b) for b in betas)
    f = np.float64
    p, m, d, s, pre = (np.asarray(state[k], dtype=f) for k in BUFFERS)
    lr, wd, coef = np.asarray(lr, dtype=f), np.asarray(wd, dtype=f), np.asarray(coef, dtype=f)
    gg = np.asarray(g, dtype=f) * f(grad_scale) * coef
    if wrong == 'pre_starts_at_zero':
        diff = gg - pre
    else:
        diff = np.zeros_like(gg) if t == 1 else gg - pre
    m = b1 * m + (1.0 - b1) * gg
    d = b2 * d + (1.0 - b2) * diff
    u = gg + diff if wrong == 'u_without_b2' else gg + b2 * diff
    s = b3 * s + (1.0 - b3) * (u * u)
    den = np.sqrt(s) / np.sqrt(1.0 - b3 ** t) + eps
    upd = (m / (1.0 - b1 ** t) + b2 * d / (1.0 - b2 ** t)) / den
    if bool(no_prox) != (wrong == 'prox_swapped'):
        p = p * (1.0 - lr * wd) - lr * upd
    else:
        p = (p - lr * upd) / (1.0 + lr * wd)
    if wrong == 'pre_never_updated' and t > 1:
        gg = pre                                        # pre_grad stays the clone made at the first step
    return dict(p=p, m=m, d=d, s=s, pre=gg + np.zeros_like(p))


def adan_rule_f32(state, g, t, lr, wd, betas=BETAS, eps=EPS, no_prox=False, coef=1.0, grad_scale=1.0, scale=1.0):
    """The float32 twin: the kernel's operations in the kernel's order, each rounded to fp32 (no contraction).  ``lr`` is
    the rate of the hyper block, ``scale`` the segment's multiplier (lr_s = fp32(lr) * fp32(scale), one multiply)."""
    f = np.float32
    b1, b2, b3, eps = f(betas[0]), f(betas[1]), f(betas[2]), f(eps)
    one = f(1.0)
    bc1 = one - f(float(betas[0]) ** t)
    bc2 = one - f(float(betas[1]) ** t)
    bc3 = np.sqrt(one - f(float(betas[2]) ** t))
    p, m, d, s, pre = (np.asarray(state[k], dtype=f) for k in BUFFERS)
    lr = np.asarray(lr, dtype=f) * np.asarray(scale, dtype=f)
    wd, coef = np.asarray(wd, dtype=f), np.asarray(coef, dtype=f)
    gg = np.asarray(g, dtype=f) * f(grad_scale)
    gg = gg * coef
    diff = np.zeros_like(gg) if t == 1 else gg - pre
    # 1 - beta: formed in double from the caller's decimal and rounded once, as the reference's scalar is
    omb1, omb2, omb3 = (f(1.0 - float(b)) for b in betas)
    m = b1 * m + omb1 * gg
    d = b2 * d + omb2 * diff
    u = gg + b2 * diff
    s = b3 * s + omb3 * (u * u)
    den = np.sqrt(s) / bc3 + eps
    upd = (m / bc1 + b2 * d / bc2) / den
    lw = lr * wd
    if no_prox:
        p = p * (one - lw) - lr * upd
    else:
        p = (p - lr * upd) / (one + lw)
    out = dict(p=p, m=m, d=d, s=s, pre=gg + np.zeros_like(p))
    assert all(v.dtype == f for v in out.values())
    return out


def ulp32(x):
    """One fp32 ulp at the largest magnitude of x."""
    a = np.float32(np.max(np.abs(x))) if np.size(x) else np.float32(0)
    return float(np.spacing(a))


def bound(ref_err, ref):
    return MARGIN * max(float(ref_err), ulp32(ref))


# ---------------------------------------------------------------------------------------------- the vectors fixture
def vector_names(z):
    return [str(n) for n in z['names']]


def vector_runs(z):
    """[(run name, no_prox)]"""
    return [(str(r), bool(f)) for r, f in zip(z['runs'], z['runs_no_prox'])]


def vector_config(z, name):
    """-> (lr multiplier, weight decay) of a tensor: its group's."""
    g = int(z['group_of'][vector_names(z).index(name)])
    return float(z['group_scale'][g]), float(z['group_wd'][g])


def trajectory(z, name, no_prox, rule=adan_rule, **kw):
    """The states of tensor ``name`` after each step of the fixture, by ``rule`` from the fixture's inputs."""
    scale, wd = vector_config(z, name)
    betas, eps = tuple(float(b) for b in z['betas']), float(z['eps'])
    if rule is adan_rule_f32:
        st, kw = zero_state(z['p0/' + name], np.float32), dict(kw, scale=scale)
        lrs = [float(v) for v in z['lr']]
    else:
        st = zero_state(z['p0/' + name])
        lrs = [float(v) * scale for v in z['lr']]
    out = []
    for t in range(1, int(z['steps']) + 1):
        st = rule(st, z['g_s%d/%s' % (t, name)], t, lrs[t - 1], wd, betas, eps, no_prox, **kw)
        out.append(st)
    return out


def _check_vectors(z):
    names = vector_names(z)
    steps = int(z['steps'])
    assert steps == 4 and len(names) >= 4 and all(z['p0/' + n].size <= 4096 and z['p0/' + n].size % 4 == 0 for n in names)
    assert sorted(set(z['group_of'].tolist())) == [0, 1]
    assert z['group_wd'].tolist() == [0.02, 0.0] and z['group_scale'].tolist() == [1.0, 0.5]
    assert sorted(f for _r, f in vector_runs(z)) == [False, True]
    # the gradient patterns: zero throughout, constant, sign flips, and a 1e3 change of scale between steps
    for n in names:
        g = np.stack([z['g_s%d/%s' % (t, n)] for t in range(1, steps + 1)])
        if g.shape[1] >= 16:
            assert (g == 0).all(0).any(), n
        if g.shape[1] >= 16 and n != str(z['scaled']):            # (the change of scale rescales every pattern)
            nz = (g[0] != 0)
            assert (nz & (g == g[0]).all(0)).any(), n
            assert (nz & (g[1:] == -g[:-1]).all(0)).any(), n
    amp = [float(np.abs(z['g_s%d/%s' % (t, str(z['scaled']))]).max()) for t in range(1, steps + 1)]
    assert max(amp[i + 1] / amp[i] for i in range(steps - 1)) >= 1e3 * 0.5 and \
        min(amp[i + 1] / amp[i] for i in range(steps - 1)) <= 2e-3
    # (1) the float64 statement reproduces the reference; (2) each wrong rule misses it by >= 100 x the bound somewhere
    worst = 0.0
    missed = {w: 0.0 for w in WRONG}
    for run, no_prox in vector_runs(z):
        for n in names:
            right = trajectory(z, n, no_prox)
            wrongs = {w: trajectory(z, n, no_prox, wrong=w) for w in WRONG}
            for t in range(1, steps + 1):
                errs = z['%s_s%d_ref_err/%s' % (run, t, n)]
                for bi, b in enumerate(BUFFERS):
                    ref = z['%s_s%d_%s/%s' % (run, t, b, n)]
                    assert ref.dtype == np.float32
                    bd = bound(errs[bi], ref)
                    err = float(np.max(np.abs(right[t - 1][b] - ref.astype(np.float64))))
                    assert err <= bd, (run, n, t, b, err, bd)
                    worst = max(worst, err / bd)
                    for w in WRONG:
                        missed[w] = max(missed[w], float(np.max(np.abs(wrongs[w][t - 1][b] - ref.astype(np.float64)))) / bd)
    for w in WRONG:
        assert missed[w] >= 100.0, ('the fixture does not tell the wrong rule %r from the right one' % w, missed[w])
    return dict(worst_ratio=worst, wrong_rule_ratios=missed)


# ---------------------------------------------------------------------------------------------- the model fixture
MODEL_RUNS = ('plain', 'clip')


def _check_model(z):
    steps = int(z['meta'][2])
    watch, elem = [str(n) for n in z['watch']], [str(n) for n in z['elementwise']]
    assert [str(r) for r in z['runs']] == list(MODEL_RUNS) and steps >= 3
    for run in MODEL_RUNS:
        for s in range(steps):
            pre = '%s_s%d_' % (run, s)
            assert np.isfinite(float(z[pre + 'loss']))
            assert z[pre + 'set_norm'].dtype == np.float64 and z[pre + 'set_coef'].dtype == np.float64
            assert z[pre + 'set_norm'].shape == (1,)
            for n in elem:
                assert z[pre + 'p/' + n].dtype == np.float32 and z[pre + 'p/' + n].size <= 4096
        coefs = np.array([float(z['%s_s%d_set_coef' % (run, s)][0]) for s in range(steps)])
        assert (coefs == 1.0).all() if run == 'plain' else (coefs < 1.0).all(), (run, coefs)
        # every watched tensor moves over the run by at least 10 x the bound used on it (pnorm, relative)
        for n in watch:
            moved = float(z['%s_move/%s' % (run, n)]) / float(z['%s_s0_pnorm/%s' % (run, n)])
            assert moved >= 10.0 * PNORM_BOUND, (run, n, moved)
    # the clipped run differs from the plain one where clipping acts: in pre_grad (the clipped gradient), by its coefficient
    for n in elem:
        a, b = z['plain_s0_pre/' + n].astype(np.float64), z['clip_s0_pre/' + n].astype(np.float64)
        c = float(z['clip_s0_set_coef'][0])
        assert np.max(np.abs(b - a * c)) <= 8 * ulp32(b) and np.max(np.abs(b - a)) > 100 * ulp32(b), n
    return dict()


def check_golden(z):
    """What a fixture file must satisfy (asserted by the generator before it writes, and by the host tests on the
    committed file).  -> a dict of the observed figures."""
    kind = str(z['kind'])
    if kind == 'vectors':
        return _check_vectors(z)
    assert kind == 'model', kind
    return _check_model(z)
