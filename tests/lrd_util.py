"""What tests/golden/mae_ft_lrd_small.npz must satisfy to test anything — asserted by its generator
(tests/golden/make_golden_mae_finetune_lrd.py) when the file is written and by tests/test_adamw_groups_host.py on the
committed file — and the readers the GPU parity test shares with them."""
import numpy as np

RUNS = ('A', 'B', 'U')          # v2 rule, v110 rule, one uniform group


def tables(z):
    """-> {run: [(name, scale, weight decay)]} for runs A and B."""
    names = [str(n) for n in z['table_names']]
    return {r: list(zip(names, [float(s) for s in z['table_%s_scale' % r]], [float(w) for w in z['table_%s_wd' % r]]))
            for r in ('A', 'B')}


def dnorm_gap(z, run, step, name):
    """Relative gap of ``dnorm`` (norm of the step's parameter change) between ``run`` and the uniform run."""
    u = float(z['U_s%d_dnorm/%s' % (step, name)])
    return abs(float(z['%s_s%d_dnorm/%s' % (run, step, name)]) - u) / u


def elem_dist(z, run, step, name):
    """D = max |p_run - p_U| of an element-wise stored tensor after ``step``."""
    return float(np.max(np.abs(z['%s_s%d_p/%s' % (run, step, name)].astype(np.float64)
                               - z['U_s%d_p/%s' % (step, name)].astype(np.float64))))


def treated_differently(z, run, name):
    """(scale differs from 1, decay differs from the uniform run's) of ``name`` in ``run``."""
    row = dict((n, (s, w)) for n, s, w in tables(z)[run])[name]
    return row[0] != 1.0, row[1] != float(z['weight_decay'])


def check_golden(z):
    steps = int(z['meta'][2])
    watch = [str(n) for n in z['watch']]
    elem = [str(n) for n in z['elementwise']]
    assert set(elem) <= set(watch) and len(watch) >= 10
    lr, wd = float(z['lr']), float(z['weight_decay'])
    for run in ('A', 'B'):
        seen_scaled = 0
        for n in watch:
            scaled, _ = treated_differently(z, run, n)
            if not scaled:
                continue
            seen_scaled += 1
            # (a) an Adam step moves every element by about lr * scale: the gap to the uniform run is 1 - scale >= 0.35
            for s in range(steps):
                assert dnorm_gap(z, run, s, n) >= 0.2, (run, s, n, dnorm_gap(z, run, s, n))
        assert seen_scaled >= 6
        for n in elem:
            scaled, decayed_differently = treated_differently(z, run, n)
            if decayed_differently:
                # (b) the decay alone is visible: D is about lr * scale * wd * |p| per step when the scale is 1
                for s in range(steps):
                    assert elem_dist(z, run, s, n) > 0, (run, s, n)
        assert any(treated_differently(z, run, n)[1] for n in elem)
    # (c) no gradient element of an element-wise stored tensor is small enough for fp32 noise to flip the sign of m
    for run in RUNS:
        for s in range(steps):
            for n in elem:
                lo, hi = float(z['%s_s%d_gmin/%s' % (run, s, n)]), float(z['%s_s%d_gmax/%s' % (run, s, n)])
                assert lo >= 1e-4 * hi, (run, s, n, lo, hi)
    assert lr > 0 and wd > 0
