"""What tests/golden/mae_ft_clip_small.npz must satisfy to test anything — asserted by its generator
(tests/golden/make_golden_mae_finetune_clip.py) when the file is written and by tests/test_grad_clip_host.py on the
committed file — and the readers the GPU parity test shares with them."""
import numpy as np

RUNS = ('N', 'P', 'T')          # no clipping, ClipGradByGlobalNorm per group, clip_grad_norm_ over all parameters
M_BOUND, V_BOUND, NORM_BOUND = 2e-3, 4e-3, 2e-3      # the GPU test's bounds: exp_avg, exp_avg_sq, set norm / coefficient


def m_dist(z, run, other, step, name, what='m'):
    """Relative distance |x_run - x_other| / |x_other| of a stored moment ('m': exp_avg, 'v': exp_avg_sq)."""
    a = z['%s_s%d_%s/%s' % (run, step, what, name)].astype(np.float64)
    b = z['%s_s%d_%s/%s' % (other, step, what, name)].astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def group_of(z, name):
    return int(z['group_of'][[str(n) for n in z['table_names']].index(name)])


def clipped_so_far(z, step, name):
    """Has run P clipped the group of ``name`` at some step <= ``step``?"""
    g = group_of(z, name)
    return any(float(z['P_s%d_group_coef' % s][g]) != 1.0 for s in range(step + 1))


def check_golden(z):
    steps = int(z['meta'][2])
    elem = [str(n) for n in z['elementwise']]
    clip_norm = float(z['clip_norm'])
    for run in RUNS:
        for s in range(steps):
            # (a) every global norm in [5, 6.5]: T's coefficient lies in 0.15 - 0.2, far from 1
            gn = float(z['%s_s%d_global_norm' % (run, s)])
            assert 5.0 <= gn <= 6.5, (run, s, gn)
            assert 0.15 <= float(z['%s_s%d_global_coef' % (run, s)]) <= 0.2
            # (b) per group: some group is not clipped (norm <= 0.5) and some group clearly is (norm >= 2)
            norms = z['%s_s%d_group_norm' % (run, s)]
            assert norms.min() <= 0.5 * clip_norm and norms.max() >= 2.0 * clip_norm, (run, s, norms.min(), norms.max())
    unclipped_seen = 0
    for n in elem:
        for s in range(steps):
            # (c) T clips everything: its first moment is >= 10 bounds away from the unclipped run's
            assert m_dist(z, 'T', 'N', s, n) >= 10 * M_BOUND, ('T', s, n, m_dist(z, 'T', 'N', s, n))
            if clipped_so_far(z, s, n):
                assert m_dist(z, 'P', 'N', s, n) >= 10 * M_BOUND, ('P', s, n, m_dist(z, 'P', 'N', s, n))
        if not clipped_so_far(z, steps - 1, n):
            # (d) a tensor of a group P never clips: P = N at the test's resolution (what is left is the drift of the
            # clipped parameters through the forward pass), and far from T — the two scopes are pinned against each other
            unclipped_seen += 1
            for s in range(steps):
                assert m_dist(z, 'P', 'N', s, n) <= M_BOUND, (s, n, m_dist(z, 'P', 'N', s, n))
                assert m_dist(z, 'P', 'T', s, n) >= 10 * M_BOUND, (s, n, m_dist(z, 'P', 'T', s, n))
    assert unclipped_seen >= 1, 'no stored tensor lies in a group that run P leaves unclipped'
    assert any(clipped_so_far(z, 0, n) for n in elem)
