"""Shared by tests/test_random_erasing_host.py, tests/test_random_erasing_gpu.py and
tests/golden/make_golden_random_erasing.py: the fixture's cases, and a numpy restatement of the kernel's definition
(include/passl_hip.h: passl_hip_random_erase) — the slice assignment, and the 'pixel' normals in float64 from
droppath_util.philox4x32_10."""
import numpy as np

from droppath_util import MASK, check_known_answers, philox4x32_10

# (random.seed, (B, H, W), RandomErasing arguments, erased samples, rejected attempts): what the reference's class gave
CASES = [
    (3, (64, 32, 32), dict(prob=.25), 13, 0),
    (4, (64, 24, 40), dict(prob=.25), 19, 2),
    (5, (32, 15, 17), dict(prob=.5), 16, 0),
    (6, (32, 16, 16), dict(prob=1, min_count=1, max_count=3), 32, 0),
    (7, (64, 8, 8), dict(prob=.5), 37, 0),
    (8, (64, 32, 32), dict(prob=.25, min_area=.3, max_area=.9), 20, 26),
]
SECOND_CALL_SEED = 3                       # a second consecutive call is recorded for this case: the stream continues
MOMENT_ARGS = dict(seed=20261018, step=0, B=16, E=3 * 16 * 16)      # 12 288 values


def normals(seed, step, b, E):
    """float64 [E]: the 'pixel' values of sample b, by position.  g = e >> 2; words = Philox4x32-10(counter (g, b,
    step_lo, step_hi), key (seed_lo, seed_hi)); u0, u2 = (float(w >> 8) + 1) 2^-24; u1, u3 = float(w >> 8) 2^-24;
    z = (r01 cos 2 pi u1, r01 sin 2 pi u1, r23 cos 2 pi u3, r23 sin 2 pi u3), r = sqrt(-2 log u); e gets z[e & 3]."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    G = (E + 3) // 4
    g = np.arange(G, dtype=np.uint64)
    w = philox4x32_10((g, np.full_like(g, b), np.full_like(g, step & MASK), np.full_like(g, step >> 32)),
                      (seed & MASK, seed >> 32))
    f = [(v >> np.uint64(8)).astype(np.float64) for v in w]
    u0, u1, u2, u3 = (f[0] + 1) * 2.0 ** -24, f[1] * 2.0 ** -24, (f[2] + 1) * 2.0 ** -24, f[3] * 2.0 ** -24
    r01, r23 = np.sqrt(-2 * np.log(u0)), np.sqrt(-2 * np.log(u2))
    z = np.stack([r01 * np.cos(2 * np.pi * u1), r01 * np.sin(2 * np.pi * u1),
                  r23 * np.cos(2 * np.pi * u3), r23 * np.sin(2 * np.pi * u3)], axis=1)
    return z.reshape(-1)[:E]


def box_mask(table, C, H, W):
    """bool [B, C, H, W]: True inside each sample's box."""
    B = len(table)
    m = np.zeros((B, C, H, W), dtype=bool)
    for b, (top, left, h, w) in enumerate(np.asarray(table).tolist()):
        if h > 0 and w > 0:
            m[b, :, top:top + h, left:left + w] = True
    return m


def erase_ref(x, table, mode, seed=0, step=0):
    """x float32 numpy [B, C, H, W] -> (float64 result, mask): x outside the boxes (exact), the fill inside."""
    B, C, H, W = x.shape
    m = box_mask(table, C, H, W)
    out = x.astype(np.float64)
    if mode == 0:
        out[m] = 0.0
    else:
        for b in range(B):
            if m[b].any():
                z = normals(seed, step, b, C * H * W).reshape(C, H, W)
                out[b][m[b]] = z[m[b]]
    return out, m


def bounding_boxes(y):
    """y [B, C, H, W] of ones with zeroed regions -> int32 [B, 4] = (top, left, h, w) of the zeroed region per sample
    (all zeros when nothing was erased); asserts that the region is that full rectangle in every channel."""
    B = len(y)
    t = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        z = y[b] == 0
        if not z.any():
            continue
        assert (z == z[0]).all()
        rows, cols = np.where(z[0].any(axis=1))[0], np.where(z[0].any(axis=0))[0]
        top, left, h, w = rows[0], cols[0], rows[-1] - rows[0] + 1, cols[-1] - cols[0] + 1
        assert z[0, top:top + h, left:left + w].all() and z[0].sum() == h * w
        t[b] = (top, left, h, w)
    return t
