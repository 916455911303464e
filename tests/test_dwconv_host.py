"""csrc/dwconv.hip without a GPU: the bounds of convnext_util.py are reachable (a float32 evaluation in a shuffled
summation order meets every one of them in every case) and not vacuous (a planted defect breaks them), the numpy
restatement of layer_scale_add is the reference's op sequence bit for bit, and the entry points refuse bad arguments
before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import convnext_util as U
from passl_amd.hip import lib as L
from passl_amd.hip import ops


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_fp32_in_a_shuffled_order_meets_every_bound(case):
    y, dx, dw, db = U.host_fp32(case)
    worst = {}
    worst['y'] = U.usage(y, *U.fwd_ref(case))
    worst['dx'] = U.usage(dx, *U.bwd_data_ref(case, True))
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    worst['dw'] = U.usage(dw, dw64, dw_bound)
    worst['dbias'] = U.usage(db, db64, db_bound)
    print('FIG host %s %s' % (U.case_id(case), ' '.join('%s %.3f' % (k, v[0]) for k, v in worst.items())))
    for name, (ratio, idx) in worst.items():
        msg = U.verdict(U.case_id(case), name, ratio, idx)
        assert msg is None, msg


@pytest.mark.parametrize('case', [c for c in U.CASES if c[0] == (3, 9, 20, 40) and c[1] != 'bigbias'], ids=U.case_id)
def test_planted_defects_break_the_bounds(case):
    """An unreversed filter in dx, a transposed filter in y, a misplaced tap in dw, a pixel missing from dbias: each
    leaves its bound.  (Not the bigbias kind: under a bf16 store u |value| of a 10^4 offset is 39, wider than the
    convolution itself.)"""
    d = U.conv_data(case)
    dtype = case[2]
    asym = case[1] != 'cancel'                     # the checkerboard is symmetric under both defects
    taps = [(r, s) for r in range(7) for s in range(7)]
    w = d['w']
    y_t = sum(U.shifted(d['x'], r, s) * w[:, 0, s, r] for r, s in taps) + d['bias']
    dx_u = sum(U.shifted(d['dy'], 6 - r, 6 - s) * w[:, 0, 6 - r, 6 - s] for r, s in taps) + d['add']
    if asym:
        assert U.usage(U.rnd(y_t, dtype), *U.fwd_ref(case))[0] > 1
        assert U.usage(U.rnd(dx_u, dtype), *U.bwd_data_ref(case, True))[0] > 1
    _, _, dw, db = U.host_fp32(case)
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    bad = dw.clone()
    bad[:, 0, 0, 0] = dw[:, 0, 0, 1]
    assert U.usage(bad, dw64, dw_bound)[0] > 1
    assert U.usage(db - d['dyw'][0, 0, 0], db64, db_bound)[0] > 1          # one pixel left out of the bias gradient


@pytest.mark.parametrize('case', U.LS_CASES, ids=U.ls_case_id)
def test_layer_scale_restatement_is_the_reference_sequence(case):
    (B, T, Cc), table, dtype = case
    d = U.ls_data(case)
    got = U.layer_scale_restated(d['branch'], d['residual'], d['gamma'], d['keep'], U.KEEP_PROB, T, torch.float32)
    ref = U.layer_scale_reference_ops(d['branch'], d['residual'], d['gamma'], d['keep'], U.KEEP_PROB, T)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    # a contracted last step (fma) is NOT the same function: the restatement can tell
    fused = torch.from_numpy((d['residual'].numpy().astype(np.float64) + (
        d['gamma'].numpy().astype(np.float64) * d['branch'].numpy().astype(np.float64))).astype(np.float32))
    if table is False and B * T * Cc >= 1000:
        assert not torch.equal(fused, ref)


@pytest.mark.parametrize('case', U.LS_CASES, ids=U.ls_case_id)
def test_layer_scale_backward_bounds_are_reachable(case):
    db, dg = U.ls_bwd_host_fp32(case)
    db64, db_bound, dg64, dg_bound = U.ls_bwd_ref(case)
    for name, r in (('dbranch', U.usage(db, db64, db_bound)), ('dgamma', U.usage(dg, dg64, dg_bound))):
        msg = U.verdict(U.ls_case_id(case), name, *r)
        assert msg is None, msg
    assert U.usage(dg * (1 + 2.0 ** -8), dg64, dg_bound)[0] > 1 or float(dg64.abs().max()) == 0


def test_workspace_formulas_match_the_header():
    """ops.py, convnext_util.py and the macros of include/passl_hip.h state the same sizes."""
    import os
    import subprocess
    import tempfile
    import shutil
    assert shutil.which('gcc'), 'this test compiles a three-line C program against include/passl_hip.h: gcc must be on PATH'
    shapes = [(1, 1, 1, 8), (3, 9, 20, 40), (128, 56, 56, 96), (128, 7, 7, 768), (2, 17, 33, 24)]
    rows = [(1, 8), (784, 96), (2100, 16), (401408, 96), (1024, 8), (1025, 8)]
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'passl_hip.h')
    body = ''.join('printf("%%lld\\n", (long long)PASSL_DWCONV7_WGRAD_WS_FLOATS(%d, %d, %d, %d));' % s for s in shapes)
    body += ''.join('printf("%%lld\\n", (long long)PASSL_LAYER_SCALE_BWD_WS_FLOATS(%d, %d));' % r for r in rows)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'ws.c'), os.path.join(tmp, 'ws')
        open(src, 'w').write('#include "%s"\n#include <stdio.h>\nint main(){%s return 0;}\n' % (header, body))
        subprocess.check_call(['gcc', src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    want = [ops.dwconv7_wgrad_ws_floats(*s) for s in shapes] + [ops.layer_scale_bwd_ws_floats(*r) for r in rows]
    assert out == want
    assert want == [U.wgrad_ws_floats(*s) for s in shapes] + [U.ls_bwd_ws_floats(*r) for r in rows]


@pytest.fixture(scope='module')
def lib():
    return L.load()


def test_arguments_are_validated_before_any_launch(lib):
    """NULL pointers, C % 8, misaligned pointers, non-positive sizes, an unknown dtype, a short workspace: a status,
    never a launch (host memory stands in for device pointers: nothing may touch it)."""
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    EINVAL, EUNSUP = L.EINVAL, L.EUNSUPPORTED
    fwd, bwd, wg = lib.passl_hip_dwconv7_fwd, lib.passl_hip_dwconv7_bwd_data, lib.passl_hip_dwconv7_bwd_weight
    lsf, lsb = lib.passl_hip_layer_scale_add_fwd, lib.passl_hip_layer_scale_add_bwd
    for i in range(4):                                              # each pointer NULL / misaligned in turn
        for bad in (None, odd):
            a = [p, p, p, p]
            a[i] = bad
            assert fwd(*a, 1, 4, 4, 8, L.F32, None) == EINVAL
            if not (i == 2 and bad is None):                        # add may be NULL
                assert bwd(*a, 1, 4, 4, 8, L.F32, None) == EINVAL
    for shape in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, -1, 8), (1, 4, 4, 0), (1, 4, 4, 12), (1, 4, 4, 4)):
        assert fwd(p, p, p, p, *shape, L.F32, None) == EINVAL
        assert bwd(p, p, None, p, *shape, L.BF16, None) == EINVAL
        assert wg(p, p, p, p, p, 1 << 20, *shape, L.F32, None) == EINVAL
    assert fwd(p, p, p, p, 1, 4, 4, 8, 7, None) == EUNSUP
    assert wg(p, p, p, p, p, 1 << 20, 1, 4, 4, 8, 7, None) == EUNSUP
    for i in range(5):
        for bad in (None, odd):
            a = [p, p, p, p, p]
            a[i] = bad
            assert wg(*a, 1 << 20, 1, 4, 4, 8, L.F32, None) == EINVAL
    need = ops.dwconv7_wgrad_ws_floats(3, 9, 20, 40)
    assert wg(p, p, p, p, p, need - 1, 3, 9, 20, 40, L.F32, None) == EINVAL
    assert wg(p, p, p, p, None, 0, 3, 9, 20, 40, L.F32, None) == EINVAL

    for i in (0, 1, 2, 5):
        for bad in (None, odd):
            a = [p, p, p, p, 0.5, p]
            a[i] = bad
            assert lsf(*a, 2, 3, 8, L.F32, None) == EINVAL
    for kp in (0.0, -0.5, 1.5, float('nan')):
        assert lsf(p, p, p, p, kp, p, 2, 3, 8, L.F32, None) == EINVAL
        assert lsb(p, p, p, p, kp, p, p, p, 1 << 20, 2, 3, 8, L.F32, None) == EINVAL
    for shape in ((0, 3, 8), (2, 0, 8), (2, 3, 0), (2, 3, 12), (2, -3, 8)):
        assert lsf(p, p, p, None, 0.0, p, *shape, L.BF16, None) == EINVAL
        assert lsb(p, p, p, None, 0.0, p, p, p, 1 << 20, *shape, L.BF16, None) == EINVAL
    assert lsf(p, p, p, None, 0.0, p, 2, 3, 8, 9, None) == EUNSUP
    assert lsb(p, p, p, None, 0.0, p, p, p, 1 << 20, 2, 3, 8, 9, None) == EUNSUP
    assert lsb(p, p, p, None, 0.0, p, p, p, 1 << 20, 2, 3, 8200, L.F32, None) == EUNSUP      # C > 8192
    for i in (0, 1, 2, 5, 6, 7):
        for bad in (None, odd):
            a = [p, p, p, p, 0.5, p, p, p]
            a[i] = bad
            assert lsb(*a, 1 << 20, 2, 3, 8, L.F32, None) == EINVAL
    assert lsb(p, p, p, p, 0.5, p, p, p, ops.layer_scale_bwd_ws_floats(2100, 16) - 1, 3, 700, 16, L.F32, None) == EINVAL
    assert all(v == 0.0 for v in buf)
