"""csrc/convmae.hip without a GPU: the bounds of convmae_util.py are reachable (a float32 evaluation in a shuffled
summation order meets every one of them in every case) and not vacuous (planted defects break them), the restatements
of the gather and token kernels agree with torch's own indexing, the workspace formulas match the header, and the entry
points refuse bad arguments before any launch."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest
import torch

import convmae_util as U
from passl_amd.hip import lib as L
from passl_amd.hip import ops


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_fp32_in_a_shuffled_order_meets_every_bound(case):
    y, dx, dw, db = U.host_fp32(case)
    worst = {}
    worst['y'] = U.usage(y, *U.fwd_ref(case))
    worst['dx'] = U.usage(dx, *U.bwd_data_ref(case))
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    worst['dw'] = U.usage(dw, dw64, dw_bound)
    worst['dbias'] = U.usage(db, db64, db_bound)
    print('FIG host %s %s' % (U.case_id(case), ' '.join('%s %.3f' % (k, v[0]) for k, v in worst.items())))
    for name, (ratio, idx) in worst.items():
        msg = U.verdict(U.case_id(case), name, ratio, idx)
        assert msg is None, msg


DEFECT_CASES = [c for c in U.CASES if c[0] in ((3, 8, 12, 40, 2), (1, 56, 56, 32, 4)) and c[1] in ('checker', 'random')]


@pytest.mark.parametrize('case', DEFECT_CASES, ids=U.case_id)
def test_planted_defects_break_the_bounds(case):
    """The mask applied at the output instead of the input, the filter not reversed in dx, an off-by-one in h / g
    (which moves the factors of y, dx and dw), a misplaced tap in dw, a pixel missing from dbias: each leaves its
    bound."""
    y, _, _, _ = U.host_fp32(case, 'mask_at_output')
    assert U.usage(y, *U.fwd_ref(case))[0] > 1
    _, dx, _, _ = U.host_fp32(case, 'unreversed')
    assert U.usage(dx, *U.bwd_data_ref(case))[0] > 1
    y, dx, dw, _ = U.host_fp32(case, 'row_off_by_one')
    dw64, dw_bound, db64, db_bound = U.bwd_weight_ref(case)
    assert U.usage(y, *U.fwd_ref(case))[0] > 1
    assert U.usage(dx, *U.bwd_data_ref(case))[0] > 1
    assert U.usage(dw, dw64, dw_bound)[0] > 1
    _, _, dw, db = U.host_fp32(case)
    bad = dw.clone()
    bad[:, 0, 0, 0] = dw[:, 0, 0, 1]
    assert U.usage(bad, dw64, dw_bound)[0] > 1
    assert U.usage(db - U.conv_data(case)['dy'][0, 0, 0], db64, db_bound)[0] > 1


def test_a_removed_map_leaves_the_bias_and_no_gradient():
    """All patches removed: y64 == bias, dx64 == 0 and dw64 == 0 exactly, so the bounds of those cases are |bias| terms
    only: the kernels' results there are compared bit for bit on the GPU."""
    case = ((3, 8, 12, 40, 2), 'removed', torch.float32)
    y, _ = U.fwd_ref(case)
    assert torch.equal(y, U.conv_data(case)['bias'].double().expand_as(y))
    assert float(U.bwd_data_ref(case)[0].abs().max()) == 0
    assert float(U.bwd_weight_ref(case)[0].abs().max()) == 0


def test_keep_map_is_the_reference_expansion():
    """keep_map indexes the table as conv_mae.py expands it: mask.reshape(-1, 14, 14) -> unsqueeze(-1).tile(..g..) ->
    reshape -> transpose, i.e. every g x g block of the map carries its patch's factor."""
    gen = torch.Generator().manual_seed(5)
    N, Hm, Wm, g = 2, 3, 4, 2
    mask = U.make_mask('random', N, Hm, Wm, gen)
    ref = 1 - mask.view(N, Hm, Wm).repeat_interleave(g, 1).repeat_interleave(g, 2)
    assert torch.equal(U.keep_map(mask, N, Hm * g, Wm * g, g)[..., 0], ref.double())
    assert not torch.equal(U.keep_map(mask, N, Hm * g, Wm * g, g, shift=1)[..., 0], ref.double())


@pytest.mark.parametrize('case', U.GATHER_CASES, ids=U.pair_id)
def test_gather_restatements_agree_with_unfold(case):
    (B, Hm, Wm, p, Cc, K), dtype = case
    d = U.gather_data(case)
    rows = d['x'].view(B, Hm, p, Wm, p, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, Hm * Wm, p * p * Cc)
    want = torch.gather(rows, 1, d['ids_keep'].long().unsqueeze(-1).expand(B, K, p * p * Cc)).reshape(B * K, -1)
    assert torch.equal(U.gather_restated(d['x'], d['ids_keep'], Hm, Wm, p), want)
    # the backward is the adjoint: <gather(x), dout> == <x, gather_bwd(dout)> (exact in float64 up to summation order)
    dx = U.gather_bwd_restated(d['dout'], d['ids_restore'], K, Hm, Wm, p, Cc)
    a = float((want.double() * d['dout'].double()).sum())
    b = float((d['x'].double() * dx.double()).sum())
    assert abs(a - b) <= 1e-9 * max(1.0, abs(a))
    kept = (d['ids_restore'] < K).sum().item()
    assert kept == B * K


@pytest.mark.parametrize('case', U.TOKEN_CASES, ids=U.pair_id)
def test_token_restatements_agree_with_the_reference_ops(case):
    (B, Ln, K, D), dtype = case
    d = U.token_data(case)
    # encoder: the reference gathers (x + pos) rows; x here is already the kept rows
    want = d['x'] + torch.gather(d['pos'].unsqueeze(0).expand(B, Ln, D), 1,
                                 d['ids_keep'].long().unsqueeze(-1).expand(B, K, D))
    assert torch.equal(U.pos_gather_add_restated(d['x'], d['pos'], d['ids_keep'], torch.float32), want)
    # decoder: cat([x, mask_tokens]) gathered by ids_restore, + pos (mae.py:516-527 without the class row)
    mt = d['mask_token'].view(1, 1, D).expand(B, Ln - K, D)
    full = torch.cat([d['x'], mt], 1)
    ref = torch.gather(full, 1, d['ids_restore'].long().unsqueeze(-1).expand(B, Ln, D)) + d['pos']
    assert torch.equal(U.unshuffle_restated(d['x'], d['mask_token'], d['pos'], d['ids_restore'], torch.float32), ref)
    # the pos gradient against autograd, to summation order
    pos = d['pos'].clone().double().requires_grad_(True)
    (torch.gather(pos.unsqueeze(0).expand(B, Ln, D), 1, d['ids_keep'].long().unsqueeze(-1).expand(B, K, D)) *
     d['dout_k'].double()).sum().backward()
    got = U.pos_gather_add_bwd_restated(d['dout_k'], d['ids_restore'], K)
    assert torch.allclose(got.double(), pos.grad, rtol=1e-5, atol=1e-5)


def test_workspace_formulas_match_the_header():
    """ops.py, convmae_util.py and the macros of include/passl_hip.h state the same sizes."""
    assert shutil.which('gcc'), 'this test compiles a three-line C program against include/passl_hip.h: gcc must be on PATH'
    shapes = [(1, 1, 1, 8), (3, 8, 12, 40), (128, 56, 56, 256), (128, 28, 28, 384), (52, 33, 17, 8)]
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'passl_hip.h')
    body = ''.join('printf("%%lld\\n", (long long)PASSL_DWCONV5_WGRAD_WS_FLOATS(%d, %d, %d, %d));' % s for s in shapes)
    body += 'printf("%lld\\n", (long long)PASSL_TOKENS_UNSHUFFLE_BWD_WS_FLOATS(512));'
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'ws.c'), os.path.join(tmp, 'ws')
        open(src, 'w').write('#include "%s"\n#include <stdio.h>\nint main(){%s return 0;}\n' % (header, body))
        subprocess.check_call(['gcc', src, '-o', exe])
        out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    want = [ops.dwconv5_wgrad_ws_floats(*s) for s in shapes] + [ops.tokens_unshuffle_bwd_ws_floats(512)]
    assert out == want
    assert want[:-1] == [U.wgrad_ws_floats(*s) for s in shapes]


@pytest.fixture(scope='module')
def lib():
    return L.load()


def test_arguments_are_validated_before_any_launch(lib):
    """NULL pointers, C % 8, misaligned pointers, non-positive sizes, an unknown dtype, a short workspace, a map that
    does not lie over the mask grid by one integer factor: a status, never a launch (host memory stands in for device
    pointers: nothing may touch it)."""
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)
    EINVAL, EUNSUP = L.EINVAL, L.EUNSUPPORTED
    fwd, bwd, wg = (lib.passl_hip_dwconv5_masked_fwd, lib.passl_hip_dwconv5_masked_bwd_data,
                    lib.passl_hip_dwconv5_masked_bwd_weight)
    for i in (0, 1, 2, 4):                                          # each pointer but the mask NULL / misaligned in turn
        for bad in (None, odd):
            a = [p, p, p, None, p]
            a[i] = bad
            assert fwd(*a, 1, 4, 4, 8, 0, 0, L.F32, None) == EINVAL
    for i in (0, 1, 3):
        for bad in (None, odd):
            a = [p, p, None, p]
            a[i] = bad
            assert bwd(*a, 1, 4, 4, 8, 0, 0, L.F32, None) == EINVAL
    for i in (0, 1, 3, 4, 5):
        for bad in (None, odd):
            a = [p, p, None, p, p, p]
            a[i] = bad
            assert wg(*a, 1 << 20, 1, 4, 4, 8, 0, 0, L.F32, None) == EINVAL
    for shape in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, -1, 8), (1, 4, 4, 0), (1, 4, 4, 12), (1, 4, 4, 4)):
        assert fwd(p, p, p, None, p, *shape, 0, 0, L.F32, None) == EINVAL
        assert bwd(p, p, None, p, *shape, 0, 0, L.BF16, None) == EINVAL
        assert wg(p, p, None, p, p, p, 1 << 20, *shape, 0, 0, L.F32, None) == EINVAL
    # the mask grid: H % Hm, W % Wm, unequal quotients, an empty grid
    for grid in ((3, 4), (4, 3), (2, 4), (4, 2), (0, 4), (4, 0), (-1, -1), (8, 8)):
        assert fwd(p, p, p, p, p, 1, 4, 4, 8, *grid, L.F32, None) == EINVAL
        assert bwd(p, p, p, p, 1, 4, 4, 8, *grid, L.F32, None) == EINVAL
        assert wg(p, p, p, p, p, p, 1 << 20, 1, 4, 4, 8, *grid, L.F32, None) == EINVAL
    assert fwd(p, p, p, None, p, 1, 4, 4, 8, 0, 0, 7, None) == EUNSUP
    assert fwd(p, p, p, p, p, 1, 4, 4, 8, 2, 2, 7, None) == EUNSUP
    assert wg(p, p, None, p, p, p, 1 << 20, 1, 4, 4, 8, 0, 0, 7, None) == EUNSUP
    need = ops.dwconv5_wgrad_ws_floats(3, 8, 12, 40)
    assert wg(p, p, None, p, p, p, need - 1, 3, 8, 12, 40, 0, 0, L.F32, None) == EINVAL
    assert wg(p, p, None, p, p, None, 0, 3, 8, 12, 40, 0, 0, L.F32, None) == EINVAL

    gf, gb = lib.passl_hip_patch_gather_fwd, lib.passl_hip_patch_gather_bwd
    for fn in (gf, gb):
        for i in range(3):
            a = [p, p, p]
            a[i] = None
            assert fn(*a, 2, 3, 2, 2, 2, 8, L.F32, None) == EINVAL
        for i in (0, 2):
            a = [p, p, p]
            a[i] = odd
            assert fn(*a, 2, 3, 2, 2, 2, 8, L.F32, None) == EINVAL
        for shape in ((0, 3, 2, 2, 2, 8), (2, 0, 2, 2, 2, 8), (2, 5, 2, 2, 2, 8), (2, 3, 0, 2, 2, 8), (2, 3, 2, -2, 2, 8),
                      (2, 3, 2, 2, 0, 8), (2, 3, 2, 2, 2, 12), (2, 3, 2, 2, 2, 0)):
            assert fn(p, p, p, *shape, L.BF16, None) == EINVAL
        assert fn(p, p, p, 2, 3, 2, 2, 2, 8, 9, None) == EUNSUP

    pa, pab = lib.passl_hip_tokens_pos_gather_add, lib.passl_hip_tokens_pos_gather_add_bwd
    un, unb = lib.passl_hip_tokens_unshuffle, lib.passl_hip_tokens_unshuffle_bwd
    for shape in ((0, 4, 2, 8), (2, 0, 2, 8), (2, 4, 0, 8), (2, 4, 5, 8), (2, 4, 2, 0), (2, 4, 2, 12)):
        assert pa(p, p, p, p, *shape, L.F32, None) == EINVAL
        assert pab(p, p, p, *shape, L.F32, None) == EINVAL
        assert un(p, p, p, p, p, *shape, L.F32, None) == EINVAL
        assert unb(p, p, p, p, p, *shape, L.F32, p, 1 << 20, None) == EINVAL
    for i in range(4):
        a = [p, p, p, p]
        a[i] = None
        assert pa(*a, 2, 4, 2, 8, L.F32, None) == EINVAL
    for i in range(3):
        a = [p, p, p]
        a[i] = None
        assert pab(*a, 2, 4, 2, 8, L.F32, None) == EINVAL
    for i in range(5):
        a = [p, p, p, p, p]
        a[i] = None
        assert un(*a, 2, 4, 2, 8, L.F32, None) == EINVAL
        assert unb(*a, 2, 4, 2, 8, L.F32, p, 1 << 20, None) == EINVAL
    assert unb(p, p, p, p, p, 2, 4, 2, 8, L.F32, None, 0, None) == EINVAL
    assert unb(p, p, p, p, p, 2, 4, 2, 8, L.F32, p, 7, None) == EINVAL           # one slab of D = 8 floats
    for fn, args in ((pa, (p, p, p, p)), (pab, (p, p, p)), (un, (p, p, p, p, p))):
        assert fn(*args, 2, 4, 2, 8, 9, None) == EUNSUP
    assert unb(p, p, p, p, p, 2, 4, 2, 8, 9, p, 1 << 20, None) == EUNSUP
    assert all(v == 0.0 for v in buf)


def test_layer_refuses_what_the_kernels_do_not_cover():
    from passl_amd.hip import nn as hnn
    for kw in (dict(dim=12), dict(dim=0), dict(dim=16, kernel_size=7), dict(dim=16, padding=3)):
        with pytest.raises(NotImplementedError):
            hnn.MaskedDepthwiseConv2D(**kw)
