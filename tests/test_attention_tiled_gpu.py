"""Key-tiled attention kernels (csrc/attention_tiled.hip) against a float64 reference, element by element, over the
shape / kind matrix of attention_tiled_util.CASES: 1 to 1024 tokens, both sides of every multiple of the key block (64)
and of the query blocks (64 and 128 rows), the 577 / 578 / 785 tokens of the models that need them.

The harness is test_attention_numerics_gpu.py's: the kernels are called through the C ABI on views into larger device
buffers; out, lse and dqkv are NaN before the call and every element must be finite afterwards; every operand sits
between two 4 KiB guard regions that must survive.  Every case is launched twice: out, lse and dqkv have equal bits.

Paths: fp32 | bf16 aligned (bf16 MFMA) | bf16 with every operand 2 bytes off 16-byte alignment (exact-fp32 MFMA).
Criteria (attention_util.py has the derivations; u = 2^-8, errors in units of the component-wise bound):
  bf16 MFMA    |got - ref| <= 2.25 u (out, dv) / 3.25 u (dq, dk); rms distance to the float64 TILED rounding model
               <= 0.75 of the model's own rms error; <= 1 % of elements further than 0.5 u from the model
  fp32 MFMA    |got - ref| <= max(4 x float32-eager error of the same case, 16 * 2^-24 sqrt(max(1, T / 208))); with bf16
               storage plus u |value| and, for dq / dk, u c_dq / c_dk (check_fp32_mfma of the dense test).  The floor
               admits accumulation-order differences, which grow with the square root of the chain length; 208 is
               where the dense figure was set.  A bf16-level defect is three orders of magnitude above it.
  lse          |got - ref| <= max(4 x float32-eager error, 2^-20 max(1, |lse|))
"""
import pytest
import torch

import attention_tiled_util as TU
import attention_util as A
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

B, H = TU.B, TU.H
IDS = [A.case_id(c) for c in TU.CASES]
OK, EINVAL, EUNSUPPORTED = 0, -1, -3


def buffers(B_, T, H_, DH, dtype, skew, d=None):
    g = {'qkv': Guarded(B_ * T * 3 * H_ * DH, dtype, skew, fill=None if d is None else d['qkv']),
         'dout': Guarded(B_ * T * H_ * DH, dtype, skew, fill=None if d is None else d['dout']),
         'out': Guarded(B_ * T * H_ * DH, dtype, skew),
         'lse': Guarded(B_ * H_ * T, torch.float32, skew),
         'dqkv': Guarded(B_ * T * 3 * H_ * DH, dtype, skew)}
    return g


def call_fwd(g, B_, T, H_, DH, scale, dt):
    return L.load().passl_hip_attention_tiled_fwd(L.ptr(g['qkv'].view), L.ptr(g['out'].view), L.ptr(g['lse'].view), B_, T,
                                                  H_, DH, scale, dt, L.stream())


def call_bwd(g, B_, T, H_, DH, scale, dt):
    return L.load().passl_hip_attention_tiled_bwd(L.ptr(g['qkv'].view), L.ptr(g['out'].view), L.ptr(g['dout'].view),
                                                  L.ptr(g['lse'].view), L.ptr(g['dqkv'].view), B_, T, H_, DH, scale, dt,
                                                  L.stream())


def launch(case, dtype, skew=0):
    """Forward and backward of a case through the C ABI, twice.  Returns CPU fp32 tensors (out, dq, dk, dv
    [B, T, H, DH], lse [B, H, T])."""
    DH, T, _, _ = case
    d = TU.case_data(case)
    g = buffers(B, T, H, DH, dtype, skew, d)
    raws = []
    for _ in range(2):
        for n in ('out', 'lse', 'dqkv'):
            g[n].reset()
        L.check(call_fwd(g, B, T, H, DH, d['scale'], L.dt(dtype)), 'attention_tiled_fwd')
        L.check(call_bwd(g, B, T, H, DH, d['scale'], L.dt(dtype)), 'attention_tiled_bwd')
        torch.cuda.synchronize()
        raws.append({n: g[n].raw() for n in ('out', 'lse', 'dqkv')})
    for name, buf in g.items():
        assert buf.intact(), '%s: a guard region of %s was written' % (A.case_id(case), name)
    assert torch.equal(g['qkv'].view.float().cpu(), d['qkv'].flatten()), 'qkv was modified'
    assert torch.equal(g['dout'].view.float().cpu(), d['dout'].flatten()), 'dout was modified'
    got = {'out': g['out'].view.float().cpu().view(B, T, H, DH), 'lse': g['lse'].view.cpu().view(B, H, T)}
    g3 = g['dqkv'].view.float().cpu().view(B, T, 3, H, DH)
    got.update(dq=g3[:, :, 0], dk=g3[:, :, 1], dv=g3[:, :, 2])
    for name in ('out', 'lse', 'dq', 'dk', 'dv'):
        fin = torch.isfinite(got[name])
        assert fin.all(), '%s: %d elements of %s were not written (first flat index %d)' % (
            A.case_id(case), int((~fin).sum()), name, int((~fin).flatten().nonzero()[0]))
    for n in ('out', 'lse', 'dqkv'):
        assert torch.equal(raws[0][n], raws[1][n]), '%s: two launches differ in %s' % (A.case_id(case), n)
    return got


def lse_violations(case, got, d):
    ref = d['ref']['lse']
    eager = float((d['eager']['lse'].double() - ref).abs().max())
    allow = torch.maximum(torch.full_like(ref, 4 * eager), 2.0 ** -20 * ref.abs().clamp_min(1.0))
    used = ((got['lse'].double() - ref).abs() / allow).flatten()
    idx = int(used.argmax())
    print('FIG %s lse used %.3f of max(4 x %.3g, 2^-20 |lse|)' % (A.case_id(case), float(used[idx]), eager))
    if not used[idx] <= 1:
        b, h, t = [int(x) for x in torch.unravel_index(torch.as_tensor(idx), ref.shape)]
        return ['lse at (b=%d, h=%d, t=%d): got %.9g, reference %.9g, allowed %.4g' % (
            b, h, t, got['lse'].flatten()[idx], ref.flatten()[idx], allow.flatten()[idx])]
    return []


def check_bf16_mfma(case, path, got):
    d = TU.case_data(case)
    for n in A.TENSORS:
        b = d['ref']['b_' + n]
        assert A.underflow_share(b) <= 0.01
        num, den, share = A.closeness(got[n], d['model'][n], d['ref'][n], b)
        err = A.scaled_error(got[n], d['ref'][n], b)[0]
        print('FIG %s %s %s err %.3f u (limit %.2f u, %.3f of it)  rms %.3g vs model %.3g  share %.3f %%' % (
            path, A.case_id(case), n, err / A.U, A.LIMIT_BF16[n] / A.U, err / A.LIMIT_BF16[n], num, den, 100 * share))
    res = A.bf16_violations(got, d['model'], d['ref'])
    msgs = sum(res.values(), []) + lse_violations(case, got, d)
    assert not msgs, '%s, %s:\n' % (path, A.case_id(case)) + '\n'.join(msgs)


def fp32_floor(T):
    return 16 * 2.0 ** -24 * max(1.0, T / 208) ** 0.5


def check_fp32_mfma(case, path, got, bf16_storage):
    d = TU.case_data(case)
    ref = d['ref']
    msgs = []
    for n in A.TENSORS:
        b = ref['b_' + n]
        assert A.underflow_share(b) <= 0.01
        eager = A.scaled_error(d['eager'][n], ref[n], b)[0]
        limit, extra = max(4 * eager, fp32_floor(case[1])), None
        if bf16_storage:                       # the derivation is check_fp32_mfma's of test_attention_numerics_gpu.py
            extra = A.U * ref[n].abs()
            if n in ('dq', 'dk'):
                extra = extra + (1 + A.U) * A.U * ref['c_' + n]
            limit = limit * (1 + A.U)
        used, _ = A.limit_usage(got[n], ref[n], b, limit, extra)
        print('FIG %s %s %s err %.1f x 2^-24 (eager %.1f), %.3f of the allowance' % (
            path, A.case_id(case), n, A.scaled_error(got[n], ref[n], b)[0] * 2 ** 24, eager * 2 ** 24, used))
        msgs += A.bound_violations(n, got[n], ref[n], b, limit, extra)
    msgs += lse_violations(case, got, d)
    assert not msgs, '%s, %s:\n' % (path, A.case_id(case)) + '\n'.join(msgs)


@pytest.mark.parametrize('case', TU.CASES, ids=IDS)
def test_bf16_mfma_kernels(case):
    check_bf16_mfma(case, 'tiled-bf16', launch(case, torch.bfloat16))


@pytest.mark.parametrize('case', TU.CASES, ids=IDS)
def test_fp32_kernels(case):
    check_fp32_mfma(case, 'tiled-fp32', launch(case, torch.float32), bf16_storage=False)


@pytest.mark.parametrize('case', TU.CASES, ids=IDS)
def test_unaligned_bf16_takes_the_fp32_mfma_kernels(case):
    check_fp32_mfma(case, 'tiled-bf16-unaligned', launch(case, torch.bfloat16, skew=1), bf16_storage=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('T,DH,dt,null,code', [
    pytest.param(1025, 64, None, None, EUNSUPPORTED, id='T1025'),
    pytest.param(0, 64, None, None, EUNSUPPORTED, id='T0'),
    pytest.param(300, 48, None, None, EUNSUPPORTED, id='DH48'),
    pytest.param(300, 64, 7, None, EUNSUPPORTED, id='dtype7'),
    pytest.param(300, 64, None, 'qkv', EINVAL, id='qkv-null'),
    pytest.param(300, 64, None, 'lse', EINVAL, id='lse-null'),
])
def test_outside_the_envelope_nothing_is_launched(T, DH, dt, null, code, dtype):
    """The status, and out / lse / dqkv still NaN in every element: no kernel ran."""
    Tb = max(T, 1)
    g = buffers(1, Tb, 2, 64, dtype, 0)
    g['qkv'].view.zero_()
    g['dout'].view.zero_()
    dt = L.dt(dtype) if dt is None else dt
    p = {n: (None if n == null else L.ptr(b.view)) for n, b in g.items()}
    lib = L.load()
    assert lib.passl_hip_attention_tiled_fwd(p['qkv'], p['out'], p['lse'], 1, T, 2, DH, 0.125, dt, L.stream()) == code
    assert lib.passl_hip_attention_tiled_bwd(p['qkv'], p['out'], p['dout'], p['lse'], p['dqkv'], 1, T, 2, DH, 0.125, dt,
                                             L.stream()) == code
    torch.cuda.synchronize()
    for n in ('out', 'lse', 'dqkv'):
        assert g[n].unwritten() == g[n].hi - g[n].lo, '%s was written' % n
        assert g[n].intact()
