"""Fused attention kernels (csrc/attention.hip, attention_bf16.hip) against a float64 reference, element by
element, on inputs chosen to hurt: every dispatch path over the shape / kind matrix of attention_util.CASES.

The kernels are called through the C ABI on views into larger device buffers: out, lse and dqkv are NaN before
the call and every element must be finite afterwards (each one was written); every operand sits between two
4 KiB guard regions of a fixed bit pattern that must survive.

Paths: fp32 | bf16 default | bf16 attn_waves=4 | bf16 attn_waves=8 | bf16 attn_f32mfma=1 | bf16 default options
with every operand 2 bytes off 16-byte alignment (must take the fp32-MFMA kernels: bit-equal to attn_f32mfma=1).
Criteria (attention_util.py has the derivations; u = 2^-8, all errors in units of the component-wise bound):
  bf16-MFMA paths   |got - ref| <= 2.25 u (out, dv) / 3.25 u (dq, dk); rms distance to the float64 rounding model
                    <= 0.75 of the model's own rms error; <= 1 % of elements further than 0.5 u from the model
  fp32-MFMA paths   |got - ref| <= max(4 x float32-eager error of the same case, 16 * 2^-24); with bf16 storage
                    plus u |value| for the store rounding and, for dq / dk, u c_dq / c_dk for the delta formed
                    from the rounded O (the same term the bf16 limit of 3 u carries)
  lse, every path   |got - ref| <= max(4 x float32-eager error, 2^-20 max(1, |lse|))

Scaled error of float32 eager attention against the float64 reference (closed-form forward and backward in
float32, on the CPU), worst tensor and worst case of each group, in units of 2^-24.  The fp32-MFMA limits are
4 x the figure of the very case and tensor, computed in the test:
  kind       T = 1       T = 15..33    T = 77..129    T = 207, 208
  plain      0.0 - 0.2   5 - 8         6 - 8          6 - 7
  negative   0.0 - 0.4   45 - 100      42 - 116       42 - 99
  ramp       0.1 - 0.4   14 - 31       50 - 100       68 - 93
  vmean      -           33 - 56       48 - 63        64 - 82
  peaked     -           43 - 172      113 - 317      302 - 412     (the score itself carries the rounding error)
"""
import pytest
import torch

import attention_util as A
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

DEV = 'cuda'
B, H = A.B, A.H
IDS = [A.case_id(c) for c in A.CASES]


@pytest.fixture
def attn_options():
    """Sets attn_waves / attn_f32mfma through the option table; both are back at 0 afterwards."""
    def select(**opts):
        for name in ('attn_waves', 'attn_f32mfma'):
            L.set_option(name, opts.get(name, 0))
    yield select
    select()
    assert L.get_option('attn_waves') == 0 and L.get_option('attn_f32mfma') == 0


def launch(case, dtype, skew=0, feed=None):
    """Forward and backward of a case through the C ABI.  `feed` = (out, lse) raw bits of another run to hand to
    the backward in place of this run's own forward results.  Returns CPU fp32 tensors (out, dq, dk, dv
    [B, T, H, DH], lse [B, H, T]) and the raw bits of out, lse and dqkv."""
    DH, T, causal, _ = case
    d = A.case_data(case)
    lib = L.load()
    qkv = Guarded(B * T * 3 * H * DH, dtype, skew, fill=d['qkv'])
    dout = Guarded(B * T * H * DH, dtype, skew, fill=d['dout'])
    out = Guarded(B * T * H * DH, dtype, skew)
    lse = Guarded(B * H * T, torch.float32, skew)
    dqkv = Guarded(B * T * 3 * H * DH, dtype, skew)
    bufs = {'qkv': qkv, 'dout': dout, 'out': out, 'lse': lse, 'dqkv': dqkv}
    L.check(lib.passl_hip_attention_fwd(L.ptr(qkv.view), L.ptr(out.view), L.ptr(lse.view), B, T, H, DH, d['scale'],
                                        int(causal), L.dt(dtype), L.stream()), 'attention_fwd')
    torch.cuda.synchronize()
    raw = {'out': out.raw(), 'lse': lse.raw()}
    if feed is not None:
        out.bits[out.lo:out.hi].copy_(feed[0])
        lse.bits[lse.lo:lse.hi].copy_(feed[1])
    L.check(lib.passl_hip_attention_bwd(L.ptr(qkv.view), L.ptr(out.view), L.ptr(dout.view), L.ptr(lse.view),
                                        L.ptr(dqkv.view), B, T, H, DH, d['scale'], int(causal), L.dt(dtype),
                                        L.stream()), 'attention_bwd')
    torch.cuda.synchronize()
    raw['dqkv'] = dqkv.raw()
    for name, g in bufs.items():
        assert g.intact(), '%s: a guard region of %s was written' % (A.case_id(case), name)
    assert torch.equal(qkv.view.float().cpu(), d['qkv'].flatten()), 'qkv was modified'
    assert torch.equal(dout.view.float().cpu(), d['dout'].flatten()), 'dout was modified'
    got = {'out': out.view.float().cpu().view(B, T, H, DH), 'lse': lse.view.cpu().view(B, H, T)}
    if feed is not None:                                   # `out` holds the fed values now
        got['out'] = raw['out'].view(dtype).float().cpu().view(B, T, H, DH)
        got['lse'] = raw['lse'].view(torch.float32).cpu().view(B, H, T)
    g3 = dqkv.view.float().cpu().view(B, T, 3, H, DH)
    got.update(dq=g3[:, :, 0], dk=g3[:, :, 1], dv=g3[:, :, 2])
    for name in ('out', 'lse', 'dq', 'dk', 'dv'):
        fin = torch.isfinite(got[name])
        assert fin.all(), '%s: %d elements of %s were not written (first flat index %d)' % (
            A.case_id(case), int((~fin).sum()), name, int((~fin).flatten().nonzero()[0]))
    return got, raw


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
    d = A.case_data(case)
    for n in A.TENSORS:
        b = d['ref']['b_' + n]
        num, den, share = A.closeness(got[n], d['model'][n], d['ref'][n], b)
        print('FIG %s %s %s err %.3f u (limit %.2f u)  rms %.3g vs model %.3g  share %.3f %%' % (
            path, A.case_id(case), n, A.scaled_error(got[n], d['ref'][n], b)[0] / A.U, A.LIMIT_BF16[n] / A.U,
            num, den, 100 * share))
    res = A.bf16_violations(got, d['model'], d['ref'])
    msgs = sum(res.values(), []) + lse_violations(case, got, d)
    assert not msgs, '%s, %s:\n' % (path, A.case_id(case)) + '\n'.join(msgs)


FP32_FLOOR = 16 * 2.0 ** -24


def check_fp32_mfma(case, path, got, bf16_storage):
    d = A.case_data(case)
    ref = d['ref']
    msgs = []
    for n in A.TENSORS:
        b = ref['b_' + n]
        eager = A.scaled_error(d['eager'][n], ref[n], b)[0]
        limit, extra = max(4 * eager, FP32_FLOOR), None
        if bf16_storage:
            # computed = ref + e32, stored = computed (1 + r), |r| <= u: |stored - ref| <= (1 + u) e32 + u |ref|;
            # e32 itself gains u c (dq, dk) from the delta the backward forms from the bf16 O it is handed
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


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
@pytest.mark.parametrize('waves', [0, 4, 8])
def test_bf16_mfma_kernels(case, waves, attn_options):
    attn_options(attn_waves=waves)
    got, _ = launch(case, torch.bfloat16)
    check_bf16_mfma(case, 'bf16-waves%d' % waves, got)


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_wave_count_changes_no_bit(case, attn_options):
    """attn_waves=4 / 8 select the workgroup size the default would not; where the default takes that size
    (forward: always 8 waves; backward: 8 waves from 8 row tiles on, T > 112) the results are the default's bits.
    The forced backward is handed the default forward's out and lse, so only its own wave count is in play."""
    T = case[1]
    attn_options()
    _, base = launch(case, torch.bfloat16)
    same_bwd = 8 if T > 112 else 4
    for waves in (4, 8):
        attn_options(attn_waves=waves)
        _, raw = launch(case, torch.bfloat16, feed=(base['out'], base['lse']))
        if waves == 8:
            assert torch.equal(raw['out'], base['out']) and torch.equal(raw['lse'], base['lse']), \
                '%s: the 8-wave forward differs from the default forward' % A.case_id(case)
        if waves == same_bwd:
            assert torch.equal(raw['dqkv'], base['dqkv']), \
                '%s: the %d-wave backward differs from the default backward' % (A.case_id(case), waves)


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_fp32_kernels(case, attn_options):
    attn_options()
    got, _ = launch(case, torch.float32)
    check_fp32_mfma(case, 'fp32', got, bf16_storage=False)


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_bf16_through_fp32_mfma_and_unaligned_fallback(case, attn_options):
    attn_options(attn_f32mfma=1)
    got, forced = launch(case, torch.bfloat16)
    check_fp32_mfma(case, 'bf16-f32mfma', got, bf16_storage=True)
    attn_options()
    got, skewed = launch(case, torch.bfloat16, skew=1)
    for n in ('out', 'lse', 'dqkv'):
        assert torch.equal(skewed[n], forced[n]), \
            '%s: %s of the unaligned call differs from the fp32-MFMA kernels' % (A.case_id(case), n)
    check_fp32_mfma(case, 'bf16-unaligned', got, bf16_storage=True)
