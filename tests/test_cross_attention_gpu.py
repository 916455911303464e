"""Cross-attention kernels (csrc/cross_attention.hip) against a float64 reference, element by element, over the shape /
kind matrix of cross_attention_util.CASES: one query to 1024, one key to 1024, both sides of the key block (64) and of
the query blocks (64 and 128 rows), the 75 queries against 196 keys of CAE pre-training.

The harness is test_attention_tiled_gpu.py's: the kernels are called through the C ABI on views into larger device
buffers; out, lse, dq, dk and dv are NaN before the call and every element must be finite afterwards; every operand
sits between two 4 KiB guard regions that must survive.  Every case is launched twice: the outputs have equal bits.

Paths: fp32 | bf16 aligned (bf16 MFMA) | bf16 with every operand 2 bytes off 16-byte alignment (exact-fp32 MFMA).
Criteria (attention_util.py has the derivations; u = 2^-8, errors in units of the component-wise bound):
  bf16 MFMA    |got - ref| <= 2.25 u (out, dv) / 3.25 u (dq, dk); rms distance to the float64 tiled rounding model
               <= 0.75 of the model's own rms error; <= 1 % of elements further than 0.5 u from the model
  fp32 MFMA    the rule of test_attention_tiled_gpu.py: |got - ref| <= max(4 x float32-eager error of the same case,
               16 * 2^-24 sqrt(max(1, n / 208))), n the length of the tensor's sums (Tk for out and dq, Tq for dk and
               dv); with bf16 storage plus u |value| and, for dq / dk, u c_dq / c_dk
  lse          |got - ref| <= max(4 x float32-eager error, 2^-20 max(1, |lse|))

With Tq = Tk and q, k, v copied out of one packed qkv the five outputs have the bits of passl_hip_attention_tiled_fwd /
_bwd.
"""
import pytest
import torch

import attention_util as A
import cross_attention_util as X
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

B, H = X.B, X.H
IDS = [X.case_id(c) for c in X.CASES]
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
INPUTS = ('q', 'k', 'v', 'dout')
OUTPUTS = ('out', 'lse', 'dq', 'dk', 'dv')


def buffers(B_, Tq, Tk, H_, DH, dtype, skew, d=None):
    nq, nk = B_ * Tq * H_ * DH, B_ * Tk * H_ * DH
    fill = (lambda n: None) if d is None else (lambda n: d[n])
    return {'q': Guarded(nq, dtype, skew, fill=fill('q')), 'k': Guarded(nk, dtype, skew, fill=fill('k')),
            'v': Guarded(nk, dtype, skew, fill=fill('v')), 'dout': Guarded(nq, dtype, skew, fill=fill('dout')),
            'out': Guarded(nq, dtype, skew), 'lse': Guarded(B_ * H_ * Tq, torch.float32, skew),
            'dq': Guarded(nq, dtype, skew), 'dk': Guarded(nk, dtype, skew), 'dv': Guarded(nk, dtype, skew)}


def call_fwd(p, B_, Tq, Tk, H_, DH, scale, dt):
    return L.load().passl_hip_cross_attention_fwd(p['q'], p['k'], p['v'], p['out'], p['lse'], B_, Tq, Tk, H_, DH, scale,
                                                  dt, L.stream())


def call_bwd(p, B_, Tq, Tk, H_, DH, scale, dt):
    return L.load().passl_hip_cross_attention_bwd(p['q'], p['k'], p['v'], p['out'], p['dout'], p['lse'], p['dq'], p['dk'],
                                                  p['dv'], B_, Tq, Tk, H_, DH, scale, dt, L.stream())


def run_twice(g, what, B_, Tq, Tk, H_, DH, scale, dtype):
    """Forward and backward on the guarded buffers, twice: finite everywhere, guards intact, equal bits.  Returns CPU
    fp32 tensors."""
    p = {n: L.ptr(b.view) for n, b in g.items()}
    raws = []
    for _ in range(2):
        for n in OUTPUTS:
            g[n].reset()
        L.check(call_fwd(p, B_, Tq, Tk, H_, DH, scale, L.dt(dtype)), 'cross_attention_fwd')
        L.check(call_bwd(p, B_, Tq, Tk, H_, DH, scale, L.dt(dtype)), 'cross_attention_bwd')
        torch.cuda.synchronize()
        raws.append({n: g[n].raw() for n in OUTPUTS})
    for name, buf in g.items():
        assert buf.intact(), '%s: a guard region of %s was written' % (what, name)
    got = {n: g[n].view.float().cpu().view(B_, Tq if n in ('out', 'dq') else Tk, H_, DH) for n in ('out', 'dq', 'dk', 'dv')}
    got['lse'] = g['lse'].view.cpu().view(B_, H_, Tq)
    for name in OUTPUTS:
        fin = torch.isfinite(got[name])
        assert fin.all(), '%s: %d elements of %s were not written (first flat index %d)' % (
            what, int((~fin).sum()), name, int((~fin).flatten().nonzero()[0]))
        assert torch.equal(raws[0][name], raws[1][name]), '%s: two launches differ in %s' % (what, name)
    return got, raws[1]


def launch(case, dtype, skew=0):
    DH, Tq, Tk, _ = case
    d = X.case_data(case)
    g = buffers(B, Tq, Tk, H, DH, dtype, skew, d)
    got, _ = run_twice(g, X.case_id(case), B, Tq, Tk, H, DH, d['scale'], dtype)
    for n in INPUTS:
        assert torch.equal(g[n].view.float().cpu(), d[n].flatten()), '%s was modified' % n
    return got


def lse_violations(case, got, d):
    ref = d['ref']['lse']
    eager = float((d['eager']['lse'].double() - ref).abs().max())
    allow = torch.maximum(torch.full_like(ref, 4 * eager), 2.0 ** -20 * ref.abs().clamp_min(1.0))
    used = ((got['lse'].double() - ref).abs() / allow).flatten()
    idx = int(used.argmax())
    print('FIG %s lse used %.3f of max(4 x %.3g, 2^-20 |lse|)' % (X.case_id(case), float(used[idx]), eager))
    if not used[idx] <= 1:
        b, h, t = [int(x) for x in torch.unravel_index(torch.as_tensor(idx), ref.shape)]
        return ['lse at (b=%d, h=%d, t=%d): got %.9g, reference %.9g, allowed %.4g' % (
            b, h, t, got['lse'].flatten()[idx], ref.flatten()[idx], allow.flatten()[idx])]
    return []


def check_bf16_mfma(case, path, got):
    d = X.case_data(case)
    for n in A.TENSORS:
        b = d['ref']['b_' + n]
        assert A.underflow_share(b) <= 0.01
        num, den, share = A.closeness(got[n], d['model'][n], d['ref'][n], b)
        err = A.scaled_error(got[n], d['ref'][n], b)[0]
        print('FIG %s %s %s err %.3f u (limit %.2f u, %.3f of it)  rms %.3g vs model %.3g  share %.3f %%' % (
            path, X.case_id(case), n, err / A.U, A.LIMIT_BF16[n] / A.U, err / A.LIMIT_BF16[n], num, den, 100 * share))
    res = A.bf16_violations(got, d['model'], d['ref'])
    msgs = sum(res.values(), []) + lse_violations(case, got, d)
    assert not msgs, '%s, %s:\n' % (path, X.case_id(case)) + '\n'.join(msgs)


def fp32_floor(n):
    return 16 * 2.0 ** -24 * max(1.0, n / 208) ** 0.5


def check_fp32_mfma(case, path, got, bf16_storage):
    _, Tq, Tk, _ = case
    d = X.case_data(case)
    ref = d['ref']
    msgs = []
    for n in A.TENSORS:
        b = ref['b_' + n]
        assert A.underflow_share(b) <= 0.01
        eager = A.scaled_error(d['eager'][n], ref[n], b)[0]
        limit, extra = max(4 * eager, fp32_floor(Tk if n in ('out', 'dq') else Tq)), None
        if bf16_storage:                       # the derivation is check_fp32_mfma's of test_attention_numerics_gpu.py
            extra = A.U * ref[n].abs()
            if n in ('dq', 'dk'):
                extra = extra + (1 + A.U) * A.U * ref['c_' + n]
            limit = limit * (1 + A.U)
        used, _ = A.limit_usage(got[n], ref[n], b, limit, extra)
        print('FIG %s %s %s err %.1f x 2^-24 (eager %.1f), %.3f of the allowance' % (
            path, X.case_id(case), n, A.scaled_error(got[n], ref[n], b)[0] * 2 ** 24, eager * 2 ** 24, used))
        msgs += A.bound_violations(n, got[n], ref[n], b, limit, extra)
    msgs += lse_violations(case, got, d)
    assert not msgs, '%s, %s:\n' % (path, X.case_id(case)) + '\n'.join(msgs)


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_bf16_mfma_kernels(case):
    check_bf16_mfma(case, 'cross-bf16', launch(case, torch.bfloat16))


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_fp32_kernels(case):
    check_fp32_mfma(case, 'cross-fp32', launch(case, torch.float32), bf16_storage=False)


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_unaligned_bf16_takes_the_fp32_mfma_kernels(case):
    check_fp32_mfma(case, 'cross-bf16-unaligned', launch(case, torch.bfloat16, skew=1), bf16_storage=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('DH', X.HEAD_DIMS)
@pytest.mark.parametrize('T', [75, 196, 257])
def test_equal_lengths_have_the_bits_of_the_tiled_self_attention(T, DH, dtype):
    """q, k, v copied out of a packed qkv, Tq = Tk: out, lse, dq, dk, dv equal passl_hip_attention_tiled_fwd / _bwd bit
    for bit, whichever number of waves either launch takes."""
    qkv, dout = A.make_inputs('plain', B, T, H, DH, 1000 * T + DH)
    scale = DH ** -0.5
    d = {'q': qkv[:, :, 0], 'k': qkv[:, :, 1], 'v': qkv[:, :, 2], 'dout': dout}
    g = buffers(B, T, T, H, DH, dtype, 0, d)
    _, raw = run_twice(g, 'T%d-d%d' % (T, DH), B, T, T, H, DH, scale, dtype)
    t = {'qkv': Guarded(qkv.numel(), dtype, 0, fill=qkv), 'dout': Guarded(dout.numel(), dtype, 0, fill=dout),
         'out': Guarded(dout.numel(), dtype), 'lse': Guarded(B * H * T, torch.float32), 'dqkv': Guarded(qkv.numel(), dtype)}
    lib = L.load()
    L.check(lib.passl_hip_attention_tiled_fwd(L.ptr(t['qkv'].view), L.ptr(t['out'].view), L.ptr(t['lse'].view), B, T, H,
                                              DH, scale, L.dt(dtype), L.stream()), 'attention_tiled_fwd')
    L.check(lib.passl_hip_attention_tiled_bwd(L.ptr(t['qkv'].view), L.ptr(t['out'].view), L.ptr(t['dout'].view),
                                              L.ptr(t['lse'].view), L.ptr(t['dqkv'].view), B, T, H, DH, scale,
                                              L.dt(dtype), L.stream()), 'attention_tiled_bwd')
    torch.cuda.synchronize()
    assert all(b.intact() for b in t.values())
    assert torch.equal(raw['out'], t['out'].raw()), 'out'
    assert torch.equal(raw['lse'], t['lse'].raw()), 'lse'
    d3 = t['dqkv'].raw().view(B, T, 3, H, DH)
    for i, n in enumerate(('dq', 'dk', 'dv')):
        assert torch.equal(raw[n].view(B, T, H, DH), d3[:, :, i]), n


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('Tq,Tk,DH,dt,null,code', [
    pytest.param(1025, 64, 64, None, None, EUNSUPPORTED, id='Tq1025'),
    pytest.param(64, 1025, 64, None, None, EUNSUPPORTED, id='Tk1025'),
    pytest.param(0, 64, 64, None, None, EUNSUPPORTED, id='Tq0'),
    pytest.param(64, 0, 64, None, None, EUNSUPPORTED, id='Tk0'),
    pytest.param(75, 196, 48, None, None, EUNSUPPORTED, id='DH48'),
    pytest.param(75, 196, 64, 7, None, EUNSUPPORTED, id='dtype7'),
    pytest.param(75, 196, 64, None, 'q', EINVAL, id='q-null'),
    pytest.param(75, 196, 64, None, 'v', EINVAL, id='v-null'),
    pytest.param(75, 196, 64, None, 'lse', EINVAL, id='lse-null'),
])
def test_outside_the_envelope_nothing_is_launched(Tq, Tk, DH, dt, null, code, dtype):
    """The status, and every output still NaN in every element: no kernel ran."""
    g = buffers(1, max(Tq, 1), max(Tk, 1), 2, 64, dtype, 0)
    for n in INPUTS:
        g[n].view.zero_()
    dt = L.dt(dtype) if dt is None else dt
    p = {n: (None if n == null else L.ptr(b.view)) for n, b in g.items()}
    assert call_fwd(p, 1, Tq, Tk, 2, DH, 0.125, dt) == code
    assert call_bwd(p, 1, Tq, Tk, 2, DH, 0.125, dt) == code
    torch.cuda.synchronize()
    for n in OUTPUTS:
        assert g[n].unwritten() == g[n].hi - g[n].lo, '%s was written' % n
        assert g[n].intact()
