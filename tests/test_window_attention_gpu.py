"""Shifted-window attention (csrc/window_attention.hip) against the float64 restatement of swin_util.py, element by
element, in fp32 and bf16.

The kernels are called through the C ABI on views between guard regions: out, lse, dqkv and dtable are NaN before the
launch and must be fully written, the guards and the inputs must survive, and a second launch must give the same bits
(dtable included: its partials are added in a fixed order).

  bf16 out, dv         2.25 u x bound      one operand rounding (P) and the store (attention_util.LIMIT_BF16)
  bf16 dq, dk          3.25 u x bound      plus the delta formed from the rounded O
  bf16 dtable          1.25 u x bound      only the rounding of the stored O enters delta (at most u a); nothing else is
                                           rounded when the gradient is taken from the fp32 dS
  fp32, every tensor   max(4 x the float32-eager error of the same case, 16 * 2^-24) x bound
  lse                  max(4 x float32-eager error, 2^-20 max(1, |lse|))

At most 1 % of a tensor may have a bound below 2^-100 (nothing to compare with); those elements are held to 2^-100.
"""
import ctypes

import pytest
import torch

import attention_util as A
import swin_util as S
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402
from passl_amd.hip import ops                  # noqa: E402

F32 = torch.float32
FP32_FLOOR = 16 * 2.0 ** -24
MATRIX = [(c, k, s) for c in S.CASES for k in S.KINDS for s in S.TABLE_STD]


def _id(v):
    return S.case_id(v) if isinstance(v, tuple) else str(v)


def launch(case, d, dtype):
    """Forward and backward twice on guarded buffers -> dict of host tensors in the layouts of swin_util."""
    B, Hp, Wp, ws, shift, nH, DH = case
    Ln, T, nW = Hp * Wp, ws * ws, (Hp // ws) * (Wp // ws)
    lib = L.load()
    ins = {'qkv': Guarded(d['qkv'].numel(), dtype, fill=d['qkv']), 'dout': Guarded(d['dout'].numel(), dtype, fill=d['dout']),
           'table': Guarded(d['table'].numel(), F32, fill=d['table'])}
    out, lse = Guarded(B * Ln * nH * DH, dtype), Guarded(B * nW * nH * T, F32)
    dqkv, dtable = Guarded(B * Ln * 3 * nH * DH, dtype), Guarded(d['table'].numel(), F32)
    wsb = Guarded(ops.window_attention_ws_floats(B * nW, nH, ws), F32)
    before = {n: g.raw() for n, g in ins.items()}
    args = (B, Hp, Wp, ws, shift, nH, DH, d['scale'], L.dt(dtype), L.stream())

    def fwd():
        return lib.passl_hip_window_attention_fwd(ins['qkv'].view.data_ptr(), ins['table'].view.data_ptr(),
                                                  out.view.data_ptr(), lse.view.data_ptr(), *args)

    def bwd():
        return lib.passl_hip_window_attention_bwd(ins['qkv'].view.data_ptr(), ins['table'].view.data_ptr(),
                                                  out.view.data_ptr(), ins['dout'].view.data_ptr(), lse.view.data_ptr(),
                                                  dqkv.view.data_ptr(), dtable.view.data_ptr(), wsb.view.data_ptr(),
                                                  wsb.view.numel(), *args)

    assert fwd() == 0
    torch.cuda.synchronize()
    first = {'out': out.raw(), 'lse': lse.raw()}
    assert bwd() == 0
    torch.cuda.synchronize()
    first.update(dqkv=dqkv.raw(), dtable=dtable.raw())
    for g in (dqkv, dtable, wsb):
        g.reset()
    assert bwd() == 0                                    # the same out and lse, fresh outputs and scratch
    torch.cuda.synchronize()
    assert torch.equal(dqkv.raw(), first['dqkv']), 'dqkv differs between two launches on the same inputs'
    assert torch.equal(dtable.raw(), first['dtable']), 'dtable differs between two launches on the same inputs'
    for g in (out, lse):
        g.reset()
    assert fwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.raw(), first['out']) and torch.equal(lse.raw(), first['lse'])
    for n, g in list(ins.items()) + [('out', out), ('lse', lse), ('dqkv', dqkv), ('dtable', dtable), ('ws', wsb)]:
        assert g.intact(), 'a guard region of %s was written' % n
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), 'the input %s was modified' % n
    for n, g in (('out', out), ('lse', lse), ('dqkv', dqkv), ('dtable', dtable)):
        assert g.unwritten() == 0, '%d elements of %s were not written' % (g.unwritten(), n)
    dq = dqkv.view.float().cpu().view(B, Ln, 3, nH, DH)
    return {'out': out.view.float().cpu().view(B, Ln, nH, DH), 'lse': lse.view.cpu().view(B * nW, nH, T),
            'dq': dq[:, :, 0], 'dk': dq[:, :, 1], 'dv': dq[:, :, 2], 'dtable': dtable.view.cpu().view(-1, nH)}


def lse_check(tag, got, d):
    ref = d['ref']['lse']
    eager = float((d['eager']['lse'].double() - ref).abs().max())
    allow = torch.maximum(torch.full_like(ref, 4 * eager), 2.0 ** -20 * ref.abs().clamp_min(1.0))
    used = ((got['lse'].double() - ref).abs() / allow).flatten().nan_to_num(nan=float('inf'))
    idx = int(used.argmax())
    print('FIG %s lse used %.3f of max(4 x %.3g, 2^-20 |lse|)' % (tag, float(used[idx]), eager))
    assert float(used[idx]) <= 1, 'lse at flat %d: got %.9g, reference %.9g, allowed %.4g' % (
        idx, got['lse'].flatten()[idx], ref.flatten()[idx], allow.flatten()[idx])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case,kind,table_std', MATRIX, ids=_id)
def test_window_attention_elementwise(case, kind, table_std, dtype):
    d = S.case_data(case, kind, table_std)
    ref = d['ref']
    got = launch(case, d, dtype)
    tag = '%s %s %s std%g' % ('bf16' if dtype == torch.bfloat16 else 'fp32', S.case_id(case), kind, table_std)
    msgs = []
    for n in S.TENSORS:
        b = ref['b_' + n]
        share = A.underflow_share(b)
        assert share <= 0.01, '%s: %.2f %% of %s has a bound below 2^-100' % (tag, 100 * share, n)
        if dtype == torch.bfloat16:
            limit, eager = S.LIMIT_BF16[n], float('nan')
        else:
            eager = A.scaled_error(d['eager'][n], ref[n], b)[0]
            limit = max(4 * eager, FP32_FLOOR)
        used, idx = S.limit_usage(got[n], ref[n], b, limit)
        print('FIG %s %s err %.4g x bound (eager %.3g), %.3f of the allowance' % (
            tag, n, A.scaled_error(got[n], ref[n], b)[0], eager, used))
        if not used <= 1:
            msgs.append('limit %.4g, %.3f of the allowance used: %s' % (limit, used, S.describe(n, got[n], ref[n], b, idx)))
    assert not msgs, tag + '\n' + '\n'.join(msgs)
    lse_check(tag, got, d)


def test_table_gradient_is_taken_from_the_fp32_dS():
    """swin_util.one_pair_inputs(): a single pair per bin and both roundings near their worst case.  A gradient summed
    from the bf16-rounded dS is 1.95 u of the bound from the reference there (tests/test_swin_host.py), the kernel's has
    to stay inside the 1.25 u limit like every other tensor inside its own."""
    qkv, dout, table, scale = S.one_pair_inputs()
    d = {'qkv': qkv, 'dout': dout, 'table': table, 'scale': scale}
    ref = S.reference(S.ONE_PAIR_CASE, qkv, dout, table, scale)
    got = launch(S.ONE_PAIR_CASE, d, torch.bfloat16)
    for n in S.TENSORS:
        used, idx = S.limit_usage(got[n], ref[n], ref['b_' + n], S.LIMIT_BF16[n])
        print('FIG bf16 one-pair %s %.3f of the allowance' % (n, used))
        assert used <= 1, S.describe(n, got[n], ref[n], ref['b_' + n], idx)


def test_bad_arguments_are_refused_without_a_launch():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(B=1, Hp=14, Wp=14, ws=7, shift=3, nH=1, DH=32, dtype=L.F32, q=p):
        return lib.passl_hip_window_attention_fwd(q, p, p, p, B, Hp, Wp, ws, shift, nH, DH, 0.1, dtype, None)

    def bwd(ws_floats=1 << 30, B=1, Hp=14, Wp=14, ws=7, shift=3, nH=1, DH=32, wsb=p):
        return lib.passl_hip_window_attention_bwd(p, p, p, p, p, p, p, wsb, ws_floats, B, Hp, Wp, ws, shift, nH, DH,
                                                  0.1, L.F32, None)

    assert fwd(q=None) == L.EINVAL and bwd(wsb=None) == L.EINVAL
    assert fwd(ws=15, Hp=15, Wp=15, shift=0) == L.EUNSUPPORTED         # T > 196
    assert fwd(DH=48) == L.EUNSUPPORTED and bwd(DH=16) == L.EUNSUPPORTED
    assert fwd(dtype=7) == L.EUNSUPPORTED
    assert fwd(Hp=15) == L.EINVAL and fwd(Wp=20) == L.EINVAL            # not multiples of the window
    assert fwd(shift=7) == L.EINVAL and fwd(shift=-1) == L.EINVAL
    assert fwd(Hp=7, shift=3) == L.EINVAL                               # a shift on a map one window high
    assert fwd(ws=0) == L.EINVAL and fwd(B=0) == L.EINVAL and fwd(nH=0) == L.EINVAL
    assert bwd(ws_floats=2 * 49 * 49 - 1) == L.EINVAL                   # 4 windows: 2 slabs of [T, T]
    assert lib.passl_hip_patch_merge(p, p, 1, 3, 2, 8, L.F32, None) == L.EINVAL
    assert lib.passl_hip_patch_merge(p, p, 1, 2, 2, 12, L.F32, None) == L.EINVAL
    assert lib.passl_hip_patch_merge_bwd(p, None, 1, 2, 2, 8, L.F32, None) == L.EINVAL


def test_autograd_front_end_returns_dqkv_and_dtable():
    from passl_amd.hip import nn as hnn
    case = S.CASES[1]
    B, Hp, Wp, ws, shift, nH, DH = case
    d = S.case_data(case, 'plain', 1.0)
    qkv = d['qkv'].reshape(B * Hp * Wp, 3 * nH * DH).cuda().requires_grad_()
    table = d['table'].cuda().requires_grad_()
    out = hnn.window_attention(qkv, table, B, Hp, Wp, ws, shift, nH, DH, d['scale'])
    out.backward(d['dout'].reshape(B * Hp * Wp, nH * DH).cuda())
    ref = d['ref']
    eager = A.scaled_error(d['eager']['dtable'], ref['dtable'], ref['b_dtable'])[0]
    used, _ = S.limit_usage(table.grad.cpu(), ref['dtable'], ref['b_dtable'], max(4 * eager, FP32_FLOOR))
    assert used <= 1 and qkv.grad.shape == qkv.shape and bool(torch.isfinite(qkv.grad).all())
