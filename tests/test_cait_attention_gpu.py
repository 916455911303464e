"""Talking-heads and class attention (csrc/cait_attention.hip) against the float64 restatement of cait_util.py, element
by element, in fp32 and bf16.

The kernels are called through the C ABI on views between guard regions: every output and the workspace are NaN before
the launch, the outputs must be fully written, the guards and the inputs must survive, and a second launch must give
the same bits (the four small gradients included: their partials are added in a fixed order).

  bf16 out, dq, dk, dv        1.25 u x bound     one rounding, the store: the arithmetic is fp32 (cait_util.LIMIT_BF16)
  bf16 dwl, dbl, dww, dbw     0.25 u x bound     fp32 throughout, never rounded to bf16
  fp32, every tensor          max(4 x the float32-eager restatement's error on the same case, 16 * 2^-24) x bound
  lse                         max(4 x float32-eager error, 2^-20 max(1, |lse|))
  bf16 out, dq, dk, dv        the rms / share criteria of attention_util.closeness_violations against the rounding model

dbl has reference 0 and is held to its bound like every other tensor.  No element of a talking-heads tensor has a bound
below 2^-100 (tests/test_cait_host.py asserts it for every case here); class attention: see that file.
"""
import pytest
import torch

import attention_util as A
import cait_util as C
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402
from passl_amd.hip import ops                  # noqa: E402

F32 = torch.float32
MATRIX = [(c, k, dv) for c in C.CASES for k in C.KINDS for dv in C.DEVS]
CLS_MATRIX = [(c, k) for c in C.CLS_CASES for k in C.KINDS]
_refs = {}


def _id(v):
    return C.case_id(v) if isinstance(v, tuple) else str(v)


def case_refs(key, make, ref):
    """(inputs, float64 reference, float32-eager restatement, rounding model) of a case, computed once for both dtypes."""
    if key not in _refs:
        d = make()
        _refs[key] = (d, ref(d), ref(d, dtype=torch.float32), ref(d, round_out=True))
    return _refs[key]


def _check_guards(ins, before, outs, scratch=()):
    for n, g in list(ins.items()) + list(outs.items()) + list(scratch):
        assert g.intact(), 'a guard region of %s was written' % n
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), 'the input %s was modified' % n
    for n, g in outs.items():
        assert g.unwritten() == 0, '%d elements of %s were not written' % (g.unwritten(), n)


def launch(case, d, dtype):
    """Forward and backward twice on guarded buffers -> dict of host tensors in the layouts of cait_util."""
    B, T, H = case
    DH = C.DH
    lib = L.load()
    ins = {n: Guarded(d[n].numel(), dtype if n in ('qkv', 'dout') else F32, fill=d[n])
           for n in ('qkv', 'dout', 'wl', 'bl', 'ww', 'bw')}
    outs = {'out': Guarded(B * T * H * DH, dtype), 'lse': Guarded(B * H * T, F32), 'dqkv': Guarded(B * T * 3 * H * DH, dtype),
            'dwl': Guarded(H * H, F32), 'dbl': Guarded(H, F32), 'dww': Guarded(H * H, F32), 'dbw': Guarded(H, F32)}
    wsb = Guarded(ops.talking_heads_attention_ws_floats(B, T, H), F32)
    before = {n: g.raw() for n, g in ins.items()}
    p = lambda g: g.view.data_ptr()                                                   # noqa: E731
    mix = [p(ins[n]) for n in ('wl', 'bl', 'ww', 'bw')]
    args = (B, T, H, DH, d['scale'], L.dt(dtype), L.stream())

    def fwd():
        return lib.passl_hip_talking_heads_attention_fwd(p(ins['qkv']), *mix, p(outs['out']), p(outs['lse']), *args)

    def bwd():
        return lib.passl_hip_talking_heads_attention_bwd(
            p(ins['qkv']), *mix, p(ins['dout']), p(outs['lse']), p(outs['dqkv']), p(outs['dwl']), p(outs['dbl']),
            p(outs['dww']), p(outs['dbw']), p(wsb), wsb.view.numel(), *args)

    assert fwd() == 0
    torch.cuda.synchronize()
    first = {n: outs[n].raw() for n in ('out', 'lse')}
    assert bwd() == 0
    torch.cuda.synchronize()
    grads = ('dqkv', 'dwl', 'dbl', 'dww', 'dbw')
    first.update({n: outs[n].raw() for n in grads})
    for g in [outs[n] for n in grads] + [wsb]:
        g.reset()
    assert bwd() == 0                                    # the same lse, fresh outputs and workspace
    torch.cuda.synchronize()
    for n in grads:
        assert torch.equal(outs[n].raw(), first[n]), '%s differs between two launches on the same inputs' % n
    for n in ('out', 'lse'):
        outs[n].reset()
    assert fwd() == 0
    torch.cuda.synchronize()
    assert torch.equal(outs['out'].raw(), first['out']) and torch.equal(outs['lse'].raw(), first['lse'])
    _check_guards(ins, before, outs, [('ws', wsb)])
    dq = outs['dqkv'].view.float().cpu().view(B, T, 3, H, DH)
    got = {'out': outs['out'].view.float().cpu().view(B, T, H, DH), 'lse': outs['lse'].view.cpu().view(B, H, T),
           'dq': dq[:, :, 0], 'dk': dq[:, :, 1], 'dv': dq[:, :, 2]}
    got.update({n: outs[n].view.cpu().view(H, H) if n in ('dwl', 'dww') else outs[n].view.cpu() for n in grads[1:]})
    return got


def launch_cls(case, d, dtype):
    B, T, H = case
    DH = C.DH
    lib = L.load()
    ins = {n: Guarded(d[n].numel(), dtype, fill=d[n]) for n in ('q', 'k', 'v', 'dout')}
    outs = {'out': Guarded(B * H * DH, dtype), 'lse': Guarded(B * H, F32), 'dq': Guarded(B * H * DH, dtype),
            'dk': Guarded(B * T * H * DH, dtype), 'dv': Guarded(B * T * H * DH, dtype)}
    before = {n: g.raw() for n, g in ins.items()}
    p = lambda g: g.view.data_ptr()                                                   # noqa: E731
    args = (B, T, H, DH, d['scale'], L.dt(dtype), L.stream())

    def run():
        assert lib.passl_hip_class_attention_fwd(p(ins['q']), p(ins['k']), p(ins['v']), p(outs['out']), p(outs['lse']),
                                                 *args) == 0
        assert lib.passl_hip_class_attention_bwd(p(ins['q']), p(ins['k']), p(ins['v']), p(ins['dout']), p(outs['lse']),
                                                 p(outs['dq']), p(outs['dk']), p(outs['dv']), *args) == 0
        torch.cuda.synchronize()
        return {n: g.raw() for n, g in outs.items()}

    first = run()
    for g in outs.values():
        g.reset()
    second = run()
    for n in outs:
        assert torch.equal(first[n], second[n]), '%s differs between two launches on the same inputs' % n
    _check_guards(ins, before, outs)
    return {'out': outs['out'].view.float().cpu().view(B, H, DH), 'lse': outs['lse'].view.cpu().view(B, H),
            'dq': outs['dq'].view.float().cpu().view(B, H, DH), 'dk': outs['dk'].view.float().cpu().view(B, T, H, DH),
            'dv': outs['dv'].view.float().cpu().view(B, T, H, DH)}


def check(tag, got, ref, eager, model, dtype, tensors, limits, big):
    msgs = []
    for n in tensors:
        b = ref['b_' + n]
        if dtype == torch.bfloat16:
            limit, e = limits[n], float('nan')
        else:
            e = A.scaled_error(eager[n], ref[n], b)[0]
            limit = max(4 * e, C.FP32_FLOOR)
        used, idx = A.limit_usage(got[n], ref[n], b, limit)
        print('FIG %s %s err %.4g x bound (eager %.3g), %.3f of the allowance' % (
            tag, n, A.scaled_error(got[n], ref[n], b)[0], e, used))
        if not used <= 1:
            g, r, bb = [x.double().flatten()[idx] for x in (got[n], ref[n], b)]
            msgs.append('%s limit %.4g, %.3f of the allowance used at flat %d: got %.9g, reference %.9g, bound %.6g'
                        % (n, limit, used, idx, g, r, bb))
        if dtype == torch.bfloat16 and n in big:
            msgs += A.closeness_violations(n, got[n], model[n], ref[n], b)
    e = float((eager['lse'].double() - ref['lse']).abs().max())
    allow = torch.maximum(torch.full_like(ref['lse'], 4 * e), 2.0 ** -20 * ref['lse'].abs().clamp_min(1.0))
    used = float(((got['lse'].double() - ref['lse']).abs() / allow).nan_to_num(nan=float('inf')).max())
    print('FIG %s lse used %.3f of max(4 x %.3g, 2^-20 |lse|)' % (tag, used, e))
    if not used <= 1:
        msgs.append('lse: %.3f of the allowance used' % used)
    assert not msgs, tag + '\n' + '\n'.join(msgs)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case,kind,dev', MATRIX, ids=_id)
def test_talking_heads_attention_elementwise(case, kind, dev, dtype):
    d, ref, eager, model = case_refs((case, kind, dev), lambda: C.make_case(case, kind, dev), C.reference)
    got = launch(case, d, dtype)
    tag = '%s th %s %s dev%g' % ('bf16' if dtype == torch.bfloat16 else 'fp32', C.case_id(case), kind, dev)
    check(tag, got, ref, eager, model, dtype, C.TENSORS, C.LIMIT_BF16, C.BIG)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case,kind', CLS_MATRIX, ids=_id)
def test_class_attention_elementwise(case, kind, dtype):
    d, ref, eager, model = case_refs(('cls', case, kind), lambda: C.make_cls_case(case, kind), C.cls_reference)
    got = launch_cls(case, d, dtype)
    tag = '%s cls %s %s' % ('bf16' if dtype == torch.bfloat16 else 'fp32', C.case_id(case), kind)
    check(tag, got, ref, eager, model, dtype, C.CLS_TENSORS, C.CLS_LIMIT_BF16, C.CLS_TENSORS)


def test_pad_key_inputs_are_inside_the_limits():
    """cait_util.pad_key_inputs(): a padded key taking part in the softmax would take nearly all of its mass."""
    d = C.pad_key_inputs()
    ref = C.reference(d)
    got = launch((2, 5, 2), d, torch.bfloat16)
    assert not C.violations(got, ref, C.LIMIT_BF16, C.TENSORS)


def test_envelope_is_refused_without_a_launch():
    """DH = 40, T = 209, H = 9 and a misaligned bf16 pointer return an error code and leave every output as it was."""
    lib = L.load()
    B, T, H, DH = 1, 16, 2, 48
    n = 2 * 209 * 3 * 9 * 48
    qkv, dout = Guarded(n, torch.bfloat16, fill=torch.zeros(n)), Guarded(n, torch.bfloat16, fill=torch.zeros(n))
    skew = Guarded(n, torch.bfloat16, skew=1, fill=torch.zeros(n))
    mixb = Guarded(128, F32, fill=torch.zeros(128))
    outs = [Guarded(n, torch.bfloat16) for _ in range(4)] + [Guarded(n, F32) for _ in range(6)]
    out, dqkv, dk, dv, lse, wsb, g0, g1, g2, g3 = outs
    p = lambda g: g.view.data_ptr()                                                   # noqa: E731
    m = [p(mixb)] * 4

    def th_fwd(q=qkv, T=T, H=H, DH=DH):
        return lib.passl_hip_talking_heads_attention_fwd(p(q), *m, p(out), p(lse), B, T, H, DH, 0.1, L.BF16, None)

    def th_bwd(q=qkv, T=T, H=H, DH=DH, ws_floats=n):
        return lib.passl_hip_talking_heads_attention_bwd(p(q), *m, p(dout), p(lse), p(dqkv), p(g0), p(g1), p(g2), p(g3),
                                                         p(wsb), ws_floats, B, T, H, DH, 0.1, L.BF16, None)

    def cls_fwd(q=qkv, T=T, H=H, DH=DH):
        return lib.passl_hip_class_attention_fwd(p(q), p(qkv), p(qkv), p(out), p(lse), B, T, H, DH, 0.1, L.BF16, None)

    def cls_bwd(q=qkv, T=T, H=H, DH=DH):
        return lib.passl_hip_class_attention_bwd(p(q), p(qkv), p(qkv), p(dout), p(lse), p(dqkv), p(dk), p(dv), B, T, H,
                                                 DH, 0.1, L.BF16, None)

    for f in (th_fwd, th_bwd, cls_fwd, cls_bwd):
        assert f(DH=40) == L.EUNSUPPORTED and f(T=209) == L.EUNSUPPORTED and f(H=9) == L.EUNSUPPORTED, f.__name__
        assert f(q=skew) == L.EINVAL and f(T=0) == L.EINVAL, f.__name__
    assert th_bwd(ws_floats=ops.talking_heads_attention_ws_floats(B, T, H) - 1) == L.EINVAL
    assert lib.passl_hip_talking_heads_attention_fwd(None, *m, p(out), p(lse), B, T, H, DH, 0.1, L.BF16, None) == L.EINVAL
    assert lib.passl_hip_cait_pos_add(p(qkv), p(mixb), p(out), 1, 2, 12, L.BF16, None) == L.EINVAL       # C % 8
    assert lib.passl_hip_cait_cls_concat(p(skew), 1, p(qkv), p(out), 1, 2, 16, L.BF16, None) == L.EINVAL
    assert lib.passl_hip_cait_cls_split(p(dout), None, p(dk), None, 1, 2, 16, L.BF16, None) == L.EINVAL
    torch.cuda.synchronize()
    for g in outs:
        assert g.intact() and g.unwritten() == g.view.numel(), 'a refused call wrote to an output'


def test_token_plumbing_moves_what_it_says():
    B, Ln, Cw = 3, 5, 16
    gen = torch.Generator().manual_seed(3)
    for dtype in (torch.float32, torch.bfloat16):
        x = A.bf16_round(torch.randn(B * Ln, Cw, generator=gen)).cuda().to(dtype)
        pos = torch.randn(Ln, Cw, generator=gen).cuda()
        c = A.bf16_round(torch.randn(B, Cw, generator=gen)).cuda().to(dtype)
        y = ops.cait_pos_add(x, pos, B, Ln)
        assert torch.equal(y, (x.float().view(B, Ln, Cw) + pos).to(dtype).view(B * Ln, Cw))
        u = ops.cait_cls_concat(c, x, B, Ln)
        assert torch.equal(u.view(B, Ln + 1, Cw), torch.cat([c.view(B, 1, Cw), x.view(B, Ln, Cw)], 1))
        u1 = ops.cait_cls_concat(c[:1].contiguous(), x, B, Ln)
        assert torch.equal(u1.view(B, Ln + 1, Cw)[:, 0], c[:1].expand(B, Cw))
        dc, dx = ops.cait_cls_split(u, None, B, Ln)
        assert torch.equal(dc, c) and torch.equal(dx, x)
        dc, dx = ops.cait_cls_split(u, y, B, Ln)
        assert torch.equal(dx, (x.float() + y.float()).to(dtype))


def test_autograd_front_ends():
    from passl_amd.hip import nn as hnn
    case = (2, 17, 3)
    B, T, H = case
    d, ref, eager, _m = case_refs((case, 'plain', 1.0), lambda: C.make_case(case, 'plain', 1.0), C.reference)
    qkv = d['qkv'].reshape(B * T, 3 * H * C.DH).cuda().requires_grad_()
    mix = [d[n].cuda().requires_grad_() for n in ('wl', 'bl', 'ww', 'bw')]
    out = hnn.talking_heads_attention(qkv, *mix, B, T, H, C.DH, d['scale'])
    out.backward(d['dout'].reshape(B * T, H * C.DH).cuda())
    for t, n in zip(mix, ('dwl', 'dbl', 'dww', 'dbw')):
        e = A.scaled_error(eager[n], ref[n], ref['b_' + n])[0]
        assert A.limit_usage(t.grad.cpu(), ref[n], ref['b_' + n], max(4 * e, C.FP32_FLOOR))[0] <= 1, n
    assert qkv.grad.shape == qkv.shape and bool(torch.isfinite(qkv.grad).all())
    ccase = (2, 17, 3)
    dc, cref, _e, _m = case_refs(('cls', ccase, 'plain'), lambda: C.make_cls_case(ccase, 'plain'), C.cls_reference)
    q = dc['q'].reshape(B, H * C.DH).cuda().requires_grad_()
    k = dc['k'].reshape(B * T, H * C.DH).cuda().requires_grad_()
    v = dc['v'].reshape(B * T, H * C.DH).cuda().requires_grad_()
    o = hnn.class_attention(q, k, v, B, T, H, C.DH, dc['scale'])
    o.backward(dc['dout'].reshape(B, H * C.DH).cuda())
    assert float((k.grad.cpu().view(B, T, H, C.DH) - cref['dk']).abs().max()) <= 1e-4 * float(cref['b_dk'].max())
    assert float((q.grad.cpu().view(B, H, C.DH) - cref['dq']).abs().max()) <= 1e-4 * float(cref['b_dq'].max())
