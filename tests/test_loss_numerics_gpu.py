"""The loss kernels (csrc/clas.hip, mixup.hip, clip.hip, head.hip, ntxent.hip) against float64 references, element by
element, over the case tables of loss_util.py (which has the derivation of every bound).

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must survive;
outputs (workspaces included) start as NaN and every element must have been written; every input must come back
bit-identical; a second run of every launch must give the same bits.  A backward launch is handed the forward
launch's own outputs.

Worst error on an MI355X in units of the element's own bound, over all cases (a record of one run, not a pass
criterion):
  kernel             tensor     worst   case
  softmax_ce_fwd     lse        0.397   4x65-offset
  softmax_ce_fwd     terms      0.199   4x65-offset
  softmax_ce_fwd     loss       0.108   3x5-offset
  softmax_ce_bwd     ds         1.000   5x64-peaked (0.9997: see below)
  sigmoid_ce_fwd     terms      0.102   3x5-offset
  sigmoid_ce_fwd     loss       0.083   3x5-offset
  sigmoid_ce_bwd     ds         0.309   33x1001-far_label
  soft_ce            lse        0.401   8x16-offset-mixup
  soft_ce            tsum       0.114   8x16-peaked-random
  soft_ce            terms      0.076   8x16-far_label-mixup
  soft_ce            loss       0.019   8x16-far_label-random
  soft_ce            ds         0.400   8x16-offset-mixup
  l2norm_fwd         y          0.071   4x65-collapsed
  l2norm_fwd         norm       0.027   3x63-collapsed
  l2norm_bwd fp32    dx         0.443   4x65-collapsed
  l2norm_bwd bf16    dx         0.991   6x2048-plain (the store rounding, which u |value| is there for)
  cosine_loss_fwd    stats      0.015   4x65-collapsed
  cosine_loss_fwd    loss       0.003   3x63-collapsed
  cosine_loss_bwd    da         0.443   6x2048-collapsed
  infonce_fwd        lse        0.028   17x128-collapsed
  infonce_fwd        logits     0.043   64x8320-plain
  infonce_fwd        loss       0.013   17x128-collapsed
  infonce_bwd        dq         0.019   17x128-collapsed, gscale given
  clip_logits_fwd    ws         0.233   257x16-duplicate
  clip_logits_fwd    logits     0.108   65x16-cold
  clip_logits_fwd    scale      exact
  clip_ce_fwd        lse        0.062   65x16-cold
  clip_ce_fwd        terms      0.048   65x16-cold
  clip_ce_fwd        out        0.011   65x16-cold
  clip_ce_bwd        dlogits    0.223   65x16-plain
  clip_logits_bwd    dimg       0.167   3x512-unnormalised
  clip_logits_bwd    dtxt       0.237   3x512-unnormalised
  clip_logits_bwd    dscale     0.053   3x512-unnormalised
  ntxent_fwd         rowstats   0.028   70-70-0-unnormalised-w0
  ntxent_fwd         loss       0.007   15-15-0-collapsed-w0
  ntxent_bwd         da         0.019   17-17-0-plain-w0
  ntxent_bwd         db         0.068   2-2-0-cold-w0, gscale given
  ntxent_bwd         dA         0.092   17-70-34-cold-w0, gscale given
  ntxent_bwd         dB         0.067   17-70-34-cold-w0
Every accuracy (242 figures) lay in its interval; the NT-Xent rank count of an ambiguous row used its whole interval
(collapsed: every count is ambiguous).  The loss terms at the common offset of -1e4 (kind `offset`), which cancel:
softmax 0.199 of the bound (4x65), sigmoid 0.102 (3x5), soft-target 0.055 (8x16, random).  softmax_ce_bwd on `peaked`
rows: 0.81 - 0.9997 in every shape but 1x1, all of it the TINY term: a probability just below 2^-126 is stored as 0
(__expf flushes denormal results), an error of the whole probability against a bound of 2^-126 |k|.  The figures of
the fused kernels are small because their bounds are dominated by the dot-product allowance dx = (D + 3) e
sum |a_d b_d| / T, which the MFMA accumulation stays far inside.  No kernel needed a change to meet its bounds.
The file's 248 tests take 4 s.
"""
import pytest
import torch

import loss_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64


def gin(t, dtype=F32, skew=0):
    return Guarded(t.numel(), dtype, skew=skew, fill=t)


def gscalar(v):
    return gin(torch.tensor([v], dtype=F32))


def sync(what):
    """A device fault ends the whole session: nothing more is launched on a GPU that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit('%s: the device reported %s' % (what, err), returncode=3)


def run(what, fn, ins, outs, written=None, unchecked=()):
    """Launches fn() twice on the guarded operands.  Asserts: the same output bits both times, every guard intact,
    every input unchanged, every output element written (`written`: only that many leading elements of an output;
    `unchecked`: outputs that may hold NaN by contract)."""
    before = {n: g.raw() for n, g in ins.items()}
    fn()
    sync(what)
    first = {n: g.raw() for n, g in outs.items()}
    for g in outs.values():
        g.reset()
    fn()
    sync(what)
    for n, g in outs.items():
        assert torch.equal(g.raw(), first[n]), '%s: %s differs between two runs of the same launch' % (what, n)
    for n, g in list(ins.items()) + list(outs.items()):
        assert g.intact(), '%s: a guard region of %s was written' % (what, n)
    for n, g in ins.items():
        assert torch.equal(g.raw(), before[n]), '%s: the input %s was modified' % (what, n)
    for n, g in outs.items():
        if n not in unchecked:
            left = g.unwritten((written or {}).get(n))
            assert left == 0, '%s: %d elements of %s were not written' % (what, left, n)


def cpu(g, n=None):
    v = g.view.float().cpu()
    return v if n is None else v[:n]


def check(kernel, what, ref, got):
    """Every tensor of `got` against ref[name] = (float64 reference, bound), or an accuracy against its interval."""
    failures = []
    for name, value in got.items():
        r = ref[name]
        if name.startswith('acc'):
            print('FIG %s %s %s %.4f in [%.4f, %.4f]' % (kernel, name, what, float(value), r[0], r[1]))
            if not U.acc_ok(value, r):
                failures.append('%s %s: %s = %.4f outside [%.4f, %.4f]' % (kernel, what, name, float(value), r[0], r[1]))
            continue
        ratio, idx = U.usage(value.reshape(r[0].shape), r[0], r[1])
        print('FIG %s %s %s %.4f of the bound' % (kernel, name, what, ratio))
        msg = U.verdict('%s %s' % (kernel, what), name, ratio, idx)
        if msg:
            failures.append(msg)
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------ dense-row CE
def softmax_fwd(what, s, labels, unchecked=()):
    N, C = s.shape
    lib = L.load()
    ins = {'s': gin(s), 'labels': gin(labels, I64)}
    outs = {'lse': Guarded(N, F32), 'out': Guarded(3, F32), 'ws': Guarded(3 * N, F32)}
    run(what + ' softmax_ce_fwd', lambda: L.check(lib.passl_hip_softmax_ce_fwd(
        L.ptr(ins['s'].view), L.ptr(ins['labels'].view), N, C, L.ptr(outs['lse'].view), L.ptr(outs['out'].view),
        L.ptr(outs['ws'].view), 3 * N, L.stream()), 'softmax_ce_fwd'), ins, outs, unchecked=unchecked)
    return ins, outs


def sigmoid_fwd(what, s, labels, unchecked=()):
    N, C = s.shape
    lib = L.load()
    ins = {'s': gin(s), 'labels': gin(labels, I64)}
    outs = {'out': Guarded(1, F32), 'ws': Guarded(N, F32)}
    run(what + ' sigmoid_ce_fwd', lambda: L.check(lib.passl_hip_sigmoid_ce_fwd(
        L.ptr(ins['s'].view), L.ptr(ins['labels'].view), N, C, U.T_ON, U.T_OFF, L.ptr(outs['out'].view),
        L.ptr(outs['ws'].view), N, L.stream()), 'sigmoid_ce_fwd'), ins, outs, unchecked=unchecked)
    return ins, outs


@pytest.mark.parametrize('case', U.CE_CASES, ids=[U.ce_id(c) for c in U.CE_CASES])
def test_softmax_ce(case):
    (N, C), kind = case
    d, ref, what = U.ce_data(case), U.softmax_ref(case), U.ce_id(case)
    lib = L.load()
    ins, outs = softmax_fwd(what, d['s'], d['labels'])
    out, ws = cpu(outs['out']), cpu(outs['ws'])
    check('softmax_ce_fwd', what, ref, dict(lse=cpu(outs['lse']), terms=ws[:N], loss=out[0], acc1=out[1], acc5=out[2]))
    ins.update(lse=outs['lse'], gloss=gscalar(U.GLOSS))
    ds = Guarded(N * C, F32)
    run(what + ' softmax_ce_bwd', lambda: L.check(lib.passl_hip_softmax_ce_bwd(
        L.ptr(ins['s'].view), L.ptr(ins['lse'].view), L.ptr(ins['labels'].view), L.ptr(ins['gloss'].view), N, C,
        L.ptr(ds.view), L.stream()), 'softmax_ce_bwd'), ins, {'ds': ds})
    check('softmax_ce_bwd', what, ref, dict(ds=cpu(ds)))


@pytest.mark.parametrize('case', U.CE_CASES, ids=[U.ce_id(c) for c in U.CE_CASES])
def test_sigmoid_ce(case):
    (N, C), kind = case
    d, ref, what = U.ce_data(case), U.sigmoid_ref(case), U.ce_id(case)
    lib = L.load()
    ins, outs = sigmoid_fwd(what, d['s'], d['labels'])
    check('sigmoid_ce_fwd', what, ref, dict(terms=cpu(outs['ws']), loss=cpu(outs['out'])[0]))
    ins['gloss'] = gscalar(U.GLOSS)
    ds = Guarded(N * C, F32)
    run(what + ' sigmoid_ce_bwd', lambda: L.check(lib.passl_hip_sigmoid_ce_bwd(
        L.ptr(ins['s'].view), L.ptr(ins['labels'].view), L.ptr(ins['gloss'].view), N, C, U.T_ON, U.T_OFF,
        L.ptr(ds.view), L.stream()), 'sigmoid_ce_bwd'), ins, {'ds': ds})
    check('sigmoid_ce_bwd', what, ref, dict(ds=cpu(ds)))


@pytest.mark.parametrize('case', U.BADLABEL_CASES, ids=[U.ce_id(c) for c in U.BADLABEL_CASES])
def test_a_label_outside_the_classes_gives_nan_loss_and_a_correct_lse(case):
    (N, C), kind = case
    d, what = U.ce_data(case), U.ce_id(case) + ' bad label'
    labels = U.bad_labels(case)
    good = torch.arange(N) != 1
    ref = U.softmax_ref(case)
    _, outs = softmax_fwd(what, d['s'], labels, unchecked=('out', 'ws'))
    out, ws, lse = cpu(outs['out']), cpu(outs['ws']), cpu(outs['lse'])
    assert torch.isnan(out[0]) and torch.isnan(ws[1]) and torch.isfinite(out[1:]).all(), (what, out, ws[:N])
    assert torch.isfinite(ws[:N][good]).all() and torch.isfinite(ws[N:]).all() and ws[N + 1] == 0 and ws[2 * N + 1] == 0
    check('softmax_ce_fwd', what, ref, dict(lse=lse))                    # every row, the bad one included
    check('softmax_ce_fwd', what, {'terms': tuple(t[good] for t in ref['terms'])}, dict(terms=ws[:N][good]))
    ref = U.sigmoid_ref(case)
    _, outs = sigmoid_fwd(what, d['s'], labels, unchecked=('out', 'ws'))
    out, ws = cpu(outs['out']), cpu(outs['ws'])
    assert torch.isnan(out[0]) and torch.isnan(ws[1]) and torch.isfinite(ws[good]).all(), (what, out, ws)


def soft_launch(what, case, skews):
    """soft_ce_fwd then soft_ce_bwd; skews: operand name -> elements past a 16-byte boundary.  -> raw bits, values."""
    (N, C), kind, tk = case
    d = U.soft_data(case)
    lib = L.load()
    sk = lambda n: skews.get(n, 0)
    ins = {'s': gin(d['s'], skew=sk('s')), 't': gin(d['t'], skew=sk('t'))}
    outs = {n: Guarded(m, F32, skew=sk(n)) for n, m in (('lse', N), ('tsum', N), ('out', 3), ('ws', 3 * N))}
    run(what + ' soft_ce_fwd', lambda: L.check(lib.passl_hip_soft_ce_fwd(
        L.ptr(ins['s'].view), L.ptr(ins['t'].view), N, C, L.ptr(outs['lse'].view), L.ptr(outs['tsum'].view),
        L.ptr(outs['out'].view), L.ptr(outs['ws'].view), 3 * N, L.stream()), 'soft_ce_fwd'), ins, outs)
    ins.update(lse=outs['lse'], tsum=outs['tsum'], gloss=gscalar(U.GLOSS))
    ds = Guarded(N * C, F32, skew=sk('ds'))
    run(what + ' soft_ce_bwd', lambda: L.check(lib.passl_hip_soft_ce_bwd(
        L.ptr(ins['s'].view), L.ptr(ins['t'].view), L.ptr(ins['lse'].view), L.ptr(ins['tsum'].view),
        L.ptr(ins['gloss'].view), N, C, L.ptr(ds.view), L.stream()), 'soft_ce_bwd'), ins, {'ds': ds})
    outs['ds'] = ds
    out, ws = cpu(outs['out']), cpu(outs['ws'])
    values = dict(lse=cpu(outs['lse']), tsum=cpu(outs['tsum']), terms=ws[:N], loss=out[0], acc1=out[1], acc5=out[2],
                  ds=cpu(ds))
    return {n: g.raw() for n, g in outs.items()}, values


@pytest.mark.parametrize('case', U.SOFT_CASES, ids=[U.ce_id(c) for c in U.SOFT_CASES])
def test_soft_ce(case):
    _, values = soft_launch(U.ce_id(case), case, {})
    check('soft_ce', U.ce_id(case), U.soft_ref(case), values)


def test_soft_ce_off_16_byte_alignment_takes_the_scalar_kernels():
    """C = 1000 with every operand 4 bytes past a 16-byte boundary: the VEC 1 kernels, which must give the bits of a
    VEC 1 run on aligned operands (only the target is off there: that alone selects VEC 1 in both launches), and
    the bounds.  The aligned VEC 4 run of the same case is in test_soft_ce."""
    case = U.SOFT_UNALIGNED
    every = {n: 1 for n in ('s', 't', 'lse', 'tsum', 'out', 'ws', 'ds')}
    bits_off, values = soft_launch('all operands off', case, every)
    check('soft_ce', U.ce_id(case) + ' unaligned', U.soft_ref(case), values)
    bits_ref, _ = soft_launch('target off', case, {'t': 1})
    for n in bits_off:
        assert torch.equal(bits_off[n], bits_ref[n]), 'soft_ce: %s differs between the two VEC 1 runs' % n


# ------------------------------------------------------------------------------------------------ l2norm / cosine
@pytest.mark.parametrize('case', U.ROW_CASES, ids=[U.row_id(c) for c in U.ROW_CASES])
def test_l2norm(case):
    (N, D), kind = case
    d, what = U.row_data(case), U.row_id(case)
    lib = L.load()
    ins = {'x': gin(d['x'])}
    outs = {'y': Guarded(N * D, F32), 'norm': Guarded(N, F32)}
    run(what + ' l2norm_fwd', lambda: L.check(lib.passl_hip_l2norm_fwd(
        L.ptr(ins['x'].view), L.ptr(outs['y'].view), L.ptr(outs['norm'].view), N, D, U.L2_EPS, L.stream()),
        'l2norm_fwd'), ins, outs)
    y, norm = cpu(outs['y']).view(N, D), cpu(outs['norm'])
    check('l2norm_fwd', what, U.l2norm_ref(case), dict(y=y, norm=norm))
    assert norm[N // 2] == U.L2_EPS and not y[N // 2].any()               # the clamped row
    ins = {'dy': gin(d['dy']), 'y': outs['y'], 'norm': outs['norm']}
    for dtype, u, name in ((F32, 0.0, 'fp32'), (BF16, U.U_BF16, 'bf16')):
        dx = Guarded(N * D, dtype)
        run(what + ' l2norm_bwd ' + name, lambda: L.check(lib.passl_hip_l2norm_bwd(
            L.ptr(ins['dy'].view), L.ptr(ins['y'].view), L.ptr(ins['norm'].view), L.ptr(dx.view), N, D, L.dt(dtype),
            L.stream()), 'l2norm_bwd'), ins, {'dx': dx})
        check('l2norm_bwd-' + name, what, {'dx': U.l2norm_bwd_ref(d['dy'], y, norm, u)}, dict(dx=cpu(dx)))


@pytest.mark.parametrize('case', U.ROW_CASES, ids=[U.row_id(c) for c in U.ROW_CASES])
def test_cosine_loss(case):
    (N, D), kind = case
    d, what = U.row_data(case), U.row_id(case)
    lib = L.load()
    ins = {'a': gin(d['x']), 'b': gin(d['b'])}
    outs = {'stats': Guarded(4 * N, F32), 'loss': Guarded(1, F32)}
    run(what + ' cosine_loss_fwd', lambda: L.check(lib.passl_hip_cosine_loss_fwd(
        L.ptr(ins['a'].view), L.ptr(ins['b'].view), N, D, U.COS_EPS, L.ptr(outs['stats'].view),
        L.ptr(outs['loss'].view), L.stream()), 'cosine_loss_fwd'), ins, outs)
    stats = cpu(outs['stats']).view(N, 4)
    check('cosine_loss_fwd', what, U.cosine_ref(case), dict(stats=stats, loss=cpu(outs['loss'])[0]))
    ins.update(stats=outs['stats'], gloss=gscalar(U.GLOSS))
    da = Guarded(N * D, F32)
    run(what + ' cosine_loss_bwd', lambda: L.check(lib.passl_hip_cosine_loss_bwd(
        L.ptr(ins['a'].view), L.ptr(ins['b'].view), L.ptr(ins['stats'].view), L.ptr(ins['gloss'].view), N, D,
        L.ptr(da.view), L.stream()), 'cosine_loss_bwd'), ins, {'da': da})
    check('cosine_loss_bwd', what, {'da': U.cosine_bwd_ref(d['x'], d['b'], stats)}, dict(da=cpu(da)))


# ------------------------------------------------------------------------------------------------ InfoNCE
@pytest.mark.parametrize('case', U.INFONCE_CASES, ids=[U.infonce_id(c) for c in U.INFONCE_CASES])
def test_infonce(case):
    (N, K), kind = case
    d, ref, what = U.infonce_data(case), U.infonce_ref(case), U.infonce_id(case)
    D, T = U.DIM, d['T']
    lib = L.load()
    ins = {'q': gin(d['q']), 'k': gin(d['k']), 'queue': gin(d['queue'])}
    bits = None
    for want_logits in (False, True):
        outs = {'out': Guarded(3, F32), 'lse': Guarded(N, F32),
                'ws': Guarded(lib.passl_hip_infonce_workspace_bytes(N, K) // 4, F32)}
        if want_logits:
            outs['logits'] = Guarded(N * (K + 1), F32)
        run('%s infonce_fwd (logits %d)' % (what, want_logits), lambda: L.check(lib.passl_hip_infonce_fwd(
            L.ptr(ins['q'].view), L.ptr(ins['k'].view), L.ptr(ins['queue'].view), N, D, K, T, L.ptr(outs['out'].view),
            L.ptr(outs['lse'].view), L.ptr(outs['logits'].view) if want_logits else None, L.ptr(outs['ws'].view),
            L.stream()), 'infonce_fwd'), ins, outs)
        now = [outs[n].raw() for n in ('out', 'lse', 'ws')]
        assert bits is None or all(torch.equal(a, b) for a, b in zip(now, bits)), \
            '%s: infonce_fwd gives other bits when it also stores the logits' % what
        bits = now
    out = cpu(outs['out'])
    check('infonce_fwd', what, ref, dict(lse=cpu(outs['lse']), logits=cpu(outs['logits']), loss=out[0], acc1=out[1],
                                         acc5=out[2]))
    ins['lse'] = outs['lse']
    dq64, Bdq = ref['dq']
    for g in (None, U.GLOSS):
        if g is not None:
            ins['gscale'] = gscalar(g)
        bouts = {'dq': Guarded(N * D, F32), 'ws': Guarded(lib.passl_hip_infonce_bwd_workspace_bytes(N, K) // 4, F32)}
        run('%s infonce_bwd (gscale %s)' % (what, g), lambda: L.check(lib.passl_hip_infonce_bwd(
            L.ptr(ins['q'].view), L.ptr(ins['k'].view), L.ptr(ins['queue'].view), L.ptr(ins['lse'].view),
            L.ptr(ins['gscale'].view) if g is not None else None, N, D, K, T, L.ptr(bouts['dq'].view),
            L.ptr(bouts['ws'].view), L.stream()), 'infonce_bwd'), ins, bouts)
        s = 1.0 if g is None else g
        check('infonce_bwd', what + (' gscale' if g else ''), {'dq': (dq64 * s, Bdq * s + U.E * (dq64 * s).abs())},
              dict(dq=cpu(bouts['dq'])))


# ------------------------------------------------------------------------------------------------ CLIP
def clip_fwd(what, B, D, img, txt, scale, unchecked=()):
    lib = L.load()
    ins = {'img': gin(img), 'txt': gin(txt)}
    outs = {'scale': gscalar(scale), 'ws': Guarded(lib.passl_hip_clip_logits_ws_floats(B, D), F32),
            'logits': Guarded(B * B, F32)}
    run(what + ' clip_logits_fwd', lambda: L.check(lib.passl_hip_clip_logits_fwd(
        L.ptr(ins['img'].view), L.ptr(ins['txt'].view), L.ptr(outs['scale'].view), B, D, U.CLIP_LO, U.CLIP_HI,
        L.ptr(outs['ws'].view), L.ptr(outs['logits'].view), L.stream()), 'clip_logits_fwd'), ins, outs,
        written={'ws': 2 * B * D + 2 * B + 1}, unchecked=unchecked)    # the workspace's last 7 floats are padding
    return outs


def test_clip_zero_row_is_nan_in_its_own_row_only():
    """clip_norm_kernel has no epsilon, like the model it follows (features / features.norm()): an all-zero image row
    gives NaN logits in that row, and every other row keeps the bits it has without the zero row."""
    (B, D), kind = case = ((3, 16), 'plain')
    d = U.clip_data(case)
    sound = clip_fwd('3x16 sound', B, D, d['img'], d['txt'], d['scale'])['logits'].view.cpu().view(B, B)
    img = d['img'].clone()
    img[1] = 0
    got = clip_fwd('3x16 zero row', B, D, img, d['txt'], d['scale'], unchecked=('ws', 'logits'))['logits'].view.cpu()
    got = got.view(B, B)
    assert torch.isnan(got[1]).all() and torch.equal(got[[0, 2]].view(torch.int32), sound[[0, 2]].view(torch.int32))


@pytest.mark.parametrize('case', U.CLIP_CASES, ids=[U.infonce_id(c) for c in U.CLIP_CASES])
def test_clip(case):
    (B, D), kind = case
    d, ref, what = U.clip_data(case), U.clip_ref(case), U.infonce_id(case)
    lib = L.load()
    nws = 2 * B * D + 2 * B + 1
    outs = clip_fwd(what, B, D, d['img'], d['txt'], d['scale'])
    gws, glogits = outs['ws'], outs['logits']
    check('clip_logits_fwd', what, ref, dict(ws=cpu(gws, nws), logits=cpu(glogits), scale=cpu(outs['scale'])[0]))
    ins = {'logits': glogits}
    outs = {'lse': Guarded(2 * B, F32), 'out': Guarded(3, F32), 'ws': Guarded(2 * B, F32)}
    run(what + ' clip_ce_fwd', lambda: L.check(lib.passl_hip_clip_ce_fwd(
        L.ptr(glogits.view), B, L.ptr(outs['lse'].view), L.ptr(outs['out'].view), L.ptr(outs['ws'].view), 2 * B,
        L.stream()), 'clip_ce_fwd'), ins, outs)
    check('clip_ce_fwd', what, ref, dict(lse=cpu(outs['lse']), terms=cpu(outs['ws']), out=cpu(outs['out'])))
    ins.update(lse=outs['lse'], gloss=gscalar(U.GLOSS))
    gdl = Guarded(B * B, F32)
    run(what + ' clip_ce_bwd', lambda: L.check(lib.passl_hip_clip_ce_bwd(
        L.ptr(glogits.view), L.ptr(ins['lse'].view), L.ptr(ins['gloss'].view), B, L.ptr(gdl.view), L.stream()),
        'clip_ce_bwd'), ins, {'dlogits': gdl})
    check('clip_ce_bwd', what, ref, dict(dlogits=cpu(gdl)))
    ins = {'dlogits': gdl, 'logits': glogits, 'ws': gws}
    outs = {'dimg': Guarded(B * D, F32), 'dtxt': Guarded(B * D, F32), 'dscale': gscalar(U.DSCALE_FILL),
            'scratch': Guarded(256, F32)}
    run(what + ' clip_logits_bwd', lambda: L.check(lib.passl_hip_clip_logits_bwd(
        L.ptr(gdl.view), L.ptr(glogits.view), L.ptr(gws.view), B, D, L.ptr(outs['dimg'].view), L.ptr(outs['dtxt'].view),
        L.ptr(outs['dscale'].view), L.ptr(outs['scratch'].view), L.stream()), 'clip_logits_bwd'), ins, outs,
        written={'scratch': min(-(-B * B // 256), 256)})
    bref = U.clip_bwd_ref(cpu(gdl), cpu(glogits), cpu(gws), B, D)
    check('clip_logits_bwd', what, bref, dict(dimg=cpu(outs['dimg']), dtxt=cpu(outs['dtxt']),
                                              dscale=cpu(outs['dscale'])[0]))


# ------------------------------------------------------------------------------------------------ NT-Xent + CO2
@pytest.mark.parametrize('case', U.NTX_CASES, ids=[U.ntx_id(c) for c in U.NTX_CASES])
def test_ntxent(case):
    (B, BL, roff), kind, w = case
    d, ref, what = U.ntx_data(case), U.ntx_ref(case), U.ntx_id(case)
    D, T = U.DIM, d['T']
    lib = L.load()
    ins = {n: gin(d[n]) for n in ('a', 'b', 'A', 'Bl')}
    outs = {'out': Guarded(2, F32), 'rowstats': Guarded(8 * B, F32)}
    run(what + ' ntxent_fwd', lambda: L.check(lib.passl_hip_ntxent_fwd(
        L.ptr(ins['a'].view), L.ptr(ins['b'].view), L.ptr(ins['A'].view), L.ptr(ins['Bl'].view), B, BL, roff, D, T, w,
        L.ptr(outs['out'].view), L.ptr(outs['rowstats'].view), L.stream()), 'ntxent_fwd'), ins, outs)
    out, stats = cpu(outs['out']), cpu(outs['rowstats']).view(B, 8)
    check('ntxent_fwd', what, ref, dict(rowstats=stats, cnt=stats[:, 6], loss=out[0], acc1=100.0 * out[1]))
    ins['rowstats'] = outs['rowstats']
    for g in (None, U.GLOSS):
        if g is not None:
            ins['gscale'] = gscalar(g)
        bouts = {'da': Guarded(B * D, F32), 'db': Guarded(B * D, F32), 'dA': Guarded(BL * D, F32),
                 'dB': Guarded(BL * D, F32)}
        run('%s ntxent_bwd (gscale %s)' % (what, g), lambda: L.check(lib.passl_hip_ntxent_bwd(
            L.ptr(ins['a'].view), L.ptr(ins['b'].view), L.ptr(ins['A'].view), L.ptr(ins['Bl'].view),
            L.ptr(ins['rowstats'].view), L.ptr(ins['gscale'].view) if g is not None else None, B, BL, roff, D, T, w,
            L.ptr(bouts['da'].view), L.ptr(bouts['db'].view), L.ptr(bouts['dA'].view), L.ptr(bouts['dB'].view),
            L.stream()), 'ntxent_bwd'), ins, bouts)
        s = 1.0 if g is None else g
        sref = {n: (ref[n][0] * s, ref[n][1] * s + U.E * (ref[n][0] * s).abs()) for n in bouts}
        check('ntxent_bwd', what + (' gscale' if g else ''), sref, {n: cpu(t) for n, t in bouts.items()})
