"""The token, index and layout kernels (csrc/vit.hip, deit_tokens.hip, clip.hip, layout_pool.hip) against the references
and bounds of token_util.py, over its case tables: bit for bit where data is moved, element by element against float64
where fp32 is summed.

The kernels are called through the C ABI.  Every operand is a view between two 4 KiB guard regions that must survive;
pure outputs start as NaN (0xA5 bytes for int32 outputs and the mask) and every element must have been written; every
read-only operand must come back bit-identical; accumulated outputs start from a non-zero fill; every launch runs twice
from the same initial state and must give the same bits; a refused call returns PASSL_EINVAL and leaves every guarded
byte as it was.  A device error after a launch ends the session.  Index operands are always in range; the token ids
of embed_fwd / embed_bwd, which the kernels test in code, are the one exception.

Worst error on an MI355X in units of the element's own bound, over all cases (a record of one run, not a pass
criterion):
  kernel              tensor        worst   case
  mae_mask            ids_keep, ids_restore, mask   exact (the denormal and the -0.0 rows too: nothing is flushed)
  mae_gather          out           exact
  mae_gather_bwd      dx            exact
  mae_gather_bwd      dcls          0.483   1-1-1-8-mask bf16 (one image onto dcls: a single addition, half the bound)
  mae_unshuffle       out           exact
  mae_unshuffle_bwd   dx            exact
  mae_unshuffle_bwd   dmask_token   0.003   3-42-10-32 fp32; bit-identical where nothing is masked (2-49-49-40)
  patchify            out           exact
  prefix_tokens_fwd   out           exact
  prefix_tokens_bwd   dx            exact
  prefix_tokens_bwd   dprefix0      0.486   1-255-2-8 bf16
  prefix_tokens_bwd   dprefix1      0.497   1-255-2-8 bf16 (one image: a single addition)
  mean2               out           exact
  embed_fwd           out           exact (an id of -1, V or 2^40 gives pos alone)
  embed_bwd           dtable        0.479   70-5-2048-3-pad bf16 decades; 0.671 on 40-9-64-50-pad fp32 scattered, where
                                            the one-sided truncation term is most of the bound (token_util.py)
  embed_bwd           dpos          0.484   2-77-512-300-text bf16 scattered
  gather_rows, scatter_rows, eot_index      exact
  nchw_to_nhwc_pad    y             exact (the stem's kernel and, with y off 8 bytes, the generic one: the same values)
  colsum              out           0.107   264-7 fp32
  colsum_acc          out           0.495   264-1 fp32 (one row onto out: a single addition)
  relu_bwd            dx            exact (+0 at y = +0, -0, NaN; dy at the positive denormals)
Every summed tensor (468 comparisons) had the bits of token_util's float32 sum in the kernel's documented order, which
the tests assert next to the bound: at many terms n 2 E sum |terms| alone is wide.  embed_bwd with a single NaN in dout
(3-12-24-7-text, at b = 1, t = 4, c = 13): dpos[4][13] NaN, the rest of dpos at most 0.248 of its bound, the other rows
of dtable at most 0.376; row text[1][4] of dtable came back finite in every column, column 13 holding the sum of its
other addends (0.113 of the bound that sum would have, the NaN counted as 0): the kernel's comment says so now.  acc
and touched were zero after every call; the 16 bytes behind them keep the launch's amax, which every call clears first.
No kernel needed a change; the four mae_gather / mae_unshuffle entries gained the 16-byte alignment refusals that their
neighbours had, and nothing in the existing suite passes them an operand that is refused.

Grid-stride loops exercised only by the cases sized for them (token_util.py says so at each): mae_gather_kernel,
mae_gather_bwd_kernel, mae_unshuffle_kernel and patchify_kernel (vit.hip caps a grid at 4096 x 256 threads, passed at
8.4 M elements, 1 M for patchify), relu_bwd_kernel (the same cap in layout_pool.hip).  Not exercised, because a grid
only reaches its cap at sizes no test should have: the loops of embed_fwd_kernel, embed_absmax_kernel,
gather_rows_kernel and scatter_rows_kernel (clip.hip caps at 262140 x 256 threads: 537 M elements); nor the loop of the
generic nchw_to_nhwc_pad_kernel (more than 1 M output pixels), whose cases keep one small image size.
The file's 324 tests take 7 s.
"""
import numpy as np
import pytest
import torch

import token_util as U
from guarded import Guarded
from test_flat_numerics_gpu import gin, refused, run, sync            # the rules of that file, shared

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

F32, BF16, I64, I32, U8 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8
LP = pytest.mark.parametrize('lp', U.LPS, ids=('fp32', 'bf16'))


def DT(lp):
    return BF16 if lp else F32


def P(g):
    return L.ptr(g.view) if g is not None else None


def gbits(g, lp):
    """The payload's bits: uint16 of a bf16 operand, uint32 of an fp32 one."""
    if lp:
        return g.view.view(torch.int16).cpu().numpy().view(np.uint16)
    return g.view.view(torch.int32).cpu().numpy().view(np.uint32)


def exact(what, got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert not len(bad), '%s: %d of %d elements differ, first at %s' % (what, len(bad), len(want), bad[:8])


def bounded(kernel, what, ref, got, twin=None):
    """Every tensor of `got` against ref[name] = (float64 reference, bound).  `twin`: the float32 sum in the kernel's
    documented order (a fixed order, or integer atomics, is what each of these kernels documents): the same bits."""
    failures = []
    for name, g in got.items():
        value = g.view.float().cpu().numpy()
        ratio, idx = U.usage(value, *ref[name])
        print('FIG %s %s %s %.4f of the bound' % (kernel, name, what, ratio))
        if twin is not None:
            diff = np.nonzero(U.bits(value) != U.bits(twin[name]).ravel())[0]
            if len(diff):
                failures.append('%s %s: %s is not the sum in the documented order at %s' % (kernel, what, name, diff[:8]))
        msg = U.verdict('%s %s' % (kernel, what), name, ratio, idx)
        if msg:
            failures.append(msg)
    assert not failures, '\n'.join(failures)


def call(name, fn):
    return lambda: L.check(fn(), name)


# ------------------------------------------------------------------------------------------------ mae_mask
@pytest.mark.parametrize('case', U.MASK_CASES, ids=U.case_id)
def test_mae_mask(case):
    Ln, lib = case[0], L.load()
    noise = U.mask_data(case)
    ins = {'noise': gin(noise)}
    for K in U.mask_keeps(Ln):
        what = 'mae_mask %s K=%d' % (U.case_id(case), K)
        outs = {'ids_keep': Guarded(U.MASK_B * K, I32), 'ids_restore': Guarded(U.MASK_B * Ln, I32),
                'mask': Guarded(U.MASK_B * Ln, F32, prefill='a5')}
        run(what, call('mae_mask', lambda: lib.passl_hip_mae_mask(
            P(ins['noise']), U.MASK_B, Ln, K, P(outs['ids_keep']), P(outs['ids_restore']), P(outs['mask']), L.stream())),
            ins, outs)
        want = U.mask_expect(noise, K)
        exact(what + ' ids_keep', outs['ids_keep'].view.cpu().numpy(), want['ids_keep'])
        exact(what + ' ids_restore', outs['ids_restore'].view.cpu().numpy(), want['ids_restore'])
        exact(what + ' mask', gbits(outs['mask'], False), U.bits(want['mask']))


def test_mae_mask_refusals():
    lib = L.load()
    g = {'noise': gin(np.zeros(3 * 4097, np.float32)), 'ids_keep': Guarded(3 * 64, I32),
         'ids_restore': Guarded(3 * 4097, I32), 'mask': Guarded(3 * 4097, F32, prefill='a5')}
    for Ln, K in U.MASK_REFUSED:
        refused('mae_mask L=%d K=%d' % (Ln, K), lambda: lib.passl_hip_mae_mask(
            P(g['noise']), 3, Ln, K, P(g['ids_keep']), P(g['ids_restore']), P(g['mask']), L.stream()), g)


# ------------------------------------------------------------------------------------------------ mae_gather(_bwd)
def gather_operands(case, lp, skew=()):
    B, Ln, K, D, _ = case
    d = U.gather_data(case, lp)
    s = lambda n: 1 if n in skew else 0
    ins = {'x': gin(d['x'], DT(lp), s('x')), 'cls': gin(d['cls'], F32, s('cls')), 'pos': gin(d['pos'], F32, s('pos')),
           'ids_keep': gin(d['ids_keep'], I32), 'dout': gin(d['dout'], DT(lp), s('dout')),
           'ids_restore': gin(d['ids_restore'], I32)}
    outs = {'out': Guarded(B * (K + 1) * D, DT(lp), s('out')), 'dx': Guarded(B * Ln * D, DT(lp), s('dx')),
            'dcls': gin(d['dcls'])}
    return ins, outs


def gather_calls(case, lp, ins, outs):
    B, Ln, K, D, _ = case
    lib = L.load()
    fwd = lambda: lib.passl_hip_mae_gather(P(ins['x']), P(ins['cls']), P(ins['pos']), P(ins['ids_keep']), P(outs['out']),
                                           B, Ln, K, D, L.dt(DT(lp)), L.stream())
    bwd = lambda: lib.passl_hip_mae_gather_bwd(P(ins['dout']), P(ins['ids_restore']), P(outs['dx']), P(outs['dcls']),
                                               B, Ln, K, D, L.dt(DT(lp)), L.stream())
    return fwd, bwd


@LP
@pytest.mark.parametrize('case', U.GATHER_CASES, ids=U.case_id)
def test_mae_gather_and_its_backward(case, lp):
    what = '%s %s' % (U.case_id(case), 'bf16' if lp else 'fp32')
    ins, outs = gather_operands(case, lp)
    fwd, bwd = gather_calls(case, lp, ins, outs)
    run('mae_gather ' + what, call('mae_gather', fwd), ins, {'out': outs['out']})
    run('mae_gather_bwd ' + what, call('mae_gather_bwd', bwd), ins, {'dx': outs['dx'], 'dcls': outs['dcls']})
    want = U.gather_expect(case, lp)
    exact('mae_gather out ' + what, gbits(outs['out'], lp), U.wbits(want['out'], lp))
    exact('mae_gather_bwd dx ' + what, gbits(outs['dx'], lp), U.wbits(want['dx'], lp))
    bounded('mae_gather_bwd', what, U.gather_ref(case, lp), {'dcls': outs['dcls']}, U.gather_eval32(case, lp))


@LP
def test_mae_gather_refuses_operands_off_16_bytes(lp):
    case = (3, 5, 2, 8, 'mask')
    for name in ('x', 'cls', 'pos', 'out', 'dout', 'dx'):
        ins, outs = gather_operands(case, lp, skew=(name,))
        fwd, bwd = gather_calls(case, lp, ins, outs)
        refused('mae_gather%s %s off' % ('' if name in ('x', 'cls', 'pos', 'out') else '_bwd', name),
                fwd if name in ('x', 'cls', 'pos', 'out') else bwd, dict(ins, **outs))


# ------------------------------------------------------------------------------------------------ mae_unshuffle(_bwd)
def unshuffle_operands(case, lp, skew=()):
    B, Ln, K, D = case
    d = U.unshuffle_data(case, lp)
    s = lambda n: 1 if n in skew else 0
    ins = {'x': gin(d['x'], DT(lp), s('x')), 'mask_token': gin(d['mask_token'], F32, s('mask_token')),
           'pos': gin(d['pos'], F32, s('pos')), 'ids_keep': gin(d['ids_keep'], I32),
           'ids_restore': gin(d['ids_restore'], I32), 'dout': gin(d['dout'], DT(lp), s('dout'))}
    outs = {'out': Guarded(B * (Ln + 1) * D, DT(lp), s('out')), 'dx': Guarded(B * (K + 1) * D, DT(lp), s('dx')),
            'dmask_token': gin(d['dmask_token'], F32, s('dmask_token')), 'ws': Guarded(U.UNSHUFFLE_WS * D, F32, s('ws'))}
    return ins, outs


def unshuffle_calls(case, lp, ins, outs, ws_floats=None):
    B, Ln, K, D = case
    lib = L.load()
    fwd = lambda: lib.passl_hip_mae_unshuffle(P(ins['x']), P(ins['mask_token']), P(ins['pos']), P(ins['ids_restore']),
                                              P(outs['out']), B, Ln, K, D, L.dt(DT(lp)), L.stream())
    bwd = lambda: lib.passl_hip_mae_unshuffle_bwd(
        P(ins['dout']), P(ins['ids_keep']), P(ins['ids_restore']), P(outs['dx']), P(outs['dmask_token']), B, Ln, K, D,
        L.dt(DT(lp)), P(outs['ws']), U.UNSHUFFLE_WS * D if ws_floats is None else ws_floats, L.stream())
    return fwd, bwd


@LP
@pytest.mark.parametrize('case', U.UNSHUFFLE_CASES, ids=U.case_id)
def test_mae_unshuffle_and_its_backward(case, lp):
    what = '%s %s' % (U.case_id(case), 'bf16' if lp else 'fp32')
    ins, outs = unshuffle_operands(case, lp)
    fwd, bwd = unshuffle_calls(case, lp, ins, outs)
    run('mae_unshuffle ' + what, call('mae_unshuffle', fwd), ins, {'out': outs['out']})
    run('mae_unshuffle_bwd ' + what, call('mae_unshuffle_bwd', bwd), ins,
        {n: outs[n] for n in ('dx', 'dmask_token', 'ws')}, unchecked=('ws',))
    want = U.unshuffle_expect(case, lp)
    exact('mae_unshuffle out ' + what, gbits(outs['out'], lp), U.wbits(want['out'], lp))
    exact('mae_unshuffle_bwd dx ' + what, gbits(outs['dx'], lp), U.wbits(want['dx'], lp))
    bounded('mae_unshuffle_bwd', what, U.unshuffle_ref(case, lp), {'dmask_token': outs['dmask_token']},
            U.unshuffle_eval32(case, lp))
    if case[1] == case[2]:                                         # nothing is masked
        exact('dmask_token ' + what, gbits(outs['dmask_token'], False), U.bits(U.unshuffle_data(case, lp)['dmask_token']))
    slabs = U.unshuffle_slabs(case[0], case[1])[0]
    assert outs['ws'].unwritten() == (U.UNSHUFFLE_WS - slabs) * case[3], what + ': the slabs in use'
    refused(what + ' ws one float short', unshuffle_calls(case, lp, ins, outs, slabs * case[3] - 1)[1], dict(ins, **outs))


@LP
def test_mae_unshuffle_refuses_operands_off_16_bytes(lp):
    case = (3, 42, 10, 32)
    forward = ('x', 'mask_token', 'pos', 'out')
    for name in forward + ('dout', 'dx', 'dmask_token', 'ws'):
        ins, outs = unshuffle_operands(case, lp, skew=(name,))
        fwd, bwd = unshuffle_calls(case, lp, ins, outs)
        refused('mae_unshuffle%s %s off' % ('' if name in forward else '_bwd', name), fwd if name in forward else bwd,
                dict(ins, **outs))


# ------------------------------------------------------------------------------------------------ patchify
@LP
@pytest.mark.parametrize('which', U.PATCHIFY_INPUTS)
@pytest.mark.parametrize('case', U.PATCHIFY_CASES + (U.PATCHIFY_LOOP,), ids=U.case_id)
def test_patchify(case, which, lp):
    B, C, H, W, p = case
    if case == U.PATCHIFY_LOOP and which == 'coded':
        return
    lib, img = L.load(), U.patchify_data(case, which)
    ins, out = {'img': gin(img)}, Guarded(img.size, DT(lp))
    what = 'patchify %s %s %s' % (U.case_id(case), which, lp)
    run(what, call('patchify', lambda: lib.passl_hip_patchify(P(ins['img']), P(out), B, C, H, W, p, L.dt(DT(lp)),
                                                              L.stream())), ins, {'out': out})
    exact(what, gbits(out, lp), U.wbits(U.patchify_expect(img, p), lp))


def test_patchify_refuses_an_image_that_is_no_multiple_of_the_patch():
    B, C, H, W, p = U.PATCHIFY_REFUSED
    lib = L.load()
    g = {'img': gin(np.ones(B * C * H * W, np.float32)), 'out': Guarded(B * C * H * W, F32)}
    refused('patchify H % p', lambda: lib.passl_hip_patchify(P(g['img']), P(g['out']), B, C, H, W, p, L.dt(F32),
                                                             L.stream()), g)


# ------------------------------------------------------------------------------------------------ prefix tokens, mean2
def prefix_operands(case, lp, skew=()):
    B, Ln, NP, C = case
    d = U.prefix_data(case, lp)
    s = lambda n: 1 if n in skew else 0
    ins = {'x': gin(d['x'], DT(lp), s('x')), 'prefix0': gin(d['prefix'][0], F32, s('prefix0')),
           'prefix1': gin(d['prefix'][1], F32, s('prefix1')), 'pos': gin(d['pos'], F32, s('pos')),
           'dout': gin(d['dout'], DT(lp), s('dout'))}
    outs = {'out': Guarded(B * (Ln + NP) * C, DT(lp), s('out')), 'dx': Guarded(B * Ln * C, DT(lp), s('dx')),
            'dprefix0': gin(d['dprefix'][0], F32, s('dprefix0')), 'dprefix1': gin(d['dprefix'][1], F32, s('dprefix1'))}
    return ins, outs


def prefix_calls(case, lp, ins, outs):
    B, Ln, NP, C = case
    lib = L.load()
    two = NP != 1
    fwd = lambda: lib.passl_hip_prefix_tokens_fwd(P(ins['x']), P(ins['prefix0']), P(ins['prefix1']) if two else None,
                                                  P(ins['pos']), P(outs['out']), B, Ln, NP, C, L.dt(DT(lp)), L.stream())
    bwd = lambda: lib.passl_hip_prefix_tokens_bwd(P(ins['dout']), P(outs['dx']), P(outs['dprefix0']),
                                                  P(outs['dprefix1']) if two else None, B, Ln, NP, C, L.dt(DT(lp)),
                                                  L.stream())
    return fwd, bwd


@LP
@pytest.mark.parametrize('case', U.PREFIX_CASES, ids=U.case_id)
def test_prefix_tokens_and_their_backward(case, lp):
    what = '%s %s' % (U.case_id(case), 'bf16' if lp else 'fp32')
    NP = case[2]
    ins, outs = prefix_operands(case, lp)
    fwd, bwd = prefix_calls(case, lp, ins, outs)
    run('prefix_tokens_fwd ' + what, call('prefix_tokens_fwd', fwd), ins, {'out': outs['out']})
    summed = {'dprefix%d' % t: outs['dprefix%d' % t] for t in range(NP)}
    ins_b = dict(ins, **{'dprefix%d' % t: outs['dprefix%d' % t] for t in range(NP, 2)})      # unused: unchanged
    run('prefix_tokens_bwd ' + what, call('prefix_tokens_bwd', bwd), ins_b, dict(summed, dx=outs['dx']))
    want = U.prefix_expect(case, lp)
    exact('prefix_tokens_fwd out ' + what, gbits(outs['out'], lp), U.wbits(want['out'], lp))
    exact('prefix_tokens_bwd dx ' + what, gbits(outs['dx'], lp), U.wbits(want['dx'], lp))
    bounded('prefix_tokens_bwd', what, U.prefix_ref(case, lp), summed, U.prefix_eval32(case, lp))


@LP
def test_prefix_tokens_refusals(lp):
    case = (3, 5, 2, 8)
    ins, outs = prefix_operands(case, lp)
    everything = dict(ins, **outs)
    for what, bad in (('NP = 3', (3, 5, 3, 8)), ('C = 12', (3, 5, 2, 12))):
        for fn in prefix_calls(bad, lp, ins, outs):
            refused('prefix_tokens ' + what, fn, everything)
    forward = ('x', 'prefix0', 'prefix1', 'pos', 'out')
    for name in forward + ('dout', 'dx', 'dprefix0', 'dprefix1'):
        ins, outs = prefix_operands(case, lp, skew=(name,))
        fwd, bwd = prefix_calls(case, lp, ins, outs)
        refused('prefix_tokens %s off' % name, fwd if name in forward else bwd, dict(ins, **outs))


@pytest.mark.parametrize('n', U.MEAN2_N)
def test_mean2(n):
    lib = L.load()
    a, b = U.mean2_data(n)
    ins, out = {'a': gin(a), 'b': gin(b)}, Guarded(n, F32)
    run('mean2 %d' % n, call('mean2', lambda: lib.passl_hip_mean2(P(ins['a']), P(ins['b']), P(out), n, L.stream())),
        ins, {'out': out})
    exact('mean2 %d' % n, gbits(out, False), U.bits(U.mean2_eval32(a, b)))
    out.reset()
    run('mean2 %d b = NULL' % n, call('mean2', lambda: lib.passl_hip_mean2(P(ins['a']), None, P(out), n, L.stream())),
        ins, {'out': out})
    exact('mean2 %d b = NULL' % n, gbits(out, False), U.bits(U.mean2_eval32(a)))


# ------------------------------------------------------------------------------------------------ embed_fwd / embed_bwd
def embed_bwd_operands(case, dkind, lp, nan_at=None):
    B, Tn, C, V, _ = case
    lib, d = L.load(), U.embed_data(case, dkind, lp, nan_at)
    acc_bytes, ws_floats = lib.passl_hip_embed_bwd_acc_bytes(V, C), lib.passl_hip_embed_bwd_ws_floats(B, Tn, C)
    assert ws_floats == U.embed_bwd_slabs(B, C)[0] * Tn * C
    ins = {'text': gin(d['text'], I64), 'dout': gin(d['dout'], DT(lp))}
    outs = {'dtable': gin(d['dtable']), 'dpos': gin(d['dpos']), 'ws': Guarded(ws_floats, F32),
            'acc': gin(np.zeros(acc_bytes, np.uint8), U8)}          # the persistent workspace: zero before, zero after
    fn = lambda: lib.passl_hip_embed_bwd(P(ins['text']), P(ins['dout']), P(outs['dtable']), P(outs['dpos']), B, Tn, C, V,
                                         L.dt(DT(lp)), P(outs['acc']), acc_bytes, P(outs['ws']), ws_floats, L.stream())
    return d, ins, outs, fn


def workspace_is_zero(acc):
    """int64 acc[V][C] and int32 touched[V] with its padding: all but the last 16 bytes, which hold the launch's own
    amax (cleared by the entry at the start of every call, not part of the contract)."""
    return not bool(acc.view[:-16].any())


@LP
@pytest.mark.parametrize('case', U.EMBED_CASES, ids=U.case_id)
def test_embed_fwd_and_bwd(case, lp):
    B, Tn, C, V, _ = case
    lib, name = L.load(), '%s %s' % (U.case_id(case), 'bf16' if lp else 'fp32')
    d = U.embed_data(case, 'normal', lp)
    ins, out = {'text': gin(d['text'], I64), 'table': gin(d['table']), 'pos': gin(d['pos'])}, Guarded(B * Tn * C, DT(lp))
    run('embed_fwd ' + name, call('embed_fwd', lambda: lib.passl_hip_embed_fwd(
        P(ins['text']), P(ins['table']), P(ins['pos']), P(out), B, Tn, C, V, L.dt(DT(lp)), L.stream())), ins, {'out': out})
    exact('embed_fwd ' + name, gbits(out, lp), U.wbits(U.embed_eval32(case, 'normal', lp)['out'], lp))
    for dkind in U.EMBED_DOUTS:
        what = '%s %s' % (name, dkind)
        d, ins, outs, fn = embed_bwd_operands(case, dkind, lp)
        run('embed_bwd ' + what, call('embed_bwd', fn), ins, outs, unchecked=('ws',))
        assert workspace_is_zero(outs['acc']), what + ': acc / touched are not zero after the call'
        bounded('embed_bwd', what, U.embed_ref(case, dkind, lp), {'dtable': outs['dtable'], 'dpos': outs['dpos']},
                U.embed_eval32(case, dkind, lp))
        if dkind == 'zero':
            exact(what + ' dtable', gbits(outs['dtable'], False), U.bits(d['dtable']))
            exact(what + ' dpos', gbits(outs['dpos'], False), U.bits(d['dpos']))


@LP
def test_embed_bwd_with_one_nan_in_dout(lp):
    """dpos[t, c] is NaN, every other element of dpos and every other row of dtable is within its bound, the workspace
    comes back zero.  Nothing is asserted about row text[b, t] of dtable: what it holds is printed."""
    case, at = U.EMBED_NAN
    b, t, c = at
    d, ins, outs, fn = embed_bwd_operands(case, 'normal', lp, at)
    run('embed_bwd one NaN', call('embed_bwd', fn), ins, outs, unchecked=('ws', 'dpos', 'dtable'))
    assert workspace_is_zero(outs['acc']), 'acc / touched are not zero after the call'
    ref = U.embed_ref(case, 'normal', lp, at)
    dpos, dtable = (outs[n].view.cpu().numpy().reshape(ref[n][0].shape) for n in ('dpos', 'dtable'))
    assert np.isnan(dpos[t, c])
    keep = np.ones(dpos.shape, bool)
    keep[t, c] = False
    ratio = U.usage(dpos[keep], ref['dpos'][0][keep], ref['dpos'][1][keep])[0]
    print('FIG embed_bwd dpos one-NaN %.4f of the bound' % ratio)
    assert ratio <= 1
    tok = int(d['text'][b, t])
    rows = np.arange(case[3]) != tok
    ratio = U.usage(dtable[rows], ref['dtable'][0][rows], ref['dtable'][1][rows])[0]
    print('FIG embed_bwd dtable one-NaN %.4f of the bound' % ratio)
    assert ratio <= 1
    err = np.abs(dtable[tok] - ref['dtable'][0][tok]) / ref['dtable'][1][tok]          # (the NaN counted as 0)
    print('FIG embed_bwd one-NaN row %d: %d NaN; column %d holds %r, %.3g of the bound of the sum without the NaN; the '
          'other columns at most %.3g' % (tok, np.isnan(dtable[tok]).sum(), c, float(dtable[tok, c]), err[c],
                                          np.nanmax(np.delete(err, c))))


def test_embed_refusals():
    case = (3, 12, 24, 7, 'text')
    B, Tn, C, V, _ = case
    lib = L.load()
    d, ins, outs, fn = embed_bwd_operands(case, 'normal', False)
    acc_bytes, ws_floats = lib.passl_hip_embed_bwd_acc_bytes(V, C), lib.passl_hip_embed_bwd_ws_floats(B, Tn, C)
    a = lambda **k: lambda: lib.passl_hip_embed_bwd(
        P(ins['text']), P(ins['dout']), P(outs['dtable']), P(outs['dpos']), B, Tn, k.get('C', C), V, L.dt(F32),
        P(outs['acc']), k.get('acc_bytes', acc_bytes), P(outs['ws']), k.get('ws_floats', ws_floats), L.stream())
    for what, f in (('C = 12', a(C=12)), ('acc one byte short', a(acc_bytes=acc_bytes - 1)),
                    ('ws one float short', a(ws_floats=ws_floats - 1))):
        refused('embed_bwd ' + what, f, dict(ins, **outs))


# ------------------------------------------------------------------------------------------------ eot_index, rows
@pytest.mark.parametrize('case', U.EOT_CASES, ids=U.case_id)
def test_eot_index(case):
    B, Tn = case
    lib = L.load()
    for shift in range(len(U.EOT_ROWS)):
        text = U.eot_text(case, shift)
        ins, idx = {'text': gin(text, I64)}, Guarded(B, I32)
        what = 'eot_index %s shift %d' % (U.case_id(case), shift)
        run(what, call('eot_index', lambda: lib.passl_hip_eot_index(P(ins['text']), B, Tn, P(idx), L.stream())), ins,
            {'idx': idx})
        exact(what, idx.view.cpu().numpy(), np.arange(B) * Tn + np.argmax(text, axis=1))


@LP
@pytest.mark.parametrize('case', U.ROWS_CASES, ids=U.case_id)
def test_gather_rows_and_scatter_rows(case, lp):
    n, C = case
    lib, d, want = L.load(), U.rows_data(case, lp), U.rows_eval(case, lp)
    what = '%s %s' % (U.case_id(case), lp)
    ins = {'x': gin(d['x'], DT(lp)), 'gidx': gin(d['gidx'], I32), 'dout': gin(d['dout'], DT(lp)),
           'sidx': gin(d['sidx'], I32)}
    outs = {'out': Guarded(n * C, DT(lp)), 'dx': Guarded(U.ROWS_TOTAL * C, DT(lp))}
    run('gather_rows ' + what, call('gather_rows', lambda: lib.passl_hip_gather_rows(
        P(ins['x']), P(ins['gidx']), P(outs['out']), n, C, L.dt(DT(lp)), L.stream())), ins, {'out': outs['out']})
    run('scatter_rows ' + what, call('scatter_rows', lambda: lib.passl_hip_scatter_rows(
        P(ins['dout']), P(ins['sidx']), P(outs['dx']), n, U.ROWS_TOTAL, C, L.dt(DT(lp)), L.stream())), ins,
        {'dx': outs['dx']})
    exact('gather_rows ' + what, gbits(outs['out'], lp), U.wbits(want['out'], lp))
    exact('scatter_rows ' + what, gbits(outs['dx'], lp), U.wbits(want['dx'], lp))      # +0 outside the scattered rows


# ------------------------------------------------------------------------------------------------ nchw_to_nhwc_pad
def pad_call(x, y, lp, C, Cp, pad, Wp):
    lib = L.load()
    return lambda: lib.passl_hip_nchw_to_nhwc_pad(P(x), P(y), U.PAD_N, C, U.PAD_H, U.PAD_W, pad, Wp, Cp, L.dt(DT(lp)),
                                                  L.stream())


@pytest.mark.parametrize('case', U.PAD_CASES, ids=U.case_id)
def test_nchw_to_nhwc_pad(case):
    lp, C, Cp, pad, ex, skew = case
    want = U.pad_expect(case)
    ins, y = {'x': gin(U.pad_data(C))}, Guarded(want.size, DT(lp), skew)
    what = 'nchw_to_nhwc_pad ' + U.case_id(case)
    run(what, call('nchw_to_nhwc_pad', pad_call(ins['x'], y, lp, C, Cp, pad, U.PAD_W + 2 * pad + ex)), ins, {'y': y})
    exact(what, gbits(y, lp), U.wbits(want, lp))


@LP
def test_nchw_to_nhwc_pad_refusals(lp):
    g = {'x': gin(U.pad_data(3)), 'y': Guarded(U.PAD_N * 11 * 13 * 9, DT(lp))}
    for what, k in U.PAD_REFUSED.items():
        refused('nchw_to_nhwc_pad ' + what, pad_call(g['x'], g['y'], lp, k['C'], k['Cp'], 3, U.PAD_W + 6 - k['short']), g)


# ------------------------------------------------------------------------------------------------ colsum, colsum_acc
def colsum_call(acc, x, out, ws, M, C, lp, ws_floats):
    lib = L.load()
    fn = lib.passl_hip_colsum_acc if acc else lib.passl_hip_colsum
    return lambda: fn(P(x), P(out), M, C, L.dt(DT(lp)), P(ws), ws_floats, L.stream())


@LP
@pytest.mark.parametrize('case', U.COLSUM_CASES, ids=U.case_id)
def test_colsum(case, lp):
    C, M = case
    d, slabs = U.colsum_data(case, lp), U.colsum_slabs(M)[0]
    ins = {'x': gin(d['x'], DT(lp))}
    for acc in (0, 1):
        what = '%s acc=%d %s' % (U.case_id(case), acc, 'bf16' if lp else 'fp32')
        outs = {'out': gin(d['out']) if acc else Guarded(C, F32)}
        if slabs > 1:                                                # a single slab takes no workspace (ws = NULL)
            outs['ws'] = Guarded(slabs * C, F32)
        run('colsum ' + what, call('colsum', colsum_call(acc, ins['x'], outs['out'], outs.get('ws'), M, C, lp, slabs * C)),
            ins, outs)
        bounded('colsum_acc' if acc else 'colsum', what, U.colsum_ref(case, lp, acc), {'out': outs['out']},
                U.colsum_eval32(case, lp, acc))


@LP
def test_colsum_refuses_several_slabs_without_their_workspace(lp):
    C, M = U.COLSUM_REFUSED
    slabs = U.colsum_slabs(M)[0]
    assert slabs == 2
    g = {'x': gin(U.colsum_data((C, M), lp)['x'], DT(lp)), 'out': gin(np.ones(C, np.float32)), 'ws': Guarded(slabs * C, F32)}
    for acc in (0, 1):
        refused('colsum ws = NULL', colsum_call(acc, g['x'], g['out'], None, M, C, lp, 0), g)
        refused('colsum ws one float short', colsum_call(acc, g['x'], g['out'], g['ws'], M, C, lp, slabs * C - 1), g)


# ------------------------------------------------------------------------------------------------ relu_bwd
@LP
@pytest.mark.parametrize('n', U.RELU_N)
def test_relu_bwd(n, lp):
    lib, d = L.load(), U.relu_data(n, lp)
    ins, dx = {'dy': gin(d['dy'], DT(lp)), 'y': gin(d['y'], DT(lp))}, Guarded(n, DT(lp), prefill='a5')
    what = 'relu_bwd %d %s' % (n, lp)
    run(what, call('relu_bwd', lambda: lib.passl_hip_relu_bwd(P(ins['dy']), P(ins['y']), P(dx), n, L.dt(DT(lp)),
                                                              L.stream())), ins, {'dx': dx})
    exact(what, gbits(dx, lp), U.wbits(U.relu_eval(n, lp), lp))
    if n == 8:
        refused('relu_bwd n = 12', lambda: lib.passl_hip_relu_bwd(P(ins['dy']), P(ins['y']), P(dx), U.RELU_REFUSED,
                                                                  L.dt(DT(lp)), L.stream()), dict(ins, dx=dx))
