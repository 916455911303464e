"""The token-merging kernels (csrc/tome.hip) through the C ABI against the float64 restatement of tome_util, on views
into guarded device buffers: outputs are NaN (0xA5 bytes for integers) before the launch and every element must have
been written, guards and inputs must be intact, a second launch must give the same bits.

Matching    dest, and node_idx of the merged rows, equal float64 exactly; every seeded case is decided (host test: all
            relevant float64 gaps >= 16 x 2 MARGIN), so no image is left out.  node_max within MARGIN.
            The planted tie is held to the documented rule, the normalisation case to float64.
Merge       |got - ref| <= allowance * bound, element-wise, bound = sum size |x| / sum size (gradient: |dx|):
            fp32 forward (n + 2) 2^-24 for a row of n sources (n fmas, one division), fp32 backward 2.5 x 2^-24 (the
            factor and the product); bf16 adds 2^-8 |ref| for the one store rounding.  size_out exact.
            Largest share of the allowance reached on an MI355X: forward fp32 0.24, bf16 1.00 (0.996); backward fp32
            0.68, bf16 0.98 — in bf16 the allowance is the store's half ulp, which a value just above a power of two
            uses up.  node_max: 0.07 of MARGIN in both dtypes.
Key bias    attention_util's criteria for `out` and lse on its input kinds with bias = log of sizes 1 .. 8; with a zero
            bias the bits of passl_hip_attention_fwd.
"""
import numpy as np
import pytest
import torch

import attention_util as A
import tome_util as U
from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
DT_ID = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}


def _intact(bufs, what):
    for name, g in bufs.items():
        assert g.intact(), '%s: a guard region of %s was written' % (what, name)


# ------------------------------------------------------------------ matching
def run_match(qkv, r, dtype, what):
    """-> dest [B, T], node_max [B, NA], node_idx [B, NA] as numpy."""
    B, T, _, H, DH = qkv.shape
    NA = (T + 1) // 2
    lib = L.load()
    q = Guarded(qkv.numel(), dtype, fill=qkv)
    dest = Guarded(B * T, torch.int32)
    nmax = Guarded(B * NA, torch.float32)
    nidx = Guarded(B * NA, torch.int32)
    bufs = {'qkv': q, 'dest': dest, 'node_max': nmax, 'node_idx': nidx}
    raws = []
    for _ in range(2):
        for g in (dest, nmax, nidx):
            g.reset()
        L.check(lib.passl_hip_tome_match(L.ptr(q.view), L.ptr(dest.view), L.ptr(nmax.view), L.ptr(nidx.view), B, T, H,
                                         DH, r, L.dt(dtype), L.stream()), 'tome_match')
        torch.cuda.synchronize()
        raws.append((dest.raw(), nmax.raw(), nidx.raw()))
    _intact(bufs, what)
    assert torch.equal(q.view.float().cpu(), qkv.flatten()), 'qkv was modified'
    assert dest.unwritten() == 0 and nidx.unwritten() == 0, '%s: unwritten elements' % what
    assert not torch.isnan(nmax.view).any(), '%s: node_max has unwritten elements' % what
    for a, b in zip(*raws):
        assert torch.equal(a, b), '%s: the second launch differs' % what
    # without the optional outputs: the same dest
    dest2 = Guarded(B * T, torch.int32)
    L.check(lib.passl_hip_tome_match(L.ptr(q.view), L.ptr(dest2.view), None, None, B, T, H, DH, r, L.dt(dtype),
                                     L.stream()), 'tome_match')
    torch.cuda.synchronize()
    assert dest2.intact() and torch.equal(dest2.raw(), raws[0][0])
    return (dest.view.cpu().view(B, T).numpy().astype(np.int64), nmax.view.cpu().view(B, NA).double().numpy(),
            nidx.view.cpu().view(B, NA).numpy().astype(np.int64))


def check_match(got, res, mg, what):
    dest, nmax, nidx = got
    assert np.array_equal(dest, res['dest']), '%s: dest differs from float64 at %s' % (
        what, np.argwhere(dest != res['dest'])[:4].tolist())
    m = res['merged']
    assert np.array_equal(nidx[m], res['node_idx'][m]), '%s: node_idx of merged rows differs' % what
    assert np.all(nidx[:, 0] == 0) and np.all(np.isneginf(nmax[:, 0])), '%s: the class row' % what
    err = np.abs(nmax[:, 1:] - res['node_max'][:, 1:]).max() if nmax.shape[1] > 1 else 0.0
    print('FIG %s node_max err %.3g = %.3f of MARGIN %.3g; smallest float64 gap %.3g' % (
        what, err, err / mg, mg, U.smallest_gap(res)))
    assert err <= mg, '%s: node_max off by %.3g > MARGIN %.3g' % (what, err, mg)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', U.MATCH_CASES, ids=[U.match_case_id(c) for c in U.MATCH_CASES])
def test_match(case, dtype):
    T, r, B, H, DH = case
    qkv, res, mg, _ = U.match_case(case)
    what = '%s %s' % (U.match_case_id(case), DT_ID[dtype])
    check_match(run_match(qkv, r, dtype, what), res, mg, what)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
def test_match_normalises_huge_and_tiny_keys(dtype):
    qkv, res, mg, _ = U.norm_case()
    check_match(run_match(qkv, U.NORM_CASE[1], dtype, 'norm'), res, mg, 'norm ' + DT_ID[dtype])


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
def test_match_ties_follow_the_documented_rule(dtype):
    """tome_util.tie_case: A rows 2 and 5 (tokens 4 and 10) both score exactly the same against B rows 1 and 3 (tokens 3
    and 7), and higher than any other row.  arg-max: the lower B index, 1.  r = 1: the lower A index, row 2, goes;
    r = 2: both go, into the same B token."""
    qkv = U.tie_case()
    B, T = qkv.shape[:2]
    NA = (T + 1) // 2
    for r in (1, 2):
        dest, nmax, nidx = run_match(qkv, r, dtype, 'tie r=%d' % r)
        assert np.all(nidx[:, 2] == 1) and np.all(nidx[:, 5] == 1)
        assert np.all(nmax[:, 2] == nmax[:, 5]) and np.all(nmax[:, 2] > np.delete(nmax, (2, 5), axis=1).max(axis=1))
        assert np.all(dest[:, 4] == NA - r + 1)
        if r == 1:
            # token 10 stays: A rows 0, 1, 3, 4 are before it
            assert np.all(dest[:, 10] == 4)
            assert np.all(dest[:, [0, 2, 6, 8, 12, 14, 16]] == np.array([0, 1, 2, 3, 5, 6, 7]))
        else:
            assert np.all(dest[:, 10] == NA - r + 1)
            assert np.all(dest[:, [0, 2, 6, 8, 12, 14, 16]] == np.arange(7))
        assert np.all(dest[:, 1::2] == NA - r + np.arange(T // 2))


def test_match_rejects_what_is_not_built():
    lib = L.load()
    q = torch.zeros(2 * 17 * 3 * 64, device='cuda')
    d = torch.zeros(2 * 17, dtype=torch.int32, device='cuda')
    args = lambda T, H, DH, r: (L.ptr(q), L.ptr(d), None, None, 2, T, H, DH, r, L.F32, None)   # noqa: E731
    assert lib.passl_hip_tome_match(*args(17, 1, 64, 9)) == L.EINVAL          # r above the clamp (T - 1) // 2 = 8
    assert lib.passl_hip_tome_match(*args(17, 1, 64, 0)) == L.EINVAL
    assert lib.passl_hip_tome_match(*args(2, 1, 64, 1)) == L.EINVAL           # clamp 0
    assert lib.passl_hip_tome_match(*args(17, 1, 48, 1)) == L.EUNSUPPORTED
    assert lib.passl_hip_tome_match(*args(209, 1, 32, 1)) == L.EUNSUPPORTED
    assert lib.passl_hip_tome_match(*args(17, 1, 64, 8)) == L.OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------ merge
def _usage(got, ref, bound, limit, extra=None):
    return A.limit_usage(got, ref, bound, limit, extra)[0]


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', U.MERGE_CASES, ids=[U.merge_case_id(c) for c in U.MERGE_CASES])
def test_merge_forward_and_backward(case, dtype):
    T, r, B, C, sizes = case
    To = T - r
    d = U.merge_case(case)
    what = '%s %s' % (U.merge_case_id(case), DT_ID[dtype])
    lib = L.load()
    bf16 = dtype == torch.bfloat16
    x = Guarded(B * T * C, dtype, fill=d['x'])
    dy = Guarded(B * To * C, dtype, fill=d['dy'])
    size = None if d['size'] is None else Guarded(B * T, torch.float32, fill=d['size'])
    dest = Guarded(B * T, torch.int32, fill=torch.as_tensor(d['dest']))
    y = Guarded(B * To * C, dtype)
    so = Guarded(B * To, torch.float32)
    lg = Guarded(B * To, torch.float32)
    dx = Guarded(B * T * C, dtype)
    bufs = {'x': x, 'dy': dy, 'dest': dest, 'y': y, 'size_out': so, 'logsize_out': lg, 'dx': dx}
    if size is not None:
        bufs['size'] = size
    sp = None if size is None else L.ptr(size.view)
    raws = []
    for _ in range(2):
        for g in (y, so, lg, dx):
            g.reset()
        L.check(lib.passl_hip_tome_merge_fwd(L.ptr(x.view), sp, L.ptr(dest.view), L.ptr(y.view), L.ptr(so.view),
                                             L.ptr(lg.view), B, T, r, C, L.dt(dtype), L.stream()), 'tome_merge_fwd')
        L.check(lib.passl_hip_tome_merge_bwd(L.ptr(dy.view), sp, L.ptr(so.view), L.ptr(dest.view), L.ptr(dx.view), B, T,
                                             r, C, L.dt(dtype), L.stream()), 'tome_merge_bwd')
        torch.cuda.synchronize()
        raws.append((y.raw(), so.raw(), lg.raw(), dx.raw()))
    _intact(bufs, what)
    for a, b in zip(*raws):
        assert torch.equal(a, b), '%s: the second launch differs' % what
    assert torch.equal(x.view.float().cpu(), d['x'].flatten()) and torch.equal(dy.view.float().cpu(), d['dy'].flatten())
    assert torch.equal(dest.view.cpu().long(), torch.as_tensor(d['dest']).flatten())
    for g, name in ((y, 'y'), (so, 'size_out'), (lg, 'logsize_out'), (dx, 'dx')):
        assert g.unwritten() == 0, '%s: %d elements of %s were not written' % (what, g.unwritten(), name)
    fwd, bwd = d['fwd'], d['bwd']
    assert torch.equal(so.view.cpu().double().view(B, To), fwd['size_out']), '%s: size_out is not exact' % what
    lerr = float((lg.view.cpu().double().view(B, To) - fwd['size_out'].log()).abs().max())
    assert lerr <= 4 * U.U32 * max(1.0, float(fwd['size_out'].log().max())), '%s: log(size_out) off by %.3g' % (what, lerr)
    gy = y.view.float().cpu().view(B, To, C)
    gdx = dx.view.float().cpu().view(B, T, C)
    lim = U.merge_fwd_limit(fwd['n']).unsqueeze(-1).expand(B, To, C) * (1 + U.U16 if bf16 else 1.0)
    # limit_usage takes one scalar limit: fold the per-row factor into the bound
    use_f = _usage(gy, fwd['y'], fwd['bound'] * lim, 1.0, U.U16 * fwd['y'].abs() if bf16 else None)
    use_b = _usage(gdx, bwd['dx'], bwd['bound'], U.MERGE_BWD_LIMIT * (1 + U.U16 if bf16 else 1.0),
                   U.U16 * bwd['dx'].abs() if bf16 else None)
    print('FIG %s merge fwd %.3f of the allowance, bwd %.3f' % (what, use_f, use_b))
    assert use_f <= 1, '%s: forward outside its allowance (%.3f)' % (what, use_f)
    assert use_b <= 1, '%s: backward outside its allowance (%.3f)' % (what, use_b)
    if d['size'] is None:
        # a row with one source of size one is that source, bit for bit
        single = (fwd['n'] == 1)
        assert torch.equal(gy[single].double(), fwd['y'][single])


def test_merge_ignores_a_dest_outside_its_range():
    """A corrupt dest must not become an out-of-bounds access: such a token joins no row, its gradient is zero."""
    B, T, r, C = 1, 17, 4, 32
    d = U.merge_case((17, 4, 3, 32, 'ones'))
    dest_np = d['dest'][:1].copy()
    dest_np[0, 6] = T + 1000
    dest_np[0, 8] = -3
    x = Guarded(B * T * C, torch.float32, fill=d['x'][:1])
    dest = Guarded(B * T, torch.int32, fill=torch.as_tensor(dest_np))
    y = Guarded(B * (T - r) * C, torch.float32)
    so = Guarded(B * (T - r), torch.float32)
    dx = Guarded(B * T * C, torch.float32)
    lib = L.load()
    L.check(lib.passl_hip_tome_merge_fwd(L.ptr(x.view), None, L.ptr(dest.view), L.ptr(y.view), L.ptr(so.view), None, B, T,
                                         r, C, L.F32, L.stream()), 'tome_merge_fwd')
    L.check(lib.passl_hip_tome_merge_bwd(L.ptr(y.view), None, L.ptr(so.view), L.ptr(dest.view), L.ptr(dx.view), B, T, r,
                                         C, L.F32, L.stream()), 'tome_merge_bwd')
    torch.cuda.synchronize()
    for g in (x, dest, y, so, dx):
        assert g.intact()
    keep = np.ones(T, dtype=bool)
    keep[[6, 8]] = False
    ref = U.merge(d['x'][:1][:, torch.as_tensor(keep)], None, dest_np[:, keep], T - r)
    rows = ref['n'][0] > 0
    assert torch.allclose(y.view.cpu().view(T - r, C)[rows].double(), ref['y'][0][rows], rtol=1e-6, atol=1e-7)
    assert float(dx.view.view(T, C)[[6, 8]].abs().max()) == 0.0


def test_merge_rejects_bad_arguments():
    lib = L.load()
    b = torch.zeros(4096, device='cuda')
    i = torch.zeros(64, dtype=torch.int32, device='cuda')
    f = lambda T, r, C: lib.passl_hip_tome_merge_fwd(L.ptr(b), None, L.ptr(i), L.ptr(b), L.ptr(b), None, 1, T, r, C,  # noqa: E731
                                                     L.F32, None)
    assert f(17, 0, 32) == L.EINVAL and f(17, 17, 32) == L.EINVAL and f(17, 4, 36) == L.EINVAL
    assert f(209, 4, 8) == L.EUNSUPPORTED


# ------------------------------------------------------------------ key-bias attention
KB_CASES = [(DH, T, kind) for DH in A.HEAD_DIMS for T in U.KEYBIAS_T for kind in A.KINDS]
KB_IDS = ['d%d-T%d-%s' % c for c in KB_CASES]
_kb_cache = {}


def kb_data(case):
    if case not in _kb_cache:
        DH, T, kind = case
        qkv, _ = A.make_inputs(kind, A.B, T, A.H, DH, 2000 * T + DH + A.KINDS.index(kind))
        bias = U.log_sizes(A.B, T, T + DH)
        scale = DH ** -0.5
        _kb_cache[case] = {'qkv': qkv, 'bias': bias, 'scale': scale,
                           'ref': U.keybias_reference(qkv, bias, scale),
                           'model': U.keybias_reference(qkv, bias, scale, round_p=True),
                           'eager': U.keybias_reference(qkv, bias, scale, dtype=torch.float32)}
    return _kb_cache[case]


def run_keybias(qkv, bias, scale, dtype, what, plain=False):
    B, T, _, H, DH = qkv.shape
    lib = L.load()
    q = Guarded(qkv.numel(), dtype, fill=qkv)
    kb = Guarded(B * T, torch.float32, fill=bias)
    out = Guarded(B * T * H * DH, dtype)
    lse = Guarded(B * H * T, torch.float32)
    raws = []
    for _ in range(1 if plain else 2):
        out.reset()
        lse.reset()
        if plain:
            L.check(lib.passl_hip_attention_fwd(L.ptr(q.view), L.ptr(out.view), L.ptr(lse.view), B, T, H, DH, scale, 0,
                                                L.dt(dtype), L.stream()), 'attention_fwd')
        else:
            L.check(lib.passl_hip_attention_fwd_keybias(L.ptr(q.view), L.ptr(kb.view), L.ptr(out.view), L.ptr(lse.view),
                                                        B, T, H, DH, scale, L.dt(dtype), L.stream()), 'keybias')
        torch.cuda.synchronize()
        raws.append((out.raw(), lse.raw()))
    _intact({'qkv': q, 'key_bias': kb, 'out': out, 'lse': lse}, what)
    assert torch.equal(q.view.float().cpu(), qkv.flatten()) and torch.equal(kb.view.cpu(), bias.flatten())
    assert out.unwritten() == 0 and lse.unwritten() == 0, '%s: unwritten elements' % what
    if not plain:
        assert torch.equal(raws[0][0], raws[1][0]) and torch.equal(raws[0][1], raws[1][1]), '%s: second launch' % what
    return out.view.float().cpu().view(B, T, H, DH), lse.view.cpu().view(B, H, T), raws[0]


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', KB_CASES, ids=KB_IDS)
def test_keybias_attention(case, dtype):
    d = kb_data(case)
    what = 'keybias %s %s' % (KB_IDS[KB_CASES.index(case)], DT_ID[dtype])
    out, lse, _ = run_keybias(d['qkv'], d['bias'], d['scale'], dtype, what)
    ref, b = d['ref'], d['ref']['b_out']
    msgs = []
    if dtype == torch.bfloat16:
        # the bf16-MFMA criteria of attention_util for `out`
        msgs += A.bound_violations('out', out, ref['out'], b, A.LIMIT_BF16['out'])
        msgs += A.closeness_violations('out', out, d['model']['out'], ref['out'], b)
        print('FIG %s err %.3f u (limit %.2f u)' % (what, A.scaled_error(out, ref['out'], b)[0] / A.U,
                                                   A.LIMIT_BF16['out'] / A.U))
    else:
        # the fp32-MFMA criterion: 4 x the float32-eager error of the same case, at least 16 x 2^-24
        eager = A.scaled_error(d['eager']['out'], ref['out'], b)[0]
        limit = max(4 * eager, 16 * 2.0 ** -24)
        msgs += A.bound_violations('out', out, ref['out'], b, limit)
        print('FIG %s err %.1f x 2^-24 (eager %.1f)' % (what, A.scaled_error(out, ref['out'], b)[0] * 2 ** 24,
                                                       eager * 2 ** 24))
    eager_l = float((d['eager']['lse'].double() - ref['lse']).abs().max())
    allow = torch.maximum(torch.full_like(ref['lse'], 4 * eager_l), 2.0 ** -20 * ref['lse'].abs().clamp_min(1.0))
    used = float(((lse.double() - ref['lse']).abs() / allow).max())
    if not used <= 1:
        msgs.append('lse uses %.3f of its allowance' % used)
    assert not msgs, what + ':\n' + '\n'.join(msgs)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('DH, T', [(32, 17), (64, 113), (64, 197), (32, 208)])
def test_keybias_of_sizes_one_is_the_plain_kernel_bit_for_bit(DH, T, dtype):
    qkv, _ = A.make_inputs('plain', A.B, T, A.H, DH, 77 + T)
    zero = torch.zeros(A.B, T)
    _, _, biased = run_keybias(qkv, zero, DH ** -0.5, dtype, 'zero bias')
    _, _, plain = run_keybias(qkv, zero, DH ** -0.5, dtype, 'plain', plain=True)
    assert torch.equal(biased[0], plain[0]), 'out differs from passl_hip_attention_fwd'
    assert torch.equal(biased[1], plain[1]), 'lse differs from passl_hip_attention_fwd'


def test_keybias_rejects_what_is_not_built():
    lib = L.load()
    p = torch.zeros(4096, device='cuda')
    assert lib.passl_hip_attention_fwd_keybias(L.ptr(p), L.ptr(p), L.ptr(p), L.ptr(p), 1, 300, 1, 64, 0.125, L.F32,
                                               None) == L.EUNSUPPORTED
    assert lib.passl_hip_attention_fwd_keybias(L.ptr(p), L.ptr(p), L.ptr(p), L.ptr(p), 1, 16, 1, 48, 0.125, L.F32,
                                               None) == L.EUNSUPPORTED
    assert lib.passl_hip_attention_fwd_keybias(L.ptr(p), None, L.ptr(p), L.ptr(p), 1, 16, 1, 64, 0.125, L.F32,
                                               None) == L.EINVAL
