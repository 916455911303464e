"""The streaming kernels of CAE pre-training (csrc/cae.hip) through the C ABI, on guarded, NaN-filled buffers.

cae_tokens_assemble / _bwd   equal a host restatement bit for bit in fp32 and bf16 (every sum is one fp32 addition per
                             element followed by one rounding, so the restatement is exact), with every output NULL in
                             turn; shapes include Nu = 1, C = 8 and a last workgroup that is partly filled.
mse_fwd                      within 4 x max(fp32 eager's own error, one fp32 ulp of the result) of float64 on rows whose
                             difference cancels and on rows with a large common offset; t0 = 0 and 1 (the target's class
                             row skipped in place); a second launch has equal bits.
mse_bwd                      gloss 2 (pred - target) / n: the difference is one fp32 rounding, the two factors and their
                             product three more, the store in bf16 one of 2^-9: within (4 * 2^-24 [+ 2^-8]) |value|.
"""
import pytest
import torch
import torch.nn.functional as F

from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

OK, EINVAL = 0, -1
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['fp32', 'bf16']
# (B, Nu, Nm, L, C): one visible row and 8 channels; the small parity model; two workgroups with a partial last one
SHAPES = [(2, 1, 3, 4, 8), (3, 22, 14, 36, 128), (2, 121, 75, 196, 72)]


def _round(x, dtype):
    return x.to(dtype).float()


def _tables(B, Nu, Nm, Ln, gen):
    ids = torch.stack([torch.randperm(Ln, generator=gen)[:Nu + Nm] for _ in range(B)])
    return ids[:, :Nu].sort(dim=1).values.int().contiguous(), ids[:, Nu:].sort(dim=1).values.int().contiguous()


def _assemble_ref(xu, xm, pos, ids_vis, ids_msk, dtype):
    pv, pm = pos[1 + ids_vis.long()], pos[1 + ids_msk.long()]
    v_in = torch.cat([xu, xm], dim=1)
    return {'q_in': _round(xm + pm, dtype), 'k_in': _round(v_in + torch.cat([pv, pm], dim=1), dtype), 'v_in': v_in}


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('u0', [0, 1])
@pytest.mark.parametrize('null', [None, 'q_in', 'k_in', 'v_in', 'kv'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-u%d-m%d-L%d-C%d' % s)
def test_tokens_assemble_forward_is_exact(shape, null, u0, dtype):
    """u0 = 1: xu carries a leading (class) row per image that is skipped in place."""
    B, Nu, Nm, Ln, C = shape
    gen = torch.Generator().manual_seed(sum(shape))
    xu = _round(torch.randn(B, u0 + Nu, C, generator=gen), dtype)
    xm = _round(torch.randn(B, Nm, C, generator=gen), dtype)
    pos = torch.randn(1 + Ln, C, generator=gen)
    ids_vis, ids_msk = _tables(B, Nu, Nm, Ln, gen)
    ref = _assemble_ref(xu[:, u0:], xm, pos, ids_vis, ids_msk, dtype)
    absent = {'kv': ('k_in', 'v_in')}.get(null, (null,))
    g = {'xu': Guarded(xu.numel(), dtype, fill=xu), 'xm': Guarded(xm.numel(), dtype, fill=xm),
         'pos': Guarded(pos.numel(), torch.float32, fill=pos),
         'ids_vis': Guarded(ids_vis.numel(), torch.int32, fill=ids_vis),
         'ids_msk': Guarded(ids_msk.numel(), torch.int32, fill=ids_msk),
         'q_in': Guarded(B * Nm * C, dtype), 'k_in': Guarded(B * (Nu + Nm) * C, dtype),
         'v_in': Guarded(B * (Nu + Nm) * C, dtype)}
    p = {n: (None if n in absent else L.ptr(b.view)) for n, b in g.items()}
    if null == 'kv':                       # the decoder's x_masked + pos: the visible side is not read
        p['xu'] = p['ids_vis'] = None
    raws = []
    for _ in range(2):
        for n in ('q_in', 'k_in', 'v_in'):
            g[n].reset()
        L.check(L.load().passl_hip_cae_tokens_assemble(p['xu'], p['xm'], p['pos'], p['ids_vis'], p['ids_msk'], p['q_in'],
                                                       p['k_in'], p['v_in'], B, u0, Nu, Nm, Ln, C, L.dt(dtype),
                                                       L.stream()),
                'cae_tokens_assemble')
        torch.cuda.synchronize()
        raws.append({n: g[n].raw() for n in ('q_in', 'k_in', 'v_in')})
    for n, b in g.items():
        assert b.intact(), 'a guard region of %s was written' % n
    for n in ('q_in', 'k_in', 'v_in'):
        assert torch.equal(raws[0][n], raws[1][n])
        if n in absent:
            assert g[n].unwritten() == g[n].hi - g[n].lo, '%s was written though NULL was passed' % n
        else:
            assert torch.equal(g[n].view.float().cpu(), ref[n].flatten()), n


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('u0', [0, 1])
@pytest.mark.parametrize('null', [None, 'dq_in', 'dk_in', 'dv_in', 'dxu'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d-u%d-m%d-L%d-C%d' % s)
def test_tokens_assemble_backward_is_exact(shape, null, u0, dtype):
    """u0 = 1: dxu carries a leading row per image, written as zeros."""
    B, Nu, Nm, _, C = shape
    gen = torch.Generator().manual_seed(sum(shape) + 1)
    d = {'dq_in': _round(torch.randn(B, Nm, C, generator=gen), dtype),
         'dk_in': _round(torch.randn(B, Nu + Nm, C, generator=gen), dtype),
         'dv_in': _round(torch.randn(B, Nu + Nm, C, generator=gen), dtype)}
    z = {n: (torch.zeros_like(t) if n == null else t) for n, t in d.items()}    # a NULL gradient counts as zero
    ref = {'dxm': _round((z['dq_in'] + z['dk_in'][:, Nu:]) + z['dv_in'][:, Nu:], dtype),
           'dxu': torch.cat([torch.zeros(B, u0, C), _round(z['dk_in'][:, :Nu] + z['dv_in'][:, :Nu], dtype)], dim=1)}
    g = {n: Guarded(t.numel(), dtype, fill=t) for n, t in d.items()}
    g.update(dxu=Guarded(B * (u0 + Nu) * C, dtype), dxm=Guarded(B * Nm * C, dtype))
    p = {n: (None if n == null else L.ptr(b.view)) for n, b in g.items()}
    raws = []
    for _ in range(2):
        g['dxu'].reset()
        g['dxm'].reset()
        L.check(L.load().passl_hip_cae_tokens_assemble_bwd(p['dq_in'], p['dk_in'], p['dv_in'], p['dxu'], p['dxm'], B, u0,
                                                           Nu, Nm, C, L.dt(dtype), L.stream()), 'cae_tokens_assemble_bwd')
        torch.cuda.synchronize()
        raws.append((g['dxu'].raw(), g['dxm'].raw()))
    for n, b in g.items():
        assert b.intact(), 'a guard region of %s was written' % n
    assert torch.equal(raws[0][0], raws[1][0]) and torch.equal(raws[0][1], raws[1][1])
    assert torch.equal(g['dxm'].view.float().cpu(), ref['dxm'].flatten())
    if null == 'dxu':
        assert g['dxu'].unwritten() == g['dxu'].hi - g['dxu'].lo
    else:
        assert torch.equal(g['dxu'].view.float().cpu(), ref['dxu'].flatten())


def test_tokens_assemble_refuses_what_it_cannot_stream():
    g = Guarded(4096, torch.float32)
    ids = Guarded(64, torch.int32)
    x, i, s = L.ptr(g.view), L.ptr(ids.view), L.stream()
    lib = L.load()
    assert lib.passl_hip_cae_tokens_assemble(x, x, x, i, i, x, x, x, 1, 0, 2, 2, 4, 12, 0, s) == EINVAL       # C % 8
    assert lib.passl_hip_cae_tokens_assemble(x, x, x, i, i, None, None, None, 1, 0, 2, 2, 4, 8, 0, s) == EINVAL
    assert lib.passl_hip_cae_tokens_assemble(None, x, x, None, i, x, x, x, 1, 0, 2, 2, 4, 8, 0, s) == EINVAL  # xu needed
    assert lib.passl_hip_cae_tokens_assemble(x, x, x, i, i, x + 4, x, x, 1, 0, 2, 2, 4, 8, 0, s) == EINVAL    # alignment
    assert lib.passl_hip_cae_tokens_assemble(x, x, x, i, i, x, x, x, 1, -1, 2, 2, 4, 8, 0, s) == EINVAL
    assert lib.passl_hip_cae_tokens_assemble_bwd(x, x, x, x, None, 1, 0, 2, 2, 8, 0, s) == EINVAL
    assert lib.passl_hip_cae_tokens_assemble_bwd(None, None, None, x, x, 1, 0, 2, 2, 8, 0, s) == EINVAL
    assert lib.passl_hip_cae_tokens_assemble_bwd(x, x, x, x, x, 1, 1, 0, 2, 8, 0, s) == EINVAL             # dxu, no row
    assert lib.passl_hip_cae_mask_ids(x, i, i, i, 1, 4, 4, s) == EINVAL                                    # Nu < L
    assert lib.passl_hip_cae_mask_ids(x, i, None, i, 1, 4, 2, s) == EINVAL
    torch.cuda.synchronize()
    assert g.unwritten() == g.hi - g.lo and g.intact()


def test_tokens_assemble_clamps_indices_to_the_table():
    """An index below 0 reads the table's first patch row, one from L on its last: no access leaves the table (it sits
    between guards) and the result is the clamped index's."""
    B, Nu, Nm, Ln, C = 1, 2, 2, 4, 8
    gen = torch.Generator().manual_seed(5)
    xu, xm, pos = torch.randn(B, Nu, C, generator=gen), torch.randn(B, Nm, C, generator=gen), torch.randn(1 + Ln, C, generator=gen)
    bad_vis, bad_msk = torch.tensor([[-7, 1]], dtype=torch.int32), torch.tensor([[Ln, 1 << 30]], dtype=torch.int32)
    ref = _assemble_ref(xu, xm, pos, bad_vis.clamp(0, Ln - 1), bad_msk.clamp(0, Ln - 1), torch.float32)
    g = {'xu': Guarded(xu.numel(), torch.float32, fill=xu), 'xm': Guarded(xm.numel(), torch.float32, fill=xm),
         'pos': Guarded(pos.numel(), torch.float32, fill=pos), 'ids_vis': Guarded(2, torch.int32, fill=bad_vis),
         'ids_msk': Guarded(2, torch.int32, fill=bad_msk), 'q_in': Guarded(B * Nm * C, torch.float32),
         'k_in': Guarded(B * (Nu + Nm) * C, torch.float32), 'v_in': Guarded(B * (Nu + Nm) * C, torch.float32)}
    p = {n: L.ptr(b.view) for n, b in g.items()}
    L.check(L.load().passl_hip_cae_tokens_assemble(p['xu'], p['xm'], p['pos'], p['ids_vis'], p['ids_msk'], p['q_in'],
                                                   p['k_in'], p['v_in'], B, 0, Nu, Nm, Ln, C, 0, L.stream()),
            'cae_tokens_assemble')
    torch.cuda.synchronize()
    assert all(b.intact() for b in g.values())
    for n in ('q_in', 'k_in', 'v_in'):
        assert torch.equal(g[n].view.cpu(), ref[n].flatten()), n


@pytest.mark.parametrize('shape', [(3, 4, 1), (2, 36, 22), (5, 196, 121), (2, 130, 64)], ids=lambda s: 'B%d-L%d-u%d' % s)
def test_mask_ids_are_the_ascending_index_tables(shape):
    """ids_vis / ids_msk are the nonzero positions of ~mask / mask per image, rank the inverse table; a mask with the
    wrong count (last case: one image all masked, one all visible) leaves the guards alone and every entry written."""
    B, Ln, Nu = shape
    gen = torch.Generator().manual_seed(sum(shape))
    mask = torch.zeros(B, Ln)
    for b in range(B):
        mask[b, torch.randperm(Ln, generator=gen)[:Ln - Nu]] = 1.0
    wrong = shape == (2, 130, 64)
    if wrong:
        mask[0] = 1.0
        mask[1] = 0.0
    g = {'mask': Guarded(mask.numel(), torch.float32, fill=mask), 'ids_vis': Guarded(B * Nu, torch.int32),
         'ids_msk': Guarded(B * (Ln - Nu), torch.int32), 'rank': Guarded(B * Ln, torch.int32)}
    p = {n: L.ptr(b.view) for n, b in g.items()}
    raws = []
    for _ in range(2):
        for n in ('ids_vis', 'ids_msk', 'rank'):
            g[n].reset()
        L.check(L.load().passl_hip_cae_mask_ids(p['mask'], p['ids_vis'], p['ids_msk'], p['rank'], B, Ln, Nu, L.stream()),
                'cae_mask_ids')
        torch.cuda.synchronize()
        raws.append([g[n].raw() for n in ('ids_vis', 'ids_msk', 'rank')])
    assert all(b.intact() for b in g.values())
    assert all(torch.equal(a, b) for a, b in zip(*raws))
    vis, msk, rank = [g[n].view.cpu() for n in ('ids_vis', 'ids_msk', 'rank')]
    for t in (vis, msk):
        assert int(t.min()) >= 0 and int(t.max()) < Ln
    if wrong:
        assert torch.equal(msk.view(B, -1)[0], torch.arange(Ln - Nu, dtype=torch.int32)) and int(msk.view(B, -1)[1].max()) == 0
        return
    vis, msk, rank = vis.view(B, Nu), msk.view(B, Ln - Nu), rank.view(B, Ln)
    for b in range(B):
        assert torch.equal(vis[b].long(), (mask[b] == 0).nonzero().flatten())
        assert torch.equal(msk[b].long(), (mask[b] != 0).nonzero().flatten())
        assert torch.equal(rank[b, vis[b].long()], torch.arange(Nu, dtype=torch.int32))
        assert torch.equal(rank[b, msk[b].long()], Nu + torch.arange(Ln - Nu, dtype=torch.int32))


# ------------------------------------------------------------------ mse
def _mse_inputs(kind, B, Tm, t0, C, dtype, gen):
    target = torch.randn(B, Tm + t0, C, generator=gen)
    if kind == 'cancelling':               # pred is the target but for a few units in the last place
        pred = target[:, t0:] * (1 + 2.0 ** -7 * torch.randn(B, Tm, C, generator=gen))
    else:                                  # 'offset': both sit on a common offset three orders above their spread
        target = target + 1000.0
        pred = 1000.0 + torch.randn(B, Tm, C, generator=gen)
    return _round(pred, dtype).contiguous(), _round(target, dtype).contiguous()


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('t0', [0, 1])
@pytest.mark.parametrize('kind', ['cancelling', 'offset'])
@pytest.mark.parametrize('shape', [(3, 5, 8), (2, 14, 136), (2, 75, 768)], ids=lambda s: 'B%d-T%d-C%d' % s)
def test_mse(shape, kind, t0, dtype):
    B, Tm, C = shape
    gen = torch.Generator().manual_seed(sum(shape) + t0)
    pred, target = _mse_inputs(kind, B, Tm, t0, C, dtype, gen)
    ref = F.mse_loss(pred.double(), target[:, t0:].double())
    eager = F.mse_loss(pred, target[:, t0:])
    ulp = float(torch.nextafter(ref.float(), torch.tensor(float('inf'))) - ref.float())
    allow = 4 * max(abs(float(eager.double() - ref)), ulp)
    gl = torch.tensor([0.75])
    g = {'pred': Guarded(pred.numel(), dtype, fill=pred), 'target': Guarded(target.numel(), dtype, fill=target),
         'gloss': Guarded(1, torch.float32, fill=gl), 'loss': Guarded(1, torch.float32),
         'ws': Guarded(B * Tm, torch.float32), 'dpred': Guarded(pred.numel(), dtype)}
    p = {n: L.ptr(b.view) for n, b in g.items()}
    raws = []
    for _ in range(2):
        for n in ('loss', 'ws', 'dpred'):
            g[n].reset()
        L.check(L.load().passl_hip_mse_fwd(p['pred'], p['target'], p['loss'], B, Tm, t0, C, L.dt(dtype), p['ws'], B * Tm,
                                           L.stream()), 'mse_fwd')
        L.check(L.load().passl_hip_mse_bwd(p['pred'], p['target'], p['gloss'], p['dpred'], B, Tm, t0, C, L.dt(dtype),
                                           L.stream()), 'mse_bwd')
        torch.cuda.synchronize()
        raws.append((g['loss'].raw(), g['dpred'].raw()))
    for n, b in g.items():
        assert b.intact(), 'a guard region of %s was written' % n
    assert torch.equal(raws[0][0], raws[1][0]) and torch.equal(raws[0][1], raws[1][1])
    got = float(g['loss'].view.cpu().double())
    print('FIG mse %s %s t0=%d %s: got %.9g, float64 %.9g, |diff| %.3g of %.3g allowed (eager %.3g, ulp %.3g)' % (
        shape, kind, t0, dtype, got, float(ref), abs(got - float(ref)), allow, abs(float(eager.double() - ref)), ulp))
    assert abs(got - float(ref)) <= allow
    dref = 0.75 * 2 * (pred.double() - target[:, t0:].double()) / pred.numel()
    dgot = g['dpred'].view.float().cpu().double().view_as(dref)
    assert torch.isfinite(dgot).all()
    rel = 4 * 2.0 ** -24 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert bool(((dgot - dref).abs() <= rel * dref.abs() + 2.0 ** -126).all())


def test_mse_refuses_a_short_workspace_and_odd_channels():
    g = Guarded(4096, torch.float32)
    x, s = L.ptr(g.view), L.stream()
    lib = L.load()
    assert lib.passl_hip_mse_fwd(x, x, x, 2, 3, 0, 8, 0, x, 5, s) == EINVAL
    assert lib.passl_hip_mse_fwd(x, x, x, 2, 3, 0, 12, 0, x, 6, s) == EINVAL
    assert lib.passl_hip_mse_bwd(x, x, None, None, 2, 3, 0, 8, 0, s) == EINVAL
    torch.cuda.synchronize()
    assert g.unwritten() == g.hi - g.lo and g.intact()
