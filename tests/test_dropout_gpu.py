"""Element-wise dropout on the MI355X (csrc/dropout.hip) and the ViTCELoss kernels (csrc/clas.hip), called through
passl_amd.hip.ops on guarded buffers (tests/guarded.py): guards intact, inputs unmodified, every output element written.

dropout / dropout_add are bit-equal to the numpy restatement (tests/dropout_util.py): the arithmetic is fully specified,
one float32 rounding per operation, then round-to-nearest-even for bf16.  The two GELU launches are compared with the
composition of the existing GELU launch and passl_hip_dropout: bit-equal in fp32; in bf16 the composition rounds its
intermediate to bf16, so the zero pattern is identical and the values agree within one bf16 ulp."""
import numpy as np
import pytest
import torch

import dropout_util as DU
import droppath_util as DP
from guarded import DEV, Guarded

pytestmark = pytest.mark.gpu

SEED = (0x1234 << 32) + 0x9abcdef1
SIZES = [8, 8 * 1024, 8 * 1025, 8 * 4097]          # one chunk, exactly one tile, a tile plus one chunk, a clamped tail
RATES = [0.0, 0.1, 0.5]
STEPS = [0, (1 << 32) + 5]                         # the second: the counter's high word is in play
SITES = [0, 7]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _as(ref32, dtype):
    """float32 numpy values (bf16-exact where dtype is bf16) as a CPU tensor of dtype."""
    return torch.from_numpy(np.ascontiguousarray(ref32)).to(dtype)


def _step_tensor(step):
    return torch.tensor([step - (1 << 64) if step >= 1 << 63 else step], dtype=torch.int64, device=DEV)


def _bf16_ulp(a, b):
    m = np.maximum(np.abs(a), np.abs(b)).astype(np.float64)
    return np.where(m > 0, np.ldexp(1.0, np.frexp(np.where(m > 0, m, 1.0))[1] - 1 - 7), 0.0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('n', SIZES)
def test_dropout_kernels(n, dtype):
    from passl_amd.hip import ops
    DP.check_known_answers()
    bf16 = dtype == torch.bfloat16
    gen = torch.Generator().manual_seed(n)
    src = {k: (torch.randn(n, generator=gen) * 2).to(dtype) for k in ('x', 'res', 'dy')}
    src['x'][0] = -0.0                                   # a dropped -0 is +0; a kept one stays -0
    np32 = {k: v.float().numpy() for k, v in src.items()}
    buf = {k: Guarded(n, dtype, fill=v) for k, v in src.items()}
    before = {k: g.raw() for k, g in buf.items()}
    out = Guarded(n, dtype)

    def run(fn, *tensors, args):
        out.reset()
        fn(*[buf[t].view for t in tensors], *args, out=out.view)
        torch.cuda.synchronize()
        assert out.intact() and all(g.intact() for g in buf.values())
        assert all(torch.equal(g.raw(), before[k]) for k, g in buf.items()), 'an input was modified'
        assert out.unwritten() == 0
        return out.view.clone()

    for p in RATES:
        thr, factor = ops.dropout_params(p)
        for step in STEPS:
            step_t = _step_tensor(step)
            for site in SITES:
                args = (thr, factor, SEED, step_t, site)
                keep = DU.keep_mask(n, SEED, step, site, thr)
                what = 'n %d %s p %g step %d site %d' % (n, dtype, p, step, site)
                if p == 0.0:
                    assert keep.all() and factor == 1.0
                elif n >= 8192:
                    assert 0.5 * p < 1.0 - keep.mean() < 1.5 * p, what
                # ---- dropout, dropout_add: bit for bit
                got = run(ops.dropout, 'x', args=args)
                assert torch.equal(_bits(got), _bits(_as(DU.dropout(np32['x'], keep, factor, bf16), dtype))), what
                assert torch.equal(_bits(run(ops.dropout, 'x', args=args)), _bits(got)), what + ': not repeatable'
                got = run(ops.dropout_add, 'x', 'res', args=args)
                want = DU.dropout_add(np32['x'], np32['res'], keep, factor, bf16)
                assert torch.equal(_bits(got), _bits(_as(want, dtype))), what
                # ---- the GELU launches against gelu -> dropout and dropout -> gelu_bwd
                fused = run(ops.gelu_dropout_fwd, 'x', args=args)
                comp = ops.dropout(ops.gelu_fwd(buf['x'].view), *args)
                fused_b = run(ops.gelu_dropout_bwd, 'dy', 'x', args=args)
                comp_b = ops.gelu_bwd(ops.dropout(buf['dy'].view, *args), buf['x'].view)
                for f, c, name in ((fused, comp, 'fwd'), (fused_b, comp_b, 'bwd')):
                    if not bf16:
                        assert torch.equal(_bits(f), _bits(c)), what + ' gelu ' + name
                        continue
                    a, b = f.float().cpu().numpy(), c.float().cpu().numpy()
                    assert np.array_equal(a == 0, b == 0), what + ' gelu %s: zero pattern' % name
                    assert np.all(np.abs(a.astype(np.float64) - b) <= _bf16_ulp(a, b)), what + ' gelu ' + name
                # the mask really is the restatement's (the composition shares the kernel's mask code)
                # a kept element is zero only where the GELU itself is (-0, or 1 + erff(x) = 0 far on the left)
                gelu_zero = ops.gelu_fwd(buf['x'].view).float().cpu().numpy() == 0
                assert np.array_equal(fused.float().cpu().numpy() == 0, ~keep | gelu_zero), what
                # against the float64 GELU: the cdf 0.5 (1 + erf) carries a few ulp of 1.0 (4e-7) as an ABSOLUTE error
                # (1 + erf cancels for negative x), scaled by what multiplies it; plus one rounding of the result
                tol = 2.0 ** -8 if bf16 else 2.0 ** -22
                ref = DU.gelu_dropout_fwd(np32['x'], keep, factor)
                slack = 4e-7 * (1.0 + np.abs(np32['x'])) * factor
                assert np.all(np.abs(fused.float().cpu().numpy() - ref) <= tol * np.abs(ref) + slack), what
                ref = DU.gelu_dropout_bwd(np32['dy'], np32['x'], keep, factor)
                slack = 4e-7 * (1.0 + np.abs(np32['x'])) * np.abs(np32['dy']) * factor + 1e-30
                assert np.all(np.abs(fused_b.float().cpu().numpy() - ref) <= tol * np.abs(ref) + slack), what


def test_advance_and_repeatability():
    """advance leaves step + 1 (the carry into the high word included); launches read the counter: the same arguments
    draw another mask after an advance and the same mask without one."""
    from passl_amd.hip import ops
    n, (thr, factor) = 8 * 1025, ops.dropout_params(0.5)
    x = torch.ones(n, device=DEV)
    for step0 in (0, (1 << 32) - 1, (1 << 63) - 1):
        step_t = _step_tensor(step0)
        a = ops.dropout(x, thr, factor, SEED, step_t, 3)
        b = ops.dropout(x, thr, factor, SEED, step_t, 3)
        ops.dropout_advance(step_t)
        c = ops.dropout(x, thr, factor, SEED, step_t, 3)
        assert (int(step_t.item()) & ((1 << 64) - 1)) == step0 + 1
        assert torch.equal(a, b) and not torch.equal(a, c)
        keep = DU.keep_mask(n, SEED, step0 + 1, 3, thr)
        assert np.array_equal(c.cpu().numpy() != 0, keep)
        assert set(np.unique(c.cpu().numpy())) == {0.0, 2.0}


# ---------------------------------------------------------------------------------------------- ViTCELoss kernels
@pytest.mark.parametrize('eps', [None, 1e-4])
@pytest.mark.parametrize('N,Cc', [(3, 5), (2, 1000), (2, 1001)])
def test_sigmoid_ce_kernels(N, Cc, eps):
    """Against float64 on logits that include +-40: the loss of every row within (C + 8) 2^-24 sum|term| (C fp32
    additions plus a few ulp per term), every gradient element within 8 2^-24 (sigmoid(x) + t) / N."""
    import os
    from passl_amd.hip import ops
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vit_sup_small.npz'))
    x = z['loss/x_%dx%d' % (N, Cc)].astype(np.float32)
    y = z['loss/y_%dx%d' % (N, Cc)]
    assert x.max() == 40.0 and x.min() == -40.0
    t_on, t_off = ops.sigmoid_ce_targets(eps)
    terms, rows, loss, dx, sig, t = DU.vit_ce(x.astype(np.float64), y, eps, targets=(t_on, t_off))
    xs = Guarded(N * Cc, torch.float32, fill=torch.from_numpy(x))
    before = xs.raw()
    labels = torch.from_numpy(y).to(DEV)
    rows_g, ds_g = Guarded(N, torch.float32), Guarded(N * Cc, torch.float32)
    scores = xs.view.view(N, Cc)
    out = ops.sigmoid_ce_fwd(scores, labels, t_on, t_off, rows=rows_g.view)
    g = torch.ones(1, device=DEV)
    ops.sigmoid_ce_bwd(scores, labels, g, t_on, t_off, out=ds_g.view.view(N, Cc))
    torch.cuda.synchronize()
    assert xs.intact() and rows_g.intact() and ds_g.intact() and torch.equal(xs.raw(), before)
    assert rows_g.unwritten() == 0 and ds_g.unwritten() == 0
    bound = (Cc + 8) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    got_rows = rows_g.view.cpu().numpy().astype(np.float64) * N
    print('rows: err / bound', np.abs(got_rows - rows) / bound)
    assert np.all(np.abs(got_rows - rows) <= bound)
    # the mean: the rows' errors, and N more additions
    assert abs(float(out.item()) - loss) <= bound.sum() / N + (N + 1) * 2.0 ** -24 * np.abs(rows).sum() / N
    got = ds_g.view.cpu().numpy().astype(np.float64).reshape(N, Cc)
    gbound = 8 * 2.0 ** -24 * (sig + t) / N
    print('grad: max err / bound', (np.abs(got - dx) / gbound).max())
    assert np.all(np.abs(got - dx) <= gbound)
    # the autograd node and the layer give the same numbers
    from passl_amd.loss import ViTCELoss
    xr = scores.clone().requires_grad_(True)
    val = ViTCELoss(epsilon=eps)({'logits': xr}, labels)['ViTCELoss']
    val.backward()
    assert val.shape == () and torch.equal(val.detach().reshape(1), out)
    assert torch.equal(xr.grad, ds_g.view.view(N, Cc))
