"""hip/nn.py's ConvNeXt layers through autograd on an EncoderArena: DepthwiseConv2D and layer_scale_add, with the
residual fork's gradient handed to the data-gradient kernel through a GradSlot or returned to autograd, against a
float64 torch evaluation of `x + keep * ((gamma * dwconv(x)) / keep_prob)` on the same (dtype-rounded) inputs.

Tolerances, relative to each tensor's own maximum: fp32 1e-3 (the project's fp32 bound).  bf16 2^-6: the output and
every gradient pass through at most three bf16 roundings of 2^-8 each (y, dbranch, dx), and the parameter gradients
sum products of such values with independent errors."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config          # noqa: E402
from passl_amd.hip import nn                            # noqa: E402

DEV = 'cuda'
TOL = {torch.float32: 1e-3, torch.bfloat16: 2.0 ** -6}
KEEP_PROB = 0.75


class Tail(nn.Layer):
    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.DepthwiseConv2D(dim)
        self.gamma = torch.nn.Parameter(torch.ones(dim, device=hip_config.get_device()))


def reference(x, w, b, gamma, keep, gout, T):
    x = x.double().requires_grad_()
    w, b, gamma = (t.double().requires_grad_() for t in (w, b, gamma))
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=w.shape[0]).permute(0, 2, 3, 1)
    t = gamma * y
    if keep is not None:
        t = t / KEEP_PROB * keep.double().view(-1, 1, 1, 1)
    out = x + t
    out.backward(gout.double())
    return out.detach(), x.grad, w.grad, b.grad, gamma.grad


@pytest.mark.parametrize('slot', (False, True), ids=('autograd-add', 'grad-slot'))
@pytest.mark.parametrize('table', (False, True), ids=('nokeep', 'table'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=('fp32', 'bf16'))
def test_block_tail_matches_float64(dtype, table, slot):
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    N, H, W, C = 3, 9, 20, 40
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, H, W, C, generator=gen).to(dtype).float()
    gout = torch.randn(N, H, W, C, generator=gen).to(dtype).float()
    w = torch.randn(C, 1, 7, 7, generator=gen) * 0.2
    b = torch.randn(C, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    keep = torch.tensor([1.0, 0.0, 1.0]) if table else None

    m = Tail(C)
    arena = nn.EncoderArena(m, trainable=True)
    missing, unexpected = m.load_state_dict({'dwconv.weight': w, 'dwconv.bias': b, 'gamma': gamma}, strict=False)
    assert not missing and not unexpected
    arena.refresh()
    assert m.dwconv.weight.shape == (C, 1, 7, 7) and m.dwconv.weight.is_contiguous()
    xd = x.to(DEV).to(dtype).requires_grad_()
    res_slot = nn.GradSlot() if slot else None
    y = m.dwconv(xd, add_slot=res_slot)
    out = nn.layer_scale_add(y.view(-1, C), xd.view(-1, C), m.gamma, keep.to(DEV) if table else None,
                             KEEP_PROB, N, H * W, res_slot=res_slot)
    out.backward(gout.to(DEV).to(dtype).view(-1, C))
    torch.cuda.synchronize()

    r_out, r_dx, r_dw, r_db, r_dg = reference(x, w, b, gamma, keep, gout, H * W)
    got = dict(out=out.detach().view(N, H, W, C), dx=xd.grad, dw=m.dwconv.weight.grad, dbias=m.dwconv.bias.grad,
               dgamma=m.gamma.grad)
    want = dict(out=r_out, dx=r_dx, dw=r_dw, dbias=r_db, dgamma=r_dg)
    for name in got:
        g, r = got[name].detach().double().cpu(), want[name]
        err = float((g - r).abs().max() / r.abs().max())
        print('FIG layers %s %s %.3e' % (name, dtype, err))
        assert err <= TOL[dtype], '%s: max error %.3e of the maximum' % (name, err)
    if slot:
        assert not res_slot.armed and res_slot.grad is None
