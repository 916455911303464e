"""The streaming unary activations (csrc/eltwise.h: GELU, tanh, QuickGELU) at the sizes where the tile form takes
another path: one chunk (255 lanes clamped to it), exactly one 4 x 256-chunk tile, one chunk into a second workgroup,
one chunk into a fifth.  The entry points are called directly with an output buffer that is longer than n, so a store
past the end is seen; the ops wrappers and the autograd path are held to the direct call bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402
from passl_amd.hip import nn as hnn            # noqa: E402
from passl_amd.hip import ops                  # noqa: E402

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
SIZES = [8, 8 * 1024, 8 * 1025, 8 * 4097]
TAIL = 64
SENTINEL = -12352.0                            # exact in bf16

# name -> (float64 reference, autograd path of passl_amd.hip.nn)
ACTS = {
    'gelu': (F.gelu, hnn.gelu),
    'tanh': (torch.tanh, lambda x: hnn.Tanh()(x)),
    'quick_gelu': (lambda x: x * torch.sigmoid(1.702 * x), lambda x: hnn.QuickGELU()(x)),
}


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def case(name, dtype, n):
    """x, dy on the device in `dtype`; y, dx of the float64 evaluation on the same (rounded) values."""
    gen = torch.Generator().manual_seed(n)
    x = (torch.randn(n, generator=gen) * 2).to(dtype).double().requires_grad_(True)
    dy = torch.randn(n, generator=gen).to(dtype).double()
    y = ACTS[name][0](x)
    y.backward(dy)
    return x.detach().to(DEV).to(dtype), dy.to(DEV).to(dtype), y.detach(), x.grad


def direct(entry, n, dtype, *inputs):
    """The library entry itself, writing into the head of a sentinel-filled buffer of n + TAIL elements."""
    out = torch.full((n + TAIL,), SENTINEL, dtype=dtype, device=DEV)
    fn = getattr(L.load(), 'passl_hip_' + entry)
    L.check(fn(*[L.ptr(t) for t in inputs], L.ptr(out), n, L.dt(dtype), L.stream()), entry)
    return out


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(ACTS))
def test_unary_sizes(name, dtype, n):
    x, dy, y_ref, dx_ref = case(name, dtype, n)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    untouched = bits(torch.full((TAIL,), SENTINEL, dtype=dtype, device=DEV))
    for entry, inputs, ref, wrapped in ((name + '_fwd', (x,), y_ref, getattr(ops, name + '_fwd')(x)),
                                        (name + '_bwd', (dy, x), dx_ref, getattr(ops, name + '_bwd')(dy, x))):
        out = direct(entry, n, dtype, *inputs)
        err = relmax(out[:n].float(), ref)
        print('%s %s n=%d relmax %.3g' % (entry, dtype, n, err))
        assert err < tol, entry
        assert torch.equal(bits(out[n:]), untouched), entry + ' wrote past n'
        assert torch.equal(wrapped, out[:n]), entry


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(ACTS))
def test_unary_autograd_noncontiguous(name, dtype):
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(40, 24, generator=gen) * 2).to(DEV).to(dtype).t().requires_grad_(True)     # [24, 40], strides (1, 24)
    dy = torch.randn(40, 24, generator=gen).to(DEV).to(dtype).t()
    assert not x.is_contiguous() and not dy.is_contiguous()
    y = ACTS[name][1](x)
    assert torch.equal(y, getattr(ops, name + '_fwd')(x.detach().contiguous()))
    y.backward(dy)
    assert torch.equal(x.grad, getattr(ops, name + '_bwd')(dy.contiguous(), x.detach().contiguous()))


@pytest.mark.parametrize('name', list(ACTS))
def test_unary_rejects_n_not_multiple_of_8(name):
    x = torch.zeros(12, device=DEV)
    with pytest.raises(L.PasslHipError):
        direct(name + '_fwd', 12, torch.float32, x)
    with pytest.raises(L.PasslHipError):
        direct(name + '_bwd', 12, torch.float32, x, x)
