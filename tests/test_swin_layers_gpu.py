"""PatchMerging's gather (passl_hip_patch_merge / _bwd, csrc/window_attention.hip) against the numpy gather of the
reference (passl/models/swin_transformer.py:343-384: x0, x1, x2, x3 concatenated), bit for bit in both dtypes, on
guarded buffers."""
import numpy as np
import pytest
import torch

from guarded import Guarded

pytestmark = pytest.mark.gpu

from passl_amd.hip import lib as L             # noqa: E402

SHAPES = ((1, 2, 2, 8), (2, 4, 6, 24), (1, 6, 2, 136))


def numpy_merge(x):
    """x [B, H, W, C] -> [B, H/2, W/2, 4C] as the reference slices it."""
    return np.concatenate([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], axis=-1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_patch_merge_is_the_numpy_gather_bit_for_bit(shape, dtype):
    B, H, W, C = shape
    lib = L.load()
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, H, W, C, generator=gen).to(dtype)
    dy = torch.randn(B, H // 2, W // 2, 4 * C, generator=gen).to(dtype)
    gx, gdy = Guarded(x.numel(), dtype, fill=x), Guarded(dy.numel(), dtype, fill=dy)
    gy, gdx = Guarded(dy.numel(), dtype), Guarded(x.numel(), dtype)
    assert lib.passl_hip_patch_merge(gx.view.data_ptr(), gy.view.data_ptr(), B, H, W, C, L.dt(dtype), L.stream()) == 0
    assert lib.passl_hip_patch_merge_bwd(gdy.view.data_ptr(), gdx.view.data_ptr(), B, H, W, C, L.dt(dtype),
                                         L.stream()) == 0
    torch.cuda.synchronize()
    for n, g in (('x', gx), ('dy', gdy), ('y', gy), ('dx', gdx)):
        assert g.intact(), 'a guard region of %s was written' % n
    assert gy.unwritten() == 0 and gdx.unwritten() == 0
    assert np.array_equal(bits(gy.view).reshape(B, H // 2, W // 2, 4 * C), numpy_merge(bits(x)))
    # the backward is the inverse copy: merging dx gives dy back
    assert np.array_equal(numpy_merge(bits(gdx.view).reshape(B, H, W, C)), bits(dy))
    assert np.array_equal(bits(gx.view), bits(x).reshape(-1)) and np.array_equal(bits(gdy.view), bits(dy).reshape(-1))


def test_patch_merge_autograd():
    from passl_amd.hip import nn as hnn
    B, H, W, C = 2, 4, 6, 24
    x = torch.randn(B * H * W, C, device='cuda', requires_grad=True)
    y = hnn.patch_merge(x, B, H, W)
    assert y.shape == (B * (H // 2) * (W // 2), 4 * C)
    g = torch.randn_like(y)
    y.backward(g)
    want = numpy_merge(x.detach().cpu().numpy().reshape(B, H, W, C)).reshape(y.shape)
    assert np.array_equal(y.detach().cpu().numpy(), want)
    assert np.array_equal(numpy_merge(x.grad.cpu().numpy().reshape(B, H, W, C)).reshape(y.shape), g.cpu().numpy())
