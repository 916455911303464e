"""hip/nn.py's ConvNeXt layers without a GPU: what DepthwiseConv2D refuses, by name, and how its parameters lie in an
EncoderArena (the reference's shapes, contiguous, 16-byte aligned: the kernels read them as they lie)."""
import pytest
import torch

from passl_amd.hip import config as hip_config
from passl_amd.hip import nn


def test_depthwise_conv_refuses_by_name():
    hip_config.set_device('cpu')
    with pytest.raises(NotImplementedError, match='kernel_size'):
        nn.DepthwiseConv2D(16, kernel_size=3, padding=1)
    with pytest.raises(NotImplementedError, match='padding'):
        nn.DepthwiseConv2D(16, kernel_size=7, padding=0)
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        nn.DepthwiseConv2D(12)


def test_depthwise_conv_parameters_in_an_arena():
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)

    class Two(nn.Layer):
        def __init__(self):
            super().__init__()
            self.a = nn.DepthwiseConv2D(8)
            self.b = nn.DepthwiseConv2D(24)

    m = Two()
    arena = nn.EncoderArena(m, trainable=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {'a.weight': (8, 1, 7, 7), 'a.bias': (8,), 'b.weight': (24, 1, 7, 7), 'b.bias': (24,)}
    for p in m.parameters():
        assert p.is_contiguous() and p.grad.is_contiguous() and p.grad.shape == p.shape
        assert (p.data_ptr() - arena.flat.data_ptr()) % 16 == 0
        assert (p.grad.data_ptr() - arena.grads.data_ptr()) % 16 == 0
    w = torch.arange(8 * 49, dtype=torch.float32).view(8, 1, 7, 7)
    m.load_state_dict({'a.weight': w}, strict=False)
    off = (m.a.weight.data_ptr() - arena.flat.data_ptr()) // 4
    assert torch.equal(arena.flat[off:off + 8 * 49], w.flatten())       # [C][49] as the reference stores it
