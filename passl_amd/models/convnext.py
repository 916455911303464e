"""``passl.models.convnext`` — ConvNeXt on the MI355X HIP path.

Names, constructor arguments, sub-layer / state_dict keys and the factories are the reference's
(passl/models/convnext.py: LayerNorm :34-65, Block :68-103, ConvNeXt :106-204, factories :206-231), so its
``.pdparams`` load.  Activations are NHWC throughout, which removes what the reference spends on layout:

  * its two ``transpose`` calls per block and the hand-written ``channels_first`` LayerNorm collapse into the row
    LayerNorm (csrc/vit.hip) over [N*H*W, C];
  * ``pwconv1`` / ``pwconv2`` are ``hnn.Linear`` (implicit GEMM, bias epilogue), GELU the streaming kernel;
  * the 4x4/4 stem is ``passl_hip_patchify`` + a GEMM over 48-element rows (the construction of ``PatchEmbed``), the
    three 2x2/2 downsample convolutions ``hnn.PatchConv2D`` (implicit GEMM with the bias as its ``shift``);
  * ``dwconv`` is ``hnn.DepthwiseConv2D`` and the block's tail ``input + drop_path(gamma * x)`` one launch,
    ``hnn.layer_scale_add`` (csrc/dwconv.hip); the gradient of the residual fork is added inside the depthwise
    convolution's data-gradient launch (GradSlot);
  * global average pool, final LayerNorm and the fp32 head as in the other classifiers.

Stochastic depth: the ladder is ``linspace(0, drop_path_rate, sum(depths))`` in fp32 (:145-147) and
``keep_prob = float32(1 - p)``.  The keep table (``hnn.DropPathState``) is [blocks with p > 0, B]: one row per such
block, in network order.  Evaluation mode and rate 0 launch no draw and pass no table.

Initialisation (:163-170): trunc-normal(0.02) weights and zero biases for every convolution and Linear, LayerNorm
(1, 0), ``gamma`` = ``layer_scale_init_value``, the head scaled by ``head_init_scale``.

Refused by name: ``layer_scale_init_value <= 0`` (no recipe sets it: the block would have no ``gamma``), an input whose
height or width is not a multiple of 32, widths that are not multiples of 8."""
import numpy as np
import torch
import torch.nn as tnn

from ..hip import config, ops
from ..hip import nn as hnn
from ..hip.nn import EncoderArena
from ..modules.vit import _PatchProj, trunc_normal_
from ..utils.checkpoint import load_lenient, read_pdparams
from .base_model import Model

__all__ = ['ConvNeXt', 'convnext_tiny', 'convnext_small', 'convnext_base', 'convnext_large', 'convnext_xlarge']


class Block(hnn.Layer):
    """ConvNeXt block over NHWC: dwconv -> LayerNorm -> pwconv1 -> GELU -> pwconv2 -> input + drop_path(gamma * x)."""

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        if not layer_scale_init_value > 0:
            raise NotImplementedError('ConvNeXt Block(layer_scale_init_value=%r): a block without gamma is not built '
                                      '(no recipe sets it)' % (layer_scale_init_value,))
        drop_path = float(drop_path)
        if not 0. <= drop_path < 1.:
            raise ValueError('drop_path must be in [0, 1), got %r' % drop_path)
        self.drop_path = drop_path
        self.keep_prob = float(np.float32(1.0) - np.float32(drop_path))
        self.dwconv = hnn.DepthwiseConv2D(dim, kernel_size=7, padding=3)
        self.norm = hnn.LayerNorm(dim, epsilon=1e-6)
        self.pwconv1 = hnn.Linear(dim, 4 * dim)
        self.pwconv2 = hnn.Linear(4 * dim, dim)
        self.gamma = tnn.Parameter(torch.full((dim,), float(layer_scale_init_value), device=config.get_device()))
        self._slot = hnn.GradSlot()

    def forward(self, x, keep_row=None):
        """x: [N, H, W, C]; keep_row: this block's row [N] of the keep table, or None (nothing can drop)."""
        N, H, W, C = x.shape
        if self.drop_path > 0. and self.training and keep_row is None:
            raise RuntimeError('Block(drop_path=%g) in training mode needs its row of the keep table' % self.drop_path)
        slot = self._slot if (torch.is_grad_enabled() and x.requires_grad) else None
        h = self.dwconv(x, add_slot=slot).view(N * H * W, C)
        h = self.pwconv2(hnn.gelu(self.pwconv1(self.norm(h))))
        out = hnn.layer_scale_add(h, x.view(N * H * W, C), self.gamma, keep_row, self.keep_prob, N, H * W,
                                  res_slot=slot)
        return out.view(N, H, W, C)


class ConvNeXt(hnn.DropPathModel, Model):
    """ConvNeXt (A ConvNet for the 2020s, https://arxiv.org/pdf/2201.03545.pdf)."""

    def __init__(self, in_chans=3, class_num=1000, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.,
                 layer_scale_init_value=1e-6, head_init_scale=1.):
        super().__init__()
        depths, dims = list(depths), list(dims)
        if len(depths) != 4 or len(dims) != 4:
            raise ValueError('ConvNeXt has four stages: depths %r, dims %r' % (depths, dims))
        if any(d <= 0 or d % 8 for d in dims):
            raise NotImplementedError('ConvNeXt(dims=%r): every width must be a multiple of 8 (16-byte rows of the HIP '
                                      'kernels)' % (dims,))
        if not layer_scale_init_value > 0:
            raise NotImplementedError('ConvNeXt(layer_scale_init_value=%r): blocks without gamma are not built (no '
                                      'recipe sets it)' % (layer_scale_init_value,))
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        self.in_chans, self.class_num, self.depths, self.dims = in_chans, class_num, depths, dims
        self.drop_path_rate = float(drop_path_rate)
        norm = lambda d: hnn.LayerNorm(d, epsilon=1e-6)            # noqa: E731
        # downsample_layers.0 = (4x4/4 convolution, LayerNorm); .i = (LayerNorm, 2x2/2 convolution)
        self.downsample_layers = tnn.ModuleList([tnn.ModuleList([_PatchProj(in_chans, dims[0], 4), norm(dims[0])])])
        for i in range(3):
            self.downsample_layers.append(tnn.ModuleList([norm(dims[i]), hnn.PatchConv2D(dims[i], dims[i + 1], 2, 2)]))
        # dp_rates = [x.item() for x in paddle.linspace(0, drop_path_rate, sum(depths))]: a float32 ladder
        self.dp_rates = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths), dtype=torch.float32)]
        self.stages = tnn.ModuleList()
        cur = 0
        for i in range(4):
            self.stages.append(tnn.ModuleList([Block(dims[i], self.dp_rates[cur + j], layer_scale_init_value)
                                               for j in range(depths[i])]))
            cur += depths[i]
        self.norm = norm(dims[-1])
        self.head = hnn.Linear(dims[-1], class_num)
        self.pool = hnn.AdaptiveAvgPool2D(1)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (hnn.Linear, hnn.PatchConv2D, hnn.DepthwiseConv2D, _PatchProj)):
                    trunc_normal_(m.weight, std=.02)
                    m.bias.zero_()
            self.head.weight.mul_(head_init_scale)
            self.head.bias.mul_(head_init_scale)
        # stochastic depth: one row of the keep table per block with p > 0; the seed is drawn after the weights (a model
        # with stochastic depth initialises as one without)
        self._seed_drop_path([blk for stage in self.stages for blk in stage if blk.drop_path > 0.], 1)
        self.arena_q = EncoderArena(self, trainable=True)

    def load_pretrained(self, path, rank=0, finetune=False):
        sd = read_pdparams(path)
        if not finetune:                               # convnext.py:198-199
            load_lenient(self, sd, what='pretrained ConvNeXt')
            self.sync_runtime_state()

    # ---- forward
    @staticmethod
    def _check_input(x):
        B, _cin, H, W = x.shape
        if H % 32 or W % 32:
            raise NotImplementedError('ConvNeXt: input %d x %d is not a multiple of 32 in both directions (4x4/4 stem and '
                                      'three 2x2/2 downsample layers)' % (H, W))
        return B, H, W

    def forward_features(self, x, drop_path_keep=None):
        B, H, W = self._check_input(x)
        keep = self._drop_path_keep(B, x.device, drop_path_keep)
        stem, stem_norm = self.downsample_layers[0]
        dtype = hnn._need_rt(stem).arena.dtype
        rows = stem_norm(stem(ops.patchify(x.contiguous().float(), 4, dtype)))
        h, w = H // 4, W // 4
        x = rows.view(B, h, w, self.dims[0])
        for i in range(4):
            if i > 0:
                norm, conv = self.downsample_layers[i]
                x = conv(norm(x.view(B * h * w, self.dims[i - 1])).view(B, h, w, self.dims[i - 1]))
                h, w = h // 2, w // 2
            for blk in self.stages[i]:
                x = blk(x, self._drop_path_rows(keep, blk))
        return self.norm(self.pool(x))                  # global average pooling, [N, H, W, C] -> [N, C]

    def forward(self, x, drop_path_keep=None):
        self._check_input(x)
        self.arena_q.refresh()                       # compute-dtype operands and data-gradient packs of the updated weights
        return self.head(self.forward_features(x, drop_path_keep), out_f32=True)


def convnext_tiny(**kwargs):
    return ConvNeXt(depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], **kwargs)


def convnext_small(**kwargs):
    return ConvNeXt(depths=[3, 3, 27, 3], dims=[96, 192, 384, 768], **kwargs)


def convnext_base(**kwargs):
    return ConvNeXt(depths=[3, 3, 27, 3], dims=[128, 256, 512, 1024], **kwargs)


def convnext_large(**kwargs):
    return ConvNeXt(depths=[3, 3, 27, 3], dims=[192, 384, 768, 1536], **kwargs)


def convnext_xlarge(**kwargs):
    return ConvNeXt(depths=[3, 3, 27, 3], dims=[256, 512, 1024, 2048], **kwargs)
