"""``passl.models.swin_transformer`` — Swin Transformer on the MI355X HIP path.

Names, constructor arguments, sub-layer / state_dict keys (the ``relative_position_index`` and ``attn_mask`` buffers
included) and the thirteen factories are the reference's (passl/models/swin_transformer.py: WindowAttention :112-200,
SwinTransformerBlock :203-340, PatchMerging :343-384, BasicLayer :387-459, SwinTransformer :462-645, factories
:648-824), so its ``.pdparams`` load.  Activations are token rows [B*L, C] of the UNSHIFTED, UNPARTITIONED map from the
patch embedding to the pool:

  * the block's ``roll`` / ``window_partition`` / ``window_reverse`` / ``roll`` back, the ``relative_position_index``
    gather and the -100 ``attn_mask`` are address arithmetic inside ``hnn.window_attention``
    (csrc/window_attention.hip): qkv is the projection of the rows as they lie, the attention output comes back in
    the same order.  The two buffers exist for the state_dict; the kernels read neither;
  * ``PatchMerging`` is ``hnn.patch_merge`` (one streaming gather) + ``hnn.LayerNorm(4C)`` + a bias-free ``hnn.Linear``;
  * ``patch_embed`` is the patchify + GEMM of the ViTs plus its LayerNorm; ``qkv`` / ``proj`` / ``fc1`` / ``fc2`` are
    ``hnn.Linear`` (the residual add of a block without stochastic depth runs in the epilogue of ``proj`` / ``fc2``),
    GELU the streaming kernel; ``x.mean(axis=1)`` is the average pool over [B, H, W, C]; the head works on fp32 rows.

The block's window rule is the reference's: ``min(input_resolution) <= window_size`` gives window
``min(input_resolution)`` and shift 0; shifts alternate 0, ``window_size // 2``.

Stochastic depth: the ladder is ``np.linspace(0, drop_path_rate, sum(depths))`` (:537) and ``keep_prob =
float32(1 - p)``.  The reference draws once per residual, so a block owns TWO rows of the keep table
(``hnn.DropPathState``): the table is [2 x blocks with p > 0, B], rows 2k, 2k + 1 the attention and the MLP residual of
the k-th such block.  Evaluation mode and rate 0 launch no draw.

Initialisation (:565-577): trunc-normal(0.02) Linear weights and bias tables, zero biases, LayerNorm (1, 0); the patch
convolution keeps Paddle's default (Normal(0, sqrt(2 / fan_in)), zero bias).

Refused by name: ``drop_rate > 0``, ``attn_drop_rate > 0`` and ``ape=True`` (no config or factory sets them), a head
dimension outside {32, 64}, a window above 14, a resolution that is not a multiple of its window, an odd resolution at
a merge, widths that are not multiples of 8."""
import numpy as np
import torch
import torch.nn as tnn

from ..hip import config, ops
from ..hip import nn as hnn
from ..hip.nn import EncoderArena
from ..modules.vit import Mlp, PatchEmbed, conv_default_normal_, to_2tuple, trunc_normal_
from ..utils.checkpoint import load_lenient, read_pdparams
from .base_model import ClassifierModel

__all__ = [
    'SwinTransformer',
    'swin_base_patch4_window12_384', 'swin_base_patch4_window7_224', 'swin_large_patch4_window12_384',
    'swin_large_patch4_window7_224', 'swin_small_patch4_window7_224', 'swin_tiny_patch4_window7_224',
    'swin_base_patch4_window12_384_in22k', 'swin_base_patch4_window7_224_in22k',
    'swin_large_patch4_window12_384_in22k', 'swin_large_patch4_window7_224_in22k',
    'swin_s3_tiny_224', 'swin_s3_small_224', 'swin_s3_base_224',
]


def to_ntuple(n):
    def parse(x):
        if isinstance(x, (tuple, list)):
            return tuple(x)
        return (x,) * n
    return parse


def get_relative_position_index(win_h, win_w):
    """[Wh*Ww, Wh*Ww] int64: (iy - jy + Wh - 1)(2 Ww - 1) + (ix - jx + Ww - 1)."""
    coords = torch.stack(torch.meshgrid(torch.arange(win_h), torch.arange(win_w), indexing='ij')).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += win_h - 1
    rel[:, :, 1] += win_w - 1
    rel[:, :, 0] *= 2 * win_w - 1
    return rel.sum(-1)


def shifted_window_mask(H, W, window_size, shift_size):
    """The reference's attn_mask [nW, T, T] fp32 of 0 / -100 (:265-285)."""
    img = torch.zeros(1, H, W, 1)
    cnt = 0
    for h in (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None)):
        for w in (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    win = img.reshape(1, H // window_size, window_size, W // window_size, window_size, 1)
    win = win.permute(0, 1, 3, 2, 4, 5).reshape(-1, window_size * window_size)
    diff = win.unsqueeze(1) - win.unsqueeze(2)
    return -100.0 * (diff != 0).float()


class WindowAttention(hnn.Layer):
    """Window based multi-head self attention with relative position bias, shifted or not.  ``forward`` takes the rows
    of the whole unshifted map and the geometry; there is no ``mask`` argument, the kernel forms it from the shift."""

    def __init__(self, dim, num_heads, head_dim=None, window_size=7, qkv_bias=True, attn_drop=0., proj_drop=0.):
        super().__init__()
        if attn_drop != 0. or proj_drop != 0.:
            raise NotImplementedError('WindowAttention(attn_drop=%r, proj_drop=%r): dropout is not built for Swin (no '
                                      'config or factory sets it)' % (attn_drop, proj_drop))
        self.dim = dim
        self.window_size = to_2tuple(window_size)
        win_h, win_w = self.window_size
        if win_h != win_w:
            raise NotImplementedError('WindowAttention: window %r is not square' % (self.window_size,))
        if win_h > ops.WINDOW_ATTENTION_MAX_WINDOW:
            raise NotImplementedError('WindowAttention: window_size %d is above %d, the largest window of the HIP kernels'
                                      % (win_h, ops.WINDOW_ATTENTION_MAX_WINDOW))
        self.window_area = win_h * win_w
        self.num_heads = num_heads
        head_dim = head_dim or dim // num_heads
        if head_dim not in ops.ATTENTION_HEAD_DIMS:
            raise NotImplementedError('WindowAttention: head dimension %d is not one of %s (the HIP kernels)'
                                      % (head_dim, sorted(ops.ATTENTION_HEAD_DIMS)))
        self.head_dim = head_dim
        attn_dim = head_dim * num_heads
        self.scale = head_dim ** -0.5
        dev = config.get_device()
        self.relative_position_bias_table = tnn.Parameter(
            torch.zeros((2 * win_h - 1) * (2 * win_w - 1), num_heads, device=dev))
        self.register_buffer('relative_position_index', get_relative_position_index(win_h, win_w).to(dev))
        self.qkv = hnn.Linear(dim, attn_dim * 3, bias_attr=None if qkv_bias else False)
        self.proj = hnn.Linear(attn_dim, dim)

    def forward(self, x, B, H, W, shift, residual=None):
        a = hnn.window_attention(self.qkv(x), self.relative_position_bias_table, B, H, W, self.window_size[0], shift,
                                 self.num_heads, self.head_dim, self.scale)
        return self.proj(a, residual=residual)


class SwinTransformerBlock(hnn.Layer):
    """x + drop_path(attn(norm1(x))), then x + drop_path(mlp(norm2(x))), over rows [B*H*W, C]."""

    def __init__(self, dim, input_resolution, num_heads=4, head_dim=None, window_size=7, shift_size=0, mlp_ratio=4.,
                 qkv_bias=True, drop=0., attn_drop=0., drop_path=0., act_layer=hnn.GELU, norm_layer=hnn.LayerNorm):
        super().__init__()
        if drop != 0.:
            raise NotImplementedError('SwinTransformerBlock(drop=%r): dropout is not built for Swin (no config or '
                                      'factory sets it)' % (drop,))
        self.dim = dim
        self.input_resolution = tuple(input_resolution)
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        if min(self.input_resolution) <= self.window_size:
            # a window as large as the map: no partition, no shift
            self.shift_size = 0
            self.window_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.window_size, 'shift_size must in 0-window_size'
        H, W = self.input_resolution
        if H % self.window_size or W % self.window_size:
            raise NotImplementedError('SwinTransformerBlock: resolution %d x %d is not a multiple of the window %d'
                                      % (H, W, self.window_size))
        drop_path = float(drop_path)
        if not 0. <= drop_path < 1.:
            raise ValueError('drop_path must be in [0, 1), got %r' % drop_path)
        self.drop_path = drop_path
        self.keep_prob = float(np.float32(1.0 - drop_path))       # paddle.to_tensor(1 - drop_prob, dtype=float32)
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, num_heads=num_heads, head_dim=head_dim, window_size=to_2tuple(self.window_size),
                                    qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        mask = None
        if self.shift_size > 0:
            mask = shifted_window_mask(H, W, self.window_size, self.shift_size).to(config.get_device())
        self.register_buffer('attn_mask', mask)

    def forward(self, x, B, keep=None):
        """x: [B*H*W, C]; keep: this block's two rows [2, B] of the keep table, or None (nothing can drop)."""
        H, W = self.input_resolution
        if x.shape[0] != B * H * W:
            raise ValueError('input feature has wrong size: %d rows for batch %d of %d x %d' % (x.shape[0], B, H, W))
        if self.drop_path > 0. and self.training:
            if keep is None:
                raise RuntimeError('SwinTransformerBlock(drop_path=%g) in training mode needs its two rows of the keep '
                                   'table' % self.drop_path)
            h, xr = self.norm1.fork(x)
            x = hnn.drop_path_add(self.attn(h, B, H, W, self.shift_size), xr, keep[0], self.keep_prob, B, H * W)
            h, xr = self.norm2.fork(x)
            return hnn.drop_path_add(self.mlp(h), xr, keep[1], self.keep_prob, B, H * W)
        h, xr = self.norm1.fork(x)
        x = self.attn(h, B, H, W, self.shift_size, residual=xr)
        h, xr = self.norm2.fork(x)
        return self.mlp(h, residual=xr)


class PatchMerging(hnn.Layer):
    """[B*H*W, C] -> [B*(H/2)*(W/2), out_dim]: gather of four neighbours, LayerNorm(4C), bias-free Linear."""

    def __init__(self, input_resolution, dim, out_dim=None, norm_layer=hnn.LayerNorm):
        super().__init__()
        self.input_resolution = tuple(input_resolution)
        H, W = self.input_resolution
        if H % 2 or W % 2:
            raise NotImplementedError('PatchMerging: x size (%d*%d) are not even.' % (H, W))
        if dim % 8:
            raise NotImplementedError('PatchMerging: dim %d is not a multiple of 8 (16-byte rows of the HIP kernels)' % dim)
        self.dim = dim
        self.out_dim = out_dim or 2 * dim
        self.norm = norm_layer(4 * dim)
        self.reduction = hnn.Linear(4 * dim, self.out_dim, bias_attr=False)

    def forward(self, x, B):
        H, W = self.input_resolution
        if x.shape[0] != B * H * W:
            raise ValueError('input feature has wrong size: %d rows for batch %d of %d x %d' % (x.shape[0], B, H, W))
        return self.reduction(self.norm(hnn.patch_merge(x, B, H, W)))


class BasicLayer(hnn.Layer):
    """One stage: ``depth`` blocks with shifts 0, window_size // 2, 0, ... and an optional PatchMerging."""

    def __init__(self, dim, out_dim, input_resolution, depth, num_heads=4, head_dim=None, window_size=7, mlp_ratio=4.,
                 qkv_bias=True, drop=0., attn_drop=0., drop_path=0., norm_layer=hnn.LayerNorm, downsample=None):
        super().__init__()
        self.dim = dim
        self.input_resolution = tuple(input_resolution)
        self.depth = depth
        self.blocks = tnn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, head_dim=head_dim,
                                 window_size=window_size, shift_size=0 if (i % 2 == 0) else window_size // 2,
                                 mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer) for i in range(depth)])
        self.downsample = None
        if downsample is not None:
            self.downsample = downsample(input_resolution, dim=dim, out_dim=out_dim, norm_layer=norm_layer)


class SwinTransformer(hnn.DropPathModel, ClassifierModel):
    """Swin Transformer: Hierarchical Vision Transformer using Shifted Windows, https://arxiv.org/pdf/2103.14030."""

    def __init__(self, img_size=224, patch_size=4, in_chans=3, num_classes=1000, global_pool='avg', embed_dim=96,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), head_dim=None, window_size=7, mlp_ratio=4.,
                 qkv_bias=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=hnn.LayerNorm, ape=False,
                 patch_norm=True, weight_init='', **kwargs):
        super().__init__()
        assert global_pool in self.GLOBAL_POOLS
        if drop_rate != 0. or attn_drop_rate != 0.:
            raise NotImplementedError('SwinTransformer(drop_rate=%r, attn_drop_rate=%r): dropout is not built for Swin '
                                      '(no config or factory sets it)' % (drop_rate, attn_drop_rate))
        if ape:
            raise NotImplementedError('SwinTransformer(ape=True): the absolute position embedding is not built (no '
                                      'config or factory sets it)')
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        depths, num_heads = tuple(depths), tuple(num_heads)
        self.num_classes = num_classes
        self.global_pool = global_pool
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.num_features = int(embed_dim * 2 ** (self.num_layers - 1))
        self.drop_path_rate = float(drop_path_rate)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        self.patch_grid = self.patch_embed.grid_size
        self.absolute_pos_embed = None
        if not isinstance(embed_dim, (tuple, list)):
            embed_dim = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        if any(d <= 0 or d % 8 for d in embed_dim):
            raise NotImplementedError('SwinTransformer: every width of %r must be a multiple of 8 (16-byte rows of the HIP '
                                      'kernels)' % (list(embed_dim),))
        embed_out_dim = list(embed_dim[1:]) + [None]
        head_dim = to_ntuple(self.num_layers)(head_dim)
        window_size = to_ntuple(self.num_layers)(window_size)
        mlp_ratio = to_ntuple(self.num_layers)(mlp_ratio)
        dpr = np.linspace(0, drop_path_rate, sum(depths)).tolist()      # stochastic depth decay rule
        self.layers = tnn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(BasicLayer(
                dim=embed_dim[i], out_dim=embed_out_dim[i],
                input_resolution=(self.patch_grid[0] // (2 ** i), self.patch_grid[1] // (2 ** i)), depth=depths[i],
                num_heads=num_heads[i], head_dim=head_dim[i], window_size=window_size[i], mlp_ratio=mlp_ratio[i],
                qkv_bias=qkv_bias, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                downsample=PatchMerging if (i < self.num_layers - 1) else None))
        self.norm = norm_layer(self.num_features)
        self.head = hnn.Linear(self.num_features, num_classes) if num_classes > 0 else None
        self.pool = hnn.AdaptiveAvgPool2D(1)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, hnn.Linear):
                    trunc_normal_(m.weight, std=.02)
                    if m.bias is not None:
                        m.bias.zero_()
                elif isinstance(m, WindowAttention):
                    trunc_normal_(m.relative_position_bias_table, std=.02)
            conv_default_normal_(self.patch_embed.proj.weight)        # Paddle's default for nn.Conv2D
            self.patch_embed.proj.bias.zero_()
        # stochastic depth: two rows of the keep table per block with p > 0; the seed is drawn after the weights (a
        # model with stochastic depth initialises as one without)
        self._blocks = [blk for layer in self.layers for blk in layer.blocks]
        self._seed_drop_path([blk for blk in self._blocks if blk.drop_path > 0.], 2)
        self.arena_q = EncoderArena(self, trainable=True)

    def load_pretrained(self, path, rank=0, finetune=False):
        load_lenient(self, read_pdparams(path), what='pretrained Swin')        # swin_transformer.py:627-642
        self.sync_runtime_state()

    def no_weight_decay(self):
        nwd = {'absolute_pos_embed'}
        for n, _ in self.named_parameters():
            if 'relative_position_bias_table' in n:
                nwd.add(n)
        return nwd

    def group_matcher(self, coarse=False):
        return dict(
            stem=r'^absolute_pos_embed|patch_embed',  # stem and embed
            blocks=r'^layers\.(\d+)' if coarse else [
                (r'^layers\.(\d+).downsample', (0, )),
                (r'^layers\.(\d+)\.\w+\.(\d+)', None),
                (r'^norm', (99999, )),
            ])

    # ---- forward
    def forward_features(self, x, drop_path_keep=None):
        """-> the normalised rows [B*L, num_features] of the last stage."""
        B = x.shape[0]
        keep = self._drop_path_keep(B, x.device, drop_path_keep)
        x = self.patch_embed(x)
        for layer in self.layers:
            for blk in layer.blocks:
                x = blk(x, B, self._drop_path_rows(keep, blk))
            if layer.downsample is not None:
                x = layer.downsample(x, B)
        return self.norm(x)

    def forward_head(self, x, B, pre_logits=False):
        if self.global_pool == 'avg':
            H, W = self.layers[-1].input_resolution
            x = self.pool(x.view(B, H, W, self.num_features))          # x.mean(axis=1)
        return x if (pre_logits or self.head is None) else self.head(x, out_f32=True)

    def forward(self, x, drop_path_keep=None):
        self.arena_q.refresh()                       # compute-dtype operands and data-gradient packs of the updated weights
        return self.forward_head(self.forward_features(x, drop_path_keep), x.shape[0])


def swin_base_patch4_window12_384(**kwargs):
    return SwinTransformer(img_size=384, patch_size=4, window_size=12, embed_dim=128, depths=(2, 2, 18, 2),
                           num_heads=(4, 8, 16, 32), **kwargs)


def swin_base_patch4_window7_224(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=128, depths=(2, 2, 18, 2),
                           num_heads=(4, 8, 16, 32), **kwargs)


def swin_large_patch4_window12_384(**kwargs):
    return SwinTransformer(img_size=384, patch_size=4, window_size=12, embed_dim=192, depths=(2, 2, 18, 2),
                           num_heads=(6, 12, 24, 48), **kwargs)


def swin_large_patch4_window7_224(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=192, depths=(2, 2, 18, 2),
                           num_heads=(6, 12, 24, 48), **kwargs)


def swin_small_patch4_window7_224(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2, 18, 2),
                           num_heads=(3, 6, 12, 24), **kwargs)


def swin_tiny_patch4_window7_224(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2, 6, 2),
                           num_heads=(3, 6, 12, 24), **kwargs)


def swin_base_patch4_window12_384_in22k(**kwargs):
    return SwinTransformer(img_size=384, patch_size=4, window_size=12, embed_dim=128, depths=(2, 2, 18, 2),
                           num_heads=(4, 8, 16, 32), **kwargs)


def swin_base_patch4_window7_224_in22k(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=128, depths=(2, 2, 18, 2),
                           num_heads=(4, 8, 16, 32), **kwargs)


def swin_large_patch4_window12_384_in22k(**kwargs):
    return SwinTransformer(img_size=384, patch_size=4, window_size=12, embed_dim=192, depths=(2, 2, 18, 2),
                           num_heads=(6, 12, 24, 48), **kwargs)


def swin_large_patch4_window7_224_in22k(**kwargs):
    return SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=192, depths=(2, 2, 18, 2),
                           num_heads=(6, 12, 24, 48), **kwargs)


def swin_s3_tiny_224(**kwargs):
    return SwinTransformer(patch_size=4, window_size=(7, 7, 14, 7), embed_dim=96, depths=(2, 2, 6, 2),
                           num_heads=(3, 6, 12, 24), **kwargs)


def swin_s3_small_224(**kwargs):
    return SwinTransformer(patch_size=4, window_size=(14, 14, 14, 7), embed_dim=96, depths=(2, 2, 18, 2),
                           num_heads=(3, 6, 12, 24), **kwargs)


def swin_s3_base_224(**kwargs):
    return SwinTransformer(patch_size=4, window_size=(7, 7, 14, 7), embed_dim=96, depths=(2, 2, 30, 2),
                           num_heads=(3, 6, 12, 24), **kwargs)
