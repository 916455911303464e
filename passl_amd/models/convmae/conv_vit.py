"""``passl.models.convmae.conv_vit`` — ConvViT, the ConvMAE encoder as a classifier, on the MI355X HIP path.

Names, constructor arguments, sub-layer / state_dict keys and shapes and the factory are the reference's
(passl/models/convmae/conv_vit.py: CMlp :31-52, CBlock :55-99, CPatchEmbed :102-130, ConvViT :175-328,
convvit_base_patch16 :331-343), so its ``.pdparams`` load.  Activations of the two convolutional stages are NHWC, which
removes the reference's ``transpose`` pairs around every LayerNorm:

  * ``conv1`` / ``conv2`` / ``fc1`` / ``fc2`` are 1x1 convolutions = GEMMs over the rows [N*H*W, C]; their parameters
    keep the reference's ``[out, in, 1, 1]`` shape (``Conv1x1``), the residual add runs in the GEMM epilogue;
  * ``attn`` is ``hnn.MaskedDepthwiseConv2D`` (csrc/convmae.hip): depthwise 5x5 of ``mask * x`` with the mask expanded
    from the patch grid by address arithmetic; without a mask (this model) the same kernels with a NULL table;
  * ``patch_embed1.proj`` (4x4/4 on the 3-channel image) is ``passl_hip_patchify`` + a GEMM over 48-element rows,
    ``patch_embed2.proj`` / ``patch_embed3.proj`` (2x2/2) ``hnn.PatchConv2D``; each is followed by the row LayerNorm and
    the streaming GELU (a fused LayerNorm + GELU would save one pass over the map: not built);
  * stage 3 is the shared pre-norm ``Block`` over token rows [B*196, D] (no class token).

Two properties of the reference that are reproduced, not repaired:
  * ``CBlock`` and ``CPatchEmbed`` build ``nn.LayerNorm(dim)`` themselves: Paddle's default epsilon 1e-5, whatever
    ``norm_layer`` the factory passes (stage 3 and the final norm get its 1e-6);
  * without ``global_pool`` the model returns ``norm(x)[:, 0]``, the FIRST PATCH token (there is no class token).

Stochastic depth: the ladder is ``np.linspace(0, drop_path_rate, sum(depth))`` (float64, :229) and every block has two
residuals, each with a draw of its own: the keep table (``hnn.DropPathState``) is [2 * sum(depth), B], row 2i the first
residual of block i, row 2i + 1 its MLP residual.  Evaluation mode and rate 0 launch no draw.

Refused by name: ``drop_rate`` / ``attn_drop_rate`` other than 0, a ``hybrid_backbone``, widths that are not multiples
of 8, stage sizes that do not chain (img_size[i + 1] == img_size[i] / patch_size[i])."""
from functools import partial

import numpy as np
import torch
import torch.nn as tnn

from ...hip import config, ops
from ...hip import nn as hnn
from ...hip.nn import EncoderArena
from ...modules.vit import Block, ViTTrunk, _PatchProj, to_2tuple, trunc_normal_
from ...utils.checkpoint import load_lenient, read_pdparams
from ..base_model import Model

__all__ = ['CMlp', 'CBlock', 'CPatchEmbed', 'ConvViT', 'convvit_base_patch16']


class PatchRowsConv2D(_PatchProj):
    """paddle.nn.Conv2D(cin, cout, p, stride=p) applied to patches that are already GEMM rows [M, p*p*cin] in the column
    order (ph, pw, c) — what ``hnn.patch_gather`` writes for the kept patches.  ``weight`` is logically
    [cout, cin, p, p] and physically [cout][p][p][cin], as ``hnn.PatchConv2D``'s.  ``residual`` is added in the
    epilogue."""
    no_dgrad = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=None):
        if stride is not None and stride != kernel_size:
            raise NotImplementedError('PatchRowsConv2D: stride %r != kernel_size %r' % (stride, kernel_size))
        if in_channels % 8 or out_channels % 8:
            raise NotImplementedError('PatchRowsConv2D: channels (%d -> %d) must be multiples of 8'
                                      % (in_channels, out_channels))
        super().__init__(in_channels, out_channels, kernel_size)

    def forward(self, rows, residual=None):
        return hnn._LinearFn.apply(rows, self.weight, self.bias, self, False, False, residual)


class Conv1x1(PatchRowsConv2D):
    """paddle.nn.Conv2D(cin, cout, 1) over NHWC rows [M, cin]: the 1 x 1 patch, ``weight`` [cout, cin, 1, 1]."""

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, out_channels, 1)


class CMlp(hnn.Layer):
    """fc2(act(fc1(x))) over NHWC rows; ``drop`` must be 0."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=hnn.GELU, drop=0.):
        super().__init__()
        if drop:
            raise NotImplementedError('CMlp(drop=%r): element-wise dropout is not built for ConvMAE' % (drop,))
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = Conv1x1(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = Conv1x1(hidden_features, out_features)

    def forward(self, rows, residual=None):
        return self.fc2(self.act(self.fc1(rows)), residual=residual)


class CBlock(hnn.Layer):
    """x + drop_path(conv2(attn(mask * conv1(norm1(x))))), then x + drop_path(mlp(norm2(x))), over NHWC."""

    def __init__(self, dim, num_heads=None, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=hnn.GELU, norm_layer=None):
        super().__init__()
        if drop or attn_drop:
            raise NotImplementedError('CBlock(drop=%r, attn_drop=%r): element-wise dropout is not built for ConvMAE'
                                      % (drop, attn_drop))
        drop_path = float(drop_path)
        if not 0. <= drop_path < 1.:
            raise ValueError('drop_path must be in [0, 1), got %r' % drop_path)
        self.drop_path = drop_path
        self.keep_prob = float(np.float32(1.0) - np.float32(drop_path))
        self.norm1 = hnn.LayerNorm(dim)                      # nn.LayerNorm(dim): epsilon 1e-5, norm_layer is not used
        self.conv1 = Conv1x1(dim, dim)
        self.conv2 = Conv1x1(dim, dim)
        self.attn = hnn.MaskedDepthwiseConv2D(dim, 5, padding=2)
        self.norm2 = hnn.LayerNorm(dim)
        self.mlp = CMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, mask=None, grid=None, keep=None):
        """x: [N, H, W, C].  mask: the fp32 table [N, Hm * Wm] (1 = removed) over ``grid`` = (Hm, Wm), or None.
        keep: this block's two rows [2, N] of the keep table (training with drop_path > 0)."""
        N, H, W, C = x.shape
        rows = x.view(N * H * W, C)
        dropping = self.drop_path > 0. and self.training
        if dropping and keep is None:
            raise RuntimeError('CBlock(drop_path=%g) in training mode needs its two rows of the keep table'
                               % self.drop_path)
        h, xr = self.norm1.fork(rows)
        h = self.attn(self.conv1(h).view(N, H, W, C), mask, grid).view(N * H * W, C)
        if dropping:
            rows = hnn.drop_path_add(self.conv2(h), xr, keep[0], self.keep_prob, N, H * W)
        else:
            rows = self.conv2(h, residual=xr)
        h, xr = self.norm2.fork(rows)
        if dropping:
            rows = hnn.drop_path_add(self.mlp(h), xr, keep[1], self.keep_prob, N, H * W)
        else:
            rows = self.mlp(h, residual=xr)
        return rows.view(N, H, W, C)


class CPatchEmbed(hnn.Layer):
    """Image to Patch Embedding: proj (p x p / stride p) -> LayerNorm(1e-5) -> GELU.  ``rows=True`` builds ``proj`` for
    patches handed over as GEMM rows (``forward_rows``: the masked model embeds the kept patches only)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, rows=False):
        super().__init__()
        img_size, patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        if patch_size[0] != patch_size[1]:
            raise NotImplementedError('CPatchEmbed: patch %s is not square' % (patch_size,))
        self.grid_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.img_size, self.patch_size = img_size, patch_size
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.embed_dim, self.in_chans = embed_dim, in_chans
        self.from_image = bool(in_chans % 8)                  # the 3-channel image: patchify + GEMM
        if self.from_image:
            self.proj = _PatchProj(in_chans, embed_dim, patch_size[0])
        elif rows:
            self.proj = PatchRowsConv2D(in_chans, embed_dim, patch_size[0], patch_size[0])
        else:
            self.proj = hnn.PatchConv2D(in_chans, embed_dim, patch_size[0], patch_size[0])
        self.norm = hnn.LayerNorm(embed_dim)                  # epsilon 1e-5
        self.act = hnn.GELU()

    def forward(self, x):
        """The image NCHW fp32 (first stage) or an NHWC map -> NHWC [B, gh, gw, embed_dim]."""
        gh, gw = self.grid_size
        if self.from_image:
            B, C, H, W = x.shape
            if (H, W) != self.img_size:
                raise ValueError("Input image size (%d*%d) doesn't match model (%d*%d)." % ((H, W) + self.img_size))
            dtype = hnn._need_rt(self.proj).arena.dtype
            rows = self.proj(ops.patchify(x.contiguous().float(), self.patch_size[0], dtype))
        else:
            B, H, W, C = x.shape
            if (H, W) != self.img_size:
                raise ValueError("Input map size (%d*%d) doesn't match model (%d*%d)." % ((H, W) + self.img_size))
            rows = self.proj(x).view(B * gh * gw, self.embed_dim)
        return self.act(self.norm(rows)).view(B, gh, gw, self.embed_dim)

    def forward_rows(self, rows):
        """Patches as GEMM rows [M, p*p*cin] -> [M, embed_dim]."""
        return self.act(self.norm(self.proj(rows)))


def check_stages(img_size, patch_size, embed_dim, depth):
    img_size, patch_size, embed_dim, depth = list(img_size), list(patch_size), list(embed_dim), list(depth)
    if not (len(img_size) == len(patch_size) == len(embed_dim) == len(depth) == 3):
        raise ValueError('ConvMAE has three stages: img_size %r, patch_size %r, embed_dim %r, depth %r'
                         % (img_size, patch_size, embed_dim, depth))
    if any(d <= 0 or d % 8 for d in embed_dim):
        raise NotImplementedError('embed_dim=%r: every width must be a multiple of 8 (16-byte rows of the HIP kernels)'
                                  % (embed_dim,))
    for i in range(2):
        if img_size[i] % patch_size[i] or img_size[i + 1] != img_size[i] // patch_size[i]:
            raise NotImplementedError('img_size %r / patch_size %r: stage %d does not hand stage %d its map'
                                      % (img_size, patch_size, i + 1, i + 2))
    if img_size[2] % patch_size[2]:
        raise NotImplementedError('img_size %r / patch_size %r: stage 3 does not tile its map' % (img_size, patch_size))
    return img_size, patch_size, embed_dim, depth


class ConvViT(hnn.DropPathModel, ViTTrunk, Model):
    """ConvViT: two stages of convolutional blocks and a Vision Transformer stage."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 hybrid_backbone=None, norm_layer=None, global_pool=False, **kwargs):
        super().__init__()
        if hybrid_backbone is not None:
            raise NotImplementedError('ConvViT(hybrid_backbone=...): the CNN feature-map embedding is not built')
        if drop_rate or attn_drop_rate:
            raise NotImplementedError('ConvViT(drop_rate=%r, attn_drop_rate=%r): element-wise dropout is not built for '
                                      'ConvMAE' % (drop_rate, attn_drop_rate))
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        img_size, patch_size, embed_dim, depth = check_stages(img_size, patch_size, embed_dim, depth)
        mlp_ratio = list(mlp_ratio) if isinstance(mlp_ratio, (list, tuple)) else [mlp_ratio] * 3
        norm_layer = norm_layer or hnn.LayerNorm
        dev = config.get_device()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.depth, self.drop_path_rate = depth, float(drop_path_rate)
        self._first = {}                                       # (B, L) -> row of every sample's first patch token
        self.patch_embed1 = CPatchEmbed(img_size[0], patch_size[0], in_chans, embed_dim[0])
        self.patch_embed2 = CPatchEmbed(img_size[1], patch_size[1], embed_dim[0], embed_dim[1])
        self.patch_embed3 = CPatchEmbed(img_size[2], patch_size[2], embed_dim[1], embed_dim[2])
        num_patches = self.patch_embed3.num_patches
        self.check_attention_envelope(img_size[0], patch_size, embed_dim[2], num_heads, num_patches)
        self.patch_embed4 = hnn.Linear(embed_dim[2], embed_dim[2])
        self.pos_embed = tnn.Parameter(torch.zeros(1, num_patches, embed_dim[2], device=dev))
        self.dp_rates = [float(v) for v in np.linspace(0, drop_path_rate, sum(depth))]
        dpr = self.dp_rates
        self.blocks1 = tnn.ModuleList([CBlock(embed_dim[0], num_heads, mlp_ratio[0], drop_path=dpr[i])
                                       for i in range(depth[0])])
        self.blocks2 = tnn.ModuleList([CBlock(embed_dim[1], num_heads, mlp_ratio[1], drop_path=dpr[depth[0] + i])
                                       for i in range(depth[1])])
        self.blocks3 = tnn.ModuleList([Block(embed_dim[2], num_heads, mlp_ratio[2], qkv_bias=qkv_bias, qk_scale=qk_scale,
                                             drop_path=dpr[depth[0] + depth[1] + i], norm_layer=norm_layer)
                                       for i in range(depth[2])])
        self.norm = norm_layer(embed_dim[-1])
        self.head = hnn.Linear(embed_dim[-1], num_classes) if num_classes > 0 else None
        trunc_normal_(self.pos_embed, std=.02)
        with torch.no_grad():
            # self.apply(self._init_weights): Linear trunc_normal(.02) / zero bias, LayerNorm (1, 0); the convolutions
            # keep nn.Conv2D's default [Paddle-semantics]: Normal(0, sqrt(2 / fan_in)), zero bias
            for m in self.modules():
                if isinstance(m, hnn.Linear):
                    trunc_normal_(m.weight, std=.02)
                    if m.bias is not None:
                        m.bias.zero_()
                elif isinstance(m, (_PatchProj, hnn.PatchConv2D, hnn.MaskedDepthwiseConv2D)):
                    w = m.weight
                    w.copy_(torch.randn(w.shape) * (2.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5)
                    m.bias.zero_()
        self.global_pool = global_pool
        if self.global_pool:
            self.fc_norm = norm_layer(embed_dim[-1])
            del self.norm                                                  # remove the original norm
        # every block owns two rows when the rate is above 0 (block 0 with keep probability 1.0)
        blocks = list(self.blocks1) + list(self.blocks2) + list(self.blocks3)
        self._seed_drop_path(blocks if self.drop_path_rate > 0. else (), 2)
        self.pool = hnn.AdaptiveAvgPool2D(1)
        self.arena_q = EncoderArena(self, trainable=True)

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def load_pretrained(self, path, rank=0, finetune=False):
        load_lenient(self, read_pdparams(path), what='pretrained ConvViT')
        self.sync_runtime_state()

    def forward_features(self, x, drop_path_keep=None):
        B = x.shape[0]
        keep = self._drop_path_keep(B, x.device, drop_path_keep)
        x = self.patch_embed1(x)
        for blk in self.blocks1:
            x = blk(x, keep=self._drop_path_rows(keep, blk))
        x = self.patch_embed2(x)
        for blk in self.blocks2:
            x = blk(x, keep=self._drop_path_rows(keep, blk))
        x = self.patch_embed3(x)                                            # [B, 14, 14, D]
        L, D = self.patch_embed3.num_patches, self.embed_dim[2]
        ids, _ = self.identity_ids(B, L, x.device)
        x = hnn.tokens_pos_gather_add(self.patch_embed4(x.view(B * L, D)), self.pos_embed, ids, ids, B, L)
        for blk in self.blocks3:
            x = blk(x, B, L, self._drop_path_rows(keep, blk))
        if self.global_pool:
            return self.fc_norm(self.pool(x.view(B, L, 1, D)))             # x.mean(axis=1), then fc_norm
        first = self._first.get((B, L))
        if first is None:
            first = self._first[(B, L)] = (torch.arange(B, dtype=torch.int32, device=x.device) * L).contiguous()
        return self.norm(hnn.gather_rows(x, first))                        # norm(x)[:, 0]: the first PATCH token

    def forward(self, x, drop_path_keep=None):
        self.arena_q.refresh()
        f = self.forward_features(x, drop_path_keep)
        return f if self.head is None else self.head(f, out_f32=True)


def convvit_base_patch16(**kwargs):
    return ConvViT(img_size=[224, 56, 28], patch_size=[4, 2, 2], embed_dim=[256, 384, 768], depth=[2, 2, 11],
                   num_heads=12, mlp_ratio=[4, 4, 4], qkv_bias=True, norm_layer=partial(hnn.LayerNorm, epsilon=1e-6),
                   **kwargs)
