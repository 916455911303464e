"""MAE (masked autoencoder, ViT encoder + light decoder) on the MI355X HIP path.

Constructor, registry name, sub-layer / state_dict names and the ``forward(imgs, mask_ratio)``
-> ``(loss, pred, mask)`` contract are the reference's ``MAE`` (passl_v110/modeling/backbones/
mae.py:318-564, twin of passl/models/mae.py:37-290); Mlp / Attention / Block / PatchEmbed and the token assembly are
the shared ones of passl_amd/modules/vit.py (re-exported here under the reference's names).
Execution: tokens are 2-D rows [B*T, C] in the compute dtype; every Linear is the implicit-GEMM
kernel (bias, residual add in the epilogue; fp32 output for the pixel prediction), LayerNorm / GELU /
attention / token gather-unshuffle / patchify / masked-patch loss are HIP kernels
(csrc/vit.hip, csrc/attention.hip).  ``pos_embed`` / ``decoder_pos_embed`` are fixed sin-cos tables
(reference: parameters with stop_gradient=True) kept as buffers under the same state_dict keys.
The per-sample noise of random_masking comes from ``torch.rand`` on the device (``noise=`` lets
tests inject the reference's draw); the argsort pair is replaced by a rank kernel.
Stochastic depth of the fine-tuning ViT (``drop_path_rate``): one device-side Philox draw per forward pass fills a keep
table, and the residual add of a block that can drop runs in csrc/drop_path.hip instead of the GEMM epilogue."""
from functools import partial

import torch
import torch.nn as tnn
from torch.autograd import Function

from ...hip import config, nn, ops
from ...modules.get_sincos_pe import get_2d_sincos_pos_embed
from ...modules.vit import (Attention, Block, Identity, Mlp, PatchEmbed, ViTTrunk, _TokensFn,      # noqa: F401
                            alias_matrix_param, conv_default_normal_, to_2tuple, trunc_normal_,
                            xavier_uniform_)
from .builder import BACKBONES


class _UnshuffleFn(Function):
    @staticmethod
    def forward(ctx, x, mask_token, pos, ids_keep, ids_restore, B):
        ctx.save_for_backward(ids_keep, ids_restore)
        ctx.tok, ctx.B = mask_token, B
        nn.param_expect_grad(mask_token)
        return ops.mae_unshuffle(x, mask_token.detach().view(-1), pos.view(-1, pos.shape[-1]), ids_restore,
                                 B, ids_keep.shape[1])

    @staticmethod
    def backward(ctx, dout):
        ids_keep, ids_restore = ctx.saved_tensors
        tok = ctx.tok
        if tok.grad is None:
            tok.grad = torch.zeros_like(tok)
        dx = ops.mae_unshuffle_bwd(dout.contiguous(), ids_keep, ids_restore, tok.grad, ctx.B)
        nn.param_grad_ready(tok)
        return dx, None, None, None, None, None


from ...loss.mae import masked_patch_loss      # the fused loss lives in passl.loss.mae


@BACKBONES.register()
class MAE(nn.Layer):
    """Masked Autoencoder with VisionTransformer backbone."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, num_heads=16,
                 decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.,
                 norm_layer=partial(nn.LayerNorm, epsilon=1e-6), norm_pix_loss=False):
        super().__init__()
        dev = config.get_device()
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = tnn.Parameter(torch.zeros(1, 1, embed_dim, device=dev))
        self.register_buffer('pos_embed', torch.zeros(1, num_patches + 1, embed_dim, device=dev))
        self.blocks = tnn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias=True, norm_layer=norm_layer)
                                      for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.decoder_embed = nn.Linear(embed_dim, decoder_embed_dim)
        self.mask_token = tnn.Parameter(torch.zeros(1, 1, decoder_embed_dim, device=dev))
        self.register_buffer('decoder_pos_embed', torch.zeros(1, num_patches + 1, decoder_embed_dim, device=dev))
        self.decoder_blocks = tnn.ModuleList([Block(decoder_embed_dim, decoder_num_heads, mlp_ratio, qkv_bias=True,
                                                    norm_layer=norm_layer) for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(decoder_embed_dim)
        self.decoder_pred = nn.Linear(decoder_embed_dim, patch_size ** 2 * in_chans)
        self.norm_pix_loss = norm_pix_loss
        self.in_chans = in_chans
        self.initialize_weights()

    @torch.no_grad()
    def initialize_weights(self):
        g = int(self.patch_embed.num_patches ** .5)
        self.pos_embed.copy_(torch.from_numpy(
            get_2d_sincos_pos_embed(self.pos_embed.shape[-1], g, cls_token=True)).float().unsqueeze(0))
        self.decoder_pos_embed.copy_(torch.from_numpy(
            get_2d_sincos_pos_embed(self.decoder_pos_embed.shape[-1], g, cls_token=True)).float().unsqueeze(0))
        trunc_normal_(self.cls_token, std=0.02)              # create_parameter(default_initializer=trunc_normal_)
        w = self.patch_embed.proj.weight                      # xavier_uniform_ on the [D, C*p*p] view
        xavier_uniform_(w, w.shape[1] * w.shape[2] * w.shape[3], w.shape[0])
        for m in self.modules():
            if isinstance(m, nn.Linear):
                xavier_uniform_(m.weight, m.weight.shape[0], m.weight.shape[1])
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, nn.LayerNorm):
                m.bias.zero_()
                m.weight.fill_(1.0)

    # -- reference helpers kept for API parity (host-side, not on the hot path) ------------------
    def patchify(self, imgs):
        p = self.patch_embed.patch_size[0]
        h = w = imgs.shape[2] // p
        x = imgs.reshape(imgs.shape[0], self.in_chans, h, p, w, p)
        return torch.einsum('nchpwq->nhwpqc', x).reshape(imgs.shape[0], h * w, p ** 2 * self.in_chans)

    def unpatchify(self, x):
        p = self.patch_embed.patch_size[0]
        h = w = int(x.shape[1] ** .5)
        x = x.reshape(x.shape[0], h, w, p, p, self.in_chans)
        return torch.einsum('nhwpqc->nchpwq', x).reshape(x.shape[0], self.in_chans, h * p, h * p)

    def random_masking_ids(self, B, L, mask_ratio, noise=None):
        len_keep = int(L * (1 - mask_ratio))
        if noise is None:
            # paddle.rand([N, L]).  torch.rand IS empty + uniform_ (same generator stream); written this way the draw is a
            # host call that stays live when the step is replayed from a native plan (hip/replay.py) — a fresh mask
            # at every replay, in the recorded buffer
            from ...hip.replay import host_call
            noise = torch.empty(B, L, device=self.cls_token.device)
            host_call(lambda: noise.uniform_())
        ids_keep, ids_restore, mask = ops.mae_mask(noise.contiguous().float(), len_keep)
        return ids_keep, ids_restore, mask, len_keep

    def forward_encoder(self, imgs, mask_ratio, noise=None):
        B = imgs.shape[0]
        L = self.patch_embed.num_patches
        x = self.patch_embed(imgs)                                       # [B*L, D]
        ids_keep, ids_restore, mask, K = self.random_masking_ids(B, L, mask_ratio, noise)
        x = _TokensFn.apply(x, self.cls_token, self.pos_embed, ids_keep, ids_restore, B, L)
        for blk in self.blocks:
            x = blk(x, B, K + 1)
        return self.norm(x), mask, (ids_keep, ids_restore)

    def forward_decoder(self, x, ids, B):
        ids_keep, ids_restore = ids
        L = ids_restore.shape[1]
        x = self.decoder_embed(x)
        x = _UnshuffleFn.apply(x, self.mask_token, self.decoder_pos_embed, ids_keep, ids_restore, B)
        for blk in self.decoder_blocks:
            x = blk(x, B, L + 1)
        x = self.decoder_norm(x)
        return self.decoder_pred(x, out_f32=True)                        # [B*(L+1), p*p*3] fp32, cls rows included

    def forward_loss(self, imgs, pred_rows, mask):
        denom = float(mask.shape[0] * (mask.shape[1] - int(self._len_keep)))
        return masked_patch_loss(pred_rows, imgs, mask, self.patch_embed.patch_size[0], self.norm_pix_loss, denom)

    def forward(self, imgs, mask_ratio=0.75, noise=None):
        B = imgs.shape[0]
        L = self.patch_embed.num_patches
        self._len_keep = int(L * (1 - mask_ratio))
        latent, mask, ids = self.forward_encoder(imgs, mask_ratio, noise)
        pred_rows = self.forward_decoder(latent, ids, B)
        loss = self.forward_loss(imgs, pred_rows, mask)
        pred = pred_rows.view(B, L + 1, -1)[:, 1:, :]                    # remove cls token
        return loss, pred, mask


# ============================================================ fine-tuning trunk (configs/mae/mae_vit_b_finetune.yaml)
class _PatchMeanFn(Function):
    """``x[:, 1:, :].mean(axis=1)`` over token rows [B*(L+1), D] (mae.py:308: global average pool of the patch tokens,
    class token excluded): the NHWC average-pool kernel over all L+1 tokens, minus the class row."""

    @staticmethod
    def forward(ctx, x, cls_rows, B, L):
        D = x.shape[-1]
        ctx.dims = (B, L, D)
        avg = ops.avgpool_fwd(x.view(B, L + 1, 1, D))
        cls = ops.gather_rows(x, cls_rows)
        return ((avg.float() * (L + 1) - cls.float()) / L).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        B, L, D = ctx.dims
        # every patch token receives dout / L: the pool's backward hands out dy / (L + 1)
        dx = ops.avgpool_bwd((dout.float() * ((L + 1.0) / L)).to(dout.dtype).contiguous(), L + 1, 1)
        dx = dx.view(B, L + 1, D)
        dx[:, 0].zero_()
        return dx.view(B * (L + 1), D), None, None, None


class VisionTransformer(nn.DropPathModel, ViTTrunk):
    """The fine-tuning ViT of the v110 tree (passl_v110/modeling/backbones/mae.py:190-277): learnable ``cls_token`` /
    ``pos_embed`` (trunc-normal 0.02), pre-norm blocks, final LayerNorm, output = the class token's row.  Same kernels as
    the pre-training encoder above.  ``drop_path_rate`` is stochastic depth with the reference's ladder
    ``linspace(0, rate, depth)`` (:234); element-wise dropout (``drop_rate`` / ``attn_drop_rate``) is not built.

    Stochastic depth (``nn.DropPathState``): the keep table is [2 * depth, B] (row 2i = attention branch of block i, row
    2i + 1 = its MLP branch); with a rate above 0 every block owns its two rows, block 0 with keep probability 1.0.  The
    seed is drawn at construction in front of the weights."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 embed_layer=PatchEmbed, norm_layer=None, act_layer=None, weight_init=''):
        super().__init__()
        if drop_rate or attn_drop_rate:
            raise NotImplementedError('element-wise dropout is not built on the HIP path')
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        dev = config.get_device()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        norm_layer = norm_layer or partial(nn.LayerNorm, epsilon=1e-6)
        act_layer = act_layer or nn.GELU
        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.check_attention_envelope(img_size, patch_size, embed_dim, num_heads, num_patches + 1)
        self.cls_token = tnn.Parameter(torch.zeros(1, 1, embed_dim, device=dev))
        self.pos_embed = tnn.Parameter(torch.zeros(1, num_patches + 1, embed_dim, device=dev))
        # dpr = [x.item() for x in paddle.linspace(0, drop_path_rate, depth)]: a float32 ladder
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth, dtype=torch.float32)]
        self.blocks = tnn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer,
                                             act_layer=act_layer, drop_path=dpr[i]) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.drop_path_rate = float(drop_path_rate)
        # every block owns two rows when the rate is above 0 (block 0 with keep probability 1.0); the seed is drawn
        # in front of the weights
        self._seed_drop_path(self.blocks if self.drop_path_rate > 0. else (), 2)
        trunc_normal_(self.cls_token, std=0.02)
        trunc_normal_(self.pos_embed, std=0.02)
        with torch.no_grad():
            # self.apply(self._init_weights): Linear trunc_normal(.02) / zero bias, LayerNorm (1, 0); the patch
            # convolution keeps nn.Conv2D's default [Paddle-semantics]: Normal(0, sqrt(2 / fan_in)), zero bias
            conv_default_normal_(self.patch_embed.proj.weight)
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    trunc_normal_(m.weight, std=0.02)
                    if m.bias is not None:
                        m.bias.zero_()

    def get_num_layers(self):
        """What build_optimizer's layer-wise lr decay asks the backbone (passl_v110/solver/builder.py:182), as the
        reference's beit_ft.py:493 answers it; the reference's own MAE_ViT has no such method."""
        return len(self.blocks)

    def _tokens(self, x, drop_path_keep=None):
        keep = self._drop_path_keep(x.shape[0], x.device, drop_path_keep)
        x, cls_rows, B, L = self.embed_tokens(x, self.cls_token, self.pos_embed)     # concat(cls, x) + pos_embed
        return self.run_blocks(x, B, L + 1, keep), cls_rows, B, L

    def forward_features(self, x, drop_path_keep=None):
        x, cls_rows, _B, _L = self._tokens(x, drop_path_keep)
        return self.cls_features(x, cls_rows, self.norm)

    def forward(self, x, drop_path_keep=None):
        return self.forward_features(x, drop_path_keep)


@BACKBONES.register()
class MAE_ViT(VisionTransformer):
    """Vision Transformer with support for global average pooling — passl_v110/modeling/backbones/mae.py:279-314:
    with ``global_pool`` the final ``norm`` is replaced by ``fc_norm`` over the mean of the patch tokens."""

    def __init__(self, global_pool=True, **kwargs):
        super().__init__(**kwargs)
        self.global_pool = global_pool
        if self.global_pool:
            self.fc_norm = nn.LayerNorm(kwargs['embed_dim'], epsilon=1e-6)
            del self.norm                                                  # remove the original norm

    def forward_features(self, x, drop_path_keep=None):
        x, cls_rows, B, L = self._tokens(x, drop_path_keep)
        if self.global_pool:
            return self.fc_norm(_PatchMeanFn.apply(x, cls_rows, B, L))
        return self.cls_features(x, cls_rows, self.norm)
