"""``passl.models.convmae.conv_mae`` — the ConvMAE masked autoencoder on the MI355X HIP path.

Names, constructor arguments, state_dict keys and shapes, the factories and the ``model(imgs, mask_ratio=0.75) ->
(loss, pred, mask)`` contract are the reference's (passl/models/convmae/conv_mae.py: MaskedAutoencoderConvViT :32-322,
convmae_convvit_base_patch16_dec512d8b :325-343).  What runs differently, with the same result:

  * the mask of a CBlock is never expanded to the map: ``hnn.MaskedDepthwiseConv2D`` reads the patch table
    [B, 196] that ``passl_hip_mae_mask`` writes and finds a pixel's factor by address arithmetic (the reference builds
    ``mask_for_patch1`` [B, 1, 56, 56] and ``mask_for_patch2`` [B, 1, 28, 28], :240-245);
  * ``stage1_output_decode`` (4x4/4), ``stage2_output_decode`` (2x2/2), ``patch_embed3`` and ``patch_embed4`` are
    functions of one patch each.  The reference runs them over all 196 patches and then keeps 49 (:249-266); here
    ``hnn.patch_gather`` writes the GEMM rows of the kept patches and the four layers run on those rows only.  The two
    stage-2 consumers share one gather; the sum ``x + stage1_embed + stage2_embed`` (:271) runs in the epilogues of
    the two decode GEMMs, in that order;
  * a map with two consumers (stage 1: the decode gather and ``patch_embed2``; the stage-2 rows: decode and
    ``patch_embed3``) goes through ``hnn.fork``, so the library, not autograd, adds the two gradients;
  * ``pos_embed`` is a PARAMETER initialised with the sin-cos table, as the reference leaves it (only
    ``decoder_pos_embed`` has ``stop_gradient``): it receives a gradient and is updated; ``decoder_pos_embed`` is a
    buffer under the same key;
  * the per-sample noise of ``random_masking`` comes from ``torch.rand`` on the device (``noise=`` injects the
    reference's draw); the argsort pair is the rank kernel.

The reference hard-codes the 14 x 14 patch grid, the 56 and 28 maps (:240-245) and ``p = 16`` in ``patchify`` (:183):
any ``img_size`` / ``patch_size`` whose stages chain is accepted here, the loss patch is the product of the three patch
sizes."""
from functools import partial

import torch
import torch.nn as tnn

from ...hip import config, ops
from ...hip import nn as hnn
from ...hip.nn import EncoderArena
from ...modules.get_sincos_pe import get_2d_sincos_pos_embed
from ...modules.vit import Block, ViTTrunk, _PatchProj, xavier_uniform_
from ...utils.checkpoint import load_pdparams
from ..base_model import Model
from .conv_vit import CBlock, CPatchEmbed, PatchRowsConv2D, check_stages

__all__ = ['MaskedAutoencoderConvViT', 'convmae_convvit_base_patch16', 'convmae_convvit_base_patch16_dec512d8b']


class MaskedAutoencoderConvViT(ViTTrunk, Model):
    """Masked Autoencoder with the ConvViT backbone."""
    _own_arena = True             # False in the v110-schema twin (modeling/backbones/convmae.py): its wrapper owns it

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=1024, depth=24, num_heads=16,
                 decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16, mlp_ratio=4.,
                 norm_layer=hnn.LayerNorm, norm_pix_loss=False):
        super().__init__()
        img_size, patch_size, embed_dim, depth = check_stages(img_size, patch_size, embed_dim, depth)
        mlp_ratio = list(mlp_ratio) if isinstance(mlp_ratio, (list, tuple)) else [mlp_ratio] * 3
        dev = config.get_device()
        self.in_chans, self.patch_sizes = in_chans, patch_size
        self.embed_dim = embed_dim
        self.patch_embed1 = CPatchEmbed(img_size[0], patch_size[0], in_chans, embed_dim[0])
        self.patch_embed2 = CPatchEmbed(img_size[1], patch_size[1], embed_dim[0], embed_dim[1])
        self.patch_embed3 = CPatchEmbed(img_size[2], patch_size[2], embed_dim[1], embed_dim[2], rows=True)
        self.patch_embed4 = hnn.Linear(embed_dim[2], embed_dim[2])
        self.stage1_output_decode = PatchRowsConv2D(embed_dim[0], embed_dim[2], patch_size[1] * patch_size[2])
        self.stage2_output_decode = PatchRowsConv2D(embed_dim[1], embed_dim[2], patch_size[2])
        num_patches = self.patch_embed3.num_patches
        self.grid = self.patch_embed3.grid_size
        self.loss_patch = patch_size[0] * patch_size[1] * patch_size[2]
        self.check_attention_envelope(img_size[0], patch_size, embed_dim[2], num_heads, num_patches)
        self.check_attention_envelope(img_size[0], patch_size, decoder_embed_dim, decoder_num_heads, num_patches)
        self.pos_embed = tnn.Parameter(torch.zeros(1, num_patches, embed_dim[2], device=dev))
        self.blocks1 = tnn.ModuleList([CBlock(embed_dim[0], num_heads, mlp_ratio[0]) for _ in range(depth[0])])
        self.blocks2 = tnn.ModuleList([CBlock(embed_dim[1], num_heads, mlp_ratio[1]) for _ in range(depth[1])])
        self.blocks3 = tnn.ModuleList([Block(embed_dim[2], num_heads, mlp_ratio[2], qkv_bias=True, norm_layer=norm_layer)
                                       for _ in range(depth[2])])
        self.norm = norm_layer(embed_dim[-1])
        self.decoder_embed = hnn.Linear(embed_dim[-1], decoder_embed_dim)
        self.mask_token = tnn.Parameter(torch.zeros(1, 1, decoder_embed_dim, device=dev))
        self.register_buffer('decoder_pos_embed', torch.zeros(1, num_patches, decoder_embed_dim, device=dev))
        self.decoder_blocks = tnn.ModuleList([Block(decoder_embed_dim, decoder_num_heads, mlp_ratio[0], qkv_bias=True,
                                                    norm_layer=norm_layer) for _ in range(decoder_depth)])
        self.decoder_norm = norm_layer(decoder_embed_dim)
        self.decoder_pred = hnn.Linear(decoder_embed_dim, self.loss_patch ** 2 * in_chans)
        self.norm_pix_loss = norm_pix_loss
        self._ones = {}
        self.initialize_weights()
        if self._own_arena:
            self.arena_q = EncoderArena(self, trainable=True)     # flat parameters / gradients (AdamW, DP reducer)

    @torch.no_grad()
    def initialize_weights(self):
        g = int(self.patch_embed3.num_patches ** .5)
        self.pos_embed.copy_(torch.from_numpy(
            get_2d_sincos_pos_embed(self.pos_embed.shape[-1], g, cls_token=False)).float().unsqueeze(0))
        self.decoder_pos_embed.copy_(torch.from_numpy(
            get_2d_sincos_pos_embed(self.decoder_pos_embed.shape[-1], g, cls_token=False)).float().unsqueeze(0))
        # every other convolution keeps nn.Conv2D's default [Paddle-semantics]: Normal(0, sqrt(2 / fan_in)), zero bias
        for m in self.modules():
            if isinstance(m, (_PatchProj, hnn.PatchConv2D, hnn.MaskedDepthwiseConv2D)):
                w = m.weight
                w.copy_(torch.randn(w.shape) * (2.0 / (w.shape[1] * w.shape[2] * w.shape[3])) ** 0.5)
                m.bias.zero_()
        w = self.patch_embed3.proj.weight                     # xavier_uniform_ on the [D, C*p*p] view (:158-161)
        xavier_uniform_(w, w.shape[1] * w.shape[2] * w.shape[3], w.shape[0])
        self.mask_token.copy_(torch.randn(self.mask_token.shape) * 0.02)
        for m in self.modules():
            if isinstance(m, hnn.Linear):
                xavier_uniform_(m.weight, m.weight.shape[0], m.weight.shape[1])
                if m.bias is not None:
                    m.bias.zero_()
            elif isinstance(m, hnn.LayerNorm):
                m.bias.zero_()
                m.weight.fill_(1.0)

    def load_pretrained(self, path, rank=0, finetune=False):
        load_pdparams(self, path, what='pretrained ConvMAE', bare_ok=True)

    # -- reference helpers kept for API parity (host-side, not on the hot path)
    def patchify(self, imgs):
        p = self.loss_patch
        h, w = imgs.shape[2] // p, imgs.shape[3] // p
        x = imgs.reshape(imgs.shape[0], self.in_chans, h, p, w, p)
        return torch.einsum('nchpwq->nhwpqc', x).reshape(imgs.shape[0], h * w, p ** 2 * self.in_chans)

    def random_masking_ids(self, B, L, mask_ratio, noise=None):
        len_keep = int(L * (1 - mask_ratio))
        if len_keep < 1:
            raise ValueError('mask_ratio %r keeps no patch of %d' % (mask_ratio, L))
        if noise is None:
            # paddle.rand([N, L]): a host call that stays live when the step is replayed from a native plan
            from ...hip.replay import host_call
            noise = torch.empty(B, L, device=self.pos_embed.device)
            host_call(lambda: noise.uniform_())
        ids_keep, ids_restore, mask = ops.mae_mask(noise.contiguous().float(), len_keep)
        return ids_keep, ids_restore, mask, len_keep

    def _ones_row(self, B, device):
        ones = self._ones.get(B)
        if ones is None:
            ones = self._ones[B] = torch.ones(B, dtype=torch.float32, device=device)      # (cached: made once per B)
        return ones

    def forward_encoder(self, imgs, mask_ratio, noise=None):
        B = imgs.shape[0]
        L, (gh, gw) = self.patch_embed3.num_patches, self.grid
        p2, p3 = self.patch_sizes[1], self.patch_sizes[2]
        D0, D1, D2 = self.embed_dim
        ids_keep, ids_restore, mask, K = self.random_masking_ids(B, L, mask_ratio, noise)
        ones = self._ones_row(B, imgs.device)
        x = self.patch_embed1(imgs)                                      # [B, H1, W1, D0]
        for blk in self.blocks1:
            x = blk(x, mask, self.grid)
        H1, W1 = x.shape[1], x.shape[2]
        xa, xb = hnn.fork(x.view(B * H1 * W1, D0), 2, ones, B, H1 * W1)
        rows1 = hnn.patch_gather(xa.view(B, H1, W1, D0), ids_keep, ids_restore, self.grid, p2 * p3)
        x = self.patch_embed2(xb.view(B, H1, W1, D0))                    # [B, H2, W2, D1]
        for blk in self.blocks2:
            x = blk(x, mask, self.grid)
        rows2 = hnn.patch_gather(x, ids_keep, ids_restore, self.grid, p3)      # [B*K, p3*p3*D1]
        ra, rb = hnn.fork(rows2, 2, ones, B, K)
        x = self.patch_embed4(self.patch_embed3.forward_rows(ra))        # the kept patches only
        x = hnn.tokens_pos_gather_add(x, self.pos_embed, ids_keep, ids_restore, B, L)
        for blk in self.blocks3:
            x = blk(x, B, K)
        x = self.stage1_output_decode(rows1, residual=x)                 # x + stage1_embed
        x = self.stage2_output_decode(rb, residual=x)                    # ... + stage2_embed
        return self.norm(x), mask, (ids_keep, ids_restore)

    def forward_decoder(self, x, ids, B):
        ids_keep, ids_restore = ids
        L = ids_restore.shape[1]
        x = self.decoder_embed(x)
        x = hnn.tokens_unshuffle(x, self.mask_token, self.decoder_pos_embed, ids_keep, ids_restore, B)
        for blk in self.decoder_blocks:
            x = blk(x, B, L)
        x = self.decoder_norm(x)
        return self.decoder_pred(x, out_f32=True)                        # [B*L, p*p*3] fp32

    def forward_loss(self, imgs, pred_rows, mask):
        denom = float(mask.shape[0] * (mask.shape[1] - int(self._len_keep)))
        return hnn.tokens_masked_patch_loss(pred_rows, imgs, mask, self.loss_patch, self.norm_pix_loss, denom)

    def forward(self, imgs, mask_ratio=0.75, noise=None):
        """-> (loss, pred [N, L, p*p*3], mask [N, L]).  ``noise``: inject the per-sample masking noise (tests)."""
        if self._own_arena:
            self.arena_q.refresh()                               # compute-dtype copies of the updated weights
        B = imgs.shape[0]
        L = self.patch_embed3.num_patches
        self._len_keep = int(L * (1 - mask_ratio))
        latent, mask, ids = self.forward_encoder(imgs, mask_ratio, noise)
        pred_rows = self.forward_decoder(latent, ids, B)
        loss = self.forward_loss(imgs, pred_rows, mask)
        return loss, pred_rows.view(B, L, -1), mask


def convmae_convvit_base_patch16_dec512d8b(**kwargs):
    return MaskedAutoencoderConvViT(img_size=[224, 56, 28], patch_size=[4, 2, 2], embed_dim=[256, 384, 768],
                                    depth=[2, 2, 11], num_heads=12, decoder_embed_dim=512, decoder_depth=8,
                                    decoder_num_heads=16, mlp_ratio=[4, 4, 4],
                                    norm_layer=partial(hnn.LayerNorm, epsilon=1e-6), **kwargs)


# set recommended archs
convmae_convvit_base_patch16 = convmae_convvit_base_patch16_dec512d8b  # decoder: 512 dim, 8 blocks
