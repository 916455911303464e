"""``passl.models.cait`` — CaiT (Going deeper with Image Transformers, https://arxiv.org/abs/2103.17239) on the MI355X HIP
path.

Names, constructor arguments, sub-layer / state_dict keys and shapes and the ten factories are the reference's
(passl/models/cait.py: ClassAttn :46-88, LayerScaleBlockClassAttn :91-134, TalkingHeadAttn :137-185, LayerScaleBlock
:188-229, Cait :232-434, factories :437-613), so its ``.pdparams`` load.  Activations are token rows [B*T, C]:

  * the trunk runs over the ``num_patches`` patch rows alone: ``pos_embed`` has ``num_patches`` rows and is added by one
    streaming launch (``hnn.pos_add``); the class token joins only for the token-only blocks;
  * ``TalkingHeadAttn`` is ``hnn.Linear`` qkv -> ``hnn.talking_heads_attention`` (csrc/cait_attention.hip) -> ``hnn.Linear``
    proj.  ``proj_l`` / ``proj_w`` are fp32 arena parameters [H, H] ([in, out]) and [H] read by the kernel: they are
    not GEMM layers;
  * ``ClassAttn`` is three ``hnn.Linear`` (q on the class rows, k and v on all rows) -> ``hnn.class_attention`` -> proj;
  * every residual is ``hnn.layer_scale_add``: residual + keep[b] * ((gamma * branch) / keep_prob), without a keep row
    when nothing can drop;
  * the token-only stage: ``concat(x_cls, x)`` is one launch (``hnn.cls_concat``) into a [B, 1 + L, C] buffer whose row 0
    is the class row, the ``expand`` of ``cls_token`` an address; the patch rows' gradients from the blocks are chained
    through the launches' backward, and the three consumers of ``norm1(u)`` through ``hnn.fork``: no ATen launch, a
    strict step plan records the step.  With ``global_pool == 'token'`` the last ``norm`` runs on the class rows alone
    (LayerNorm is per row).  ``global_pool`` 'avg' and '' construct and are refused at the forward.

Stochastic depth: ``dpr = [drop_path_rate] * depth`` (:282), the same rate for every trunk block, two draws per block
(one per residual) and ``keep_prob = float32(1 - p)``; the token-only blocks have rate 0 and own no row.  The keep table
(``hnn.DropPathState``) is [2 * depth, B], rows 2k, 2k + 1 the attention and the MLP residual of trunk block k.
Evaluation mode and rate 0 launch no draw.

Envelope: the kernels take head dimension 48 (every factory's), at most 8 heads and 208 tokens.  The three 224-pixel
factories (``cait_xxs24_224``, ``cait_xxs36_224``, ``cait_s24_224``) run.  The seven 384- / 448-pixel factories (576 /
784 patch tokens, 16 heads for the m sizes) construct with the reference's keys and raise the library's unsupported
error (PASSL_EUNSUPPORTED) when run, as the large v2 ViT factories do: they need a key-tiled talking-heads kernel that is not built.

Initialisation (:324-335): trunc-normal(0.02) Linear weights (proj_l / proj_w included), ``pos_embed`` and ``cls_token``,
zero biases, LayerNorm (1, 0), gamma = ``init_values``; the patch convolution keeps Paddle's default.

Refused by name in the constructor: ``drop_rate > 0``, ``attn_drop_rate > 0``, ``qk_scale``."""
from functools import partial

import numpy as np
import torch
import torch.nn as tnn

from ..hip import config
from ..hip import nn as hnn
from ..hip.nn import EncoderArena
from ..modules.vit import Mlp, PatchEmbed, conv_default_normal_, trunc_normal_
from ..utils.checkpoint import load_lenient, read_pdparams
from .base_model import ClassifierModel

__all__ = [
    'Cait', 'ClassAttn', 'LayerScaleBlock', 'LayerScaleBlockClassAttn', 'TalkingHeadAttn',
    'cait_xxs24_224', 'cait_xxs24_384', 'cait_xxs36_224', 'cait_xxs36_384', 'cait_xs24_384', 'cait_s24_224',
    'cait_s24_384', 'cait_s36_384', 'cait_m36_384', 'cait_m48_448',
]


def _refuse_dropout(who, **rates):
    for name, v in rates.items():
        if v:
            raise NotImplementedError('%s(%s=%r): dropout is not built for CaiT (no config or factory sets it)'
                                      % (who, name, v))


def _refuse_qk_scale(who, qk_scale):
    if qk_scale is not None:
        raise NotImplementedError('%s(qk_scale=%r): only the default head_dim ** -0.5 is built' % (who, qk_scale))


class _HeadMix(hnn.Layer):
    """The parameters of a Linear over the head axis (``proj_l`` / ``proj_w``): weight fp32 [H, H] ([in, out]) and bias
    [H].  The attention kernel applies it to every (query, key) pair; there is no GEMM layer."""

    def __init__(self, num_heads):
        super().__init__()
        dev = config.get_device()
        self.weight = tnn.Parameter(torch.empty(num_heads, num_heads, device=dev))
        self.bias = tnn.Parameter(torch.zeros(num_heads, device=dev))


class ClassAttn(hnn.Layer):
    """One query per head from the class row; keys and values from the class row and the patch rows."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        _refuse_dropout('ClassAttn', attn_drop=attn_drop, proj_drop=proj_drop)
        _refuse_qk_scale('ClassAttn', qk_scale)
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        bias_attr = None if qkv_bias else False
        self.q = hnn.Linear(dim, dim, bias_attr=bias_attr)
        self.k = hnn.Linear(dim, dim, bias_attr=bias_attr)
        self.v = hnn.Linear(dim, dim, bias_attr=bias_attr)
        self.proj = hnn.Linear(dim, dim)

    def forward(self, u, cls_rows, ones, B, T):
        """u: the normalised rows [B*T, C] whose row 0 of every image is the class row -> rows [B, C]."""
        uq, uk, uv = hnn.fork(u, 3, ones, B, T)
        q = self.q(hnn.gather_rows(uq, cls_rows))
        a = hnn.class_attention(q, self.k(uk), self.v(uv), B, T, self.num_heads, self.head_dim, self.scale)
        return self.proj(a)


class TalkingHeadAttn(hnn.Layer):
    """Self-attention whose scores are mixed over the heads before and after the softmax."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        _refuse_dropout('TalkingHeadAttn', attn_drop=attn_drop, proj_drop=proj_drop)
        _refuse_qk_scale('TalkingHeadAttn', qk_scale)
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = hnn.Linear(dim, dim * 3, bias_attr=None if qkv_bias else False)
        self.proj = hnn.Linear(dim, dim)
        self.proj_l = _HeadMix(num_heads)
        self.proj_w = _HeadMix(num_heads)

    def forward(self, x, B, T):
        a = hnn.talking_heads_attention(self.qkv(x), self.proj_l.weight, self.proj_l.bias, self.proj_w.weight,
                                        self.proj_w.bias, B, T, self.num_heads, self.head_dim, self.scale)
        return self.proj(a)


class _LayerScale(hnn.Layer):
    """What the two block kinds share: norms, attention, MLP, the two gammas and the stochastic-depth rate."""

    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer, norm_layer,
                 attn_block, mlp_block, init_values):
        super().__init__()
        drop_path = float(drop_path)
        if not 0. <= drop_path < 1.:
            raise ValueError('drop_path must be in [0, 1), got %r' % drop_path)
        self.drop_path = drop_path
        self.keep_prob = float(np.float32(1.0 - drop_path))       # paddle.to_tensor(1 - drop_prob, dtype=float32)
        self.norm1 = norm_layer(dim)
        self.attn = attn_block(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                               proj_drop=drop)
        self.norm2 = norm_layer(dim)
        self.mlp = mlp_block(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        dev = config.get_device()
        self.gamma_1 = tnn.Parameter(torch.full((dim,), float(init_values), device=dev))
        self.gamma_2 = tnn.Parameter(torch.full((dim,), float(init_values), device=dev))


class LayerScaleBlockClassAttn(_LayerScale):
    """x_cls + gamma_1 * attn(norm1(concat(x_cls, x))), then x_cls + gamma_2 * mlp(norm2(x_cls)): the class row alone
    is updated."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=hnn.GELU, norm_layer=hnn.LayerNorm, attn_block=ClassAttn, mlp_block=Mlp, init_values=1e-4):
        if drop_path != 0.:
            raise NotImplementedError('LayerScaleBlockClassAttn(drop_path=%r): the token-only blocks have rate 0 '
                                      '(cait.py:307)' % (drop_path,))
        super().__init__(dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer,
                         norm_layer, attn_block, mlp_block, init_values)

    def forward(self, x, x_cls, cls_rows, ones, B, L, slot_in=None, slot_out=None):
        """x: patch rows [B*L, C]; x_cls: rows [B, C], or the ``cls_token`` parameter -> the new class rows [B, C]."""
        u = hnn.cls_concat(x, x_cls, B, L, slot_in, slot_out)
        h, ur = self.norm1.fork(u)
        x_cls = hnn.layer_scale_add(self.attn(h, cls_rows, ones, B, L + 1), hnn.gather_rows(ur, cls_rows), self.gamma_1,
                                    None, 1.0, B, 1)
        h, xr = self.norm2.fork(x_cls)
        return hnn.layer_scale_add(self.mlp(h), xr, self.gamma_2, None, 1.0, B, 1)


class LayerScaleBlock(_LayerScale):
    """x + drop_path(gamma_1 * attn(norm1(x))), then x + drop_path(gamma_2 * mlp(norm2(x))), over rows [B*T, C]."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=hnn.GELU, norm_layer=hnn.LayerNorm, attn_block=TalkingHeadAttn, mlp_block=Mlp,
                 init_values=1e-4):
        super().__init__(dim, num_heads, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path, act_layer,
                         norm_layer, attn_block, mlp_block, init_values)

    def forward(self, x, B, T, keep=None):
        """keep: this block's two rows [2, B] of the keep table, or None (nothing can drop)."""
        k0 = k1 = None
        if self.drop_path > 0. and self.training:
            if keep is None:
                raise RuntimeError('LayerScaleBlock(drop_path=%g) in training mode needs its two rows of the keep table'
                                   % self.drop_path)
            k0, k1 = keep[0], keep[1]
        h, xr = self.norm1.fork(x)
        x = hnn.layer_scale_add(self.attn(h, B, T), xr, self.gamma_1, k0, self.keep_prob, B, T)
        h, xr = self.norm2.fork(x)
        return hnn.layer_scale_add(self.mlp(h), xr, self.gamma_2, k1, self.keep_prob, B, T)


class Cait(hnn.DropPathModel, ClassifierModel):
    GLOBAL_POOLS = ('', 'token', 'avg')

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, global_pool='token', embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4., qkv_bias=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 block_layers=LayerScaleBlock, block_layers_token=LayerScaleBlockClassAttn, patch_layer=PatchEmbed,
                 norm_layer=partial(hnn.LayerNorm, epsilon=1e-6), act_layer=hnn.GELU, attn_block=TalkingHeadAttn,
                 mlp_block=Mlp, init_values=1e-4, attn_block_token_only=ClassAttn, mlp_block_token_only=Mlp,
                 depth_token_only=2, mlp_ratio_token_only=4.0, qk_scale=None):
        super().__init__()
        assert global_pool in self.GLOBAL_POOLS
        _refuse_dropout('Cait', drop_rate=drop_rate, attn_drop_rate=attn_drop_rate)
        _refuse_qk_scale('Cait', qk_scale)
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        if embed_dim % num_heads or embed_dim % 8:
            raise NotImplementedError('Cait(embed_dim=%d, num_heads=%d): the width must be a multiple of the head count '
                                      'and of 8 (16-byte rows of the HIP kernels)' % (embed_dim, num_heads))
        dev = config.get_device()
        self.num_classes = num_classes
        self.global_pool = global_pool
        self.num_features = self.embed_dim = embed_dim
        self.drop_path_rate = float(drop_path_rate)
        self.patch_embed = patch_layer(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = tnn.Parameter(torch.zeros(1, 1, embed_dim, device=dev))
        self.pos_embed = tnn.Parameter(torch.zeros(1, num_patches, embed_dim, device=dev))
        dpr = [drop_path_rate for _ in range(depth)]
        self.blocks = tnn.ModuleList([
            block_layers(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                         attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer,
                         attn_block=attn_block, mlp_block=mlp_block, init_values=init_values) for i in range(depth)])
        self.blocks_token_only = tnn.ModuleList([
            block_layers_token(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio_token_only, qkv_bias=qkv_bias,
                               drop=0.0, attn_drop=0.0, drop_path=0.0, norm_layer=norm_layer, act_layer=act_layer,
                               attn_block=attn_block_token_only, mlp_block=mlp_block_token_only,
                               init_values=init_values) for _ in range(depth_token_only)])
        self.norm = norm_layer(embed_dim)
        self.feature_info = [dict(num_chs=embed_dim, reduction=0, module='head')]
        self.head = hnn.Linear(embed_dim, num_classes) if num_classes > 0 else None
        with torch.no_grad():
            trunc_normal_(self.pos_embed, std=.02)
            trunc_normal_(self.cls_token, std=.02)
            for m in self.modules():
                if isinstance(m, (hnn.Linear, _HeadMix)):
                    trunc_normal_(m.weight, std=.02)
                    if m.bias is not None:
                        m.bias.zero_()
            conv_default_normal_(self.patch_embed.proj.weight)        # Paddle's default for nn.Conv2D
            self.patch_embed.proj.bias.zero_()
        # the token-only blocks hand the patch rows' gradient backwards: block t puts it where block t - 1 takes it
        self._x_slots = [hnn.GradSlot() for _ in range(max(depth_token_only - 1, 0))]
        self._rows = {}
        # stochastic depth: two rows of the keep table per trunk block with p > 0, none for the token-only blocks; the
        # seed is drawn after the weights (a model with stochastic depth initialises as one without)
        self._seed_drop_path([blk for blk in self.blocks if blk.drop_path > 0.], 2)
        self.arena_q = EncoderArena(self, trainable=True)

    def load_pretrained(self, path, rank=0, finetune=False):
        sd = read_pdparams(path)
        if finetune:                                   # cait.py:397-428
            own = self.state_dict()
            for k in ['head.weight', 'head.bias']:
                if k in sd and (k not in own or tuple(sd[k].shape) != tuple(own[k].shape)):
                    print(f'Removing key {k} from pretrained checkpoint')
                    del sd[k]
            pos = torch.as_tensor(sd['pos_embed']).float()
            n_new = self.patch_embed.num_patches
            extra = self.pos_embed.shape[-2] - n_new
            orig, new = int((pos.shape[-2] - extra) ** 0.5), int(n_new ** 0.5)
            # bicubic interpolation of the position tokens on the host (once)
            tok = pos[0, extra:].reshape(-1, orig, orig, pos.shape[-1]).permute(0, 3, 1, 2)
            tok = torch.nn.functional.interpolate(tok, size=(new, new), mode='bicubic', align_corners=False)
            sd['pos_embed'] = torch.cat([pos[:, :extra], tok.permute(0, 2, 3, 1).flatten(1, 2)], dim=1).numpy()
        load_lenient(self, sd, what='pretrained CaiT')
        self.sync_runtime_state()

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    # ---- forward
    def _batch_rows(self, B, L, device):
        """-> (cls_rows int32 [B] = the class row of each image in a [B, 1 + L] buffer, ones fp32 [B]), cached."""
        key = (B, L)
        if key not in self._rows:
            self._rows[key] = ((torch.arange(B, dtype=torch.int32, device=device) * (L + 1)).contiguous(),
                               torch.ones(B, dtype=torch.float32, device=device))
        return self._rows[key]

    def forward_features(self, x, drop_path_keep=None):
        """-> the normalised class rows [B, C] (``global_pool == 'token'``: the rows forward_head selects)."""
        if self.global_pool != 'token':
            raise NotImplementedError("Cait(global_pool=%r): only 'token' is built (the last norm runs on the class "
                                      "rows alone)" % (self.global_pool,))
        B, L = x.shape[0], self.patch_embed.num_patches
        keep = self._drop_path_keep(B, x.device, drop_path_keep)
        x = hnn.pos_add(self.patch_embed(x), self.pos_embed, B, L)
        for blk in self.blocks:
            x = blk(x, B, L, self._drop_path_rows(keep, blk))
        cls_rows, ones = self._batch_rows(B, L, x.device)
        x_cls = self.cls_token
        n = len(self.blocks_token_only)
        for t, blk in enumerate(self.blocks_token_only):
            x_cls = blk(x, x_cls, cls_rows, ones, B, L, slot_in=self._x_slots[t] if t < n - 1 else None,
                        slot_out=self._x_slots[t - 1] if t > 0 else None)
        if n == 0:
            raise NotImplementedError('Cait(depth_token_only=0) is not built')
        return self.norm(x_cls)

    def forward_head(self, x, pre_logits=False):
        if pre_logits or self.head is None:
            return x
        if x.dtype == torch.float32 or self.num_features % 64 == 0:
            return self.head(x, out_f32=True)
        # bf16 rows of a width that is no multiple of 64 (none of the factories): the GEMM with an fp32 output is not
        # built for them, so the logits are rounded to bf16 once and widened
        return hnn.to_f32(self.head(x))

    def forward(self, x, drop_path_keep=None):
        self.arena_q.refresh()                       # compute-dtype operands and data-gradient packs of the updated weights
        return self.forward_head(self.forward_features(x, drop_path_keep))


def _cait(img_size, embed_dim, depth, num_heads, init_values, **kwargs):
    return Cait(img_size=img_size, patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4,
                qkv_bias=True, norm_layer=partial(hnn.LayerNorm, epsilon=1e-6), init_values=init_values,
                depth_token_only=2, **kwargs)


def cait_xxs24_224(**kwargs):
    return _cait(224, 192, 24, 4, 1e-5, **kwargs)


def cait_xxs24_384(**kwargs):
    return _cait(384, 192, 24, 4, 1e-5, **kwargs)


def cait_xxs36_224(**kwargs):
    return _cait(224, 192, 36, 4, 1e-5, **kwargs)


def cait_xxs36_384(**kwargs):
    return _cait(384, 192, 36, 4, 1e-5, **kwargs)


def cait_xs24_384(**kwargs):
    return _cait(384, 288, 24, 6, 1e-5, **kwargs)


def cait_s24_224(**kwargs):
    return _cait(224, 384, 24, 8, 1e-5, **kwargs)


def cait_s24_384(**kwargs):
    return _cait(384, 384, 24, 8, 1e-5, **kwargs)


def cait_s36_384(**kwargs):
    return _cait(384, 384, 36, 8, 1e-6, **kwargs)


def cait_m36_384(**kwargs):
    return _cait(384, 768, 36, 16, 1e-6, **kwargs)


def cait_m48_448(**kwargs):
    return _cait(448, 768, 48, 16, 1e-6, **kwargs)
