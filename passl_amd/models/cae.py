"""``passl.models.cae`` — the Context Autoencoder (CAE, https://arxiv.org/abs/2202.03026) for pre-training on the
MI355X HIP path.

Names, constructor arguments (the ``args`` namespace included), state_dict keys and shapes and the three factories are
the reference's (passl/models/cae.py: CAEMlp :36-58, CAEAttention :61-168, CAECrossAttention :176-261, CAEBlock
:315-375, CAEDecoderBlock :383-448, CAEEncoder :524-687, CAERegressorDecoder :697-830, CAEPretrain :833-1029,
factories :1328-1370).  ``forward(x, bool_masked_pos, num_masked=None) -> (logits [B Nm, V] fp32, latent_pred
[B, Nm, C], latent_target [B, Nm, C])`` as the reference returns them.  What runs differently, with the same result:

  * tokens are rows [B*T, C] in the compute dtype; the index tables of the mask come from one launch
    (``passl_hip_cae_mask_ids``) on the fp32 0/1 mask — visible and masked patches in ascending order, the order of the
    reference's boolean indexing — and feed the MAE keep-gather (student on the visible, teacher on the masked ids);
  * ``q_bias`` / ``v_bias`` are the parameters, the qkv Linear has no bias of its own: the bias vector of the fused
    projection, ``[q_bias | 0 | v_bias]``, is assembled into a buffer whose key third stays zero (it is not a parameter
    and gets no update); the bias gradient is one column sum whose outer thirds are added to the two parameters;
  * the regressor's cross-attention runs on three tensors with Tq = Nm queries and Tk = Nu + Nm keys
    (``hnn.cross_attention``); its operands ``x_q + pos_q``, ``concat(x_u, x_q) + pos_k`` and ``concat(x_u, x_q)`` come
    from one launch per block (``hnn.cae_tokens_assemble``): no expanded position tensor, no concat copy;
  * a tensor with several consumers goes through ``hnn.fork``, so the library, not autograd, adds its gradients; no
    ATen kernel is launched in a training step: a strict step plan records it;
  * the teacher lives in an arena of its own (``arena_k``), runs without a tape and is absent from the optimizer; its
    update ``t = ema t + (1 - ema) s`` is one launch over the arena, inside ``forward`` after the teacher's pass, where
    the reference does it (:981-989): the teacher lags the student by one optimizer step even at ema = 0.  Evaluation
    mode launches no update;
  * ``pos_embed`` is the fixed sin-cos table, a buffer under the reference's key (there: a parameter with
    ``stop_gradient``).  With ``decoder_embed_dim != embed_dim`` the regressor's table is the sin-cos table of the
    decoder's width, which is what the reference's ``try: expand ... except: build`` arrives at (:1000-1006).

Refused with NotImplementedError, never ignored: ``use_abs_pos_emb=True`` or neither position flag, ``drop_path_rate`` /
``drop_rate`` / ``attn_drop_rate`` other than 0, ``init_values <= 0`` (either), ``attn_head_dim``, ``qk_scale``,
``qkv_bias=False``, head dimensions other than 32 / 64, token counts beyond the attention kernels."""
from functools import partial
from types import SimpleNamespace

import torch
import torch.nn as tnn
from torch.autograd import Function

from ..hip import config, ops
from ..hip import nn as hnn
from ..hip.nn import EncoderArena
from ..modules.vit import PatchEmbed, ViTTrunk, _TokensFn, conv_default_normal_, trunc_normal_, xavier_uniform_
from ..utils.checkpoint import load_pdparams
from .base_model import Model

__all__ = ['CAEMlp', 'CAEAttention', 'CAECrossAttention', 'CAEBlock', 'CAEDecoderBlock', 'CAEEncoder',
           'CAERegressorDecoder', 'CAEPretrain', 'cae_pretrain_args', 'latent_loss', 'cae_small_patch16_224_8k_vocab',
           'cae_base_patch16_224_8k_vocab', 'cae_large_patch16_224_8k_vocab']


def cae_pretrain_args(**overrides):
    """The values of tasks/ssl/cae/pretrain.sh (and the defaults of main_pretrain.py it leaves alone) that the model and
    the loop read, as the namespace the reference's constructor takes."""
    a = dict(sincos_pos_emb=True, abs_pos_emb=False, rel_pos_bias=False, layer_scale_init_value=0.1,
             decoder_layer_scale_init_value=0.1, mask_generator='block', num_mask_patches=75,
             max_mask_patches_per_block=None, min_mask_patches_per_block=16, regressor_depth=4,
             num_decoder_self_attention=4, decoder_embed_dim=768, decoder_num_heads=12, decoder_num_classes=8192,
             dual_loss_weight=2.0, dual_loss_type='mse', dual_path_ema=0.0, target_mode='random', drop_path=0.0,
             clip_grad=3.0, lr=1.5e-3, min_lr=1e-5, warmup_epochs=10, epochs=800, weight_decay=0.05, batch_size=64,
             input_size=224, print_freq=10, max_train_step=None)
    unknown = sorted(set(overrides) - set(a))
    if unknown:
        raise ValueError('cae_pretrain_args: unknown names %s' % unknown)
    a.update(overrides)
    return SimpleNamespace(**a)


def _refuse(who, **rates):
    for name, v in rates.items():
        if v:
            raise NotImplementedError('%s(%s=%r) is not built for CAE (the pre-training recipe sets 0)' % (who, name, v))


def _check_heads(who, dim, num_heads, attn_head_dim=None, qk_scale=None, qkv_bias=True):
    if attn_head_dim is not None:
        raise NotImplementedError('%s(attn_head_dim=%r) is not built' % (who, attn_head_dim))
    if qk_scale is not None:
        raise NotImplementedError('%s(qk_scale=%r): only the default head_dim ** -0.5 is built' % (who, qk_scale))
    if not qkv_bias:
        raise NotImplementedError('%s(qkv_bias=False) is not built (every factory sets it)' % who)
    if dim % num_heads or dim // num_heads not in ops.ATTENTION_HEAD_DIMS:
        raise NotImplementedError('%s(dim=%d, num_heads=%d): head dimension %s is outside the HIP attention kernels (%s)'
                                  % (who, dim, num_heads, dim / float(num_heads), sorted(ops.ATTENTION_HEAD_DIMS)))
    return dim // num_heads


def _check_init_values(who, init_values):
    if init_values is None or not init_values > 0:
        raise NotImplementedError('%s(init_values=%r): blocks without layer scale are not built (the recipe sets 0.1)'
                                  % (who, init_values))


class _ExtBiasLinearFn(Function):
    """hnn._LinearFn for a bias-free ``hnn.Linear`` whose bias vector belongs to the owning attention layer: ``parts`` =
    ((parameter, offset), ...) of the output columns.  One part at offset 0 that covers every column is used in place;
    otherwise the vector is assembled in ``buf`` (zero where no part lies) and the bias gradient, one column sum, is
    added part by part.  Weight and data gradients run on the main stream."""

    @staticmethod
    def forward(ctx, x, weight, layer, parts, buf):
        rt = hnn._need_rt(layer)
        N = x.shape[0]
        pl = layer._plan(N)
        whole = len(parts) == 1 and parts[0][1] == 0 and parts[0][0].numel() == layer.out_features
        if whole:
            shift = parts[0][0].detach()
        else:
            for p, o in parts:
                ops.copy_into(buf[o:o + p.numel()], p.detach())
            shift = buf
        y = torch.empty(N, layer.out_features, dtype=x.dtype, device=x.device)
        ops.conv_igemm(pl.fd, x, rt.w_fwd, y, shift=shift)
        if any(ctx.needs_input_grad):
            rt.arena.expect_grad(rt.indices)
            hnn.param_expect_grad(*[p for p, _o in parts])
        ctx.save_for_backward(x)
        ctx.layer, ctx.pl, ctx.parts, ctx.whole = layer, pl, parts, whole
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer, pl = ctx.layer, ctx.pl
        rt = layer._rt
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = ops.cast_to(dy, x.dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape[0], layer.in_features, dtype=x.dtype, device=x.device)
            d = pl.dds[0]
            ops.conv_igemm(d, dy, rt.w_dgrad[id(d.pack)], dx)
        ops.conv_wgrad(pl.wd, x, dy, rt.dw)
        if ctx.whole:
            ops.colsum_into(dy, ctx.parts[0][0].grad.view(-1), accumulate=True)
        else:
            cols = torch.empty(layer.out_features, dtype=torch.float32, device=dy.device)
            ops.colsum_into(dy, cols)
            for p, o in ctx.parts:
                ops.add_into(p.grad.view(-1), cols[o:o + p.numel()])
        rt.arena.grad_ready(rt.indices)
        hnn.param_grad_ready(*[p for p, _o in ctx.parts])
        return dx, None, None, None, None


class CAEMlp(hnn.Layer):
    """fc2(act(fc1(x))); ``drop`` must be 0."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=hnn.GELU, drop=0.):
        super().__init__()
        _refuse('CAEMlp', drop=drop)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = hnn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = hnn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _BiasOwner(hnn.Layer):
    """q_bias / v_bias [all_head_dim], zero-initialised (cae.py:80-84), and the buffers of _ExtBiasLinearFn."""

    def _make_biases(self, all_head_dim):
        dev = config.get_device()
        self.q_bias = tnn.Parameter(torch.zeros(all_head_dim, device=dev))
        self.v_bias = tnn.Parameter(torch.zeros(all_head_dim, device=dev))
        self._bufs = {}

    def _bias_buffer(self, n, device):
        buf = self._bufs.get(device)
        if buf is None:
            buf = self._bufs[device] = torch.zeros(n, dtype=torch.float32, device=device)
        return buf


class CAEAttention(_BiasOwner):
    """Self-attention over the fused qkv projection with the bias [q_bias | 0 | v_bias] (cae.py:132-168)."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., window_size=None,
                 attn_head_dim=None):
        super().__init__()
        _refuse('CAEAttention', attn_drop=attn_drop, proj_drop=proj_drop, window_size=window_size)
        self.num_heads = num_heads
        self.head_dim = _check_heads('CAEAttention', dim, num_heads, attn_head_dim, qk_scale, qkv_bias)
        self.scale = self.head_dim ** -0.5
        self.qkv = hnn.Linear(dim, dim * 3, bias_attr=False)
        self._make_biases(dim)
        self.proj = hnn.Linear(dim, dim)

    def forward(self, x, B, T):
        D = self.q_bias.numel()
        qkv = _ExtBiasLinearFn.apply(x, self.qkv.weight, self.qkv, ((self.q_bias, 0), (self.v_bias, 2 * D)),
                                     self._bias_buffer(3 * D, x.device))
        return self.proj(hnn.attention(qkv, B, T, self.num_heads, self.head_dim, self.scale))


class CAECrossAttention(_BiasOwner):
    """softmax(q k^T scale) v with q = Linear_q(x_q) + q_bias, k = Linear_k(x_k), v = Linear_v(x_v) + v_bias
    (cae.py:216-261); Tq queries against Tk keys."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., window_size=None,
                 attn_head_dim=None):
        super().__init__()
        _refuse('CAECrossAttention', attn_drop=attn_drop, proj_drop=proj_drop, window_size=window_size)
        self.num_heads = num_heads
        self.head_dim = _check_heads('CAECrossAttention', dim, num_heads, attn_head_dim, qk_scale, qkv_bias)
        self.scale = self.head_dim ** -0.5
        self.q = hnn.Linear(dim, dim, bias_attr=False)
        self.k = hnn.Linear(dim, dim, bias_attr=False)
        self.v = hnn.Linear(dim, dim, bias_attr=False)
        self._make_biases(dim)
        self.proj = hnn.Linear(dim, dim)

    def forward(self, x_q, x_k, x_v, B, Tq, Tk):
        q = _ExtBiasLinearFn.apply(x_q, self.q.weight, self.q, ((self.q_bias, 0),), None)
        k = self.k(x_k)
        v = _ExtBiasLinearFn.apply(x_v, self.v.weight, self.v, ((self.v_bias, 0),), None)
        return self.proj(hnn.cross_attention(q, k, v, B, Tq, Tk, self.num_heads, self.head_dim, self.scale))


def _gamma(dim, value):
    return tnn.Parameter(torch.full((dim,), float(value), device=config.get_device()))


class CAEBlock(hnn.Layer):
    """x + gamma_1 attn(norm1(x)), then x + gamma_2 mlp(norm2(x)) (cae.py:360-375)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 init_values=None, act_layer=hnn.GELU, norm_layer=hnn.LayerNorm, window_size=None, attn_head_dim=None):
        super().__init__()
        _refuse('CAEBlock', drop=drop, drop_path=drop_path)
        _check_init_values('CAEBlock', init_values)
        self.norm1 = norm_layer(dim)
        self.attn = CAEAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                                 proj_drop=drop, window_size=window_size, attn_head_dim=attn_head_dim)
        self.norm2 = norm_layer(dim)
        self.mlp = CAEMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.gamma_1 = _gamma(dim, init_values)
        self.gamma_2 = _gamma(dim, init_values)

    def forward(self, x, B, T):
        h, xr = self.norm1.fork(x)
        x = hnn.layer_scale_add(self.attn(h, B, T), xr, self.gamma_1, None, 1.0, B, T)
        h, xr = self.norm2.fork(x)
        return hnn.layer_scale_add(self.mlp(h), xr, self.gamma_2, None, 1.0, B, T)


class CAEDecoderBlock(hnn.Layer):
    """A block of the latent regressor (cae.py:439-448):
        x = x_q + gamma_1_cross cross_attn(norm1_q(x_q + pos_q), k = norm1_k(x_kv + pos_k), v = norm1_v(x_kv))
        x = norm2_cross(x);  x = x + gamma_2_cross mlp_cross(x)
    — the second residual is taken from the NORMALISED rows."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 init_values=None, act_layer=hnn.GELU, norm_layer=hnn.LayerNorm, window_size=None, attn_head_dim=None):
        super().__init__()
        _refuse('CAEDecoderBlock', drop=drop, drop_path=drop_path)
        _check_init_values('CAEDecoderBlock', init_values)
        self.norm1_q_cross = norm_layer(dim)
        self.norm1_k_cross = norm_layer(dim)
        self.norm1_v_cross = norm_layer(dim)
        self.norm2_cross = norm_layer(dim)
        self.cross_attn = CAECrossAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                            attn_drop=attn_drop, proj_drop=drop, window_size=window_size,
                                            attn_head_dim=attn_head_dim)
        self.mlp_cross = CAEMlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.gamma_1_cross = _gamma(dim, init_values)
        self.gamma_2_cross = _gamma(dim, init_values)

    def forward(self, x_q, x_u, pos, ids_vis, ids_msk, B, ones):
        """x_q rows [B*Nm, C], x_u rows [B*(1 + Nu), C]: this block's branch of the encoder's output, whose class row is
        skipped in place (x_unmasked[:, 1:], cae.py:1017)."""
        Nu, Nm = ids_vis.shape[1], ids_msk.shape[1]
        xr, xa = hnn.fork(x_q, 2, ones, B, Nm)
        q_in, k_in, v_in = hnn.cae_tokens_assemble(x_u, xa, pos, ids_vis, ids_msk, B, u0=1)
        a = self.cross_attn(self.norm1_q_cross(q_in), self.norm1_k_cross(k_in), self.norm1_v_cross(v_in), B, Nm, Nu + Nm)
        x = self.norm2_cross(hnn.layer_scale_add(a, xr, self.gamma_1_cross, None, 1.0, B, Nm))
        xr, xm = hnn.fork(x, 2, ones, B, Nm)
        return hnn.layer_scale_add(self.mlp_cross(xm), xr, self.gamma_2_cross, None, 1.0, B, Nm)


def sincos_table(grid_size, embed_dim, temperature=10000.):
    """build_2d_sincos_position_embedding(use_cls_token=True), cae.py:600-624, in fp32 as the reference computes it:
    [1, 1 + h w, embed_dim], row 0 (the class token's) zero."""
    h, w = grid_size
    if embed_dim % 4:
        raise ValueError('Embed dimension must be divisible by 4 for 2D sin-cos position embedding')
    gw, gh = torch.meshgrid(torch.arange(w, dtype=torch.float32), torch.arange(h, dtype=torch.float32), indexing='ij')
    pos_dim = embed_dim // 4
    omega = 1. / (temperature ** (torch.arange(pos_dim, dtype=torch.float32) / pos_dim))
    out_w = torch.einsum('m,d->md', gw.flatten(), omega)
    out_h = torch.einsum('m,d->md', gh.flatten(), omega)
    emb = torch.cat([torch.sin(out_w), torch.cos(out_w), torch.sin(out_h), torch.cos(out_h)], dim=1)
    return torch.cat([torch.zeros(1, embed_dim), emb], dim=0).unsqueeze(0)


class CAEEncoder(ViTTrunk):
    """The ViT that encodes the visible patches (student) or the masked ones (teacher): ``forward(x, ids_keep,
    ids_restore)`` -> norm(blocks([cls | x[ids_keep]] + pos)) as rows [B*(1 + K), C]."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, vocab_size=8192, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=None, init_values=None, attn_head_dim=None, use_abs_pos_emb=True, init_std=0.02, args=None,
                 **kwargs):
        super().__init__()
        _refuse('CAEEncoder', drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate)
        if use_abs_pos_emb or not getattr(args, 'sincos_pos_emb', False):
            raise NotImplementedError('CAEEncoder: only the fixed sin-cos position table is built (use_abs_pos_emb=False '
                                      'and args.sincos_pos_emb=True, as pretrain.sh sets them)')
        if getattr(args, 'rel_pos_bias', False):
            raise NotImplementedError('CAEEncoder: args.rel_pos_bias is not built')
        _check_init_values('CAEEncoder', init_values)
        _check_heads('CAEEncoder', embed_dim, num_heads, attn_head_dim, qk_scale, qkv_bias)
        norm_layer = norm_layer or hnn.LayerNorm
        dev = config.get_device()
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        self.num_patches = self.patch_embed.num_patches
        if self.num_patches + 1 > ops.ATTENTION_TILED_MAX_TOKENS:
            raise NotImplementedError('CAEEncoder: %d tokens are beyond the attention kernels (%d)'
                                      % (self.num_patches + 1, ops.ATTENTION_TILED_MAX_TOKENS))
        self.cls_token = tnn.Parameter(torch.zeros(1, 1, embed_dim, device=dev))
        self.register_buffer('pos_embed', sincos_table(self.patch_embed.grid_size, embed_dim).to(dev))
        self.blocks = tnn.ModuleList([CAEBlock(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                                               qk_scale=qk_scale, norm_layer=norm_layer, init_values=init_values)
                                      for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.init_std = init_std

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_num_layers(self):
        return len(self.blocks)

    def forward(self, x, ids_keep, ids_restore):
        B, K = ids_keep.shape
        rows = self.patch_embed(x)                                               # [B*L, C]
        rows = _TokensFn.apply(rows, self.cls_token, self.pos_embed, ids_keep, ids_restore, B, self.num_patches)
        for blk in self.blocks:
            rows = blk(rows, B, K + 1)
        return self.norm(rows)


class CAERegressorDecoder(hnn.Layer):
    """The latent contextual regressor (cross-attention blocks), the decoder (self-attention blocks) and the head."""

    def __init__(self, patch_size=16, num_classes=8192, embed_dim=768, depth=6, num_heads=12, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=None, init_values=None,
                 num_patches=196, init_std=0.02, args=None, patch_shape=(14, 14)):
        super().__init__()
        _refuse('CAERegressorDecoder', drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate)
        _check_init_values('CAERegressorDecoder', init_values)
        _check_heads('CAERegressorDecoder', embed_dim, num_heads, None, qk_scale, qkv_bias)
        if num_classes <= 0:
            raise NotImplementedError('CAERegressorDecoder(num_classes=%r): the head is a Linear' % (num_classes,))
        norm_layer = norm_layer or hnn.LayerNorm
        self.num_features = self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.args = args
        kw = dict(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  norm_layer=norm_layer, init_values=init_values)
        self.blocks = tnn.ModuleList([CAEDecoderBlock(**kw) for _ in range(depth)])
        self.self_att_blocks = tnn.ModuleList([CAEBlock(**kw) for _ in range(args.num_decoder_self_attention)])
        self.norm = norm_layer(embed_dim)
        if args.num_decoder_self_attention > 0:
            self.norm2 = norm_layer(embed_dim)
        self.head = hnn.Linear(embed_dim, num_classes)
        self.init_std = init_std

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_num_layers(self):
        return len(self.blocks)

    def forward(self, x_masked, x_unmasked, pos, ids_vis, ids_msk, B, ones):
        """x_masked rows [B*Nm, C], x_unmasked rows [B*(1 + Nu), C] with the class row in place -> (logits fp32
        [B*Nm, V], latent_pred rows [B*Nm, C])."""
        Nu, Nm = ids_vis.shape[1], ids_msk.shape[1]
        n = len(self.blocks)
        xus = hnn.fork(x_unmasked, n, ones, B, 1 + Nu) if n > 1 else (x_unmasked,)
        for blk, xu in zip(self.blocks, xus):
            x_masked = blk(x_masked, xu, pos, ids_vis, ids_msk, B, ones)
        x_masked = self.norm(x_masked)
        latent_pred, x_masked = hnn.fork(x_masked, 2, ones, B, Nm)       # the last norm feeds both
        if len(self.self_att_blocks) > 0:
            x_masked = hnn.cae_pos_add(x_masked, pos, ids_msk, B)
            for blk in self.self_att_blocks:
                x_masked = blk(x_masked, B, Nm)
            x_masked = self.norm2(x_masked)
        return self.head(x_masked, out_f32=True), latent_pred


class CAEPretrain(Model):
    """Student encoder on the visible patches, teacher encoder on the masked ones, latent regressor, decoder, head."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, vocab_size=8192, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer=None, init_values=None, attn_head_dim=None, use_abs_pos_emb=True, init_std=0.02, args=None,
                 **kwargs):
        super().__init__()
        if args is None:
            raise ValueError('CAEPretrain needs the args namespace (cae_pretrain_args() has pretrain.sh\'s values)')
        norm_layer = norm_layer or partial(hnn.LayerNorm, epsilon=1e-6)
        enc = dict(img_size=img_size, patch_size=patch_size, in_chans=in_chans, vocab_size=vocab_size, embed_dim=embed_dim,
                   depth=depth, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                   drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
                   norm_layer=norm_layer, init_values=init_values, attn_head_dim=attn_head_dim,
                   use_abs_pos_emb=use_abs_pos_emb, init_std=init_std, args=args)
        dev = config.get_device()
        self.encoder = CAEEncoder(**enc)
        self.teacher_network = CAEEncoder(**enc)
        self.init_std = init_std
        self.args = args
        self.num_patches = self.encoder.patch_embed.num_patches
        dec_dim = args.decoder_embed_dim
        self.regressor_and_decoder = CAERegressorDecoder(
            patch_size=patch_size, num_classes=args.decoder_num_classes, embed_dim=dec_dim, depth=args.regressor_depth,
            num_heads=args.decoder_num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
            drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer,
            init_values=args.decoder_layer_scale_init_value, num_patches=self.num_patches, init_std=init_std, args=args)
        if dec_dim != embed_dim:
            self.encoder_to_decoder = hnn.Linear(embed_dim, dec_dim)
            self.encoder_to_decoder_norm = norm_layer(dec_dim)
        else:
            self.encoder_to_decoder = None
        self.mask_token = tnn.Parameter(torch.zeros(1, 1, dec_dim, device=dev))
        # the regressor's table: the encoder's, or (another width) the sin-cos table of the decoder's width
        self._pos = self.encoder.pos_embed[0] if dec_dim == embed_dim else \
            sincos_table(self.encoder.patch_embed.grid_size, dec_dim)[0].to(dev).contiguous()
        with torch.no_grad():
            self._init_values()
        for p in self.teacher_network.parameters():
            p.requires_grad_(False)
        teacher = list(self.teacher_network.modules())
        self.arena_q = EncoderArena(self, trainable=True, exclude=teacher)       # what the optimizer / reducer see
        self.arena_k = EncoderArena(self.teacher_network, trainable=False)
        # the encoder's parameters are one run of the student's arena, laid out as the teacher's arena is
        first = self.encoder.cls_token._passl_index
        self._enc = (self.arena_q.param_slices[first][0], self.arena_k.n_train)
        for i, (o, n) in enumerate(self.arena_k.param_slices):
            assert self.arena_q.param_slices[first + i] == (self._enc[0] + o, n), 'encoder and teacher layouts differ'
        self._const = {}

    @property
    def arena(self):
        return self.arena_q

    def _init_values(self):
        """cae.py:591-598, 765-769, 934-940: trunc-normal(init_std) tokens, then CAEPretrain's own ``apply`` overwrites
        every Linear with xavier-uniform and zero bias (the encoders' rescaled trunc-normal draws do not survive it);
        LayerNorm (1, 0); the patch convolution keeps Paddle's default; the teacher starts as the encoder's copy."""
        trunc_normal_(self.encoder.cls_token, std=self.init_std)
        trunc_normal_(self.mask_token, std=self.init_std)
        conv_default_normal_(self.encoder.patch_embed.proj.weight)
        self.encoder.patch_embed.proj.bias.zero_()
        for m in self.modules():
            if isinstance(m, hnn.Linear):
                xavier_uniform_(m.weight, m.weight.shape[0], m.weight.shape[1])
                if m.bias is not None:
                    m.bias.zero_()
        self._init_teacher()

    @torch.no_grad()
    def _init_teacher(self):
        for t, s in zip(self.teacher_network.parameters(), self.encoder.parameters()):
            t.copy_(s)
        arena_k = getattr(self, 'arena_k', None)
        if arena_k is not None and arena_k.flat.is_cuda:
            arena_k.refresh()

    def sync_runtime_state(self):
        self.arena_q.refresh()
        self.arena_k.refresh()

    def load_pretrained(self, path, rank=0, finetune=False):
        load_pdparams(self, path, what='pretrained CAE', bare_ok=True)

    @torch.no_grad()
    def _update_ema_variables(self, ema_decay):
        o, n = self._enc
        k, q = self.arena_k, self.arena_q
        ops.ema_update(k.flat[:n], q.flat[o:o + n], float(ema_decay), k.lp[:n] if k.lp is not None else None)

    def _constants(self, B, Nm, C, dtype, device):
        key = (B, Nm, C, dtype)
        c = self._const.get(key)
        if c is None:
            c = self._const[key] = SimpleNamespace(
                ones=torch.ones(B, dtype=torch.float32, device=device),
                one_rows=torch.ones(B * Nm, C, dtype=dtype, device=device),
                zero_rows=torch.zeros(B * Nm, C, dtype=dtype, device=device))
        return c

    def forward(self, x, bool_masked_pos, num_masked=None, return_all_tokens=None):
        """x [B, 3, H, W]; bool_masked_pos [B, L], 1 / True = masked (an fp32 0/1 mask costs no conversion);
        ``num_masked``: ones per image as the host knows it (None: read from the device once)."""
        B, L = x.shape[0], self.num_patches
        mask = bool_masked_pos.reshape(B, L)
        if mask.dtype != torch.float32:
            mask = mask.float()
        if num_masked is None:
            num_masked = int(round(float(mask[0].sum())))
        Nm, Nu = int(num_masked), L - int(num_masked)
        if not 0 < Nm < L:
            raise ValueError('num_masked must be in (0, %d), got %d' % (L, Nm))
        if Nm > ops.CROSS_ATTENTION_MAX_TOKENS:
            raise NotImplementedError('%d masked tokens are beyond the attention kernels' % Nm)
        self.arena_q.refresh()
        ids_vis, ids_msk, rank = ops.cae_mask_ids(mask.contiguous(), Nu)
        # ---- student on the visible patches
        xu = self.encoder(x, ids_vis, rank)                                      # [B*(1 + Nu), C_e]
        if self.encoder_to_decoder is not None:
            xu = self.encoder_to_decoder_norm(self.encoder_to_decoder(xu))
        # ---- teacher on the masked patches, no tape; then its update
        with torch.no_grad():
            lt = self.teacher_network(x, ids_msk, rank)                          # [B*(1 + Nm), C_e]; rank is not read
            if self.encoder_to_decoder is not None:
                lt = self.encoder_to_decoder_norm(self.encoder_to_decoder(lt))
            if self.training:
                self._update_ema_variables(self.args.dual_path_ema)
        C = lt.shape[-1]
        latent_target = lt.view(B, 1 + Nm, C)[:, 1:]                             # the class row stays where it is
        # ---- latent contextual regressor and decoder
        c = self._constants(B, Nm, C, xu.dtype, xu.device)
        x_masked = hnn.layer_scale_add(c.one_rows, c.zero_rows, self.mask_token, None, 1.0, B, Nm)   # the expand
        logits, latent_pred = self.regressor_and_decoder(x_masked, xu, self._pos, ids_vis, ids_msk, B, c.ones)
        return logits, latent_pred.view(B, Nm, C), latent_target


def latent_loss(latent_pred, latent_target):
    """F.mse_loss(latent_pred.float(), latent_target.float()) (engine_pretrain.py:29-31, 143-146) as one device scalar.
    ``latent_target`` is read in place: either contiguous [B, Nm, C], or — as ``CAEPretrain.forward`` returns it — the
    rows of [B, 1 + Nm, C] behind every image's class row (strides ((1 + Nm) C, C, 1)), which the kernel skips.  Any
    other layout is refused: no copy is made behind the caller's back."""
    B, Nm, C = latent_pred.shape
    if tuple(latent_target.shape) != (B, Nm, C):
        raise ValueError('latent_target %s does not match latent_pred %s' % (tuple(latent_target.shape), (B, Nm, C)))
    if latent_target.is_contiguous():
        rows, t0 = latent_target.view(B * Nm, C), 0
    elif latent_target.stride() == ((Nm + 1) * C, C, 1) and latent_target.storage_offset() >= C:
        rows, t0 = latent_target.as_strided((B * (Nm + 1), C), (C, 1), latent_target.storage_offset() - C), 1
    else:
        raise ValueError('latent_target with strides %s is neither contiguous nor the rows behind a class row: make it '
                         'contiguous first' % (latent_target.stride(),))
    return hnn.mse_loss(latent_pred.reshape(B * Nm, C), rows, B, Nm, t0)


def _cae(embed_dim, depth, num_heads, **kwargs):
    kwargs.setdefault('args', cae_pretrain_args())
    kwargs.setdefault('use_abs_pos_emb', False)
    kwargs.setdefault('init_values', kwargs['args'].layer_scale_init_value)
    kwargs.pop('drop_block_rate', None)
    return CAEPretrain(patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4, qkv_bias=True,
                       norm_layer=partial(hnn.LayerNorm, epsilon=1e-6), vocab_size=8192, **kwargs)


def cae_small_patch16_224_8k_vocab(**kwargs):
    return _cae(384, 12, 12, **kwargs)


def cae_base_patch16_224_8k_vocab(**kwargs):
    return _cae(768, 12, 12, **kwargs)


def cae_large_patch16_224_8k_vocab(**kwargs):
    return _cae(1024, 24, 16, **kwargs)
