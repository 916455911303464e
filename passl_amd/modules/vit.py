"""The Vision Transformer host code shared by the four towers: the MAE pre-training encoder / decoder and fine-tuning
ViT (modeling/backbones/mae.py), the CLIP image and text towers (modeling/backbones/vision_transformer.py), the v2
``VisionTransformer`` (models/vision_transformer.py) and ``MoCoV3ViT`` (models/mocov3.py).  It imports only from
passl_amd/hip; the towers import from here and not from each other.

Mlp / Attention / Block follow passl_v110/modeling/backbones/mae.py:61-189 and vision_transformer.py:69-189 (additive
attention mask before the softmax), PatchEmbed :228-264.  Execution: tokens are 2-D rows [B*T, C] in the compute
dtype; every Linear is the implicit-GEMM kernel (bias / residual add in the epilogue), LayerNorm / GELU / QuickGELU /
attention / token assembly are HIP kernels (csrc/vit.hip, csrc/attention.hip).  The only attention mask the reference
builds is CLIP's causal ``triu(-inf, 1)`` (clip.py:284-286): ``attn_mask`` is accepted as the string ``'causal'`` or a
tensor equal to that matrix and becomes the kernels' causal flag; any other mask raises.

A tower keeps what really differs: parameter names and registration order, its init rule, sin-cos buffer versus
learnable position table, its head.  ``ViTTrunk`` holds the steps they share."""
import math

import numpy as np
import torch
import torch.nn as tnn
from torch.autograd import Function

from ..hip import config, nn, ops, plan as P


def to_2tuple(x):
    """(x, x); a pair passes through (a non-square image size, as swin_transformer.py's own to_2tuple allows)."""
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


process_rank = nn.process_rank          # (the towers take it from here)


class Identity(nn.Layer):
    def forward(self, x):
        return x


# ---- initialisers: drawn on the host from torch's global generator, then copied to the parameter
@torch.no_grad()
def uniform_(w, a):
    w.copy_((torch.rand(w.shape) * 2 - 1) * a)


def xavier_uniform_(w, fan_in, fan_out):
    uniform_(w, math.sqrt(6.0 / (fan_in + fan_out)))


@torch.no_grad()
def trunc_normal_(w, std=0.02):
    # paddle TruncatedNormal(std): N(0, std) re-sampled (not wrapped) into [-2 std, 2 std]
    t = torch.empty(w.shape)
    torch.nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std)
    w.copy_(t)


@torch.no_grad()
def conv_default_normal_(w):
    """nn.Conv2D's default weight initialiser [Paddle-semantics]: Normal(0, sqrt(2 / (C * k * k))), the fan-in of the
    filter.  ``w``: [Cout, C, k, k]."""
    w.copy_(torch.randn(w.shape) * math.sqrt(2.0 / (w.shape[1] * w.shape[2] * w.shape[3])))


def resolve_norm_layer(norm_layer):
    """The reference evaluates the string ``norm_layer`` ("nn.LayerNorm"); a callable passes through."""
    if isinstance(norm_layer, str):
        if norm_layer != 'nn.LayerNorm':
            raise NotImplementedError("norm_layer %r (supported: ['nn.LayerNorm'])" % norm_layer)
        return nn.LayerNorm
    return norm_layer


def _is_causal(attn_mask):
    if attn_mask is None:
        return False
    if isinstance(attn_mask, str):
        if attn_mask != 'causal':
            raise NotImplementedError('attn_mask %r' % attn_mask)
        return True
    m = torch.as_tensor(attn_mask).float().cpu()
    T = m.shape[-1]
    ref = torch.triu(torch.full((T, T), -math.inf), 1)
    if m.shape != ref.shape or not torch.equal(m, ref):
        raise NotImplementedError('only the causal triu(-inf, 1) attention mask is supported by the HIP '
                                  'attention kernel')
    return True


def alias_matrix_param(parent, attr):
    """state_dict key '<attr>' <-> the bias-free Linear parent.<attr>.weight."""
    def save_hook(module, sd, prefix, local_metadata):
        k = prefix + attr + '.weight'
        if k in sd:
            sd[prefix + attr] = sd.pop(k)

    def load_hook(sd, prefix, *args):
        k = prefix + attr
        if k in sd:
            sd[prefix + attr + '.weight'] = sd.pop(k)
    parent._register_state_dict_hook(save_hook)
    parent._register_load_state_dict_pre_hook(load_hook)


# ---- layers
class _PatchProj(nn.Layer):
    """The 16x16/stride-16 patch-embedding convolution as a GEMM over patchified rows.  ``weight`` is
    logically [embed_dim, in_chans, p, p] (reference layout) and physically [embed_dim][p][p][in_chans]
    = the K-order the patchify kernel writes."""
    krsc_weight = True
    no_dgrad = True           # the image needs no gradient

    def __init__(self, in_chans, embed_dim, patch, bias=True):
        super().__init__()
        dev = config.get_device()
        self.patch, self.in_chans, self.out_features = patch, in_chans, embed_dim
        self.in_features = in_chans * patch * patch
        self.geom = P.ConvGeom(self.in_features, embed_dim, 1, 1, 0)
        self.weight = tnn.Parameter(torch.empty(embed_dim, in_chans, patch, patch, device=dev))
        self.bias = tnn.Parameter(torch.zeros(embed_dim, device=dev)) if bias else None
        self._rt = None
        self._plans = {}

    _plan = nn.Linear._plan

    def forward(self, rows):
        return nn._LinearFn.apply(rows, self.weight, self.bias, self, False, False, None)


class PatchEmbed(nn.Layer):
    """Image to Patch Embedding: the p x p / stride-p convolution as a GEMM over patchified rows."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten=True,
                 patch_bias=True):
        super().__init__()
        self.img_size, self.patch_size = to_2tuple(img_size), to_2tuple(patch_size)
        self.grid_size = (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1])
        self.patches_resolution = list(self.grid_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = _PatchProj(in_chans, embed_dim, self.patch_size[0], bias=patch_bias)
        self.norm = norm_layer(embed_dim) if norm_layer else Identity()

    def forward(self, x):
        B, C, H, W = x.shape
        assert H == self.img_size[0], f"Input image height ({H}) doesn't match model ({self.img_size[0]})."
        assert W == self.img_size[1], f"Input image width ({W}) doesn't match model ({self.img_size[1]})."
        dtype = nn._need_rt(self.proj).arena.dtype
        rows = ops.patchify(x.contiguous().float(), self.patch_size[0], dtype)
        return self.norm(self.proj(rows))                    # [B*L, embed_dim]


def _dropout_sites(layer, rate, sites, count):
    """The (DropoutState, site, ...) a layer with a non-zero rate needs in training mode; no fall-back to 'no dropout'."""
    if sites is None or len(sites) != 1 + count:
        raise RuntimeError('%s with dropout rate %g in training mode needs a DropoutState and %d site number(s)'
                           % (type(layer).__name__, rate, count))
    return sites


def _drop_or_add(y, residual, state, site):
    return nn.dropout(y, state, site) if residual is None else nn.dropout_add(y, residual, state, site)


class Mlp(nn.Layer):
    """fc2(drop(act(fc1(x)))) then drop again (vision_transformer.py:106-112: one Dropout layer applied at two
    places = two sites here).  With a rate, in training mode: the first dropout runs inside the GELU launch, the second
    with the residual add in one launch after fc2, whose epilogue then adds nothing.  ``sites``: (state, site after the
    activation, site after fc2)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        if self.drop.p > 0. and not isinstance(self.act, nn.GELU):
            raise NotImplementedError('Mlp(drop=%g): the dropout after the activation is built into the GELU launch '
                                      'only (csrc/dropout.hip), not %s' % (drop, type(self.act).__name__))

    def forward(self, x, residual=None, sites=None):
        if self.drop.p > 0. and self.training:
            state, s_act, s_out = _dropout_sites(self, self.drop.p, sites, 2)
            y = self.fc2(nn.gelu_dropout(self.fc1(x), state, s_act))
            return _drop_or_add(y, residual, state, s_out)
        return self.fc2(self.act(self.fc1(x)), residual=residual)


class Attention(nn.Layer):
    """``proj_drop``: dropout after the output projection (vision_transformer.py:153-155); in training mode it runs
    with the residual add in one launch after proj.  ``sites``: (state, site).  ``attn_drop`` would need the draw
    inside the attention kernel and is not built."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_mask=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        if attn_drop != 0.:
            raise NotImplementedError('attn_drop (dropout of the attention probabilities) is not built on the HIP path')
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = qk_scale or self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias_attr=None if qkv_bias else False)
        self.causal = _is_causal(attn_mask)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x, B, T, residual=None, sites=None):
        a = nn.attention(self.qkv(x), B, T, self.num_heads, self.head_dim, self.scale, causal=self.causal)
        if self.proj_drop.p > 0. and self.training:
            state, site = _dropout_sites(self, self.proj_drop.p, sites, 1)
            return _drop_or_add(self.proj(a), residual, state, site)
        return self.proj(a, residual=residual)


class Block(nn.Layer):
    """Pre-norm transformer block.  ``norm_layer``: the string 'nn.LayerNorm' or a callable; ``epsilon`` is handed to
    it when given (the CLIP towers do, the MAE-style towers bind it with ``partial``)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_mask=None,
                 attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, epsilon=None):
        super().__init__()
        # reference: DropPath(drop_path) if drop_path > 0. else Identity() (a layer without state); here the rate itself
        # and keep_prob = float32(1 - p), the value drop_path() turns into a tensor and divides by (mae.py:36-40)
        drop_path = float(drop_path)
        if not 0. <= drop_path < 1.:
            raise ValueError('drop_path must be in [0, 1), got %r' % drop_path)
        self.drop_path = drop_path
        self.keep_prob = float(np.float32(1.0) - np.float32(drop_path))
        # element-wise dropout after proj, after the activation and after fc2 (reference: proj_drop=drop, Mlp(drop=drop));
        # the owning model binds its DropoutState and the first of the block's three site numbers
        self.drop = float(drop)
        self._drop_state, self._drop_site = None, 0
        if self.drop > 0. and self.drop_path > 0.:
            raise NotImplementedError('Block(drop=%g, drop_path=%g): dropout and stochastic depth in one block are not '
                                      'built (no recipe sets both)' % (self.drop, self.drop_path))
        norm_layer = resolve_norm_layer(norm_layer)
        norm_kw = {} if epsilon is None else {'epsilon': epsilon}
        self.norm1 = norm_layer(dim, **norm_kw)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_mask=attn_mask,
                              attn_drop=attn_drop, proj_drop=drop)
        self.norm2 = norm_layer(dim, **norm_kw)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, B, T, keep=None):
        # x + attn(norm1(x)) and x + mlp(norm2(x)): the add runs in the epilogue of proj / fc2, the
        # fork's gradient add inside the LayerNorm backward kernel (nn.LayerNorm.fork)
        if self.drop_path > 0. and self.training:
            return self._forward_drop_path(x, B, T, keep)
        if self.drop > 0. and self.training:
            return self._forward_dropout(x, B, T)
        h, xr = self.norm1.fork(x)
        x = self.attn(h, B, T, residual=xr)
        h, xr = self.norm2.fork(x)
        return self.mlp(h, residual=xr)

    def _forward_drop_path(self, x, B, T, keep):
        # x + drop_path(f(norm(x))) (mae.py:186-187): the factor is per sample, the epilogue's are per column, so the
        # branch's last Linear runs without a residual and the add is a pass of its own.  keep: fp32 [2, B] on the
        # device (row 0 the attention branch, row 1 the MLP branch), 1 = kept
        if keep is None:
            raise RuntimeError('Block(drop_path=%g) in training mode needs its two rows of the keep table' % self.drop_path)
        h, xr = self.norm1.fork(x)
        x = nn.drop_path_add(self.attn(h, B, T), xr, keep[0], self.keep_prob, B, T)
        h, xr = self.norm2.fork(x)
        return nn.drop_path_add(self.mlp(h), xr, keep[1], self.keep_prob, B, T)

    def bind_dropout(self, state, first_site):
        """Sites first_site (after proj), first_site + 1 (after the activation), first_site + 2 (after fc2)."""
        self._drop_state, self._drop_site = state, int(first_site)

    def _forward_dropout(self, x, B, T):
        # x + drop(proj(.)) and x + drop(fc2(drop(act(.)))): the mask is per element, the epilogue's factors are per
        # column, so — as under stochastic depth — proj / fc2 run without a residual and the add is the dropout launch
        if self._drop_state is None:
            raise RuntimeError('Block(drop=%g) in training mode is not bound to a DropoutState (bind_dropout)' % self.drop)
        st, s = self._drop_state, self._drop_site
        h, xr = self.norm1.fork(x)
        x = self.attn(h, B, T, residual=xr, sites=(st, s))
        h, xr = self.norm2.fork(x)
        return self.mlp(h, residual=xr, sites=(st, s + 1, s + 2))


class _TokensFn(Function):
    """rows[b, 0] = cls + pos[0];  rows[b, 1 + k] = x[b, ids_keep[b, k]] + pos[1 + ids_keep[b, k]]: the MAE keep-gather,
    and with identity ids the reference's expand + concat + add (vision_transformer.py:352-357).  ``pos`` is a fixed
    buffer (sin-cos tables) or a learnable table; the latter's gradient is one column sum over the batch, which needs
    every token in place (identity ids)."""

    @staticmethod
    def forward(ctx, x, cls, pos, ids_keep, ids_restore, B, L):
        K = ids_keep.shape[1]
        learnable_pos = isinstance(pos, tnn.Parameter) and pos.requires_grad
        if learnable_pos and K != L:
            raise ValueError('a learnable position table needs all %d tokens kept, got %d' % (L, K))
        ctx.save_for_backward(ids_restore)
        ctx.params = (cls, pos) if learnable_pos else (cls,)
        ctx.dims = (B, L, K)
        nn.param_expect_grad(*ctx.params)
        return ops.mae_gather(x, cls.detach().view(-1), pos.detach().view(-1, pos.shape[-1]), ids_keep, B, L)

    @staticmethod
    def backward(ctx, dout):
        (ids_restore,) = ctx.saved_tensors
        B, L, K = ctx.dims
        for p in ctx.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dout = dout.contiguous()
        dx = ops.mae_gather_bwd(dout, ids_restore, ctx.params[0].grad, B, L, K)     # dx rows + dcls += sum_b dout[b, 0]
        for pos in ctx.params[1:]:
            ops.colsum_into(dout.view(B, -1), pos.grad.view(-1), accumulate=True)    # dpos[t] += sum_b dout[b, t]
        nn.param_grad_ready(*ctx.params)
        return dx, None, None, None, None, None, None


class ViTTrunk(nn.Layer):
    """What the towers' ``forward_features`` share: [cls | patches] + pos over all tokens, the block loop, the final norm
    over the class rows.  A tower owns its parameters, their names and their initialisation."""

    def __init__(self):
        super().__init__()
        self._ids = {}

    @staticmethod
    def check_attention_envelope(img_size, patch_size, embed_dim, num_heads, tokens):
        # the attention kernels' envelope (csrc/attention.hip: head dimension 32 or 64, at most 208 tokens): a model
        # outside it would build and then fail at its first forward — say so at construction (the reference is
        # shape-generic: passl/models/vision_transformer.py:142-156)
        if embed_dim % num_heads or embed_dim // num_heads not in ops.ATTENTION_HEAD_DIMS or \
                tokens > ops.ATTENTION_MAX_TOKENS:
            raise NotImplementedError(
                'VisionTransformer(img_size=%s, patch_size=%s, embed_dim=%d, num_heads=%d): %d tokens x head dimension '
                '%s is outside the HIP attention kernels (head dimension in %s, at most %d tokens; csrc/attention.hip) '
                '— 384^2 inputs and the huge / g / G / 6B widths need the key-tiled kernel that is not built'
                % (img_size, patch_size, embed_dim, num_heads, tokens, embed_dim / float(num_heads),
                   sorted(ops.ATTENTION_HEAD_DIMS), ops.ATTENTION_MAX_TOKENS))

    def identity_ids(self, B, L, device):
        """-> (ids [B, L] = arange(L) per sample, cls_rows [B] = the class token's row of each sample), cached."""
        key = (B, L)
        if key not in self._ids:
            self._ids[key] = (torch.arange(L, dtype=torch.int32, device=device).repeat(B, 1).contiguous(),
                              (torch.arange(B, dtype=torch.int32, device=device) * (L + 1)).contiguous())
        return self._ids[key]

    def embed_tokens(self, imgs, cls, pos):
        """-> (rows [B*(L+1), D] = concat(cls, patch_embed(imgs)) + pos, cls_rows, B, L)"""
        B = imgs.shape[0]
        L = self.patch_embed.num_patches
        x = self.patch_embed(imgs)                                        # [B*L, D]
        ids, cls_rows = self.identity_ids(B, L, x.device)
        return _TokensFn.apply(x, cls, pos, ids, ids, B, L), cls_rows, B, L

    def run_blocks(self, x, B, T, keep=None):
        """``keep``: the stochastic-depth table of this pass (a tower with nn.DropPathModel hands each block its two
        rows of it), or None."""
        if keep is None:
            for blk in self.blocks:
                x = blk(x, B, T)
        else:
            for blk in self.blocks:
                x = blk(x, B, T, self._drop_path_rows(keep, blk))
        return x

    def cls_features(self, x, cls_rows, norm):
        return norm(nn.gather_rows(x, cls_rows))                          # norm(x)[:, 0]: LayerNorm is per token
