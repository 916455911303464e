"""``passl.models.deit`` — DeiT (Training data-efficient image transformers & distillation through attention,
https://arxiv.org/abs/2012.12877) on the MI355X HIP path.

Names, constructor arguments, sub-layer / state_dict keys and shapes and the eight factories are the reference's
(passl/models/deit.py: DeitVisionTransformer :44-193, DistilledVisionTransformer :196-259, factories :262-365), so its
``.pdparams`` load.  The trunk is the shared one of passl_amd/modules/vit.py (``ViTTrunk``: Block / Attention / Mlp /
PatchEmbed over token rows [B*T, C]); what is DeiT's own:

  * stochastic depth with the ladder ``np.linspace(0, drop_path_rate, depth)`` (:84) over ``hnn.DropPathModel``: ONE
    keep-table draw per training forward, table [2 * depth, B], rows 2i / 2i + 1 the attention / MLP residual of block
    i (block 0 has rate 0 and ignores its rows), ``keep_prob = float32(1 - p)``; evaluation and rate 0 draw nothing;
  * sequences beyond the dense attention kernels: ``hnn.attention`` sends more than ``ops.ATTENTION_MAX_TOKENS`` (208)
    tokens to the key-tiled kernels (csrc/attention_tiled.hip), so the two 384-pixel factories (577 and 578 tokens) run,
    forward and backward;
  * the distilled class: two prefix rows ``cls_token`` / ``dist_token`` and a position table of ``num_patches + 2``
    rows, assembled by one streaming launch (``hnn.prefix_tokens``, csrc/deit_tokens.hip); both rows of every image are
    gathered at once, normalised (LayerNorm is per row) and split; ``forward`` returns
    ``(head(x) + head_dist(x_dist)) / 2`` in training and evaluation alike, as the reference does (:255-259; there
    is no teacher here).  No ATen launch: a strict step plan records the step.

Envelope, checked at construction: head dimension 32 or 64 and at most ``ops.ATTENTION_TILED_MAX_TOKENS`` (1024) tokens.

Initial values [Paddle-semantics] (:106-117, :234-236; only initial values): trunc-normal(0.002) Linear weights,
``pos_embed`` and ``cls_token`` of the plain class, zero biases, LayerNorm (1, 0); the distilled class redraws
``pos_embed`` and draws ``dist_token`` with trunc-normal(0.02); the patch convolution keeps Paddle's default.

Refused by name in the constructor: ``drop_rate > 0``, ``attn_drop_rate > 0``, ``qk_scale``."""
import numpy as np
import torch
import torch.nn as tnn

from ..hip import config, ops
from ..hip import nn as hnn
from ..hip.nn import EncoderArena
from ..modules.vit import (Block, Identity, PatchEmbed, ViTTrunk, conv_default_normal_, resolve_norm_layer,
                           trunc_normal_)
from ..utils.checkpoint import load_lenient, read_pdparams
from .base_model import Model

__all__ = [
    'DeiT_tiny_patch16_224', 'DeiT_small_patch16_224', 'DeiT_base_patch16_224', 'DeiT_tiny_distilled_patch16_224',
    'DeiT_small_distilled_patch16_224', 'DeiT_base_distilled_patch16_224', 'DeiT_base_patch16_384',
    'DeiT_base_distilled_patch16_384', 'DeitVisionTransformer', 'DistilledVisionTransformer',
]


class DeitVisionTransformer(hnn.DropPathModel, ViTTrunk, Model):
    """Vision Transformer with support for patch input."""

    NUM_PREFIX = 1                   # prefix rows in front of the patch rows: cls_token

    def __init__(self, img_size=224, patch_size=16, in_chans=3, class_num=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4, qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 norm_layer='nn.LayerNorm', epsilon=1e-5, **kwargs):
        super().__init__()
        who = type(self).__name__
        for name, v in (('drop_rate', drop_rate), ('attn_drop_rate', attn_drop_rate)):
            if v:
                raise NotImplementedError('%s(%s=%r): dropout is not built for DeiT (no config or factory sets it)'
                                          % (who, name, v))
        if qk_scale is not None:
            raise NotImplementedError('%s(qk_scale=%r): only the default head_dim ** -0.5 is built' % (who, qk_scale))
        if not 0. <= drop_path_rate < 1.:
            raise ValueError('drop_path_rate must be in [0, 1), got %r' % (drop_path_rate,))
        dev = config.get_device()
        self.class_num = class_num
        self.num_features = self.embed_dim = embed_dim
        self.drop_path_rate = float(drop_path_rate)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.check_tiled_attention_envelope(img_size, patch_size, embed_dim, num_heads, num_patches + self.NUM_PREFIX)
        self.pos_embed = tnn.Parameter(torch.zeros(1, num_patches + self.NUM_PREFIX, embed_dim, device=dev))
        self.cls_token = tnn.Parameter(torch.zeros(1, 1, embed_dim, device=dev))
        dpr = np.linspace(0, drop_path_rate, depth)
        self.blocks = tnn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias=qkv_bias, drop_path=dpr[i],
                                            norm_layer=norm_layer, epsilon=epsilon) for i in range(depth)])
        self.norm = resolve_norm_layer(norm_layer)(embed_dim, epsilon=epsilon)
        self.head = hnn.Linear(embed_dim, class_num) if class_num > 0 else Identity()
        self._make_extra_parameters(dev)
        with torch.no_grad():
            self._init_values()
        # every block owns two rows of the keep table when the rate is above 0 (block 0 with keep probability 1); the
        # seed is drawn after the weights (a model with stochastic depth initialises as one without)
        self._seed_drop_path(self.blocks if self.drop_path_rate > 0. else (), 2)
        self._prefix_rows = {}
        self.arena_q = EncoderArena(self, trainable=True)

    @staticmethod
    def check_tiled_attention_envelope(img_size, patch_size, embed_dim, num_heads, tokens):
        """DeiT's own envelope: the dense attention kernels up to ops.ATTENTION_MAX_TOKENS, the key-tiled ones beyond."""
        if embed_dim % num_heads or embed_dim // num_heads not in ops.ATTENTION_HEAD_DIMS or \
                tokens > ops.ATTENTION_TILED_MAX_TOKENS:
            raise NotImplementedError(
                'DeiT(img_size=%s, patch_size=%s, embed_dim=%d, num_heads=%d): %d tokens x head dimension %s is outside '
                'the HIP attention kernels (head dimension in %s, at most %d tokens; csrc/attention_tiled.hip)'
                % (img_size, patch_size, embed_dim, num_heads, tokens, embed_dim / float(num_heads),
                   sorted(ops.ATTENTION_HEAD_DIMS), ops.ATTENTION_TILED_MAX_TOKENS))

    def _make_extra_parameters(self, dev):
        """The distilled class adds its parameters here: after ``head``, the reference's registration order."""

    def _init_values(self):
        trunc_normal_(self.pos_embed, std=.002)
        trunc_normal_(self.cls_token, std=.002)
        for m in self.modules():
            if isinstance(m, hnn.Linear):
                trunc_normal_(m.weight, std=.002)
                if m.bias is not None:
                    m.bias.zero_()
        conv_default_normal_(self.patch_embed.proj.weight)            # Paddle's default for nn.Conv2D
        self.patch_embed.proj.bias.zero_()

    # ---- forward
    def _logits(self, layer, x):
        if isinstance(layer, Identity):
            return x
        if x.dtype == torch.float32 or self.num_features % 64 == 0:
            return layer(x, out_f32=True)
        return hnn.to_f32(layer(x))      # bf16 rows of a width that is no multiple of 64: rounded once, then widened

    def forward_features(self, x, drop_path_keep=None):
        keep = self._drop_path_keep(x.shape[0], x.device, drop_path_keep)
        x, cls_rows, B, L = self.embed_tokens(x, self.cls_token, self.pos_embed)     # concat(cls, x) + pos_embed
        return self.cls_features(self.run_blocks(x, B, L + 1, keep), cls_rows, self.norm)

    def forward(self, x, drop_path_keep=None):
        self.arena_q.refresh()                       # compute-dtype operands and data-gradient packs of the updated weights
        return self._logits(self.head, self.forward_features(x, drop_path_keep))

    # ---- deit.py:137-190
    def load_pretrained(self, path, rank=0, finetune=False):
        sd = read_pdparams(path)
        if finetune:
            own = self.state_dict()
            # the reference names the head alone; its set_dict then skips a head_dist of another shape with a warning
            # [Paddle-semantics], which torch's load_state_dict would refuse
            for k in ['head.weight', 'head.bias', 'head_dist.weight', 'head_dist.bias']:
                if k in sd and (k not in own or tuple(sd[k].shape) != tuple(own[k].shape)):
                    print(f'Removing key {k} from pretrained checkpoint')
                    del sd[k]
            pos = torch.as_tensor(sd['pos_embed']).float()
            n_new = self.patch_embed.num_patches
            extra = self.pos_embed.shape[-2] - n_new             # class_token and dist_token are kept unchanged
            orig, new = int((pos.shape[-2] - extra) ** 0.5), int(n_new ** 0.5)
            # bicubic interpolation of the position tokens on the host (once)
            tok = pos[0, extra:].reshape(-1, orig, orig, pos.shape[-1]).permute(0, 3, 1, 2)
            tok = torch.nn.functional.interpolate(tok, size=(new, new), mode='bicubic', align_corners=False)
            sd['pos_embed'] = torch.cat([pos[:, :extra], tok.permute(0, 2, 3, 1).flatten(1, 2)], dim=1).numpy()
        load_lenient(self, sd, what='pretrained DeiT')
        self.sync_runtime_state()


class DistilledVisionTransformer(DeitVisionTransformer):
    NUM_PREFIX = 2                   # cls_token, dist_token

    def __init__(self, img_size=224, patch_size=16, class_num=1000, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4,
                 qkv_bias=False, norm_layer='nn.LayerNorm', epsilon=1e-5, **kwargs):
        super().__init__(img_size=img_size, patch_size=patch_size, class_num=class_num, embed_dim=embed_dim, depth=depth,
                         num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, norm_layer=norm_layer,
                         epsilon=epsilon, **kwargs)

    def _make_extra_parameters(self, dev):
        self.dist_token = tnn.Parameter(torch.zeros(1, 1, self.embed_dim, device=dev))
        self.head_dist = hnn.Linear(self.embed_dim, self.class_num) if self.class_num > 0 else Identity()

    def _init_values(self):
        super()._init_values()
        trunc_normal_(self.dist_token, std=.02)
        trunc_normal_(self.pos_embed, std=.02)

    def _two_rows(self, B, T, device):
        """-> int32 [2 B]: the class row of every image, then the distillation row of every image; cached."""
        key = (B, T)
        if key not in self._prefix_rows:
            first = torch.arange(B, dtype=torch.int32, device=device) * T
            self._prefix_rows[key] = torch.cat([first, first + 1]).contiguous()
        return self._prefix_rows[key]

    def forward_features(self, x, drop_path_keep=None):
        B, L = x.shape[0], self.patch_embed.num_patches
        keep = self._drop_path_keep(B, x.device, drop_path_keep)
        x = hnn.prefix_tokens(self.patch_embed(x), (self.cls_token, self.dist_token), self.pos_embed, B, L)
        x = self.run_blocks(x, B, L + 2, keep)
        x = self.norm(hnn.gather_rows(x, self._two_rows(B, L + 2, x.device)))     # norm(x)[:, 0], norm(x)[:, 1]
        return hnn.split_rows(x, B)

    def forward(self, x, drop_path_keep=None):
        self.arena_q.refresh()
        x, x_dist = self.forward_features(x, drop_path_keep)
        return hnn.mean2(hnn.to_f32(self._logits(self.head, x)), hnn.to_f32(self._logits(self.head_dist, x_dist)))


def _deit(cls, img_size, embed_dim, num_heads, **kwargs):
    kwargs.setdefault('img_size', img_size)
    return cls(patch_size=16, embed_dim=embed_dim, depth=12, num_heads=num_heads, mlp_ratio=4,
               qkv_bias=True, epsilon=1e-6, **kwargs)


def DeiT_tiny_patch16_224(**kwargs):
    return _deit(DeitVisionTransformer, 224, 192, 3, **kwargs)


def DeiT_small_patch16_224(**kwargs):
    return _deit(DeitVisionTransformer, 224, 384, 6, **kwargs)


def DeiT_base_patch16_224(**kwargs):
    return _deit(DeitVisionTransformer, 224, 768, 12, **kwargs)


def DeiT_base_patch16_384(**kwargs):
    return _deit(DeitVisionTransformer, 384, 768, 12, **kwargs)


def DeiT_tiny_distilled_patch16_224(**kwargs):
    return _deit(DistilledVisionTransformer, 224, 192, 3, **kwargs)


def DeiT_small_distilled_patch16_224(**kwargs):
    return _deit(DistilledVisionTransformer, 224, 384, 6, **kwargs)


def DeiT_base_distilled_patch16_224(**kwargs):
    return _deit(DistilledVisionTransformer, 224, 768, 12, **kwargs)


def DeiT_base_distilled_patch16_384(**kwargs):
    return _deit(DistilledVisionTransformer, 384, 768, 12, **kwargs)
