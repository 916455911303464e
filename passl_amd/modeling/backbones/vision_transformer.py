"""The CLIP image tower and text transformer on the MI355X HIP kernels.

Constructor arguments, registry name and sub-layer / state_dict names follow
passl_v110/modeling/backbones/vision_transformer.py: Block :140-189 (pre-norm, QuickGELU, LayerNorm eps 1e-5),
Transformer :192-225, VisionTransformer :267-366 (patch conv, class_embedding concat, + positional_embedding,
norm_pre, blocks, ``norm_post(x[:, 0]) @ proj``).  Mlp / Attention / PatchEmbed, the block's forward, the causal
``attn_mask`` handling and the token assembly are the shared ones of passl_amd/modules/vit.py (re-exported here under
the reference's names); ``Block`` below only carries this file's constructor defaults.  The raw matrix parameters
``proj`` (and CLIP's ``text_projection``) keep their state_dict key but live in a bias-free Linear so that they run on
the GEMM kernels (``named_parameters`` shows them as ``<name>.weight``).  Dropout and stochastic depth are not used by
the CLIP recipe: both towers refuse a non-zero rate."""
import torch
import torch.nn as tnn

from ...hip import config, nn
from ...modules import vit
from ...modules.vit import (Attention, Identity, Mlp, PatchEmbed, ViTTrunk, _is_causal,      # noqa: F401
                            alias_matrix_param, conv_default_normal_, resolve_norm_layer, to_2tuple, trunc_normal_,
                            xavier_uniform_)
from .builder import BACKBONES

QuickGELU = nn.QuickGELU


class Block(vit.Block):
    """vit.Block with the defaults of vision_transformer.py:140-189: QuickGELU, 'nn.LayerNorm' with eps 1e-5."""

    def __init__(self, *args, act_layer=QuickGELU, norm_layer='nn.LayerNorm', epsilon=1e-5, **kwargs):
        super().__init__(*args, act_layer=act_layer, norm_layer=norm_layer, epsilon=epsilon, **kwargs)


class Transformer(nn.Layer):
    def __init__(self, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_mask=None, attn_drop_rate=0.0, drop_path_rate=0.0,
                 norm_layer='nn.LayerNorm', epsilon=1e-5, **args):
        super().__init__()
        assert drop_path_rate == 0.0, 'stochastic depth is not used by the CLIP recipe'
        assert drop_rate == 0.0, 'element-wise dropout is built for the v2 VisionTransformer only'
        self.embed_dim = embed_dim
        self.depth = depth
        self.blocks = tnn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_mask=attn_mask, attn_drop=attn_drop_rate, norm_layer=norm_layer,
                  epsilon=epsilon) for _ in range(depth)])

    def forward(self, x, B, T):
        for blk in self.blocks:
            x = blk(x, B, T)
        return x


@BACKBONES.register()
class VisionTransformer(ViTTrunk):
    """Vision Transformer with support for patch input (the CLIP image tower)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, class_dim=0, width=768, out_dim=512, depth=12,
                 num_heads=12, mlp_ratio=4, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0,
                 drop_path_rate=0.0, norm_layer='nn.LayerNorm', pre_norm=False, proj=False, output_cls_token=True,
                 patch_bias=True, epsilon=1e-5, **args):
        super().__init__()
        assert drop_rate == 0.0
        assert drop_path_rate == 0.0, 'stochastic depth is not used by the CLIP recipe'
        dev = config.get_device()
        self.class_dim = class_dim
        self.num_features = self.width = width
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=width,
                                      patch_bias=patch_bias)
        num_patches = self.patch_embed.num_patches
        scale = width ** -0.5
        self.class_embedding = tnn.Parameter(torch.zeros(1, 1, width, device=dev))
        self.positional_embedding = tnn.Parameter(torch.zeros(1, num_patches + 1, width, device=dev))
        self.proj = None
        if proj:
            self.proj = nn.Linear(width, out_dim, bias_attr=False)
            alias_matrix_param(self, 'proj')
        self.output_cls_token = output_cls_token
        norm = resolve_norm_layer(norm_layer)
        self.norm_pre = norm(width, epsilon=epsilon) if pre_norm else Identity()
        self.blocks = tnn.ModuleList([
            Block(dim=width, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, norm_layer=norm_layer, epsilon=epsilon)
            for _ in range(depth)])
        self.norm_post = norm(width, epsilon=epsilon)
        with torch.no_grad():
            # vision_transformer.py:331-342: every Linear trunc_normal(.02) / zero bias, LayerNorm (1, 0);
            # the patch conv keeps nn.Conv2D's default Normal(0, sqrt(2 / (k*k*in)))
            conv_default_normal_(self.patch_embed.proj.weight)
            trunc_normal_(self.positional_embedding)
            trunc_normal_(self.class_embedding)
            if self.proj is not None:
                self.proj.weight.copy_(torch.randn(self.proj.weight.shape) * scale)
            for m in self.modules():
                if isinstance(m, nn.Linear) and m is not self.proj:
                    trunc_normal_(m.weight)
                    if m.bias is not None:
                        m.bias.zero_()

    def forward_features(self, x):
        if self.proj is None:
            raise NotImplementedError('VisionTransformer without `proj` (dense patch-token outputs) is outside '
                                      'the CLIP pre-training path')
        x, cls_rows, B, L = self.embed_tokens(x, self.class_embedding, self.positional_embedding)
        x = self.run_blocks(self.norm_pre(x), B, L + 1)
        x = self.cls_features(x, cls_rows, self.norm_post)                # norm_post(x[:, 0, :])
        return self.proj(x, out_f32=True)                                 # @ proj, fp32 features

    def forward(self, x):
        return self.forward_features(x)
