"""``ConvMAE`` — the v110-schema name of the ConvMAE masked autoencoder, so that a YAML with
``model: {name: MAE_PRETRAIN, architecture: {name: ConvMAE, ...}}`` trains through the v110 Trainer as the plain MAE
does.  The model is passl_amd/models/convmae/conv_mae.py's; the ``MAE_PRETRAIN`` wrapper owns the parameter arena (as
for ``MAE``), and ``epsilon`` stands for the factories' ``norm_layer=partial(nn.LayerNorm, epsilon=1e-6)``, which a
YAML cannot spell.  The defaults are convmae_convvit_base_patch16's."""
from functools import partial

from ...hip import nn
from ...models.convmae.conv_mae import MaskedAutoencoderConvViT
from .builder import BACKBONES


@BACKBONES.register()
class ConvMAE(MaskedAutoencoderConvViT):
    _own_arena = False

    def __init__(self, img_size=(224, 56, 28), patch_size=(4, 2, 2), in_chans=3, embed_dim=(256, 384, 768),
                 depth=(2, 2, 11), num_heads=12, decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=16,
                 mlp_ratio=(4, 4, 4), epsilon=1e-6, norm_pix_loss=False):
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, depth=depth,
                         num_heads=num_heads, decoder_embed_dim=decoder_embed_dim, decoder_depth=decoder_depth,
                         decoder_num_heads=decoder_num_heads, mlp_ratio=mlp_ratio,
                         norm_layer=partial(nn.LayerNorm, epsilon=epsilon), norm_pix_loss=norm_pix_loss)
