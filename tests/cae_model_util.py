"""What tests/golden/make_golden_cae.py (the reference run) and the CAE model tests share: the two small models, their
seed-defined state, inputs and masks, the solver settings and the fixture file (pure torch / numpy, no GPU).

Model 1: 96 pixels, patch 16 (6 x 6 = 36 patches, 14 of them masked by the block generator), embed_dim =
decoder_embed_dim = 128, 4 heads (head dimension 32), depth 2, regressor_depth 2, num_decoder_self_attention 2, a
vocabulary of 64, layer scale 0.1 with the gammas then set to order 1 by the fixture state, dual_path_ema 0.
Model 2: dual_path_ema 0.5 and decoder_embed_dim 64 (2 heads), so that encoder_to_decoder and its norm run, on the
teacher's output too.

The state is a function of the parameter names and shapes (convmae_model_util.py does the same); the teacher starts as
the encoder's copy, as the constructor leaves it.  The fixture then holds only what the reference COMPUTED."""
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
IMG, PATCH, GRID, L, NM = 96, 16, 6, 36, 14
VOCAB, BATCH, STEPS = 64, 2, 2
NORM_EPS = 1e-6
BASE_ARGS = dict(sincos_pos_emb=True, decoder_num_classes=VOCAB, decoder_embed_dim=128, decoder_num_heads=4,
                 regressor_depth=2, num_decoder_self_attention=2, decoder_layer_scale_init_value=0.1, dual_path_ema=0.0)
MODELS = {'m1': dict(), 'm2': dict(decoder_embed_dim=64, decoder_num_heads=2, dual_path_ema=0.5)}
MODEL_KW = dict(img_size=IMG, patch_size=PATCH, embed_dim=128, depth=2, num_heads=4, mlp_ratio=4, qkv_bias=True,
                vocab_size=VOCAB, drop_path_rate=0., use_abs_pos_emb=False, init_values=0.1)
# AdamW in the reference's two groups (main_pretrain.py:519-541), a clip that binds (the gradient norm is of order 1)
SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.05, clip_grad=0.05, dual_loss_weight=2.0)
MASK_SEED = 77
ROWS = 4                          # rows of logits / latents that the fixture records
BIG = 512                         # arrays with more elements are recorded as their first BIG elements (flat)


def args_of(name):
    return SimpleNamespace(**dict(BASE_ARGS, **MODELS[name]))


def fixture_state(keys_shapes, seed=4107):
    """name -> fp32 tensor for the STUDENT's keys (encoder.*, regressor_and_decoder.*, encoder_to_decoder*, mask_token),
    drawn in the order of the sorted names.  pos_embed keeps the constructor's sin-cos table; teacher_network.* is then
    the copy of encoder.*."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in sorted((n, tuple(sh)) for n, sh in keys_shapes):
        leaf = name.rsplit('.', 1)[-1]
        if name.startswith('teacher_network.') or leaf == 'pos_embed':
            continue
        if leaf in ('mask_token', 'cls_token'):
            t = torch.randn(shape, generator=gen) * 0.2
        elif leaf.startswith('gamma_'):                         # layer scale of order 1
            t = 0.5 + torch.rand(shape, generator=gen)
        elif leaf in ('bias', 'q_bias', 'v_bias'):
            t = torch.randn(shape, generator=gen) * 0.1
        elif len(shape) == 1:                                   # LayerNorm weight
            t = 1.0 + torch.randn(shape, generator=gen) * 0.1
        else:                                                   # the patch convolution [out, in, k, k], Linears [in, out]
            fan_in = int(np.prod(shape[1:])) if len(shape) == 4 else shape[0]
            t = torch.randn(shape, generator=gen) * (1.0 / fan_in) ** 0.5
        out[name] = t
    for name, shape in keys_shapes:
        if name.startswith('teacher_network.') and not name.endswith('pos_embed'):
            out[name] = out['encoder.' + name[len('teacher_network.'):]].clone()
    return out


def block_masks(n, grid=GRID, num_mask=NM, seed=MASK_SEED, min_num_patches=4):
    """n masks [n, grid * grid] int32 from the block generator after random.seed(seed) (the product's generator; the
    fixture holds the reference's for the same seed)."""
    from passl_amd.datasets.preprocess.masking import MaskingGenerator
    random.seed(seed)
    g = MaskingGenerator(grid, num_mask, min_num_patches=min_num_patches)
    return np.stack([g().reshape(-1) for _ in range(n)]).astype(np.int32)


def batches(masks):
    """[(imgs [B, 3, 96, 96] fp32, mask bool [B, L], labels int64 [B * NM])] for STEPS steps; ``masks``: int [STEPS * B, L]."""
    gen = torch.Generator().manual_seed(913)
    out = []
    for s in range(STEPS):
        imgs = torch.randn(BATCH, 3, IMG, IMG, generator=gen)
        ids = torch.randint(0, VOCAB, (BATCH, L), generator=gen)
        m = torch.from_numpy(np.asarray(masks[s * BATCH:(s + 1) * BATCH])).bool()
        out.append((imgs, m, ids[m]))
    return out


def decay_groups(named_params, skip=('pos_embed', 'cls_token')):
    """main_pretrain.py:519-541 on (name, shape) pairs of the student's trainable parameters -> (no_decay names, decay
    names).  The skip list holds the model's names 'pos_embed' / 'cls_token', which no full parameter name equals."""
    no_decay = [n for n, sh in named_params if len(sh) == 1 or n.endswith('.bias') or n in skip]
    return no_decay, [n for n, sh in named_params if n not in set(no_decay)]


def clip(a):
    a = np.asarray(a)
    return a.copy() if a.size <= BIG else a.reshape(-1)[:BIG].copy()


def load(name='cae_small'):
    with np.load(os.path.join(HERE, 'golden', name + '.npz')) as z:
        return {k: z[k] for k in z.files}
