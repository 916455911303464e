"""ConvMAE without a GPU: the fixtures against a live run of the reference (when its tree is present), state_dict keys
and shapes of the small models and the two factories against the lists recorded from the reference classes
(tests/golden/convmae_keys.json), the drop-path ladder, the refusals, the package alias, and that the fixtures load."""
import json
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

import convmae_model_util as MU
from passl_amd.hip import config as hip_config
from passl_amd.hip import nn as hnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir('/root/reference/passl/models/convmae')
KEYS = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'convmae_keys.json')))


@pytest.mark.skipif(not HAVE_REF, reason='reference tree not present')
def test_fixtures_equal_a_live_reference_run():
    """tests/golden/make_golden_convmae.py --check in a process of its own (the reference's `passl` package cannot live
    next to the product's): the three fixture files and the key lists, exactly."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'golden', 'make_golden_convmae.py'), '--check'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'fixtures equal the live reference run' in r.stdout


def _host():
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    import passl.models as PM
    return PM, partial(hnn.LayerNorm, epsilon=MU.NORM_EPS)


def _product(name):
    PM, norm = _host()
    if name == 'convmae_small':
        return PM.MaskedAutoencoderConvViT(norm_layer=norm, **MU.MAE_MODEL)
    if name == 'convvit_small':
        return PM.ConvViT(norm_layer=norm, **MU.VIT_MODEL)
    if name == 'convvit_small_pool':
        return PM.ConvViT(norm_layer=norm, global_pool=True, **MU.VIT_MODEL)
    return PM.build_model(dict(name=name))


@pytest.mark.parametrize('name', sorted(KEYS))
def test_state_dict_keys_and_shapes_are_the_reference_classes(name):
    got = {k: list(v.shape) for k, v in _product(name).state_dict().items()}
    want = dict((k, s) for k, s in KEYS[name])
    assert sorted(got) == sorted(want)
    assert got == want


def test_key_lists_hold_what_the_issue_names():
    base = dict((k, s) for k, s in KEYS['convmae_convvit_base_patch16'])
    assert base['blocks1.0.attn.weight'] == [256, 1, 5, 5] and base['blocks2.1.attn.weight'] == [384, 1, 5, 5]
    assert base['blocks1.0.conv1.weight'] == [256, 256, 1, 1] and base['blocks1.0.mlp.fc1.weight'] == [1024, 256, 1, 1]
    assert base['stage1_output_decode.weight'] == [768, 256, 4, 4]
    assert base['stage2_output_decode.weight'] == [768, 384, 2, 2]
    assert base['patch_embed3.proj.weight'] == [768, 384, 2, 2] and base['patch_embed4.weight'] == [768, 768]
    assert base['pos_embed'] == [1, 196, 768] and base['decoder_pos_embed'] == [1, 196, 512]
    assert base['mask_token'] == [1, 1, 512] and base['decoder_pred.weight'] == [512, 768]
    assert 'cls_token' not in base
    vit = dict((k, s) for k, s in KEYS['convvit_base_patch16'])
    assert vit['head.weight'] == [768, 1000] and 'norm.weight' in vit and 'fc_norm.weight' not in vit
    pool = dict((k, s) for k, s in KEYS['convvit_small_pool'])
    assert 'fc_norm.weight' in pool and 'norm.weight' not in pool


def test_the_scripts_import_path_resolves():
    import passl.models.convmae as A
    import passl_amd.models.convmae as B
    assert A is B
    assert A.convmae_convvit_base_patch16 is A.convmae_convvit_base_patch16_dec512d8b
    for n in ('CMlp', 'CBlock', 'CPatchEmbed', 'ConvViT', 'MaskedAutoencoderConvViT', 'convvit_base_patch16'):
        assert hasattr(A, n), n
    import passl.models as PM
    assert PM.convvit_base_patch16 is A.convvit_base_patch16 and PM.MaskedAutoencoderConvViT is A.MaskedAutoencoderConvViT


def test_epsilons_and_trainable_set_are_the_references():
    """CBlock / CPatchEmbed norm at Paddle's default 1e-5 whatever norm_layer says; stage 3, norm and the decoder at the
    factory's 1e-6; pos_embed trainable, decoder_pos_embed a buffer."""
    m = _product('convmae_small')
    assert m.blocks1[0].norm1._epsilon == 1e-5 and m.blocks2[0].norm2._epsilon == 1e-5
    assert m.patch_embed1.norm._epsilon == 1e-5 and m.patch_embed3.norm._epsilon == 1e-5
    assert m.blocks3[0].norm1._epsilon == 1e-6 and m.norm._epsilon == 1e-6 and m.decoder_norm._epsilon == 1e-6
    names = dict(m.named_parameters())
    assert 'pos_embed' in names and names['pos_embed'].requires_grad and 'decoder_pos_embed' not in names
    assert 'decoder_pos_embed' in dict(m.named_buffers())
    fx = MU.load('convmae_small')
    assert sorted('s0_grad/' + n for n in names) == sorted(k for k in fx if k.startswith('s0_grad/'))
    assert float(np.abs(fx['s0_grad/pos_embed']).max()) > 0, 'the reference does update pos_embed'


def test_drop_path_ladder_is_the_fixtures():
    PM, norm = _host()
    for name, rate in MU.VIT_CASES.items():
        fx = MU.load(name)
        model = PM.ConvViT(norm_layer=norm, drop_path_rate=rate, **MU.VIT_MODEL)
        assert np.array_equal(np.asarray(model.dp_rates, dtype=np.float64), fx['dp_rates'])
        blocks = list(model.blocks1) + list(model.blocks2) + list(model.blocks3)
        assert [b.drop_path for b in blocks] == model.dp_rates
        _rates, keep_prob = MU.ladder(rate)
        assert [b.keep_prob for b in blocks if b.drop_path > 0 for _ in range(2)] == keep_prob
        owners = model._drop_path.blocks if model._drop_path is not None else []
        assert len(owners) == (len(blocks) if rate else 0)
        if rate:
            for prefix, _pool in MU.POOLS:
                k = fx[prefix + 's0_keep']
                assert k.shape == (2 * (len(blocks) - 1), MU.BATCH) and set(np.unique(k)) <= {0.0, 1.0}


def test_fixtures_load_and_hold_what_the_tests_read():
    fx = MU.load('convmae_small')
    assert fx['s0_noise'].shape == (MU.BATCH, MU.L) and fx['s0_mask'].shape == (MU.BATCH, MU.L)
    assert fx['s0_ids_restore'].dtype == np.int32 and int(fx['s0_mask'].sum()) == MU.BATCH * (MU.L - MU.K)
    assert fx['s0_pred'].shape == (MU.BATCH, MU.PRED_ROWS, MU.P)
    assert np.isfinite(fx['s0_loss']) and np.isfinite(fx['s1_loss']) and fx['s0_loss'] != fx['s1_loss']
    noise = MU.batches()[0][2].numpy()
    assert np.array_equal(noise, fx['s0_noise'])
    assert np.array_equal(np.argsort(np.argsort(noise, 1, kind='stable'), 1, kind='stable').astype(np.int32),
                          fx['s0_ids_restore'])
    for name in MU.VIT_CASES:
        fx = MU.load(name)
        for prefix, _pool in MU.POOLS:
            assert fx[prefix + 's0_logits'].shape == (MU.BATCH, MU.VIT_MODEL['num_classes'])
            assert any(k.startswith(prefix + 'final/') for k in fx)
    for f in ('convmae_small.npz', 'convvit_small.npz', 'convvit_small_dp.npz', 'convmae_keys.json'):
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f)) < 1 << 20


def test_refusals():
    PM, norm = _host()
    with pytest.raises(NotImplementedError):
        PM.ConvViT(drop_rate=0.1, **MU.VIT_MODEL)
    with pytest.raises(NotImplementedError):
        PM.ConvViT(attn_drop_rate=0.1, **MU.VIT_MODEL)
    with pytest.raises(NotImplementedError):
        PM.ConvViT(hybrid_backbone=object(), **MU.VIT_MODEL)
    with pytest.raises(ValueError):
        PM.ConvViT(drop_path_rate=1.0, **MU.VIT_MODEL)
    with pytest.raises(NotImplementedError):
        PM.ConvViT(**dict(MU.VIT_MODEL, embed_dim=[12, 24, 64]))
    with pytest.raises(NotImplementedError):
        PM.ConvViT(**dict(MU.VIT_MODEL, img_size=[224, 60, 28]))
    with pytest.raises(NotImplementedError):
        PM.MaskedAutoencoderConvViT(**dict(MU.MAE_MODEL, img_size=[224, 56, 30]))
    with pytest.raises(NotImplementedError):                 # head dimension 48: outside the attention kernels
        PM.MaskedAutoencoderConvViT(**dict(MU.MAE_MODEL, embed_dim=[16, 24, 96]))
    from passl.models.convmae import CBlock, CMlp
    with pytest.raises(NotImplementedError):
        CBlock(16, drop=0.1)
    with pytest.raises(NotImplementedError):
        CMlp(16, 64, drop=0.1)
    m = PM.MaskedAutoencoderConvViT(norm_layer=norm, **MU.MAE_MODEL)
    with pytest.raises(ValueError):
        m.random_masking_ids(2, 196, 0.999)


def test_yaml_carries_the_scripts_values_and_builds():
    """configs/mae/convmae_convvit_b_synthetic.yaml: the values of pretrain_convmae.sh, and the v110 builder makes the
    model from it (at a reduced width: only the construction path is exercised here)."""
    from passl_amd.modeling.architectures import build_model
    from passl_amd.utils.config import get_config
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    cfg = get_config(os.path.join(ROOT, 'configs', 'mae', 'convmae_convvit_b_synthetic.yaml'), [])
    assert cfg.epochs == 1600 and cfg.lr_scheduler.warmup_steps == 40 and cfg.model.mask_ratio == 0.75
    assert cfg.dataloader.train.sampler.batch_size == 128
    assert cfg.optimizer.weight_decay == 0.05 and cfg.optimizer.beta2 == 0.95
    assert abs(cfg.lr_scheduler.learning_rate.learning_rate - 1.5e-4 * 128 / 256) < 1e-15
    arch = cfg.model.architecture
    assert arch.norm_pix_loss is True and arch.epsilon == 1e-6
    full = dict((k, s) for k, s in KEYS['convmae_convvit_base_patch16'])
    assert [full['blocks1.0.attn.weight'][0], full['blocks2.0.attn.weight'][0], full['pos_embed'][2]] == \
        list(arch.embed_dim)
    arch.update(embed_dim=[16, 24, 64], depth=[1, 1, 2], num_heads=2, decoder_embed_dim=64, decoder_depth=1,
                decoder_num_heads=2)
    model = build_model(cfg.model)
    assert type(model.backbone).__name__ == 'ConvMAE' and not hasattr(model.backbone, 'arena_q')
    got = {k: list(v.shape) for k, v in model.backbone.state_dict().items()}
    assert got == dict((k, s) for k, s in KEYS['convmae_small'])
