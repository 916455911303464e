"""DeiT (passl_amd/models/deit.py) without a GPU: the state_dict keys and shapes of the fixture models and of the eight
factories against the reference's own (tests/golden/deit_layers.npz, deit_small.npz, deit_long.npz;
tests/golden/make_golden_deit.py), the refusals, ``load_pretrained(finetune=True)`` with its bicubic position-table
interpolation against the reference's, and the new YAML through the Engine on the CPU device."""
import collections
import os

import numpy as np
import pytest
import torch

import deit_model_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_model(**kw):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    hip_config.set_device('cpu')
    return PM.build_model(dict(kw))


def _keys(model):
    return ['%s:%s' % (k, 'x'.join(map(str, v.shape))) for k, v in model.state_dict().items()]


def test_state_dict_keys_and_shapes_of_the_fixture_models_and_all_eight_factories():
    import passl.models as PM
    from passl_amd.models import deit as DM
    for name, cases in MU.CASES.items():
        fx = MU.load(name)
        for tag, (cls_name, args, rate) in cases.items():
            model = _cpu_model(name=cls_name, drop_path_rate=rate, **args)
            # the reference lists a layer's own parameters where they were created, torch in front: the same set
            assert sorted(_keys(model)) == sorted(fx[tag + '/keys']), (name, tag)
            assert [b.drop_path for b in model.blocks] == MU.block_rates(rate, args['depth'])
    want = collections.defaultdict(list)
    for row in bytes(MU.load(MU.LAYERS)['factory_keys']).decode().split('\n'):
        f, k = row.split('|')
        want[f].append(k)
    assert sorted(want) == sorted(MU.FACTORIES) and len(want) == 8
    assert sorted(n for n in DM.__all__ if n.startswith('DeiT_')) == sorted(MU.FACTORIES)
    for f in want:
        model = getattr(PM, f)()
        assert sorted(_keys(model)) == sorted(want[f]), f
        assert type(model).__name__ == ('DistilledVisionTransformer' if 'distilled' in f else 'DeitVisionTransformer')
        assert model.norm._epsilon == 1e-6 and model.blocks[0].norm1._epsilon == 1e-6
    assert tuple(PM.DeiT_base_distilled_patch16_384().pos_embed.shape) == (1, 578, 768)


def test_identity_heads_without_classes():
    from passl_amd.modules.vit import Identity
    model = _cpu_model(name='DistilledVisionTransformer', **dict(MU.SMALL, class_num=0))
    assert isinstance(model.head, Identity) and isinstance(model.head_dist, Identity)
    assert not any(k.startswith('head') for k in model.state_dict())


def test_refusals_are_by_name():
    for cls_name in ('DeitVisionTransformer', 'DistilledVisionTransformer'):
        for kw, word in ((dict(drop_rate=0.1), 'drop_rate'), (dict(attn_drop_rate=0.1), 'attn_drop_rate'),
                         (dict(qk_scale=0.5), 'qk_scale')):
            with pytest.raises(NotImplementedError, match=word):
                _cpu_model(name=cls_name, **dict(MU.SMALL, **kw))
        with pytest.raises(ValueError):
            _cpu_model(name=cls_name, **dict(MU.SMALL, drop_path_rate=1.0))
    assert _cpu_model(name='DeitVisionTransformer', **dict(MU.SMALL, drop_rate=0.0)).drop_path_rate == 0.


def test_the_model_s_own_envelope_is_checked_at_construction():
    from passl_amd.hip import ops
    assert ops.ATTENTION_TILED_MAX_TOKENS == 1024 and ops.ATTENTION_MAX_TOKENS == 208
    # 32 x 32 patches + 1 = 1025 tokens; 1023 + 1 and 1022 + 2 fit
    with pytest.raises(NotImplementedError, match='1025 tokens'):
        _cpu_model(name='DeitVisionTransformer', **dict(MU.SMALL, img_size=64, patch_size=2))
    with pytest.raises(NotImplementedError, match='head dimension'):
        _cpu_model(name='DeitVisionTransformer', **dict(MU.SMALL, embed_dim=96, num_heads=2))
    with pytest.raises(NotImplementedError, match='head dimension'):
        _cpu_model(name='DeitVisionTransformer', **dict(MU.SMALL, embed_dim=64, num_heads=3))
    edge = dict(MU.SMALL, img_size=(62, 66), patch_size=2, depth=1)            # 31 x 33 = 1023 patch tokens
    assert _cpu_model(name='DeitVisionTransformer', **edge).pos_embed.shape[1] == 1024
    with pytest.raises(NotImplementedError, match='1025 tokens'):
        _cpu_model(name='DistilledVisionTransformer', **edge)
    assert _cpu_model(name='DeitVisionTransformer', **MU.LONG).pos_embed.shape[1] == 226


@pytest.mark.parametrize('tag,cls_name', [('plain', 'DeitVisionTransformer'), ('dist', 'DistilledVisionTransformer')])
def test_finetune_loading_interpolates_the_position_table_as_the_reference_does(tag, cls_name, tmp_path):
    from passl_amd.utils.checkpoint import dump_pdparams
    fx = MU.load(MU.LAYERS)
    src = _cpu_model(name=cls_name, **MU.POS_FROM)
    state = MU.fixture_state([(k, tuple(v.shape)) for k, v in src.state_dict().items()], seed=11)
    assert np.array_equal(state['pos_embed'].numpy(), fx['pos/%s/from' % tag])
    path = str(tmp_path / tag)
    dump_pdparams({k: v.numpy() for k, v in state.items()}, path)
    dst = _cpu_model(name=cls_name, **MU.POS_TO)
    dst.sync_runtime_state = lambda: None                  # the arena's device operands: there is no device here
    head = dst.head.weight.detach().clone()
    dst.load_pretrained(path, finetune=True)
    extra = 2 if tag == 'dist' else 1
    want = torch.from_numpy(fx['pos/%s/to' % tag])
    assert tuple(dst.pos_embed.shape) == tuple(want.shape) == (1, 25 + extra, 64)
    assert torch.equal(dst.pos_embed.detach()[:, :extra], state['pos_embed'][:, :extra])      # the extra tokens are kept
    assert float((dst.pos_embed.detach() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert bool(fx['pos/%s/head_kept' % tag]) and torch.equal(dst.head.weight.detach(), head)   # another shape: dropped
    assert bool(fx['pos/%s/cls_loaded' % tag]) and torch.equal(dst.cls_token.detach(), state['cls_token'])
    assert bool(fx['pos/%s/qkv_loaded' % tag])
    assert torch.equal(dst.blocks[1].attn.qkv.weight.detach(), state['blocks.1.attn.qkv.weight'])
    # a head of the same shape is loaded, not dropped
    same = _cpu_model(name=cls_name, **dict(MU.POS_TO, class_num=5))
    same.sync_runtime_state = lambda: None
    same.load_pretrained(path, finetune=True)
    assert torch.equal(same.head.weight.detach(), state['head.weight'])


def test_the_yaml_loads_and_the_engine_builds_its_no_decay_groups(tmp_path):
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    path = os.path.join(ROOT, 'configs', 'v2', 'deit_base_patch16_224_synthetic.yaml')
    header = open(path).read().split('\nGlobal:')[0]
    for word in ('TimmAutoAugment', 'TransformOpSampler', 'RandomResizedCrop', 'RandomErasing', 'RepeatedAugSampler',
                 'GradScaler', 'Export'):
        assert word in header, 'the header must say that %s is left out' % word
    cfg = get_config(path, ['Global.device=cpu', 'Global.output_dir=%s' % tmp_path,
                            'DataLoader.Train.dataset.num_samples=16', 'DataLoader.Train.dataset.num_classes=8',
                            'DataLoader.Train.sampler.batch_size=8', 'DataLoader.Eval.dataset.num_samples=8',
                            'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=8'])
    assert cfg['Model'] == dict(name='DeiT_base_patch16_224', drop_path_rate=0.1, drop_rate=0.0, class_num=1000)
    assert cfg['LRScheduler']['name'] == 'TimmCosine' and cfg['LRScheduler']['learning_rate'] == 1e-3
    assert cfg['LRScheduler']['eta_min'] == 1e-5 and cfg['LRScheduler']['warmup_start_lr'] == 1e-6
    assert cfg['LRScheduler']['decay_unit'] == 'epoch' and cfg['LRScheduler']['warmup_epoch'] == 5
    assert cfg['Optimizer']['weight_decay'] == 0.05 and list(cfg['Optimizer']['no_weight_decay_name']) == MU.NO_DECAY
    assert cfg['Optimizer']['eps'] == 1e-8 and cfg['Global']['seed'] == 42 and cfg['Global']['epochs'] == 300
    assert 'grad_clip' not in cfg['Optimizer']
    eng = Engine(cfg, mode='train')                        # the full DeiT-B builds on the CPU device
    assert type(eng.model).__name__ == 'DeitVisionTransformer' and type(eng.optimizer).__name__ == 'AdamW'
    rates = [b.drop_path for b in eng.model.blocks]
    assert rates == [float(r) for r in np.linspace(0, 0.1, 12)]
    cfg['Model'] = dict(name='DeitVisionTransformer', drop_path_rate=0.5, **MU.SMALL)
    eng = Engine(cfg, mode='train')
    fx = MU.load('deit_small')
    assert eng.no_weight_decay_names(MU.NO_DECAY) == list(fx['dp5/no_decay'])
    table = {n: wd for rows in eng.optimizer._param_table for n, _s, wd in rows}
    assert collections.Counter(table.values()) == {0.0: len(fx['dp5/no_decay']),
                                                   0.05: len(list(eng.model.parameters())) - len(fx['dp5/no_decay'])}
    assert eng.lr_decay_unit == 'epoch'


def test_fixtures_hold_what_the_issue_lists():
    for name, cases in MU.CASES.items():
        assert os.path.getsize(os.path.join(MU.HERE, 'golden', name + '.npz')) < 1 << 20
        fx = MU.load(name)
        for tag, (_cls, args, rate) in cases.items():
            keys = list(fx[tag + '/keys'])
            grads = [k for k in fx if k.startswith(tag + '/s0_grad/')]
            assert len(grads) == len(keys) and tag + '/s1_loss' in fx and tag + '/s0_logits' in fx
            assert float(fx[tag + '/rate']) == rate
            finals = {k[len(tag + '/final/'):] for k in fx if k.startswith(tag + '/final/')}
            assert finals == {k.split(':')[0] for k in keys
                              if int(np.prod([int(s) for s in k.split(':')[1].split('x')])) <= MU.FINAL_MAX}
            if rate:
                keep = fx[tag + '/s0_keep']
                assert keep.shape == (2 * args['depth'], MU.BATCH) and (keep[:2] == 1).all() and (keep == 0).any()
            for n in MU.zero_grad_names([k.split(':')[0] for k in keys]):
                g = fx[tag + '/s0_grad/' + n]
                assert float(np.abs(g[g.size // 3:2 * g.size // 3]).max()) <= 1e-6, n        # the key third
    long_keys = [k.split(':')[0] for k in MU.load('deit_long')['dist/keys']]
    assert 'dist_token' in long_keys and 'head_dist.weight' in long_keys
    assert 'pos_embed:1x227x64' in list(MU.load('deit_long')['dist/keys'])
