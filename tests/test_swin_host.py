"""Swin on the CPU: the float64 restatement of tests/swin_util.py against what the reference's own WindowAttention and
SwinTransformerBlock computed (tests/golden/swin_layers.npz), the kernels' closed forms against the literal roll /
partition / mask / index constructions, planted defects against the criteria of the GPU test, and the model's names,
groups and refusals.  No GPU, no kernel."""
import collections
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_util as A
import swin_model_util as MU
import swin_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYER_CASE = (2, 8, 12, 4, 2, 2, 32)          # the recorded block: 8 x 12 map, window 4, shift 2, 2 heads of 32


def _layers():
    z = MU.load(MU.LAYERS)
    st = {k[len('layer/state/'):]: torch.from_numpy(v).double() for k, v in z.items() if k.startswith('layer/state/')}
    return z, st


def _attention(st, x_map):
    """qkv Linear -> swin_util.reference (map order) -> out [B, L, C] before proj."""
    B, Hp, Wp, ws, shift, nH, DH = LAYER_CASE
    qkv = (x_map @ st['attn.qkv.weight'] + st['attn.qkv.bias']).reshape(B, Hp * Wp, 3, nH, DH)
    r = S.reference(LAYER_CASE, qkv, torch.zeros(B, Hp * Wp, nH, DH), st['attn.relative_position_bias_table'], DH ** -0.5)
    return r['out'].reshape(B, Hp * Wp, nH * DH)


def test_restatement_equals_the_reference_layers():
    z, st = _layers()
    B, Hp, Wp, ws, shift, nH, DH = LAYER_CASE
    assert np.array_equal(z['layer/index'], S.relative_position_index(ws).numpy())
    assert np.array_equal(z['layer/attn_mask'], S.attn_mask(Hp, Wp, ws, shift).numpy().astype(np.float32))
    # WindowAttention on recorded windows: put them where the shifted, partitioned map has them
    xw = torch.from_numpy(z['layer/xw']).double()
    x_map = S._from_windows(xw, B, Hp, Wp, ws, shift)
    out = S._to_windows(_attention(st, x_map), B, Hp, Wp, ws, shift) @ st['attn.proj.weight'] + st['attn.proj.bias']
    ref = torch.from_numpy(z['layer/attn_out']).double()
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # the whole shifted block
    x = torch.from_numpy(z['layer/x']).double()
    C = x.shape[-1]
    h = F.layer_norm(x, (C,), st['norm1.weight'], st['norm1.bias'], 1e-5)
    x1 = x + _attention(st, h) @ st['attn.proj.weight'] + st['attn.proj.bias']
    h = F.layer_norm(x1, (C,), st['norm2.weight'], st['norm2.bias'], 1e-5)
    h = F.gelu(h @ st['mlp.fc1.weight'] + st['mlp.fc1.bias']) @ st['mlp.fc2.weight'] + st['mlp.fc2.bias']
    ref = torch.from_numpy(z['layer/block_out']).double()
    assert float((x1 + h - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize('case', S.CASES + (LAYER_CASE,), ids=S.case_id)
def test_closed_forms_equal_the_literal_constructions(case):
    B, Hp, Wp, ws, shift, nH, DH = case
    assert np.array_equal(S.closed_index(ws), S.relative_position_index(ws).numpy())
    assert np.array_equal(S.closed_mask(Hp, Wp, ws, shift), S.attn_mask(Hp, Wp, ws, shift).numpy())
    token = torch.arange(Hp * Wp, dtype=torch.float64).reshape(1, Hp * Wp, 1)
    rows = S._to_windows(token, 1, Hp, Wp, ws, shift).reshape(-1, ws * ws).long().numpy()
    assert np.array_equal(rows, S.closed_rows(Hp, Wp, ws, shift))
    back = S._from_windows(S._to_windows(token, 1, Hp, Wp, ws, shift), 1, Hp, Wp, ws, shift)
    assert torch.equal(back, token)
    if shift:
        lab = S.closed_labels(Hp, Wp, ws, shift)
        assert lab.min() == 0 and lab.max() == 8 and len(np.unique(lab[-1])) == 4       # the corner window: four regions


def _verdicts(case, kind, std, defect):
    """{tensor: share of the bf16 allowance used} of the rounding model (with a planted defect) against the reference."""
    d = S.case_data(case, kind, std)
    m = S.reference(case, d['qkv'], d['dout'], d['table'], d['scale'], model=True, defect=defect)
    return {n: S.limit_usage(m[n], d['ref'][n], d['ref']['b_' + n], S.LIMIT_BF16[n])[0] for n in S.TENSORS}


@pytest.mark.parametrize('case', [S.CASES[1], S.CASES[2]], ids=S.case_id)
def test_criteria_pass_the_rounding_model_and_see_planted_defects(case):
    for kind in S.KINDS:
        for std in S.TABLE_STD:
            used = _verdicts(case, kind, std, None)
            assert max(used.values()) <= 1, (kind, std, used)
            ref = S.case_data(case, kind, std)['ref']
            for n in S.TENSORS:
                assert A.underflow_share(ref['b_' + n]) <= 0.01, (kind, std, n)
    for defect in S.DEFECTS[:3]:
        used = _verdicts(case, 'plain', 1.0, defect)
        assert max(used.values()) > 1, 'the criteria do not see the planted defect %s: %s' % (defect, used)


def test_criteria_see_a_table_gradient_taken_from_the_rounded_dS():
    """The fourth planted defect: dtable summed from the bf16-rounded dS instead of the fp32 one.  On
    swin_util.one_pair_inputs() the rounding model is inside every limit and the defective gradient is outside dtable's
    1.25 u (and inside every other tensor's)."""
    qkv, dout, table, scale = S.one_pair_inputs()
    assert torch.equal(qkv, A.bf16_round(qkv)) and torch.equal(dout, A.bf16_round(dout))
    ref = S.reference(S.ONE_PAIR_CASE, qkv, dout, table, scale)
    used = {}
    for defect in (None, 'dtable_rounded'):
        m = S.reference(S.ONE_PAIR_CASE, qkv, dout, table, scale, model=True, defect=defect)
        used[defect] = {n: S.limit_usage(m[n], ref[n], ref['b_' + n], S.LIMIT_BF16[n]) for n in S.TENSORS}
    print('share of the allowance used:', {d: {n: round(u[0], 3) for n, u in v.items()} for d, v in used.items()})
    assert max(u for u, _i in used[None].values()) <= 1, used[None]
    worst, idx = used['dtable_rounded']['dtable']
    assert worst > 1 and idx == int(S.relative_position_index(2)[3, 0]), (worst, idx)     # the bin of the pair (3, 0)
    assert all(used['dtable_rounded'][n][0] <= 1 for n in S.TENSORS if n != 'dtable')


def _cpu_model(**kw):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    hip_config.set_device('cpu')
    return PM.build_model(dict(kw))


def _keys(model):
    return ['%s:%s' % (k, 'x'.join(map(str, v.shape))) for k, v in model.state_dict().items()]


def test_state_dict_keys_and_shapes_of_the_fixture_model_and_all_thirteen_factories():
    import passl.models as PM
    from passl_amd.models import swin_transformer as ST
    fx = MU.load('swin_small')
    model = _cpu_model(name='SwinTransformer', drop_path_rate=0.5, **MU.MODEL)
    assert _keys(model) == list(fx['keys'])
    assert sorted(model.no_weight_decay()) == list(fx['model_no_weight_decay'])
    assert np.array_equal(model.layers[0].blocks[1].attn_mask.numpy(), S.attn_mask(8, 16, 4, 2).numpy().astype(np.float32))
    assert [b.shift_size for layer in model.layers for b in layer.blocks] == [0, 2, 0, 0]      # 4 x 8 map: no shift
    assert [b.drop_path for b in model._blocks] == np.linspace(0, 0.5, 4).tolist()
    assert model.group_matcher()['stem'] == r'^absolute_pos_embed|patch_embed' and model.get_classifier() is model.head
    want = collections.defaultdict(list)
    for row in bytes(MU.load(MU.LAYERS)['factory_keys']).decode().split('\n'):
        f, k = row.split('|')
        want[f].append(k)
    assert sorted(want) == sorted(n for n in ST.__all__ if n != 'SwinTransformer') and len(want) == 13
    for f in want:
        assert _keys(getattr(PM, f)()) == want[f], f


def test_engine_builds_the_no_decay_groups_of_the_yaml(tmp_path):
    from passl.engine.engine import Engine
    from passl_amd.utils.config import AttrDict, get_config
    path = os.path.join(ROOT, 'configs', 'v2', 'swin_base_synthetic.yaml')
    header = open(path).read().split('\nGlobal:')[0]
    for word in ('TimmAutoAugment', 'TransformOpSampler', 'RandomResizedCrop'):
        assert word in header, 'the header must say that %s is left out' % word
    cfg = get_config(path, ['Global.device=cpu', 'Global.output_dir=%s' % tmp_path,
                            'DataLoader.Train.dataset.num_samples=16', 'DataLoader.Train.dataset.image_size=64',
                            'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=8',
                            'DataLoader.Eval.dataset.num_samples=8', 'DataLoader.Eval.dataset.image_size=64',
                            'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=8'])
    assert cfg['Model'] == dict(name='swin_base_patch4_window7_224', num_classes=1000, drop_path_rate=0.5)
    assert cfg['LRScheduler']['name'] == 'TimmCosine' and cfg['LRScheduler']['learning_rate'] == 1e-3
    assert cfg['LRScheduler']['eta_min'] == 1e-5 and cfg['LRScheduler']['warmup_start_lr'] == 1e-6
    assert cfg['Optimizer']['weight_decay'] == 0.05 and list(cfg['Optimizer']['no_weight_decay_name']) == MU.NO_DECAY
    assert cfg['Optimizer']['grad_clip']['clip_norm'] == 5.0 and cfg['Global']['seed'] == 2023
    cfg['Model'] = dict(name='SwinTransformer', drop_path_rate=0.5, **MU.MODEL)
    cfg['DataLoader']['Train']['dataset']['image_size'] = 64
    cfg['Model']['img_size'] = MU.MODEL['img_size']
    eng = Engine(cfg, mode='train')
    fx = MU.load('swin_small')
    assert eng.no_weight_decay_names(MU.NO_DECAY) == list(fx['no_decay'])
    table = {n: wd for rows in eng.optimizer._param_table for n, _s, wd in rows}
    assert collections.Counter(table.values()) == {0.0: len(fx['no_decay']),
                                                   0.05: len(list(eng.model.parameters())) - len(fx['no_decay'])}
    assert eng.optimizer._grad_clip.clip_norm == 5.0
    # every other optimizer keeps refusing the key, and layer_decay stays refused
    c = get_config(path, ['Global.device=cpu'])
    c.Optimizer = AttrDict(name='AdamW', weight_decay=0.05, layer_decay=0.65)
    with pytest.raises(NotImplementedError, match='layer_decay'):
        eng._build_optimizer(c, c['Global'])
    c.Optimizer = AttrDict(name='Momentum', learning_rate=0.1, no_weight_decay_name=['bias'])
    with pytest.raises(NotImplementedError, match='no_weight_decay_name'):
        eng._build_optimizer(c, c['Global'])


def test_refusals_are_by_name():
    small = dict(MU.MODEL)
    for kw, word in ((dict(drop_rate=0.1), 'drop_rate'), (dict(attn_drop_rate=0.1), 'attn_drop_rate'),
                     (dict(ape=True), 'ape'), (dict(num_heads=(2, 4)), 'head dimension'),
                     (dict(img_size=(64, 64), window_size=16), 'window_size'),
                     (dict(img_size=(40, 64)), 'multiple of the window'),
                     (dict(img_size=(24, 24), window_size=3, depths=(2, 2, 2), num_heads=(1, 2, 4)), 'not even'),
                     (dict(embed_dim=36, num_heads=(1, 2), head_dim=32), 'multiple of 8')):
        with pytest.raises(NotImplementedError, match=word):
            _cpu_model(name='SwinTransformer', **dict(small, **kw))
    with pytest.raises(ValueError):
        _cpu_model(name='SwinTransformer', **dict(small, drop_path_rate=1.0))
