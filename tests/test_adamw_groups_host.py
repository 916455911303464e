"""AdamW parameter groups (layer-wise lr decay, no-decay sets) — everything that needs no GPU: the two grouping rules
against the committed fixture and against the reference's own functions, the optimizer's constructor, build_optimizer,
the choice between the flat and the grouped launch, the table validation of the ops wrapper, the fixture's conditions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lrd_util
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mae_ft_lrd_small.npz')
SMALL = dict(name='MAE_ViT', patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4, img_size=64)
NO_DECAY_V2 = {'pos_embed', 'cls_token', 'dist_token'}
LR, WD, LAYER_DECAY = 1e-3, 0.05, 0.65


def _model():
    from passl_amd.modeling import build_model
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    return build_model(dict(name='MAE_FINETUNE', architecture=dict(SMALL),
                            head=dict(name='VisionTransformerClsHead', num_classes=16, in_channels=128)))


@pytest.fixture(scope='module')
def model():
    return _model()


def _groups(model, rule):
    from passl_amd.solver import lr_decay as LD
    if rule == 'A':
        return LD.param_groups_lrd(model, WD, NO_DECAY_V2, LAYER_DECAY)
    n = model.backbone.get_num_layers()
    a = LD.LayerDecayValueAssigner([LAYER_DECAY ** (n + 1 - i) for i in range(n + 2)])
    return LD.get_parameter_groups(dict(weight_decay=WD), model, get_num_layer=a.get_layer_id, get_layer_scale=a.get_scale)


def _by_name(model, opt):
    """param_table() (arena order, Paddle auto-names) against model.named_parameters(): same order."""
    named = list(model.named_parameters())
    assert [p._passl_index for _n, p in named] == list(range(len(named)))
    table = opt.param_table()
    assert len(table) == len(named)
    return [(n, s, w) for (n, _p), (_auto, s, w) in zip(named, table)]


@pytest.mark.parametrize('rule', ['A', 'B'])
def test_tables_equal_the_fixture_exactly(model, rule):
    from passl_amd.solver import lr_decay as LD
    from passl_amd.solver.optimizer import AdamW
    want = lrd_util.tables(np.load(GOLDEN))[rule]
    groups = _groups(model, rule)
    assert LD.table_by_name(model, groups) == want                       # names, Python-float scales, decays: equal
    opt = AdamW(LR, weight_decay=WD, parameters=groups)
    assert _by_name(model, opt) == want
    # what the rules are about
    row = {n: (s, w) for n, s, w in want}
    assert row['backbone.pos_embed'] == (LAYER_DECAY ** 5, 0.0 if rule == 'A' else WD)
    assert row['backbone.cls_token'] == (LAYER_DECAY ** 5, 0.0 if rule == 'A' else WD)
    assert row['backbone.blocks.2.mlp.fc1.weight'] == (LAYER_DECAY ** 2, WD)
    assert row['backbone.blocks.2.mlp.fc1.bias'] == (LAYER_DECAY ** 2, 0.0)
    assert row['backbone.fc_norm.weight'] == (1.0, 0.0) and row['head.fc_cls.weight'] == (1.0, WD)


def test_tables_equal_the_reference_functions_run_live(model):
    """The reference's own lr_decay.py / builder.py executed on the reference's model (paddle shim, a process of its
    own) against the product's rules on the product's model."""
    from oracle import ref_runner, ref_runner_v2
    if not (ref_runner.available() and ref_runner_v2.available()):
        pytest.skip('the reference tree is not on this machine')
    from passl_amd.solver import lr_decay as LD
    code = r'''
import json, sys
sys.path.insert(0, 'tests'); sys.path.insert(0, 'tests/golden')
import make_golden_mae_finetune_lrd as G
from oracle import ref_runner
ns = ref_runner.load()
lrd, builder = G.load_rules()
model, _ = G.build(ns)
out = {}
for run in ('A', 'B'):
    of = {id(p): (g['lr_scale'], g['weight_decay']) for g in G.groups_of(run, model, lrd, builder) for p in g['params']}
    out[run] = [[n, of[id(p)][0], of[id(p)][1]] for n, p in model.named_parameters()]
print('TABLES ' + json.dumps(out))
'''
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    live = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('TABLES ')][0][7:])
    for rule in ('A', 'B'):
        assert LD.table_by_name(model, _groups(model, rule)) == [tuple(row) for row in live[rule]]


def test_constructor_validation(model):
    from passl_amd.solver.optimizer import AdamW
    params = list(model.parameters())
    with pytest.raises(ValueError, match='more than once'):
        AdamW(LR, parameters=[{'params': params}, {'params': params[:1], 'lr_scale': 0.5}])
    with pytest.raises(ValueError, match='more than once'):
        AdamW(LR, parameters=params + params[:1])
    with pytest.raises(NotImplementedError, match='subset of an arena'):
        AdamW(LR, parameters=[{'params': params[1:]}])
    with pytest.raises(ValueError, match='twice'):
        AdamW(LR, parameters=[{'params': params, 'lr_scale': 0.5, 'learning_rate': 0.5}])
    with pytest.raises(ValueError, match='weight_decay'):
        AdamW(LR, parameters=[{'params': params, 'weight_decay': -0.1}])
    with pytest.raises(ValueError, match='weight_decay'):
        AdamW(LR, parameters=params, weight_decay=-0.1)
    with pytest.raises(ValueError):
        AdamW(LR, parameters=[{'params': params, 'lr': 0.5}])                 # an unknown key is not ignored
    with pytest.raises(ValueError):
        AdamW(LR, parameters=[{'params': params[:1]}] + params[1:])           # tensors and groups mixed
    with pytest.raises(NotImplementedError):
        AdamW(LR, parameters=params, grad_clip=object())


def test_lr_ratio_and_apply_decay_param_fun(model):
    from passl_amd.solver.optimizer import AdamW
    params = list(model.parameters())
    half = [{'params': params[:3], 'learning_rate': 0.5}, {'params': params[3:], 'weight_decay': 0.2}]
    opt = AdamW(LR, weight_decay=WD, parameters=half, lr_ratio=lambda p: 0.25 if p is params[0] else 1.0,
                apply_decay_param_fun=lambda name: not name.endswith('.b_0'))
    table = opt.param_table()
    names = [n for n, _s, _w in table]
    assert len(set(names)) == len(names)                                      # auto-names are unique
    assert table[0][1:] == (0.125, WD) and table[1][1:] == (0.5, WD) and table[3][1:] == (1.0, 0.0)
    assert names[3].endswith('.b_0') and table[4][1:] == (1.0, 0.2)
    for (n, _s, w), p in zip(table, params):
        assert (w == 0.0) == n.endswith('.b_0')
    # the table is configuration, not state
    assert sorted(k for k in opt.state_dict()) == ['moment1_0', 'moment2_0', 't']


def test_build_optimizer_layer_decay_and_exclude(model):
    from passl_amd.solver.builder import build_optimizer
    from passl_amd.utils.config import get_config
    want = lrd_util.tables(np.load(GOLDEN))['B']
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_lrd_synthetic.yaml'), [])
    assert cfg.optimizer.layer_decay == LAYER_DECAY and cfg.optimizer.weight_decay == WD
    opt = build_optimizer(cfg.optimizer, LR, [model])
    assert _by_name(model, opt) == want
    assert opt._tables[0] is not None and opt._tables[0]['n_seg'] < len(want)      # adjacent equal rows are merged
    ocfg = dict(name='AdamW', weight_decay=WD, layer_decay=LAYER_DECAY, exclude_from_weight_decay=['pos_embed', 'fc2'])
    opt = build_optimizer(ocfg, LR, [model])
    got = _by_name(model, opt)
    for (n, s, w), (_n, s0, w0) in zip(got, want):
        assert s == s0 and w == (0.0 if ('pos_embed' in n or 'fc2' in n) else w0), n
    assert dict((n, w) for n, _s, w in got)['backbone.cls_token'] == WD
    # exclusion without layer decay: a table of two decays, every multiplier 1
    opt = build_optimizer(dict(name='AdamW', weight_decay=WD, exclude_from_weight_decay=['norm']), LR, [model])
    got = _by_name(model, opt)
    assert all(s == 1.0 and w == (0.0 if 'norm' in n else WD) for n, s, w in got) and opt._tables[0] is not None
    with pytest.raises(NotImplementedError):
        build_optimizer(dict(name='AdamW', weight_decay=WD, grad_clip=dict(name='global_norm', value=1.0)), LR, [model])


def test_flat_path_is_kept_when_nothing_differs(model, monkeypatch):
    from passl_amd.hip import ops
    from passl_amd.solver import optimizer as O
    from passl_amd.solver.builder import build_optimizer
    calls = []
    monkeypatch.setattr(ops, 'adamw_dev', lambda *a, **k: calls.append(('flat', a[8])))
    monkeypatch.setattr(ops, 'adamw_groups_dev', lambda *a, **k: calls.append(('groups', a[4]['n_seg'])))
    monkeypatch.setattr(O, '_grads_complete', lambda arena: None)
    params = list(model.parameters())

    def kind(opt):
        del calls[:]
        opt.step()
        return calls

    assert kind(O.AdamW(LR, weight_decay=WD, parameters=params)) == [('flat', WD)]
    assert kind(build_optimizer(dict(name='AdamW', weight_decay=WD, layer_decay=1.0), LR, [model])) == [('flat', WD)]
    assert kind(build_optimizer(dict(name='AdamW', weight_decay=WD), LR, [model])) == [('flat', WD)]
    # groups that say nothing new: multipliers exactly 1, one decay
    same = [{'params': params[:5], 'lr_scale': 1.0, 'weight_decay': 0.1}, {'params': params[5:], 'weight_decay': 0.1}]
    assert kind(O.AdamW(LR, weight_decay=WD, parameters=same)) == [('flat', 0.1)]
    assert kind(O.AdamW(LR, weight_decay=WD, parameters=params, lr_ratio=lambda p: 1.0)) == [('flat', WD)]
    # anything else takes the grouped launch
    two = [{'params': params[:5], 'weight_decay': 0.0}, {'params': params[5:]}]
    assert kind(O.AdamW(LR, weight_decay=WD, parameters=two)) == [('groups', 2)]
    assert kind(O.AdamW(LR, weight_decay=WD, parameters=params, lr_ratio=lambda p: 0.5)) == [('groups', 1)]
    lrd = build_optimizer(dict(name='AdamW', weight_decay=WD, layer_decay=LAYER_DECAY), LR, [model])
    assert kind(lrd) == [('groups', lrd._tables[0]['n_seg'])]


def test_device_table_is_in_arena_order_with_padding_in_front(model):
    from passl_amd.solver.optimizer import AdamW
    arena = model.arena_q
    opt = AdamW(LR, weight_decay=WD, parameters=_groups(model, 'A'))
    t = opt._tables[0]
    ends, scales, wds = t['seg_end'].tolist(), t['seg_lr_scale'].tolist(), t['seg_wd'].tolist()
    assert ends[-1] == arena.n_train == t['n'] and all(e % 4 == 0 for e in ends) and ends == sorted(set(ends))
    starts = [off for off, _n in arena.param_slices]
    assert set(ends) <= set(starts[1:] + [arena.n_train])                    # a segment ends where a slot begins
    rows = opt.param_table()
    s = 0
    for (off, n), (_name, scale, wd) in zip(arena.param_slices, rows):
        while off >= ends[s]:
            s += 1
        assert off + n <= ends[s] and scales[s] == np.float32(scale) and wds[s] == np.float32(wd)
    assert all((scales[i], wds[i]) != (scales[i + 1], wds[i + 1]) for i in range(len(ends) - 1))


def test_ops_wrapper_refuses_bad_tables():
    from passl_amd.hip import ops
    ok = ops.adamw_groups_table([8, 24, 4104], [1.0, 0.5, 0.25], [0.05, 0.0, 0.05], 4104, 'cpu')
    assert ok['n_seg'] == 3 and ok['seg_end'].dtype == torch.int64 and ok['seg_lr_scale'].dtype == torch.float32
    bad = [([24, 8, 4104], [1.0] * 3, [0.0] * 3, 4104),            # unsorted
           ([8, 8, 4104], [1.0] * 3, [0.0] * 3, 4104),             # an empty segment
           ([8, 24], [1.0] * 2, [0.0] * 2, 4104),                  # short
           ([8, 24, 4108], [1.0] * 3, [0.0] * 3, 4104),            # long
           ([8, 22, 4104], [1.0] * 3, [0.0] * 3, 4104),            # not a multiple of 4
           ([8, 24, 4102], [1.0] * 3, [0.0] * 3, 4102),            # n not a multiple of 4
           ([8, 24, 4104], [1.0, float('nan'), 1.0], [0.0] * 3, 4104),
           ([8, 24, 4104], [1.0, float('inf'), 1.0], [0.0] * 3, 4104),
           ([8, 24, 4104], [1.0] * 3, [0.0, -0.05, 0.0], 4104),
           ([8, 24, 4104], [1.0] * 2, [0.0] * 3, 4104),
           ([], [], [], 0)]
    for ends, scales, wds, n in bad:
        with pytest.raises(ValueError):
            ops.adamw_groups_table(ends, scales, wds, n, 'cpu')
    p = torch.zeros(4100)
    with pytest.raises(ValueError):
        ops.adamw_groups_dev(p, p, p, p, ok, torch.zeros(4), 0.9, 0.999, 1e-8)       # a table for another buffer


def test_fixture_conditions():
    """Conditions (a) - (c) of the generator, on the committed file."""
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert [int(v) for v in z['meta']] == [8, 64, 3, 16]
    assert (float(z['lr']), float(z['weight_decay']), float(z['layer_decay'])) == (LR, WD, LAYER_DECAY)
    lrd_util.check_golden(z)
    # the two rules differ exactly where they are documented to differ
    a, b = lrd_util.tables(z)['A'], lrd_util.tables(z)['B']
    assert [n for (n, _s, w), (_n, _s2, w2) in zip(a, b) if w != w2] == ['backbone.cls_token', 'backbone.pos_embed']
    assert [s for _n, s, _w in a] == [s for _n, s, _w in b]
    for n in z['elementwise']:
        assert z['A_s0_p/%s' % n].size <= 4096


def test_get_num_layers(model):
    assert model.backbone.get_num_layers() == 4
