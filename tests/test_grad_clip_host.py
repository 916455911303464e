"""Global-norm gradient clipping — everything that needs no GPU: the fixture's conditions, the configuration object, the
chunk table / CSR index / segment sets AdamW builds from a CPU model (scopes, exclusions), the validation of the ops
wrappers, the launch sequence of a clipped step and of an unclipped one, and the v2 Engine's ``Optimizer.grad_clip``."""
import math
import os

import numpy as np
import pytest
import torch

import grad_clip_util
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mae_ft_clip_small.npz')
SMALL = dict(name='MAE_ViT', patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4, img_size=64)
LR, WD, LAYER_DECAY = 1e-3, 0.05, 0.65


@pytest.fixture(scope='module')
def model():
    from passl_amd.modeling import build_model
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    return build_model(dict(name='MAE_FINETUNE', architecture=dict(SMALL),
                            head=dict(name='VisionTransformerClsHead', num_classes=16, in_channels=128)))


def reference_groups(model):
    """The 13 groups of the fixture: the v2 layer-decay rule on the backbone, the head as two groups at multiplier 1."""
    from passl_amd.solver.lr_decay import param_groups_lrd
    groups = param_groups_lrd(model.backbone, WD, {'pos_embed', 'cls_token', 'dist_token'}, LAYER_DECAY)
    head = list(model.head.parameters())
    groups.append({'lr_scale': 1.0, 'weight_decay': WD, 'params': [p for p in head if p.ndim != 1]})
    groups.append({'lr_scale': 1.0, 'weight_decay': 0., 'params': [p for p in head if p.ndim == 1]})
    return groups


# ---------------------------------------------------------------------------------------------- fixture
def test_fixture_satisfies_its_conditions():
    z = np.load(GOLDEN)
    grad_clip_util.check_golden(z)
    ref = np.load(os.path.join(ROOT, 'tests', 'golden', 'mae_ft_lrd_small.npz'))
    for s in range(int(z['meta'][2])):
        assert float(z['N_s%d_loss' % s]) == float(ref['A_s%d_loss' % s])          # run N is run A of the lrd fixture
        assert z['P_s%d_group_norm' % s].shape == (13,)
    assert [str(k) for k in z['keys']] == [str(k) for k in ref['keys']]


def test_fixture_groups_are_the_products_groups(model):
    z = np.load(GOLDEN)
    groups = reference_groups(model)
    of = {id(p): gi for gi, g in enumerate(groups) for p in g['params']}
    named = list(model.named_parameters())
    assert [n for n, _p in named] == [str(n) for n in z['table_names']]
    assert [of[id(p)] for _n, p in named] == z['group_of'].tolist()


# ---------------------------------------------------------------------------------------------- the object
def test_object_fields_and_validation():
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C, build_grad_clip
    c = C()
    assert (c.clip_norm, c.clip_norm_max, c.always_clip, c.no_clip_list, c.scope) == (1.0, None, False, [], 'group')
    c = C(clip_norm=3, clip_norm_max=2, always_clip=1, no_clip_list=('linear_0',), scope='global')
    assert (c.clip_norm, c.clip_norm_max, c.always_clip, c.no_clip_list, c.scope) == (3.0, 2.0, True, ['linear_0'], 'global')
    assert not callable(c)                                        # configuration, not a function over tensors
    t = C.like_clip_grad_norm_(3.0)
    assert (t.clip_norm, t.clip_norm_max, t.always_clip, t.scope) == (3.0, 1.0, True, 'global') and type(t) is C
    for bad in (dict(clip_norm=0), dict(clip_norm=-1), dict(clip_norm=float('nan')), dict(clip_norm=float('inf')),
                dict(clip_norm_max=0), dict(scope='tensor'), dict(no_clip_list='linear')):
        with pytest.raises(ValueError):
            C(**bad)
    p = torch.nn.Parameter(torch.zeros(4))
    assert not C().excludes(p, 'linear_3.w_0') and C(no_clip_list=['linear_3.']).excludes(p, 'linear_3.w_0')
    p.need_clip = False
    assert C().excludes(p, 'x')
    b = build_grad_clip(dict(clip_norm=2.0, always_clip=True))     # name defaults to ClipGradByGlobalNorm
    assert type(b) is C and b.clip_norm == 2.0 and b.always_clip
    assert build_grad_clip(dict(name='ClipGradByGlobalNorm', clip_norm=0.5, scope='global')).scope == 'global'
    with pytest.raises(NotImplementedError, match='ClipGradByNorm'):
        build_grad_clip(dict(name='ClipGradByNorm', clip_norm=1.0))
    with pytest.raises(NotImplementedError):
        build_grad_clip(dict(name='__import__("os")'))             # a dict lookup, not eval


# ---------------------------------------------------------------------------------------------- tables
def _check_plan(opt, arena):
    """Chunks tile every set exactly: each element of a clipped parameter (with the padding behind it) lies in exactly
    one chunk, that chunk belongs to the parameter's set, nothing of an excluded parameter is covered, every chunk is
    listed once in the CSR index — under its own set."""
    from passl_amd.hip import ops
    plan, host = opt._clip, opt._clip['host']
    assert ops.GRAD_CLIP_CHUNK == 16384 and len(host['chunk_off']) == 1
    offs, lens, csets = host['chunk_off'][0], host['chunk_len'][0], host['chunk_set'][0]
    cover = np.full(arena.n_train, -1, dtype=np.int64)
    for c, (o, l, st) in enumerate(zip(offs, lens, csets)):
        assert o % 4 == 0 and l % 4 == 0 and 0 < l <= ops.GRAD_CLIP_CHUNK and o + l <= arena.n_train
        assert (cover[o:o + l] == -1).all()                                  # chunks are disjoint
        cover[o:o + l] = c
    sets = [st for _n, st in opt.clip_sets()]
    ends = [off for off, _n in arena.param_slices[1:]] + [arena.n_train]
    for (off, _n), end, st in zip(arena.param_slices, ends, sets):
        if st < 0:
            assert (cover[off:end] == -1).all()                              # excluded: in no chunk
        else:
            ids = np.unique(cover[off:end])
            assert ids.min() >= 0 and all(csets[c] == st for c in ids)       # covered, by chunks of its own set only
    ptr, idx = host['set_ptr'], host['set_chunks']
    assert ptr[0] == 0 and ptr[-1] == len(idx) == plan['total'] == len(offs) and len(ptr) == plan['n_sets'] + 1
    assert sorted(idx) == list(range(len(offs)))                             # every chunk in exactly one set
    for s in range(plan['n_sets']):
        mine = idx[ptr[s]:ptr[s + 1]]
        assert mine == sorted(mine) and all(csets[c] == s for c in mine)
    assert plan['set_ptr'].tolist() == ptr and plan['set_chunks'].tolist() == idx
    assert plan['chunk_off'][0].tolist() == offs and plan['chunk_len'][0].tolist() == lens
    assert plan['chunk_off'][0].dtype == torch.int64 and plan['chunk_len'][0].dtype == torch.int32
    assert tuple(plan['out'].shape) == (plan['n_sets'], 2) and plan['partial'].numel() == len(offs)
    return sets


def test_group_scope_one_set_per_group(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    groups = reference_groups(model)
    opt = AdamW(LR, weight_decay=WD, parameters=groups, grad_clip=C(1.0))
    sets = _check_plan(opt, model.arena_q)
    of = {id(p): gi for gi, g in enumerate(groups) for p in g['params']}
    assert sets == [of[id(p)] for p in model.parameters()] and opt._clip['n_sets'] == 13
    # decay / no-decay groups interleave in arena order: some set owns chunks that are not consecutive
    host = opt._clip['host']
    assert any(np.any(np.diff(host['set_chunks'][host['set_ptr'][s]:host['set_ptr'][s + 1]]) > 1) for s in range(13))
    # a parameter larger than a chunk is split: blocks.*.mlp.fc1.weight holds 65536 elements
    assert max(host['chunk_len'][0]) == 16384 and len(host['chunk_off'][0]) > len(list(model.parameters()))
    t = opt._tables[0]
    assert t['seg_set'].dtype == torch.int32 and t['seg_set'].numel() == t['n_seg'] and t['n_sets'] == 13
    assert opt.grad_norms() is opt._clip['out']
    assert sorted(opt.state_dict()) == ['moment1_0', 'moment2_0', 't']        # clipping is configuration, not state


def test_global_scope_and_plain_list_are_one_set(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    params = list(model.parameters())
    a = model.arena_q
    for opt in (AdamW(LR, parameters=reference_groups(model), grad_clip=C.like_clip_grad_norm_(1.0)),
                AdamW(LR, parameters=params, grad_clip=C(1.0)), AdamW(LR, parameters=params, grad_clip=C(1.0, scope='global'))):
        sets = _check_plan(opt, a)
        assert set(sets) == {0} and opt._clip['n_sets'] == 1
        host = opt._clip['host']
        assert len(host['chunk_off'][0]) == -(-a.n_train // 16384)            # one run: the whole arena, tiled
        assert sum(host['chunk_len'][0]) == a.n_train
    # a plain list with nothing excluded: the flat clip launch reading the one coefficient
    assert opt._tables[0] is None and opt._clip_coef[0].data_ptr() == opt._clip['out'][0, 1:].data_ptr()


def test_excluded_parameters_are_in_no_set(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    params = list(model.parameters())
    names = [n for n, _s, _w in AdamW(LR, parameters=params).param_table()]
    frag = names[7].split('.')[0] + '.'                                       # e.g. 'linear_0.': weight and bias
    want_out = {i for i, n in enumerate(names) if frag in n}
    assert 1 <= len(want_out) < len(names)
    params[20].need_clip = False
    try:
        opt = AdamW(LR, parameters=params, grad_clip=C(1.0, no_clip_list=[frag]))
        sets = _check_plan(opt, model.arena_q)
        assert {i for i, s in enumerate(sets) if s < 0} == want_out | {20}
        # a flat optimizer with an excluded parameter takes the grouped clip variant: seg_set = -1 for what is left out
        t = opt._tables[0]
        assert t is not None and sorted(set(t['seg_set'].tolist())) == [-1, 0] and set(t['seg_lr_scale'].tolist()) == {1.0}
        # everything excluded: nothing to clip, today's launches
        none = AdamW(LR, parameters=params, grad_clip=C(1.0, no_clip_list=['_']))
        assert none._clip is None and none.grad_norms() is None and none._tables[0] is None
    finally:
        del params[20].need_clip


def test_plan_and_table_validation():
    from passl_amd.hip import ops
    dev = torch.device('cpu')
    ok = ops.grad_clip_plan([[(0, 8, 1), (8, 40000, 0)], []], [40000, 16], 2, dev)
    assert ok['n_chunks'] == [4, 0] and ok['base'] == [0, 4] and ok['host']['set_ptr'] == [0, 3, 4]
    assert ok['host']['chunk_len'][0] == [8, 16384, 16384, 40000 - 8 - 2 * 16384]
    for runs, sizes, n_sets in (([[(0, 6, 0)]], [8], 1),            # end not a multiple of 4
                                ([[(2, 8, 0)]], [8], 1),            # start not a multiple of 4
                                ([[(0, 12, 0)]], [8], 1),           # beyond the buffer
                                ([[(0, 8, 0), (4, 12, 0)]], [16], 1),   # overlapping
                                ([[(8, 12, 0), (0, 4, 0)]], [16], 1),   # not ascending
                                ([[(4, 4, 0)]], [16], 1),           # empty
                                ([[(0, 8, 1)]], [8], 1),            # set out of range
                                ([[(0, 8, -1)]], [8], 1),
                                ([[(0, 8, 0)]], [10], 1),           # buffer not a multiple of 4
                                ([[]], [8], 1),                     # nothing to clip
                                ([[(0, 8, 0)]], [8], 0),
                                ([[(0, 8, 0)]], [8, 8], 1)):
        with pytest.raises(ValueError):
            ops.grad_clip_plan(runs, sizes, n_sets, dev)
    t = ops.adamw_groups_clip_table([8, 16], [1.0, 0.5], [0.0, 0.1], [-1, 1], 16, 2, dev)
    assert t['seg_set'].tolist() == [-1, 1] and t['n_sets'] == 2 and t['n_seg'] == 2
    for sets in ([0], [0, 2], [-2, 0]):
        with pytest.raises(ValueError):
            ops.adamw_groups_clip_table([8, 16], [1.0, 0.5], [0.0, 0.1], sets, 16, 2, dev)


# ---------------------------------------------------------------------------------------------- launches
def _spy(monkeypatch):
    from passl_amd.hip import ops
    from passl_amd.solver import optimizer as O
    calls = []
    for name in ('adamw_dev', 'adamw_groups_dev', 'adamw_clip_dev', 'adamw_groups_clip_dev', 'grad_sumsq', 'grad_clip_finalize'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    monkeypatch.setattr(O, '_grads_complete', lambda arena: calls.append('complete'))
    return calls


def test_no_grad_clip_keeps_todays_launches(model, monkeypatch):
    from passl_amd.solver.optimizer import AdamW
    calls = _spy(monkeypatch)
    AdamW(LR, parameters=list(model.parameters()), grad_clip=None).step()
    assert calls == ['complete', 'adamw_dev']
    del calls[:]
    AdamW(LR, parameters=reference_groups(model), grad_clip=None).step()
    assert calls == ['complete', 'adamw_groups_dev']


def test_clipped_step_is_sums_then_one_finalize_then_updates(model, monkeypatch):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import AdamW
    calls = _spy(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'item', lambda self: pytest.fail('.item() in a clipped step'))
    AdamW(LR, parameters=list(model.parameters()), grad_clip=C(1.0)).step()
    assert calls == ['complete', 'grad_sumsq', 'grad_clip_finalize', 'adamw_clip_dev']
    del calls[:]
    AdamW(LR, parameters=reference_groups(model), grad_clip=C(1.0)).step()
    assert calls == ['complete', 'grad_sumsq', 'grad_clip_finalize', 'adamw_groups_clip_dev']


def test_other_grad_clip_objects_and_other_optimizers_still_refuse(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.builder import build_optimizer
    from passl_amd.solver.optimizer import AdamW, Momentum
    params = list(model.parameters())
    for bad in (object(), 1.0, dict(clip_norm=1.0), C):
        with pytest.raises(NotImplementedError):
            AdamW(LR, parameters=params, grad_clip=bad)
    with pytest.raises(NotImplementedError):
        Momentum(LR, parameters=params, grad_clip=C(1.0))
    with pytest.raises(NotImplementedError):                                  # v110 users pass the object to AdamW
        build_optimizer(dict(name='AdamW', weight_decay=WD, grad_clip=dict(name='ClipGradByGlobalNorm', clip_norm=1.0)),
                        LR, [model])


# ---------------------------------------------------------------------------------------------- Engine
def _engine_cfg(grad_clip, optimizer=None):
    from passl_amd.utils.config import AttrDict, get_config
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_synthetic.yaml'),
                     ['Global.device=cpu', 'Global.epochs=2', 'DataLoader.Train.dataset.num_samples=8',
                      'DataLoader.Train.sampler.batch_size=2'])
    cfg.Optimizer.grad_clip = AttrDict(grad_clip) if isinstance(grad_clip, dict) else grad_clip
    if optimizer:
        cfg.Optimizer = AttrDict(optimizer, grad_clip=cfg.Optimizer.grad_clip)
    return cfg


def test_engine_builds_the_object_from_the_optimizer_block():
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.engine.engine import Engine
    prev = hip_config.get_compute_dtype()
    try:
        eng = Engine(_engine_cfg(dict(clip_norm=3.0, clip_norm_max=1.0, always_clip=True)), mode='train')
        gc = eng.optimizer._grad_clip
        assert type(gc) is C and (gc.clip_norm, gc.clip_norm_max, gc.always_clip, gc.scope) == (3.0, 1.0, True, 'group')
        a = eng.model.arena_q
        plan = eng.optimizer._clip
        assert plan['n_sets'] == 1 and plan['total'] == -(-a.n_train // 16384) and eng.optimizer._tables == [None]
        # the same engine, other Optimizer blocks (the model is built once: _build_optimizer is what reads the block)
        def rebuild(cfg):
            eng._build_optimizer(cfg, cfg['Global'])
            return eng.optimizer
        with pytest.raises(NotImplementedError, match='ClipGradByNorm'):
            rebuild(_engine_cfg(dict(name='ClipGradByNorm', clip_norm=1.0)))
        with pytest.raises(NotImplementedError, match='AdamW only'):
            rebuild(_engine_cfg(dict(clip_norm=1.0), optimizer=dict(name='Momentum', momentum=0.9)))
        cfg = _engine_cfg(None)
        cfg.Optimizer.layer_decay = 0.65
        with pytest.raises(NotImplementedError, match='layer_decay'):
            rebuild(cfg)
        assert rebuild(_engine_cfg(None))._clip is None
        assert rebuild(_engine_cfg(dict(name='ClipGradByGlobalNorm', clip_norm=2.0, scope='global')))._grad_clip.scope == 'global'
    finally:
        hip_config.set_compute_dtype(prev)


def test_rule_in_float32_matches_its_statement():
    """The numpy-float32 evaluation the GPU test compares the finalize kernel with, pinned to the statement of the rule."""
    f = np.float32

    def rule(sq, clip_norm, clip_max, always):
        norm = np.sqrt(f(sq))
        if not always and norm <= f(clip_norm):
            return norm, f(1.0)
        coef = f(clip_norm) / (norm + f(1e-6))
        return norm, (f(clip_max) if clip_max is not None and coef > f(clip_max) else coef)
    assert rule(0.25, 1.0, None, False) == (f(0.5), f(1.0))
    assert rule(1.0, 1.0, None, False) == (f(1.0), f(1.0))                    # equal: not clipped
    n, c = rule(4.0, 1.0, None, False)
    assert n == f(2.0) and c == f(1.0) / (f(2.0) + f(1e-6)) and c < 0.5
    assert rule(0.25, 1.0, None, True)[1] == f(1.0) / (f(0.5) + f(1e-6))      # always_clip scales up ...
    assert rule(0.25, 1.0, 1.0, True)[1] == f(1.0)                            # ... unless clip_norm_max holds it
    assert math.isnan(rule(float('nan'), 1.0, 1.0, False)[1])                 # a NaN norm is "not <=": it propagates
