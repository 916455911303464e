"""Adan — everything that needs no GPU: the fixtures' conditions, the float32 twin of the rule, the registry and the
constructor's validation, the launch the optimizer chooses per arena from a CPU model (flat / grouped, each with or
without the clip coefficient), the 8-wide hyper block with its first-step flag, and the YAML."""
import os

import numpy as np
import pytest
import torch

import adan_util as U
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, 'tests', 'golden', 'adan_vectors.npz')
MODEL = os.path.join(ROOT, 'tests', 'golden', 'adan_mae_ft_small.npz')
SMALL = dict(name='MAE_ViT', patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4, img_size=64)
LR, WD, LAYER_DECAY = 1e-3, 0.05, 0.65


@pytest.fixture(scope='module')
def model():
    from passl_amd.modeling import build_model
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    return build_model(dict(name='MAE_FINETUNE', architecture=dict(SMALL),
                            head=dict(name='VisionTransformerClsHead', num_classes=16, in_channels=128)))


def _groups(model):
    from passl_amd.solver.lr_decay import param_groups_lrd
    groups = param_groups_lrd(model.backbone, WD, {'pos_embed', 'cls_token', 'dist_token'}, LAYER_DECAY)
    head = list(model.head.parameters())
    groups.append({'lr_scale': 1.0, 'weight_decay': WD, 'params': [p for p in head if p.ndim != 1]})
    groups.append({'lr_scale': 1.0, 'weight_decay': 0., 'params': [p for p in head if p.ndim == 1]})
    return groups


# ---------------------------------------------------------------------------------------------- fixtures
def test_fixtures_satisfy_their_conditions():
    figures = U.check_golden(np.load(VECTORS))
    print(figures)
    assert figures['worst_ratio'] <= 1.0 and min(figures['wrong_rule_ratios'].values()) >= 100.0
    U.check_golden(np.load(MODEL))
    for f in (VECTORS, MODEL):
        assert os.path.getsize(f) < 1 << 20


def test_float32_twin_stays_within_the_bound_of_the_fixture():
    """The numpy-float32 evaluation the GPU size test compares the kernel with lies within the kernel's own bound of the
    reference: 4 x max(ref_err, one fp32 ulp of the tensor's largest magnitude)."""
    z = np.load(VECTORS)
    worst = 0.0
    for run, no_prox in U.vector_runs(z):
        for n in U.vector_names(z):
            traj = U.trajectory(z, n, no_prox, rule=U.adan_rule_f32)
            for t in range(1, int(z['steps']) + 1):
                errs = z['%s_s%d_ref_err/%s' % (run, t, n)]
                for bi, b in enumerate(U.BUFFERS):
                    ref = z['%s_s%d_%s/%s' % (run, t, b, n)]
                    bd = U.bound(errs[bi], ref)
                    err = float(np.max(np.abs(traj[t - 1][b].astype(np.float64) - ref.astype(np.float64))))
                    assert err <= bd, (run, n, t, b, err, bd)
                    worst = max(worst, err / bd)
    print('float32 twin against the reference: largest err / bound %.3f' % worst)


def test_rule_exact_conditions():
    """A gradient that is zero throughout leaves every state at exactly zero and moves p by the decay alone; at t == 1
    the contents of pre have no influence."""
    p0 = np.array([1.5, -2.0, 0.25, 3.0])
    for rule, dt in ((U.adan_rule, np.float64), (U.adan_rule_f32, np.float32)):
        st = U.zero_state(p0, dt)
        for t in (1, 2, 3):
            st = rule(st, np.zeros(4), t, 0.1, 0.02)
            assert all(not st[b].any() for b in ('m', 'd', 's', 'pre'))
        want = p0.astype(dt)
        for t in range(3):
            want = want / (dt(1.0) + dt(0.1) * dt(0.02))
        assert np.array_equal(st['p'], want)
        a, b = U.zero_state(p0, dt), U.zero_state(p0, dt)
        b['pre'] = np.full(4, 1e15, dtype=dt)
        g = np.array([0.5, -1.0, 2.0, 0.0])
        ra, rb = rule(a, g, 1, 0.1, 0.02), rule(b, g, 1, 0.1, 0.02)
        assert all(np.array_equal(ra[k], rb[k]) for k in U.BUFFERS)
        rb2 = rule(b, g, 2, 0.1, 0.02)
        assert not np.array_equal(rule(a, g, 2, 0.1, 0.02)['d'], rb2['d'])


# ---------------------------------------------------------------------------------------------- the class
def test_registry_holds_adan():
    from passl_amd.solver.builder import OPTIMIZERS
    from passl_amd.solver.optimizer import Adan, AdamW, _GroupedArenaOptimizer
    assert OPTIMIZERS.get('Adan') is Adan and Adan.type == 'adan'
    assert issubclass(Adan, _GroupedArenaOptimizer) and issubclass(AdamW, _GroupedArenaOptimizer)
    assert [k for k, _a in Adan._STATE] == ['exp_avg', 'exp_avg_diff', 'exp_avg_sq', 'pre_grad']
    # the shared code is the base's: neither optimizer restates the tables or the clip sequence
    for name in ('_init_groups', 'step', 'grad_norms', 'clip_sets', 'param_table', 'state_dict', 'set_state_dict'):
        assert name not in vars(Adan) and name not in vars(AdamW), name


def test_constructor_validation(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import Adan
    params = list(model.parameters())
    with pytest.raises(NotImplementedError, match='is_vanilla'):
        Adan(LR, parameters=params, is_vanilla=True)
    with pytest.raises(NotImplementedError, match='lr_func'):
        Adan(LR, parameters=params, lr_func=lambda group, step: None)
    for bad in (object(), 1.0, dict(clip_norm=1.0), C):
        with pytest.raises(NotImplementedError, match='grad_clip'):
            Adan(LR, parameters=params, grad_clip=bad)
    for betas in ((1.0, 0.92, 0.99), (0.98, -0.1, 0.99), (0.98, 0.92, 1.5)):
        with pytest.raises(ValueError, match='beta'):
            Adan(LR, parameters=params, betas=betas)
    with pytest.raises(ValueError, match='epsilon'):
        Adan(LR, parameters=params, eps=-1e-8)
    with pytest.raises(ValueError, match='weight_decay'):
        Adan(LR, parameters=params, weight_decay=-0.1)
    for flag in (True, False, None):
        opt = Adan(LR, parameters=params, use_master_param=flag)
        assert (opt._b1, opt._b2, opt._b3, opt._eps, opt._wd, opt._no_prox) == (0.98, 0.92, 0.99, 1e-8, 0.0, False)
    assert Adan(parameters=params, lr=0.5).get_lr() == 0.5 and Adan(parameters=params).get_lr() == 1e-3
    assert Adan(LR, parameters=params, betas=(0.0, 0.0, 0.0), eps=0.0, no_prox=True)._no_prox is True
    sd = Adan(LR, parameters=params).state_dict()
    assert sorted(sd) == ['exp_avg_0', 'exp_avg_diff_0', 'exp_avg_sq_0', 'pre_grad_0', 't'] and sd['t'] == 0


def _spy(monkeypatch):
    from passl_amd.hip import ops
    from passl_amd.solver import optimizer as O
    calls = []
    for name in ('adan_dev', 'adan_clip_dev', 'adan_groups_dev', 'adan_groups_clip_dev', 'adamw_dev', 'adamw_groups_dev',
                 'adamw_clip_dev', 'adamw_groups_clip_dev', 'grad_sumsq', 'grad_clip_finalize'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    monkeypatch.setattr(O, '_grads_complete', lambda arena: calls.append(('complete', (), {})))
    return calls


def test_launch_choice_per_arena(model, monkeypatch):
    """A plain list -> the flat launch; groups -> the table (its segment count that of AdamW over the same groups); a
    clip plan -> the clip variants; nothing comes back to the host."""
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.solver.optimizer import Adan, AdamW
    calls = _spy(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'item', lambda self: pytest.fail('.item() in a step'))
    params, a = list(model.parameters()), model.arena_q

    def names():
        out = [c[0] for c in calls]
        del calls[:]
        return out

    opt = Adan(LR, weight_decay=0.02, parameters=params)
    assert opt._tables == [None] and opt._flat_wd == [0.02] and opt._clip is None and not opt.grouped
    opt.step()
    (name, args, _k), = [c for c in calls if c[0] != 'complete']
    assert name == 'adan_dev' and len(args) == 14
    assert [x.data_ptr() for x in args[:6]] == [a.flat.data_ptr(), a.grads.data_ptr(), opt._m[0].data_ptr(),
                                                opt._d[0].data_ptr(), opt._s[0].data_ptr(), opt._pre[0].data_ptr()]
    assert args[6] is opt._hyper_dev and args[7:] == (0.98, 0.92, 0.99, 1e-8, 0.02, False, 1.0)
    assert names() == ['complete', 'adan_dev']

    grouped = Adan(LR, weight_decay=WD, parameters=_groups(model))
    twin = AdamW(LR, weight_decay=WD, parameters=_groups(model))
    t, tw = grouped._tables[0], twin._tables[0]
    assert grouped.grouped and 'seg_set' not in t and t['n_seg'] == tw['n_seg'] >= 13 and t['n'] == a.n_train
    for k in ('seg_end', 'seg_lr_scale', 'seg_wd'):
        assert torch.equal(t[k], tw[k])
    assert grouped.param_table() == twin.param_table()
    grouped.step()
    assert names() == ['complete', 'adan_groups_dev']

    Adan(LR, parameters=params, grad_clip=C(1.0)).step()
    assert names() == ['complete', 'grad_sumsq', 'grad_clip_finalize', 'adan_clip_dev']
    clipped = Adan(LR, weight_decay=WD, parameters=_groups(model), grad_clip=C(1.0), no_prox=True)
    assert clipped._clip['n_sets'] == 13 and clipped._tables[0]['seg_set'].numel() == clipped._tables[0]['n_seg']
    assert clipped.clip_sets() == AdamW(LR, weight_decay=WD, parameters=_groups(model), grad_clip=C(1.0)).clip_sets()
    clipped.step()
    assert [c[0] for c in calls] == ['complete', 'grad_sumsq', 'grad_clip_finalize', 'adan_groups_clip_dev']
    assert calls[-1][1][8] is clipped._clip['out'] and calls[-1][1][-2:] == (True, 1.0)
    del calls[:]
    one = Adan(LR, parameters=_groups(model), grad_clip=C(1.0, scope='global'))
    assert one._clip['n_sets'] == 1 and set(one._tables[0]['seg_set'].tolist()) == {0}


def test_adamw_tables_of_the_same_model_are_what_they_were(model):
    """The tables AdamW builds through the shared base, pinned against their statement from the rows: the merge of
    adjacent parameters with equal (multiplier, decay), slot padding with the parameter in front of it."""
    from passl_amd.solver.optimizer import AdamW
    a = model.arena_q
    opt = AdamW(LR, weight_decay=WD, parameters=_groups(model))
    rows = opt.param_table()
    ends = [off for off, _n in a.param_slices[1:]] + [a.n_train]
    want = []
    for end, (_name, scale, wd) in zip(ends, rows):
        if want and want[-1][1:] == (scale, wd):
            want[-1] = (end, scale, wd)
        else:
            want.append((end, scale, wd))
    t = opt._tables[0]
    assert t['seg_end'].tolist() == [e for e, _s, _w in want] and t['n_seg'] == len(want)
    assert t['seg_lr_scale'].tolist() == [float(np.float32(s)) for _e, s, _w in want]
    assert t['seg_wd'].tolist() == [float(np.float32(w)) for _e, _s, w in want]
    assert sorted({s for _n, s, _w in rows})[0] == LAYER_DECAY ** 5 and {w for _n, _s, w in rows} == {0.0, WD}
    flat = AdamW(LR, weight_decay=WD, parameters=list(model.parameters()))
    assert flat._tables == [None] and flat._flat_wd == [WD] and flat._clip_coef == [None]
    assert flat._hyper_dev.numel() == 4 and sorted(flat.state_dict()) == ['moment1_0', 'moment2_0', 't']


def test_hyper_block_is_8_wide_and_first_is_set_once(model):
    from passl_amd.solver.optimizer import Adan, Momentum
    params = list(model.parameters())
    opt = Adan(0.25, parameters=params)
    assert opt._hyper_dev.shape == (8,) and not opt._hyper_dev.any()
    opt.push_hyper()
    f = np.float32
    assert opt._hyper_dev.tolist() == [0.25, float(f(0.98)), float(f(0.92)), float(f(0.99)), 1.0, 0.0, 0.0, 0.0]
    opt.push_hyper()
    assert opt._hyper_dev.tolist() == [0.25, float(f(0.98 ** 2)), float(f(0.92 ** 2)), float(f(0.99 ** 2)), 0.0, 0.0, 0.0, 0.0]
    assert opt.state_dict()['t'] == 2
    assert Momentum(0.1, parameters=params)._hyper_dev.shape == (4,)          # the width of the others is unchanged
    # a resumed run never takes the first-step branch again
    fresh = Adan(0.25, parameters=params)
    sd = opt.state_dict()
    fresh.set_state_dict(sd)
    fresh.push_hyper()
    assert fresh._hyper_dev[4].item() == 0.0 and fresh.state_dict()['t'] == 3
    assert fresh._hyper_dev[1].item() == float(f(0.98 ** 3))
    with pytest.raises(KeyError):
        fresh.set_state_dict({k: v for k, v in sd.items() if k != 'pre_grad_0'})


def test_ops_wrappers_validate_before_the_library_is_asked():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    z = [torch.zeros(16) for _ in range(6)]
    hyper = torch.zeros(8)
    with pytest.raises(ValueError, match='hyper'):
        ops.adan_dev(*z, torch.zeros(4), 0.98, 0.92, 0.99, 1e-8, 0.0)         # AdamW's 4-wide block
    with pytest.raises(ValueError, match='equal sizes'):
        ops.adan_dev(*z[:5], torch.zeros(12), hyper, 0.98, 0.92, 0.99, 1e-8, 0.0)
    t = ops.adamw_groups_clip_table([8, 32], [1.0, 0.5], [0.0, 0.1], [-1, 1], 32, 2, torch.device('cpu'))
    with pytest.raises(ValueError, match='table covers'):
        ops.adan_groups_dev(*z, t, hyper, 0.98, 0.92, 0.99, 1e-8)
    z32 = [torch.zeros(32) for _ in range(6)]
    with pytest.raises(ValueError, match='names 2 sets'):
        ops.adan_groups_clip_dev(*z32, t, hyper, torch.zeros(3, 2), 0.98, 0.92, 0.99, 1e-8)
    with pytest.raises(L.PasslHipError):
        ops.adan_dev(*z, hyper, 0.98, 0.92, 0.99, 1e-8, 0.0)                  # host tensors: no CPU fall-back


def test_library_refuses_bad_arguments_without_a_gpu():
    import ctypes as C
    from passl_amd.hip import lib as L
    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    p += (-p) % 16
    six = [p] * 6
    cfg = (0.98, 0.92, 0.99, 1e-8)
    assert lib.passl_hip_adan_dev(*six, 0, p, *cfg, 0.0, 0, 1.0, None) == L.OK               # n == 0: nothing to do
    assert lib.passl_hip_adan_dev(*six, 6, p, *cfg, 0.0, 0, 1.0, None) == L.EINVAL           # n % 4
    assert lib.passl_hip_adan_dev(*six, -4, p, *cfg, 0.0, 0, 1.0, None) == L.EINVAL
    assert lib.passl_hip_adan_dev(*six, 8, None, *cfg, 0.0, 0, 1.0, None) == L.EINVAL        # no hyper block
    for i in range(6):
        bad = list(six)
        bad[i] = p + 4
        assert lib.passl_hip_adan_dev(*bad, 8, p, *cfg, 0.0, 0, 1.0, None) == L.EINVAL       # not 16-byte aligned
        bad[i] = None
        assert lib.passl_hip_adan_clip_dev(*bad, 8, p, p, *cfg, 0.0, 0, 1.0, None) == L.EINVAL
    assert lib.passl_hip_adan_clip_dev(*six, 8, p, None, *cfg, 0.0, 0, 1.0, None) == L.EINVAL
    assert lib.passl_hip_adan_groups_dev(*six, 8, p, p, p, 0, p, *cfg, 0, 1.0, None) == L.EINVAL        # n_seg <= 0
    assert lib.passl_hip_adan_groups_dev(*six, 8, p + 4, p, p, 1, p, *cfg, 0, 1.0, None) == L.EINVAL    # int64 table
    assert lib.passl_hip_adan_groups_dev(*six, 0, p, p, p, 1, p, *cfg, 0, 1.0, None) == L.OK
    assert lib.passl_hip_adan_groups_clip_dev(*six, 8, p, p, p, p, 1, p, p, 0, *cfg, 0, 1.0, None) == L.EINVAL   # n_sets <= 0
    assert lib.passl_hip_adan_groups_clip_dev(*six, 8, p, p, p, None, 1, p, p, 1, *cfg, 0, 1.0, None) == L.EINVAL
    assert lib.passl_hip_adan_groups_clip_dev(*six, 0, p, p, p, p, 1, p, p, 1, *cfg, 0, 1.0, None) == L.OK


# ---------------------------------------------------------------------------------------------- Engine / YAML
def test_yaml_loads_names_what_is_built_and_carries_the_reference_values():
    from passl_amd.solver.builder import OPTIMIZERS
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_adan_synthetic.yaml'), [])
    assert dict(cfg.Optimizer) == dict(name='Adan', weight_decay=0.02, use_master_param=True)
    assert OPTIMIZERS.get(cfg.Optimizer.name).__name__ == 'Adan'
    sched = dict(cfg.LRScheduler)
    assert sched == dict(name='ViTLRScheduler', learning_rate=1.5e-2, decay_type='cosine', warmup_steps=20000)
    assert cfg.Global.epochs == 150 and cfg.Global.accum_steps == 2 and cfg.FP16.level == 'O2'
    assert dict(cfg.Model) == dict(name='ViT_base_patch16_224', class_num=1000, drop_rate=0.1)
    assert cfg.DataLoader.Train.dataset.name == 'SyntheticLabeled' and cfg.DataLoader.Train.sampler.batch_size == 512
    assert cfg.DataLoader.Train.sampler.drop_last is True
    # the reference file differs from the AdamW recipe in the solver only
    sup = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_sup_synthetic.yaml'), [])
    for block in ('Model', 'Loss', 'Metric', 'FP16', 'DistributedStrategy'):
        assert cfg[block] == sup[block], block


def test_engine_builds_adan_and_its_grad_clip():
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm as C
    from passl_amd.engine.engine import Engine
    from passl_amd.utils.config import AttrDict, get_config
    prev = hip_config.get_compute_dtype()
    try:
        cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_synthetic.yaml'),
                         ['Global.device=cpu', 'Global.epochs=2', 'DataLoader.Train.dataset.num_samples=8',
                          'DataLoader.Train.sampler.batch_size=2'])
        cfg.Optimizer = AttrDict(name='Adan', weight_decay=0.02, use_master_param=True,
                                 grad_clip=AttrDict(name='ClipGradByGlobalNorm', clip_norm=2.0))
        eng = Engine(cfg, mode='train')
        opt = eng.optimizer
        assert type(opt).__name__ == 'Adan' and type(opt._grad_clip) is C and opt._grad_clip.clip_norm == 2.0
        assert opt._clip['n_sets'] == 1 and opt._tables == [None] and opt._wd == 0.02

        def rebuild(**kw):
            c = get_config(os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_synthetic.yaml'), ['Global.device=cpu'])
            c.Optimizer = AttrDict(name='Adan', weight_decay=0.02, **kw)
            eng._build_optimizer(c, c['Global'])
            return eng.optimizer
        assert rebuild()._clip is None
        for key, val in (('layer_decay', 0.65), ('no_weight_decay_name', ['pos_embed'])):
            with pytest.raises(NotImplementedError, match=key):
                rebuild(**{key: val})
        with pytest.raises(NotImplementedError, match='ClipGradByNorm'):
            rebuild(grad_clip=AttrDict(name='ClipGradByNorm', clip_norm=1.0))
    finally:
        hip_config.set_compute_dtype(prev)
