"""Element-wise dropout, ViTCELoss and ViTLRScheduler of the supervised ViT recipe — everything that needs no GPU: the
mask restatement (statistics, dependence on site / step / seed, threshold edge cases), argument validation of the C
entry points, the scheduler and the loss against values recorded from the reference's own classes
(tests/golden/vit_sup_small.npz), the float32 evaluation of the loss against its bound, the constructors, the YAML."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import dropout_util as DU
import droppath_util as DP
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'vit_sup_small.npz')
SMALL = dict(img_size=64, patch_size=16, embed_dim=64, depth=2, num_heads=2, class_num=10)
SEED, STEP = (0x1234 << 32) + 0x9abcdef1, (1 << 32) + 5


# ---------------------------------------------------------------------------------------------- 1. the mask
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropped_share_is_the_threshold(p):
    """Over 2^20 elements the dropped share lies within 6 sqrt(p (1 - p) / n) of thr / 65536 (a binomial's six sigma),
    for the (thr, factor) the product derives from p."""
    from passl_amd.hip import ops
    DP.check_known_answers()
    thr, factor = ops.dropout_params(p)
    assert (thr, np.float32(factor)) == DU.thr_factor(p)
    assert thr == int(math.floor(p * 65536 + 0.5)) and factor == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    n = 1 << 20
    keep = DU.keep_mask(n, SEED, STEP, 3, thr)
    share = 1.0 - keep.mean()
    print('p %.2f: thr %d, dropped %.6f, expected %.6f' % (p, thr, share, thr / 65536.0))
    assert abs(share - thr / 65536.0) <= 6.0 * math.sqrt(p * (1 - p) / n)
    # every one of the 8 positions of a chunk gets its own 16 bits: no two columns of the chunk view agree
    cols = keep.reshape(-1, 8)
    for a in range(8):
        for b in range(a + 1, 8):
            assert 0.05 < np.mean(cols[:, a] != cols[:, b]) < 0.95, (a, b)


def test_masks_of_another_site_step_or_seed_differ():
    from passl_amd.hip import nn as hnn
    st = hnn.DropoutState(0.5, seed=SEED, step=STEP)
    assert (st.seed, st.step(), st.ordinal) == (SEED, STEP, 0)
    n = 8 * 1024
    base = DU.keep_mask(n, st.seed, st.step(), 1, st.thr)
    for seed, step, site in [(SEED, STEP, 2), (SEED, STEP + 1, 1), (SEED, STEP + (1 << 32), 1), (SEED + 1, STEP, 1),
                             (SEED + (1 << 32), STEP, 1)]:
        other = DU.keep_mask(n, seed, step, site, st.thr)
        assert 0.4 < np.mean(other != base) < 0.6, (seed, step, site)
    assert np.array_equal(base, DU.keep_mask(n, SEED, STEP, 1, st.thr))
    # a lower threshold keeps a superset: the mask is a comparison of fixed 16-bit draws
    assert np.all(DU.keep_mask(n, SEED, STEP, 1, 100)[base])


def test_threshold_edge_cases_and_refusals():
    from passl_amd.hip import lib as L, nn as hnn, ops
    from passl_amd.csrc.build import build
    assert ops.dropout_params(0.0) == (0, 1.0)
    assert DU.keep_mask(4096, SEED, STEP, 0, 0).all()                       # thr 0: r >= 0 always
    x = np.linspace(-3, 3, 4096, dtype=np.float32)
    assert np.array_equal(DU.dropout(x, DU.keep_mask(4096, SEED, STEP, 0, 0), 1.0), x)
    assert ops.dropout_params(0.99999)[0] == 65535
    for bad in (1.0, -0.1, 1.5, 0.999995, float('nan')):                    # 0.999995 rounds to thr = 65536
        with pytest.raises(ValueError):
            ops.dropout_params(bad)
        with pytest.raises(ValueError):
            hnn.Dropout(bad)
    with pytest.raises(NotImplementedError):
        hnn.Dropout(0.1, mode='downscale_in_infer')
    d = hnn.Dropout(0.1)
    t = torch.zeros(8)
    assert d.eval()(t) is t and hnn.Dropout(0.0).train()(t) is t            # identity: no launch, no copy
    with pytest.raises(RuntimeError):
        d.train()(t)                                                        # unbound: never a silent identity
    # the C entry points validate before any launch (host pointers: a launch would fault)
    if not os.path.exists(L.LIB_PATH):
        build()
    lib = L.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = (8, 6554, 1.0, 1, p, 0, L.F32, None)
    assert lib.passl_hip_dropout(p, p, 8, 65536, 1.0, 1, p, 0, L.F32, None) == L.EINVAL
    assert lib.passl_hip_dropout(p, p, 8, -1, 1.0, 1, p, 0, L.F32, None) == L.EINVAL
    assert lib.passl_hip_dropout(p, p, 12, 6554, 1.0, 1, p, 0, L.F32, None) == L.EINVAL          # n % 8
    assert lib.passl_hip_dropout(p, p, 8, 6554, 1.0, 1, None, 0, L.F32, None) == L.EINVAL        # no step counter
    assert lib.passl_hip_dropout(p, p, 8, 6554, 1.0, 1, p, 0, 7, None) == L.EUNSUPPORTED         # dtype
    for name, tensors in [('dropout', 2), ('dropout_add', 3), ('gelu_dropout_fwd', 2), ('gelu_dropout_bwd', 3)]:
        fn = getattr(lib, 'passl_hip_' + name)
        assert fn(*([p] * tensors), (1 << 35) + 8, *ok[1:]) == L.EUNSUPPORTED, name            # chunk index > 32 bits
        assert fn(*([None] * tensors), *ok) == L.EINVAL, name
    assert lib.passl_hip_dropout_advance(None, None) == L.EINVAL


# ---------------------------------------------------------------------------------------------- 2. the scheduler
def test_vit_lr_scheduler_matches_the_reference_values():
    from passl_amd.solver.builder import LRSCHEDULERS
    klass = LRSCHEDULERS.get('ViTLRScheduler')
    z = np.load(GOLDEN)
    cases = json.loads(str(z['sched_args']))         # the constructor arguments the golden script used
    assert sorted('sched/' + k for k in cases) == sorted(k for k in z.files if k.startswith('sched/'))
    for name, kw in cases.items():
        want = z['sched/' + name]
        s = klass(**kw)
        assert s.last_epoch == 0                             # the base constructor took the first step
        got = [s()]
        for _ in range(len(want) - 1):
            s.step()
            got.append(s())
            assert s() == s.get_lr() == s.last_lr
        assert np.array_equal(np.asarray(got), want), (name, got, want.tolist())
    assert z['sched/cos_warm'][0] == 0.0 and z['sched/cos_warm'][6] == 3e-3 and z['sched/cos_warm'][-1] == 0.0
    assert z['sched/lin_plain'][-1] == 0.01


def test_vit_lr_scheduler_with_a_warmup_longer_than_the_run():
    """warmup_steps >= T_max is cut to T_max (lr_scheduler.py:96-97); the reference then divides 0 by 0 at the first
    value asked for.  Here the decay counts as over and the warm-up factor shapes the rate alone."""
    from passl_amd.solver.lr_scheduler import ViTLRScheduler
    for kind, end in (('cosine', 0.0), ('linear', 1e-5)):
        s = ViTLRScheduler(0.5, step_each_epoch=2, epochs=2, decay_type=kind, warmup_steps=9)
        assert s.warmup_steps == s.T_max == 4
        for k in range(1, 7):
            s.step()
            assert s() == end * min(1.0, k / 4.0)
    with pytest.raises(ValueError):
        ViTLRScheduler(0.5, step_each_epoch=2, epochs=2, decay_type='step')


# ---------------------------------------------------------------------------------------------- 3. the loss
LOSS_CASES = [(3, 5), (2, 1000), (2, 1001)]
EPS = {'none': None, '1e-4': 1e-4}


def test_vit_ce_restatement_matches_the_reference_values():
    """The float64 restatement the GPU test compares the kernels with is the reference's number: equal to what
    passl/loss/celoss.py ViTCELoss returned on the same logits once it is given the target values as the reference's
    line forms them (in float32); with the targets of the product (double, rounded once) it moves by no more than those
    two roundings can explain."""
    from passl_amd.hip import ops
    from passl_amd.loss import _LOSSES, ViTCELoss
    assert _LOSSES['ViTCELoss'] is ViTCELoss
    z = np.load(GOLDEN)
    for N, Cc in LOSS_CASES:
        x, y = z['loss/x_%dx%d' % (N, Cc)], z['loss/y_%dx%d' % (N, Cc)]
        assert x.dtype == np.float64 and x.max() == 40.0 and x.min() == -40.0
        for tag, eps in EPS.items():
            want, gwant = float(z['loss/value_%dx%d_%s' % (N, Cc, tag)]), z['loss/grad_%dx%d_%s' % (N, Cc, tag)]
            _t, _rows, loss, dx, _s, _tt = DU.vit_ce(x, y, eps, targets=DU.vit_ce_targets_ref32(eps))
            assert abs(loss - want) <= 1e-13 * abs(want), (N, Cc, tag, loss, want)
            assert np.abs(dx - gwant).max() <= 1e-15
            layer = ViTCELoss(epsilon=eps)
            t_on, t_off = layer.targets
            assert (t_on, t_off) == ops.sigmoid_ce_targets(eps)
            assert t_on == float(np.float32(DU.vit_ce_targets(eps)[0])) and t_off == float(np.float32(DU.vit_ce_targets(eps)[1]))
            _t, _rows, loss_p, _dx, _s, _tt = DU.vit_ce(x, y, eps, targets=(t_on, t_off))
            assert abs(loss_p - want) <= 2.0 ** -23 * np.abs(x).sum() / N * max(t_on, 1e-4) + 1e-13 * abs(want)


@pytest.mark.parametrize('tag', sorted(EPS))
@pytest.mark.parametrize('N,Cc', LOSS_CASES)
def test_vit_ce_in_float32_meets_the_kernel_bounds(N, Cc, tag):
    """The bounds tests/test_dropout_gpu.py holds the kernels to, met by a float32 numpy evaluation of the same
    formulas with the product's target values: row loss within (C + 8) 2^-24 sum|term| (C additions and a few ulp per
    term), gradient within 8 2^-24 (sigmoid(x) + t) / N."""
    from passl_amd.hip import ops
    z = np.load(GOLDEN)
    x64, y = z['loss/x_%dx%d' % (N, Cc)], z['loss/y_%dx%d' % (N, Cc)]
    x = x64.astype(np.float32)
    targets = ops.sigmoid_ce_targets(EPS[tag])
    terms, rows, _loss, dx, sig, t = DU.vit_ce(x.astype(np.float64), y, EPS[tag], targets=targets)
    _t32, rows32, _l32, dx32, _s32, _tt32 = DU.vit_ce(x, y, EPS[tag], dtype=np.float32, targets=targets)
    assert rows32.dtype == np.float32 and dx32.dtype == np.float32
    bound = (Cc + 8) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    print('rows: err / bound', (np.abs(rows32 - rows) / bound).max())
    assert np.all(np.abs(rows32 - rows) <= bound)
    gbound = 8 * 2.0 ** -24 * (sig + t) / N
    print('grad: err / bound', (np.abs(dx32 - dx) / gbound).max())
    assert np.all(np.abs(dx32 - dx) <= gbound)


# ---------------------------------------------------------------------------------------------- 4. constructors, YAML
def test_vision_transformer_builds_with_drop_rate():
    hip_config.set_device('cpu')
    import passl.models as PM
    from passl_amd.hip import nn as hnn
    torch.manual_seed(3)
    plain = PM.VisionTransformer(**SMALL)
    torch.manual_seed(3)
    m = PM.VisionTransformer(drop_rate=0.1, **SMALL)
    assert list(plain.state_dict()) == list(m.state_dict())                 # no new entry
    for (k, a), b in zip(plain.state_dict().items(), m.state_dict().values()):
        assert torch.equal(a, b), k                                         # and the same initialisation
    assert plain._dropout is None and plain.dropout_step() == 0 and plain.pos_drop.p == 0.0
    st = m._dropout
    assert isinstance(m.pos_drop, hnn.Dropout) and (m.pos_drop.state, m.pos_drop.site) == (st, 0)
    assert (st.thr, st.factor) == (6554, float(np.float32(1) / (np.float32(1) - np.float32(0.1))))
    for i, blk in enumerate(m.blocks):
        assert blk.drop == 0.1 and (blk._drop_state, blk._drop_site) == (st, 1 + 3 * i)
        assert blk.attn.proj_drop.p == 0.1 and blk.mlp.drop.p == 0.1
    assert m.dropout_step() == 0
    m.set_dropout_seed(12345, step=(1 << 40) + 7)
    assert st.seed == 12345 and m.dropout_step() == (1 << 40) + 7
    with pytest.raises(ValueError):
        plain.set_dropout_seed(1)


def test_dropout_seed_follows_the_global_generator_and_the_rank(monkeypatch):
    hip_config.set_device('cpu')
    import passl.models as PM

    def seed_of(manual, rank=None):
        if rank is None:
            monkeypatch.delenv('RANK', raising=False)
        else:
            monkeypatch.setenv('RANK', str(rank))
        torch.manual_seed(manual)
        return PM.VisionTransformer(drop_rate=0.1, **SMALL)._dropout.seed
    a = seed_of(3)
    assert a == seed_of(3) and a != seed_of(4)
    assert seed_of(3, rank=2) == (a + 2) & (2 ** 64 - 1)


def test_what_stays_refused():
    hip_config.set_device('cpu')
    import passl.models as PM
    from passl_amd.loss import ViTCELoss
    from passl_amd.modules.vit import Attention, Block, Mlp
    from passl_amd.hip import nn as hnn
    PM.VisionTransformer(drop_rate=0.1, **SMALL)                            # builds
    for kw in (dict(drop_path_rate=0.1), dict(attn_drop_rate=0.1), dict(drop_rate=0.1, attn_drop_rate=0.1),
               dict(qk_scale=0.5)):
        with pytest.raises(NotImplementedError):
            PM.VisionTransformer(**kw, **SMALL)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            PM.VisionTransformer(drop_rate=bad, **SMALL)
    with pytest.raises(NotImplementedError):
        ViTCELoss(type='softmax')
    with pytest.raises(AssertionError):
        ViTCELoss(type='focal')
    with pytest.raises(NotImplementedError):
        Attention(64, num_heads=2, attn_drop=0.1)
    with pytest.raises(NotImplementedError):
        Block(64, 2, drop=0.1, drop_path=0.1)
    with pytest.raises(NotImplementedError):
        Mlp(64, act_layer=hnn.QuickGELU, drop=0.1)
    assert Mlp(64, drop=0.1).drop.p == 0.1 and Attention(64, num_heads=2, proj_drop=0.1).proj_drop.p == 0.1
    # the other towers
    from passl_amd.models.mocov3 import MoCoV3ViT
    with pytest.raises(NotImplementedError):
        MoCoV3ViT(drop_rate=0.1, **{k: v for k, v in SMALL.items() if k != 'class_num'})


def test_supervised_vit_yaml_names_what_is_built():
    from passl_amd.loss import ViTCELoss, build_loss
    from passl_amd.solver.builder import LRSCHEDULERS
    from passl_amd.utils.config import get_config
    import passl.models as PM
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_sup_synthetic.yaml'), [])
    assert cfg['Model']['name'] == 'ViT_base_patch16_224' and cfg['Model']['drop_rate'] == 0.1
    assert callable(getattr(PM, cfg['Model']['name']))
    assert cfg['Global']['accum_steps'] == 2 and cfg['Optimizer']['grad_clip']['clip_norm'] == 1.0
    loss = build_loss([{k: dict(v) for k, v in e.items()} for e in cfg['Loss']['Train']])
    assert isinstance(loss.loss_func[0], ViTCELoss) and loss.loss_func[0].epsilon == 1e-4
    sched = dict(cfg['LRScheduler'])
    klass = LRSCHEDULERS.get(sched.pop('name'))
    s = klass(step_each_epoch=2503, epochs=cfg['Global']['epochs'], **sched)
    assert s.warmup_steps == 10000 and s.T_max == 300 * 2503 and s() == 0.0
    s.step(10000)
    assert s() == 3e-3
