"""Mixup / CutMix and soft-target cross-entropy — everything that needs no GPU: the parameter stream against the
reference's (tests/golden/mixup_params.npz), the committed fixtures, build_dataloader, the YAML, CELoss's constructor."""
import copy
import glob
import os

import numpy as np
import pytest
import torch
import yaml

import mixup_util as MU
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
RECIPE_YAML = os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml')
DROPPATH_YAML = os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_droppath_synthetic.yaml')


def _params():
    return np.load(os.path.join(GOLDEN, 'mixup_params.npz'))


# ---------------------------------------------------------------------------------------------- 1. parameter stream
@pytest.mark.parametrize('seed', MU.PARAM_SEEDS)
def test_draw_follows_the_reference_stream(seed):
    """Mixup.draw under RandomState(seed) = the reference's Mixup under np.random.seed(seed): same kind, same box,
    lambda equal as float64.  A second call on the same stream continues it as the reference's second call does."""
    from passl_amd.datasets.preprocess import Mixup
    z = _params()
    fn = Mixup(num_classes=16, rng=np.random.RandomState(seed), **MU.RECIPE)
    use_cutmix, lam, box = fn.draw((8, 3, 64, 64))
    assert use_cutmix == bool(z['use_cutmix'][seed])
    assert isinstance(lam, float) and lam == float(z['lam'][seed])
    if use_cutmix:
        assert tuple(box) == tuple(int(v) for v in z['box'][seed])
    else:
        assert box is None
    second = [int(s) for s in z['second_seeds']]
    if seed in second:
        k = second.index(seed)
        use_cutmix, lam, box = fn.draw((8, 3, 64, 64))
        assert use_cutmix == bool(z['second_use_cutmix'][k]) and lam == float(z['second_lam'][k])
        assert (tuple(box) if use_cutmix else (0, 0, 0, 0)) == tuple(int(v) for v in z['second_box'][k])


def test_draw_defaults_to_the_global_numpy_stream():
    from passl_amd.datasets.preprocess import Mixup
    z = _params()
    np.random.seed(2)
    use_cutmix, lam, box = Mixup(num_classes=16, **MU.RECIPE).draw((8, 3, 64, 64))
    assert use_cutmix and lam == float(z['lam'][2]) and tuple(box) == tuple(int(v) for v in z['box'][2])


def test_unmixed_and_single_kind_draws():
    from passl_amd.datasets.preprocess import Mixup
    shape = (8, 3, 64, 64)
    # prob 0: one draw (the rand() < prob test), nothing mixed
    rng = np.random.RandomState(5)
    assert Mixup(0.8, 1.0, prob=0., rng=rng).draw(shape) == (False, 1., None)
    assert rng.rand() == np.random.RandomState(5).rand(2)[1]
    fn = Mixup(0.8, 1.0, rng=np.random.RandomState(5))
    fn.mixup_enabled = False
    assert fn.draw(shape) == (False, 1., None)
    # one kind only: no switch draw
    ref = np.random.RandomState(7)
    ref.rand()
    assert Mixup(0.8, 0., rng=np.random.RandomState(7)).draw(shape) == (False, float(ref.beta(0.8, 0.8)), None)
    for s in range(4):
        use_cutmix, lam, (yl, yh, xl, xh) = Mixup(0., 1.0, rng=np.random.RandomState(s)).draw(shape)
        assert use_cutmix and 0 <= yl <= yh <= 64 and 0 <= xl <= xh <= 64
        assert lam == 1. - (yh - yl) * (xh - xl) / float(64 * 64)
    use_cutmix, lam, box = Mixup(0., 1.0, correct_lam=False, rng=np.random.RandomState(3)).draw(shape)
    ref = np.random.RandomState(3)
    ref.rand()
    assert use_cutmix and lam == float(ref.beta(1.0, 1.0))


# ---------------------------------------------------------------------------------------------- 2. the fixtures
def test_params_fixture_is_sane():
    z = _params()
    kinds = z['use_cutmix']
    assert len(kinds) == 12 and kinds.any() and not kinds.all()
    for s in range(12):
        yl, yh, xl, xh = [int(v) for v in z['box'][s]]
        if kinds[s]:
            assert yh > yl and xh > xl and float(z['lam'][s]) == 1. - (yh - yl) * (xh - xl) / 4096.
        assert 0. < float(z['lam'][s]) < 1.
        assert np.abs(z['target'][s].sum(axis=1) - 1.).max() <= 1e-6
        assert np.array_equal(z['target'][s], MU.mixup_target_ref(z['labels'], 16, float(z['lam'][s]), 0.1))
    assert z['x_mixed_sub'].shape == (12, 8, 3, 8, 8) and z['x_mixed_sub'].dtype == np.float32
    # the restatement the GPU test compares the kernel with reproduces the reference's batch bit for bit
    gen = torch.Generator().manual_seed(909)
    x = torch.randn(8, 3, 64, 64, generator=gen)
    y = torch.randint(0, 16, (8,), generator=gen)
    assert np.array_equal(y.numpy(), z['labels'])
    for s in range(12):
        got = MU.batch_mix_ref(x, float(z['lam'][s]), tuple(int(v) for v in z['box'][s]) if kinds[s] else None)
        assert np.array_equal(got[:, :, ::8, ::8].numpy().view(np.int32), z['x_mixed_sub'][s].view(np.int32)), s
    # the two losses of the reference's util/loss.py, restated in float64
    scores = torch.from_numpy(z['scores'])
    assert abs(MU.soft_ce_ref(scores, torch.from_numpy(MU.mixup_target_ref(z['labels'], 16, 1., 0.1)))[0]
               - float(z['ce_label_smoothing'])) < 1e-5
    assert abs(MU.soft_ce_ref(scores, torch.from_numpy(z['target'][11]))[0] - float(z['ce_soft_target'])) < 1e-5


@pytest.mark.parametrize('name', ['mae_ft_mix_small', 'mae_ft_mix_vit_b'])
def test_finetune_fixtures_discriminate_mixed_from_plain(name):
    """What tests/golden/make_golden_mixup.py asserts when it writes the files, on the committed files: the mixed step 0
    is farther from the plain step than 2 x the fp32 loss bound and 3 x the fp32 feature bound of the GPU test."""
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    N, _hw, steps, _classes = [int(v) for v in z['meta']]
    assert N == 8 and steps == 2
    assert not bool(z['s0_use_cutmix']) and bool(z['s1_use_cutmix'])
    yl, yh, xl, xh = [int(v) for v in z['s1_box']]
    assert yh > yl and xh > xl
    d_loss = abs(float(z['s0_loss']) - float(z['s0_loss_plain'])) / abs(float(z['s0_loss_plain']))
    f, f0 = z['s0_feat_head'], z['s0_feat_head_plain']
    d_feat = np.abs(f - f0).max() / np.abs(f0).max()
    print(name, 'mixed vs plain: loss %.3e rel, feat %.3e of max' % (d_loss, d_feat))
    assert d_loss > 2 * MU.FT_TOL_F32['loss'] and d_feat > 3 * MU.FT_TOL_F32['feat']
    assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < 64 * 1024


# ---------------------------------------------------------------------------------------------- 3. builder, YAML
def _yaml_train_blocks():
    for path in sorted(glob.glob(os.path.join(ROOT, 'configs', '**', '*.yaml'), recursive=True)):
        with open(path) as f:
            cfg = yaml.safe_load(f)
        block = ((cfg or {}).get('dataloader') or {}).get('train')
        if block and 'dataset' in block:
            yield path, block


def _shrunk(block):
    block = copy.deepcopy(block)
    block['dataset'].update(num_samples=4, image_size=16)
    block['sampler'] = dict(block.get('sampler') or {}, batch_size=2)
    block['loader'] = {}
    return block


def test_build_dataloader_builds_the_recipe_mixup_only():
    from passl_amd.datasets import build_dataloader
    from passl_amd.datasets.preprocess import Mixup, build_mixup
    hip_config.set_device('cpu')
    seen = built = 0
    for path, block in _yaml_train_blocks():
        seen += 1
        recipe = os.path.samefile(path, RECIPE_YAML)
        fn = build_mixup(block['dataset'].get('batch_transforms'))
        assert (fn is not None) == recipe, path
        if str(block['dataset'].get('name', '')).startswith('Synthetic'):
            _loader, fn = build_dataloader(_shrunk(block), torch.device('cpu'))
            built += 1
            assert (fn is not None) == recipe, path
            if recipe:
                assert isinstance(fn, Mixup)
                assert (fn.mixup_alpha, fn.cutmix_alpha, fn.mix_prob, fn.switch_prob, fn.mode) == (0.8, 1.0, 1., 0.5, 'batch')
                assert (fn.label_smoothing, fn.num_classes, fn.correct_lam, fn.rng) == (0.1, 1000, True, None)
    assert seen >= 5 and built >= 3
    # label_smoothing / num_classes of the block are passed on (the reference's builder drops them)
    fn = build_mixup([dict(name='Mixup', mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax='', prob=1., switch_prob=0.5,
                           mode='batch', label_smoothing=0.2, num_classes=16)])
    assert (fn.label_smoothing, fn.num_classes) == (0.2, 16)
    assert build_mixup([dict(name='Mixup', mixup_alpha=0., cutmix_alpha=0., prob=1., switch_prob=0.5, mode='batch')]) is None
    assert build_mixup(None) is None


def test_what_is_not_built_raises():
    from passl_amd.datasets.preprocess import Mixup, build_mixup
    with pytest.raises(NotImplementedError):
        build_mixup([dict(name='LVViTMixup', lam=1., smoothing=0.1, label_size=14, num_classes=1000)])
    for mode in ('elem', 'pair'):
        with pytest.raises(NotImplementedError):
            build_mixup([dict(name='Mixup', mixup_alpha=0.8, cutmix_alpha=1.0, prob=1., switch_prob=0.5, mode=mode)])
    with pytest.raises(NotImplementedError):
        Mixup(0.8, 1.0, cutmix_minmax=(0.2, 0.8))
    with pytest.raises(AssertionError):                       # an odd batch, before anything is drawn or launched
        Mixup(0.8, 1.0)(torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.int64))


def test_recipe_yaml_is_the_droppath_yaml_plus_one_block():
    from passl_amd.modeling import build_model
    from passl_amd.utils.config import get_config
    hip_config.set_device('cpu')
    with open(RECIPE_YAML) as f:
        new = yaml.safe_load(f)
    with open(DROPPATH_YAML) as f:
        old = yaml.safe_load(f)
    block = new['dataloader']['train']['dataset'].pop('batch_transforms')
    assert new == old
    assert block == [dict(name='Mixup', mixup_alpha=0.8, cutmix_alpha=1.0, prob=1., switch_prob=0.5, mode='batch')]
    cfg = get_config(RECIPE_YAML, [])
    model = build_model(cfg.model)
    assert type(model).__name__ == 'MAE_FINETUNE' and model.backbone.drop_path_rate == 0.1


# ---------------------------------------------------------------------------------------------- 4. CELoss
def test_celoss_constructor():
    from passl_amd.loss.celoss import CELoss
    assert CELoss().epsilon is None
    assert CELoss(epsilon=0.1).epsilon == 0.1
    with pytest.raises(AssertionError):
        CELoss(epsilon=1.5)
