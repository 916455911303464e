"""Random erasing — everything that needs no GPU: the box stream against the reference's
(tests/golden/random_erasing_boxes.npz), refusals, the numpy restatement of the 'pixel' normals, build_dataloader and
the YAML."""
import copy
import glob
import os
import random

import numpy as np
import pytest
import torch
import yaml

import random_erasing_util as RU
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
ERASE_YAML = os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_erase_synthetic.yaml')
DROPPATH_YAML = os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_droppath_synthetic.yaml')


def _fixture():
    return np.load(os.path.join(GOLDEN, 'random_erasing_boxes.npz'))


# ---------------------------------------------------------------------------------------------- 1. the box stream
@pytest.mark.parametrize('case', RU.CASES, ids=lambda c: 'seed%d' % c[0])
def test_draw_follows_the_reference_stream(case):
    """RandomErasing.draw under random.Random(seed) = the reference's class under random.seed(seed), sample by sample:
    the same boxes, rejected attempts included; a second call continues the stream as the reference's does."""
    from passl_amd.datasets.preprocess import RandomErasing
    seed, (B, H, W), kw, erased, _rejected = case
    z = _fixture()
    fn = RandomErasing(rng=random.Random(seed), seed=1, **kw)
    t = fn.draw(B, H, W)
    assert t.dtype == np.int32 and t.shape == (B, 4)
    assert np.array_equal(t, z['boxes_%d' % seed])
    assert int((t[:, 2] > 0).sum()) == erased == int(z['counts_%d' % seed][0])
    RandomErasing.validate(t, H, W)
    if seed == RU.SECOND_CALL_SEED:
        assert np.array_equal(fn.draw(B, H, W), z['boxes_%d_second' % seed])


def test_fixture_is_sane():
    z = _fixture()
    for seed, (B, H, W), kw, erased, rejected in RU.CASES:
        t = z['boxes_%d' % seed]
        assert t.shape == (B, 4) and t.dtype == np.int32
        assert tuple(z['counts_%d' % seed]) == (erased, rejected) and erased >= 8
        on = t[:, 2] > 0
        assert int(on.sum()) == erased and (t[~on] == 0).all() and (t[on, 3] > 0).all()
        assert (t[:, 0] + t[:, 2] <= H).all() and (t[:, 1] + t[:, 3] <= W).all() and (t >= 0).all()
        if (H, W) == (24, 40):
            assert (t[:, 2] != t[:, 3]).any()               # an axis swap cannot hide
        if 'max_count' in kw:
            assert on.all()                                 # prob 1: one box each, whatever count was drawn
    assert os.path.getsize(os.path.join(GOLDEN, 'random_erasing_boxes.npz')) < 64 * 1024


def test_draw_defaults_to_the_global_random_stream():
    from passl_amd.datasets.preprocess import RandomErasing
    z = _fixture()
    seed, (B, H, W), kw, _e, _r = RU.CASES[1]
    random.seed(seed)
    fn = RandomErasing(seed=1, **kw)
    assert fn.rng is None
    assert np.array_equal(fn.draw(B, H, W), z['boxes_%d' % seed])


def test_num_splits_leaves_the_first_part_untouched_and_undrawn():
    from passl_amd.datasets.preprocess import RandomErasing
    t = RandomErasing(prob=1., num_splits=2, rng=random.Random(11), seed=1).draw(16, 32, 32)
    assert (t[:8] == 0).all() and (t[8:, 2] > 0).all()
    # nothing was drawn for the first half: the second half is what a batch of 8 draws from the same seed
    assert np.array_equal(t[8:], RandomErasing(prob=1., rng=random.Random(11), seed=1).draw(8, 32, 32))
    t3 = RandomErasing(prob=1., num_splits=3, rng=random.Random(11), seed=1).draw(16, 32, 32)
    assert (t3[:5] == 0).all() and (t3[5:, 2] > 0).all()


def test_from_v2_draws_what_the_v110_spelling_draws():
    from passl_amd.datasets.preprocess import RandomErasing
    a = RandomErasing.from_v2(EPSILON=.25, sl=.02, sh=1 / 3, r1=.3, attempt=10, use_log_aspect=True, mode='pixel',
                              rng=random.Random(4), seed=1)
    b = RandomErasing(prob=.25, mode='pixel', max_count=1, rng=random.Random(4), seed=1)
    assert a.mode == 'pixel' and a.attempts == 10
    ta = a.draw(64, 24, 40)
    assert np.array_equal(ta, b.draw(64, 24, 40)) and np.array_equal(ta, _fixture()['boxes_4'])
    # the v2 defaults: 100 attempts, the aspect ratio uniform in (r1, 1 / r1) without the exp
    c = RandomErasing.from_v2(EPSILON=1., rng=random.Random(4), seed=1)
    assert c.attempts == 100 and c.max_area == 0.4 and c.mode == 'const'
    ref = random.Random(4)
    assert not ref.random() > 1.
    area, aspect = ref.uniform(.02, .4) * 32 * 32, ref.uniform(.3, 1 / .3)
    h, w = int(round(np.sqrt(area * aspect))), int(round(np.sqrt(area / aspect)))
    assert h < 32 and w < 32
    want = (ref.randint(0, 32 - h), ref.randint(0, 32 - w), h, w)
    assert tuple(c.draw(1, 32, 32)[0]) == want
    assert RandomErasing.from_v2(EPSILON='0.25', sl='0.02', sh='1/3', r1='0.3', seed=1).max_area == 1 / 3


def test_refusals(monkeypatch):
    from passl_amd.datasets.preprocess import RandomErasing, build_random_erasing
    with pytest.raises(NotImplementedError, match='width is not 3'):
        RandomErasing(mode='rand')
    with pytest.raises(NotImplementedError):
        RandomErasing.from_v2(mode='rand')
    with pytest.raises(NotImplementedError):
        RandomErasing.from_v2(mean=[0.5, 0., 0.])
    with pytest.raises(NotImplementedError):
        build_random_erasing([dict(name='RandomErasing', prob=0.25, mode='rand')])
    for prob in (-0.1, 1.5):
        with pytest.raises(ValueError):
            RandomErasing(prob=prob)
    with pytest.raises(ValueError):
        RandomErasing(min_area=0.5, max_area=0.4)
    with pytest.raises(ValueError):
        RandomErasing(mode='colour')
    ok = np.array([[0, 0, 0, 0], [3, 2, 5, 6], [0, 0, 7, 9], [7, 9, 1, 1]], dtype=np.int32)
    RandomErasing.validate(ok, 8, 10)
    for row in ([4, 0, 5, 1], [0, 5, 1, 6], [-1, 0, 2, 2], [0, -1, 2, 2], [0, 0, -2, 2], [0, 0, 2, -2], [8, 0, 1, 1],
                [0, 0, 2 ** 31 - 1, 1]):
        bad = ok.copy()
        bad[2] = row
        with pytest.raises(ValueError, match='row 2'):
            RandomErasing.validate(bad, 8, 10)
    # __call__ validates before anything reaches a device
    fn = RandomErasing(prob=1., seed=1)
    monkeypatch.setattr(fn, 'draw', lambda B, H, W: np.array([[0, 0, 9, 1]] * B, dtype=np.int32))
    with pytest.raises(ValueError):
        fn(torch.zeros(2, 3, 8, 8))
    assert fn.step == 0


# ---------------------------------------------------------------------------------------------- 2. the normals
def test_normal_restatement_moments_and_steps():
    """The float64 restatement of the kernel's 'pixel' definition: Philox's known answers, then mean within 5 / sqrt(n)
    and variance within 5 sqrt(2 / n) of (0, 1) (5 sigma of the sample mean / variance of n normals) on 16 samples of
    3 x 16 x 16; another step gives other values."""
    RU.check_known_answers()
    a = RU.MOMENT_ARGS
    z = np.concatenate([RU.normals(a['seed'], a['step'], b, a['E']) for b in range(a['B'])])
    n = z.size
    assert n == 12288 and np.isfinite(z).all()
    print('mean %.4f var %.4f max |z| %.2f' % (z.mean(), z.var(), np.abs(z).max()))
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    z1 = np.concatenate([RU.normals(a['seed'], a['step'] + 1, b, a['E']) for b in range(a['B'])])
    assert not np.any(z == z1)
    # by position: a shorter sample is a prefix, samples differ
    assert np.array_equal(RU.normals(5, 0, 2, 765), RU.normals(5, 0, 2, 768)[:765])
    assert not np.any(RU.normals(5, 0, 2, 64) == RU.normals(5, 0, 3, 64))


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


def test_build_dataloader_builds_the_eraser_for_the_new_yaml_only(monkeypatch):
    from passl_amd.datasets import build_dataloader
    from passl_amd.datasets.preprocess import RandomErasing, build_random_erasing
    from passl_amd.hip import ops
    hip_config.set_device('cpu')
    launched = []
    monkeypatch.setattr(ops, 'random_erase', lambda *a, **k: launched.append(a))
    seen = built = 0
    for path, block in _yaml_train_blocks():
        seen += 1
        new = os.path.samefile(path, ERASE_YAML)
        assert (build_random_erasing(block['dataset'].get('transforms')) is not None) == new, path
        if str(block['dataset'].get('name', '')).startswith('Synthetic'):
            loader, mixup_fn = build_dataloader(_shrunk(block), torch.device('cpu'))
            built += 1
            fn = loader.batch_transform
            assert (fn is not None) == new, path
            if new:
                assert isinstance(fn, RandomErasing) and (fn.prob, fn.mode) == (0.25, 'pixel')
                assert (fn.min_count, fn.max_count, fn.rng, fn.step) == (1, 1, None, 0)
                assert mixup_fn is None
    assert seen >= 6 and built >= 4
    assert not launched                                      # building on the CPU launches nothing
    assert build_random_erasing(None) is None and build_random_erasing([]) is None
    assert build_random_erasing([dict(name='RandomResizedCrop', size=224), dict(name='RandomHorizontalFlip')]) is None
    fn = build_random_erasing([dict(name='RandomResizedCrop', size=224),
                               dict(name='RandomErasing', prob=0.25, mode='pixel', max_count=1, seed=9)])
    assert (fn.prob, fn.mode, fn.seed) == (0.25, 'pixel', 9)
    fn = build_random_erasing([dict(name='RandomErasing', EPSILON=0.25, sl=0.02, sh=1 / 3, r1=0.3, attempt=10,
                                    use_log_aspect=True, mode='pixel')])
    assert (fn.prob, fn.mode, fn.attempts) == (0.25, 'pixel', 10)


def test_other_sources_take_no_eraser():
    """Two-view and image-text sources are not touched, whatever their transforms list says."""
    from passl_amd.datasets import build_dataloader
    hip_config.set_device('cpu')
    tf = [dict(name='RandomErasing', prob=0.25, mode='pixel', max_count=1)]
    for name in ('SyntheticTwoView', 'SyntheticImageText'):
        loader, _ = build_dataloader(dict(dataset=dict(name=name, num_samples=4, image_size=16, transforms=tf),
                                          sampler=dict(batch_size=2)), torch.device('cpu'))
        assert loader.batch_transform is None
        assert len(next(iter(loader))) == 2


def test_default_seed_comes_from_the_torch_generator_plus_rank(monkeypatch):
    from passl_amd.datasets.preprocess import RandomErasing
    torch.manual_seed(77)
    want = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(77)
    assert RandomErasing().seed == want
    monkeypatch.setenv('RANK', '3')
    torch.manual_seed(77)
    assert RandomErasing().seed == want + 3


def test_erase_yaml_is_the_droppath_yaml_plus_one_entry():
    with open(ERASE_YAML) as f:
        new = yaml.safe_load(f)
    with open(DROPPATH_YAML) as f:
        old = yaml.safe_load(f)
    entry = new['dataloader']['train']['dataset'].pop('transforms')
    assert new == old
    assert entry == [dict(name='RandomErasing', prob=0.25, mode='pixel', max_count=1)]
    assert 'batch_transforms' not in new['dataloader']['train']['dataset']
