"""Colour jitter, grayscale, blur, solarise and the two views of one image, without a GPU: the numpy restatement
(tests/view_aug_util.py) against Pillow itself and against what the reference's classes produced
(tests/golden/view_aug_small.npz); the __host__ build of csrc/view_aug_pixel.h against the restatement over all 2^24
colours; the draws against the observed decisions; refusals, table validation, build_dataloader and the YAML files."""
import copy
import glob
import os
import random
import subprocess

import numpy as np
import pytest
import torch
import yaml
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

import crop_resize_util as CU
import view_aug_util as VU
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
VIEWS_YAML = os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_views_synthetic.yaml')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'view_aug_small.npz'))


@pytest.fixture(scope='module')
def colours():
    return VU.all_colours()


@pytest.fixture(scope='module')
def conversions(colours):
    """(RGB -> HSV, HSV -> RGB) of the restatement over all 2^24 triples, computed once."""
    return VU.rgb2hsv(colours), VU.hsv2rgb(colours)


# ---------------------------------------------------------------------------------------------- 1. Pillow
def test_conversions_equal_pillow_over_all_colours(colours, conversions):
    assert np.array_equal(conversions[0], np.asarray(Image.fromarray(colours).convert('HSV')))
    assert np.array_equal(conversions[1], np.asarray(Image.fromarray(colours, 'HSV').convert('RGB')))


def test_blends_gray_and_solarize_equal_pillow():
    """Factors inside and outside [0, 1], the ColorJitter range of the recipe (0.6 .. 1.4) sampled densely."""
    img = CU.block_noise(11, 1, 37, 41)[0]
    pil = Image.fromarray(img)
    factors = [0.0, 1.0, -0.5, 0.999, 1.001, 2.5, 3.0] + list(np.linspace(0.6, 1.4, 41))
    for f in factors:
        f = float(f)
        assert np.array_equal(VU.brightness(img, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f))), f
        assert np.array_equal(VU.saturation(img, f), np.asarray(ImageEnhance.Color(pil).enhance(f))), f
        assert np.array_equal(VU.contrast(img, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f))), f
    assert np.array_equal(VU.gray(img), np.asarray(pil.convert('L')))
    assert np.array_equal(VU.solarize(img), np.asarray(ImageOps.solarize(pil)))
    for shift in (1, 25, 128, 230, 255):
        h, s, v = pil.convert('HSV').split()
        want = Image.merge('HSV', (Image.fromarray(((np.array(h, np.int32) + shift) % 256).astype(np.uint8), 'L'), s, v))
        assert np.array_equal(VU.hue(img, shift), np.asarray(want.convert('RGB'))), shift


def test_blur_equals_pillow():
    """240 radii over [0.1, 2.3] on each of seven shapes, 1 x 1, 3 x 5 and 5 x 3 among them: box radii 0 and 1."""
    rs = np.random.RandomState(3)
    seen = set()
    n = 0
    for shape in ((1, 1), (3, 5), (5, 3), (2, 7), (1, 9), (17, 16), (37, 41)):
        img = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
        for radius in np.linspace(0.1, 2.3, 240):
            radius = float(radius)
            want = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius=radius)))
            assert np.array_equal(VU.gaussian_blur(img, radius), want), (shape, radius)
            seen.add(VU.box_weights(radius)[0])
            n += 1
    assert seen == {0, 1} and n >= 200
    assert VU.box_weights(1.41)[0] == 0 and VU.box_weights(1.42)[0] == 1 and float(VU.box_radius(2.0)) == 1.375


# ---------------------------------------------------------------------------------------------- 2. the reference
@pytest.mark.parametrize('view', [1, 2])
def test_restatement_equals_the_reference_stage_by_stage(golden, view):
    st = golden['stages_%d' % view]
    for b, (box, ops_, flip) in enumerate(VU.golden_samples(golden, view)):
        top, left, h, w = box
        assert np.array_equal(CU.resize_u8(golden['src'][b, top:top + h, left:left + w], 32), st[0, b])
        jitter = [o for o in ops_ if o[0] <= VU.OP_HUE]
        assert np.array_equal(VU.apply_ops(st[0, b], jitter), st[1, b]), b
        assert np.array_equal(VU.apply_ops(st[0, b], [o for o in ops_ if o[0] <= VU.OP_GRAY]), st[2, b]), b
        assert np.array_equal(VU.apply_ops(st[0, b], ops_), st[3, b]), b
        u8, f32 = VU.view_ref(st[0, b], ops_, flip, CU.SCALE, CU.MEAN, CU.STD)
        assert np.array_equal(u8, st[4, b]) and f32.dtype == np.float32
        assert np.array_equal(f32.view(np.int32), golden['f32_%d' % view][b].view(np.int32)), b
    for b, (box, ops_, flip) in enumerate(VU.golden_samples(golden, view, '_second')):
        top, left, h, w = box
        u8 = CU.resize_u8(golden['src'][b, top:top + h, left:left + w], 32)
        assert np.array_equal(VU.view_ref(u8, ops_, flip, CU.SCALE, CU.MEAN, CU.STD)[0], golden['stages_%d_second' % view][b])
    assert os.path.getsize(os.path.join(GOLDEN, 'view_aug_small.npz')) < 256 * 1024


def _view_cfg(view, S=32):
    crop = {'MAERandCropImage': dict(size=S, scale=[0.2, 1.0], interpolation='bicubic', backend='pil')}
    jit = dict(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1)
    tail = [{'RandomHorizontalFlip': None},
            {'NormalizeImage': dict(scale='1.0/255.0', mean=list(CU.MEAN), std=list(CU.STD), order='hwc')},
            {'ToCHWImage': None}]
    if view == 1:
        mid = [{'ColorJitter': dict(p=0.7, **jit)}, {'RandomGrayscale': dict(p=0.3)},
               {'SimCLRGaussianBlur': dict(sigma=[.1, 2.], p=0.6)}]
    else:
        mid = [{'RandomApply': dict(transforms=[{'ColorJitter': dict(p=1.0, **jit)}], p=0.7)},
               {'RandomGrayscale': dict(p=0.3)}, {'BYOLSolarize': dict(p=0.5)}]
    return [crop] + mid + tail


def _two_views():
    from passl_amd.datasets.preprocess import build_two_views
    return build_two_views([{'TwoViewsTransform': dict(base_transform1=_view_cfg(1), base_transform2=_view_cfg(2))}])


def _close(a, b):
    return a[0] == b[0] and a[2] == b[2] and len(a[1]) == len(b[1]) and \
        all(x[0] == y[0] and x[1] == y[1] for x, y in zip(a[1], b[1]))


def test_draws_equal_the_observed_decisions(golden):
    """random.seed(0) and np.random.seed(0), the global generators: per sample the whole of view 1, then the whole of
    view 2 — boxes, jitter lists and factors, grayscale, blur radii, solarisation and flips are what the reference's
    classes chose; a second consecutive call continues the streams."""
    two = _two_views()
    random.seed(0)
    np.random.seed(0)
    for suffix in ('', '_second'):
        s1, s2 = two.draw(8, 40, 56)
        for v, got in ((1, s1), (2, s2)):
            want = VU.golden_samples(golden, v, suffix)
            for b in range(8):
                assert _close(got[b], want[b]), (suffix, v, b, got[b], want[b])
    # generators of one's own give the same draws and leave the global ones alone
    from passl_amd.datasets.preprocess import (BYOLSolarize, ColorJitter, RandomApply, RandomGrayscale,
                                               SimCLRGaussianBlur)
    rng, nrng = random.Random(7), np.random.RandomState(7)
    random.seed(7)
    np.random.seed(7)
    jit = dict(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1)
    mine = [ColorJitter(0.8, rng=rng, **jit), RandomGrayscale(0.5, np_rng=nrng), SimCLRGaussianBlur(p=0.5, rng=rng),
            BYOLSolarize(0.5, rng=rng), RandomApply([RandomGrayscale(0.5, np_rng=nrng)], 0.5, np_rng=nrng)]
    theirs = [ColorJitter(0.8, **jit), RandomGrayscale(0.5), SimCLRGaussianBlur(p=0.5), BYOLSolarize(0.5),
              RandomApply([RandomGrayscale(0.5)], 0.5)]
    state = (random.getstate(), np.random.get_state()[1].copy())
    a = [t.draw() for _ in range(6) for t in mine]
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1])
    assert a == [t.draw() for _ in range(6) for t in theirs]


def test_jitter_rule_and_hue_shift():
    from passl_amd.datasets.preprocess import ColorJitter
    from passl_amd.datasets.preprocess import view_aug as VA
    j = ColorJitter(0.8, 0.4, 0.4, 0.2, 0.1)
    assert j.entries == [(e[0], e[1], e[2]) for e in VU.jitter_entries(0.4, 0.4, 0.2, 0.1)]
    assert [e[0] for e in j.entries] == [VA.OP_BRIGHTNESS, VA.OP_CONTRAST, VA.OP_SATURATION, VA.OP_HUE]
    assert j.entries[0][1:] == (0.6, 1.4) and j.entries[3][1:] == (-0.1, 0.1)
    assert ColorJitter().entries == [] and ColorJitter(brightness=2.0).entries == [(VA.OP_BRIGHTNESS, 0, 3.0)]
    assert ColorJitter(hue=[-0.2, 0.3]).entries == [(VA.OP_HUE, -0.2, 0.3)]
    with pytest.raises(ValueError):
        ColorJitter(hue=0.6)
    assert VU.hue_shift(-0.05) == 244 and VU.hue_shift(0.05) == 12 and VU.hue_shift(-0.001) == 0
    for radius in (0.1, 0.7, 1.41, 1.42, 2.0):
        assert VA.box_weights(radius) == VU.box_weights(radius)


# ---------------------------------------------------------------------------------------------- 3. the pixel header
PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "view_aug_pixel.h"
using namespace view_aug;
static int32_t bits(float f) { union { float f; int32_t i; } u; u.f = f; return u.i; }
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const size_t n = (size_t)1 << 24;
  unsigned char* buf = (unsigned char*)malloc(n * 3);
  const char* names[6] = {"rgb2hsv", "hsv2rgb", "hue", "sat", "contrast", "solgray"};
  for (int which = 0; which < 6; ++which) {
    for (size_t i = 0; i < n; ++i) {
      Rgb p{(int)(i >> 16) & 255, (int)(i >> 8) & 255, (int)i & 255}, q;
      switch (which) {
        case 0: q = rgb2hsv(p); break;
        case 1: q = hsv2rgb(p); break;
        case 2: q = apply_op(p, kOpHue, 37, 0); break;
        case 3: q = apply_op(p, kOpSaturation, bits(1.3f), 0); break;
        case 4: q = apply_op(apply_op(p, kOpBrightness, bits(0.6f), 0), kOpContrast, bits(1.39f), 117); break;
        default: q = apply_op(apply_op(p, kOpSolarize, 0, 0), kOpGray, 0, 0); break;
      }
      buf[3 * i] = (unsigned char)q.r; buf[3 * i + 1] = (unsigned char)q.g; buf[3 * i + 2] = (unsigned char)q.b;
    }
    char path[4096];
    snprintf(path, sizeof path, "%s/%s.bin", argv[1], names[which]);
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(buf, 3, n, f) != n) return 3;
    fclose(f);
  }
  return 0;
}
'''


def _clang():
    for c in (os.environ.get('PASSL_HOST_CXX'), '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        if c and os.path.exists(c):
            return c
    raise AssertionError('the ROCm clang++ was not found (set PASSL_HOST_CXX)')


def test_host_build_of_the_pixel_header_equals_the_restatement(tmp_path, colours, conversions):
    """csrc/view_aug_pixel.h compiled for the host by the ROCm clang, as a stand-alone program, over all 2^24 colours:
    both conversions, a hue shift, a saturation factor outside [0, 1], brightness then contrast, solarise then gray."""
    src = tmp_path / 'pixel_check.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'pixel_check'
    r = subprocess.run([_clang(), '-O2', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'passl_amd', 'csrc'),
                        str(src), '-o', str(exe), '-lm'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    subprocess.run([str(exe), str(tmp_path)], check=True)

    def got(name):
        return np.fromfile(str(tmp_path / (name + '.bin')), dtype=np.uint8).reshape(4096, 4096, 3)
    assert np.array_equal(got('rgb2hsv'), conversions[0])
    assert np.array_equal(got('hsv2rgb'), conversions[1])
    shifted = conversions[0].copy()
    shifted[..., 0] += 37                                                  # uint8: wraps
    assert np.array_equal(got('hue'), VU.hsv2rgb(shifted))
    assert np.array_equal(got('sat'), VU.saturation(colours, 1.3))
    assert np.array_equal(got('contrast'), VU.contrast(VU.brightness(colours, 0.6), 1.39, m=117))
    assert np.array_equal(got('solgray'), VU.grayscale(VU.solarize(colours)))


# ---------------------------------------------------------------------------------------------- 4. refusals, tables
def test_refusals():
    from passl_amd.datasets.preprocess import GaussianBlur, build_two_views, build_view_pipeline
    with pytest.raises(NotImplementedError, match='cv2'):
        GaussianBlur()
    assert GaussianBlur(_PIL=True, np_rng=np.random.RandomState(1)).draw()[0][0] == 7
    ok = _view_cfg(1)
    build_view_pipeline(ok)
    for bad, what in (({'RandomResizedCrop': dict(size=32)}, 'RandomResizedCrop'), ({'ToTensor': None}, 'ToTensor'),
                      ({'Normalize': dict(mean=[0.5] * 3, std=[0.5] * 3)}, 'Normalize'),
                      ({'RandAugment': None}, 'RandAugment'), ({'GaussianBlur': dict(sigma=[.1, 2.])}, 'cv2')):
        with pytest.raises(NotImplementedError, match=what):
            build_view_pipeline(ok[:1] + [bad] + ok[1:])
    with pytest.raises(NotImplementedError, match='cv2'):
        build_view_pipeline([{'MAERandCropImage': dict(size=32, interpolation='bicubic')}] + ok[1:])     # the default backend
    with pytest.raises(ValueError, match='must read'):
        build_view_pipeline(ok[1:])                                        # no crop
    with pytest.raises(ValueError, match='must read'):
        build_view_pipeline(ok[:4] + [ok[4], ok[1]] + ok[5:])              # a colour entry behind the flip
    blur = {'SimCLRGaussianBlur': dict(p=1.0)}
    with pytest.raises(NotImplementedError, match='more than one'):
        build_view_pipeline(ok[:4] + [blur] + ok[4:])
    with pytest.raises(NotImplementedError, match='behind a blur'):
        build_view_pipeline([ok[0], blur, ok[1]] + ok[4:])
    with pytest.raises(ValueError, match='TwoViewsTransform'):
        build_two_views(ok)
    with pytest.raises(ValueError, match='TwoViewsTransform'):
        build_two_views(None)


def test_table_validation(golden):
    from passl_amd.datasets.preprocess import DeviceViewPipeline as P
    for v in (1, 2):
        crop, table = P.encode(VU.golden_samples(golden, v))
        P.validate(table)
        assert (crop[:, 4:] == 0).all() and table.dtype == np.int32 and table.shape == (8, 24)
    _c, good = P.encode(VU.golden_samples(golden, 1))
    b = int(np.argmax(good[:, 6] >= 0))
    k = int(good[b, 6])
    blurred = int(np.argmax(good[:, 2] >= 0))

    def broken(row, col, value):
        t = good.copy()
        t[row, col] = value
        return t
    nan = int(np.array([np.nan], np.float32).view(np.int32)[0])
    inf = int(np.array([np.inf], np.float32).view(np.int32)[0])
    for t in (broken(0, 0, 9), broken(0, 0, -1), broken(0, 1, 2), broken(b, 8 + k, 7), broken(b, 8 + k, 0),
              broken(b, 16 + k, nan), broken(b, 16 + k, inf), broken(b, 6, -1), broken(b, 6, k + 1), broken(0, 7, 1),
              broken(blurred, 2, 2), broken(blurred, 3, 0), broken(blurred, 5, 9), broken(0, 15, 3),
              good.astype(np.int64), good[:, :23]):
        with pytest.raises(ValueError):
            P.validate(t)
    with pytest.raises(ValueError, match='do not fit'):
        P.encode([((0, 0, 4, 4), [(5, 0)] * 9, False)])
    with pytest.raises(ValueError, match='do not fit'):
        P.encode([((0, 0, 4, 4), [(7, 1.0), (7, 1.0)], False)])
    two = _two_views()
    with pytest.raises(ValueError, match='uint8'):
        two.base_transform1(torch.zeros(2, 3, 8, 8))


# ---------------------------------------------------------------------------------------------- 5. builder, YAML
def _launches_replaced(monkeypatch, order):
    from passl_amd.hip import ops
    monkeypatch.setattr(ops, 'crop_resize_u8', lambda src, t, size: order.append('crop') or
                        torch.zeros(src.shape[0], size, size, 3, dtype=torch.uint8))
    monkeypatch.setattr(ops, 'view_gray_sum', lambda img, t: order.append('sum') or torch.zeros(img.shape[0], dtype=torch.int64))
    monkeypatch.setattr(ops, 'view_pointwise', lambda img, t, sums, part, norm: order.append('point%d' % part) or (
        img if norm is None else torch.zeros(img.shape[0], 3, img.shape[1], img.shape[2])))
    monkeypatch.setattr(ops, 'gaussian_blur_u8', lambda img, t, r: order.append('blur%d' % r) or img)


@pytest.mark.parametrize('ring', [0, 3])
def test_build_dataloader_on_the_new_block(monkeypatch, ring):
    """The block of the new YAML, shrunk: a TwoViewsTransform of two pipelines; the loader yields (x_q, x_k); per view
    crop, gray sum only with a contrast entry, pointwise, and blur + second pointwise only when a sample blurs."""
    from passl_amd.datasets import build_dataloader
    from passl_amd.datasets.preprocess import DeviceViewPipeline, TwoViewsTransform
    hip_config.set_device('cpu')
    with open(VIEWS_YAML) as f:
        block = yaml.safe_load(f)['DataLoader']['Train']
    block['dataset'].update(num_samples=8, source_h=40, source_w=56)
    block['sampler'] = dict(batch_size=4)
    block['loader'] = dict(host_ring=ring) if ring else {}
    loader, mix = build_dataloader(block, torch.device('cpu'))
    two = loader.batch_transform
    assert isinstance(two, TwoViewsTransform) and mix is None and type(loader).__name__ == \
        ('HostRingLoader' if ring else 'SyntheticLoader')
    v1, v2 = two.base_transform1, two.base_transform2
    assert isinstance(v1, DeviceViewPipeline) and v1.size == v2.size == 224
    assert [type(t).__name__ for t in v1.ops] == ['ColorJitter', 'RandomGrayscale', 'SimCLRGaussianBlur']
    assert [type(t).__name__ for t in v2.ops] == ['ColorJitter', 'RandomGrayscale', 'BYOLSolarize']
    assert (v1.ops[0].p, v1.ops[1].p, v1.ops[2].p, v1.ops[2].sigma, v2.ops[2].p) == (0.8, 0.2, 1.0, [.1, 2.], 0.2)
    assert type(v1.crop).__name__ == 'MAERandCropImage' and v1.crop.scale == [0.08, 1.0] and v1.flip.p == 0.5
    slot = (loader._host if ring else loader._cache)[0]
    assert len(slot) == 1 and slot[0].dtype == torch.uint8 and tuple(slot[0].shape) == (4, 40, 56, 3)
    order = []
    _launches_replaced(monkeypatch, order)
    random.seed(1)
    np.random.seed(1)
    xq, xk = next(iter(loader))
    assert tuple(xq.shape) == tuple(xk.shape) == (4, 3, 224, 224) and two.step == v1.step == v2.step == 1
    assert order == ['crop', 'sum', 'point1', 'blur1', 'point2', 'crop', 'sum', 'point0'], order
    # no contrast entry and no blur anywhere: crop and one pointwise launch
    order.clear()
    v2.ops[0].entries = [e for e in v2.ops[0].entries if e[0] != 2]
    v2(slot[0])
    assert order == ['crop', 'point0']


def _train_blocks():
    for path in sorted(glob.glob(os.path.join(ROOT, 'configs', '**', '*.yaml'), recursive=True)):
        with open(path) as f:
            cfg = yaml.safe_load(f) or {}
        block = (cfg.get('dataloader') or {}).get('train') or (cfg.get('DataLoader') or {}).get('Train')
        if block and 'dataset' in block:
            yield path, block


def test_every_other_yaml_builds_what_it_built_before(monkeypatch):
    """Only the new file names the raw two-view source; every other synthetic config, in either schema, builds a loader
    without a TwoViewsTransform whose batches are the tensors it cached, and launches nothing of this feature."""
    from passl_amd.datasets import build_dataloader
    from passl_amd.datasets.preprocess import TwoViewsTransform
    hip_config.set_device('cpu')
    order = []
    _launches_replaced(monkeypatch, order)
    seen = built = 0
    for path, block in _train_blocks():
        seen += 1
        name = str(block['dataset'].get('name', ''))
        new = os.path.samefile(path, VIEWS_YAML)
        assert (name == 'SyntheticRawTwoView') == new, path
        if new or not name.startswith('Synthetic'):
            continue
        block = copy.deepcopy(block)
        block['dataset'].update(num_samples=4, image_size=16)
        block['sampler'] = dict(block.get('sampler') or {}, batch_size=2)
        block['loader'] = {}
        loader, _mix = build_dataloader(block, torch.device('cpu'))
        built += 1
        assert not isinstance(loader.batch_transform, TwoViewsTransform), path
        if loader.batch_transform is None:
            assert all(a is b for a, b in zip(next(iter(loader)), loader._cache[0])), path
    assert seen >= 12 and built >= 8 and not order
