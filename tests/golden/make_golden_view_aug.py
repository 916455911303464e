"""Generate tests/golden/view_aug_small.npz by EXECUTING THE REFERENCE's own file under the paddle shim:
passl/data/preprocess/basic_transforms.py — TwoViewsTransform, Compose, MAERandCropImage, RandomApply, RandomGrayscale,
SimCLRGaussianBlur, BYOLSolarize, RandomHorizontalFlip, NormalizeImage, ToCHWImage — on PIL images.

    python tests/golden/make_golden_view_aug.py

Stand-ins as in make_golden_crop_resize.py (cv2, paddle.vision.transforms, passl.utils.logger: imported by the file,
unused on this path).  ColorJitter inherits paddle.vision's class, which is not in the reference tree: the stand-in here
draws its list by the RESTATED rule (tests/view_aug_util.py:draw_color_jitter) and applies it with Pillow itself —
ImageEnhance.Brightness / Contrast / Color and convert('HSV') — so the pixel arithmetic is Pillow's, not a restatement.

One case, random.seed(SEED) and np.random.seed(SEED) before it, 8 block-noise images of 40 x 56, S = 32, two consecutive
calls of the reference's TwoViewsTransform image by image:
  view 1  MAERandCropImage(32, [0.2, 1]), ColorJitter(0.7, 0.4, 0.4, 0.2, 0.1), RandomGrayscale(0.3),
          SimCLRGaussianBlur([.1, 2.], 0.6), RandomHorizontalFlip, NormalizeImage(hwc), ToCHWImage
  view 2  MAERandCropImage(32, [0.2, 1]), RandomApply([ColorJitter(1.0, 0.4, 0.4, 0.2, 0.1)], 0.7), RandomGrayscale(0.3),
          BYOLSolarize(0.5), RandomHorizontalFlip, NormalizeImage(hwc), ToCHWImage
Stored per call c in ('', '_second') and view v in (1, 2), everything OBSERVED at the transforms, not restated: box_v
int32 [B, 4], jit_codes_v int32 [B, 4] and jit_vals_v float64 [B, 4] (the list the stand-in drew; codes 0 behind its
end), gray_v / sol_v / flip_v uint8 [B], blur_v float64 [B] (the radius handed to ImageFilter.GaussianBlur; -1: skipped),
stages_v uint8 [5, B, 32, 32, 3] (after crop, jitter, grayscale, blur or solarise, flip), f32_v [B, 3, 32, 32]; of the
second call the decisions and stages_v_second uint8 [B, 32, 32, 3], the images after the flip, only (the size limit).
Nothing is written unless the first call contains every item of check_coverage."""
import importlib.util
import os
import random
import sys

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import crop_resize_util as CU                      # noqa: E402
import view_aug_util as VU                         # noqa: E402
from make_golden_crop_resize import load_reference_transforms      # noqa: E402
from oracle import ref_runner                      # noqa: E402

S, B, HW, SEED = 32, 8, (40, 56), 0
JITTER = dict(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1)


class PilColorJitter(object):
    """The stand-in for ColorJitter: the reference's ``random.random() < p`` (basic_transforms.py:779), the restated
    inner rule, Pillow's own arithmetic."""

    def __init__(self, p):
        self.p = p
        self.entries = VU.jitter_entries(**JITTER)
        self.log = []

    def __call__(self, img):
        ops = VU.draw_color_jitter(self.p, self.entries)
        self.log.append(ops)
        for code, v in ops:
            if code == VU.OP_BRIGHTNESS:
                img = ImageEnhance.Brightness(img).enhance(v)
            elif code == VU.OP_CONTRAST:
                img = ImageEnhance.Contrast(img).enhance(v)
            elif code == VU.OP_SATURATION:
                img = ImageEnhance.Color(img).enhance(v)
            else:
                h, s, val = img.convert('HSV').split()
                np_h = (np.array(h, dtype=np.int32) + v) % 256
                img = Image.merge('HSV', (Image.fromarray(np_h.astype(np.uint8), 'L'), s, val)).convert('RGB')
        return img


class Tap(object):
    """Runs a transform and keeps what came out."""

    def __init__(self, fn):
        self.fn = fn
        self.out = []

    def __call__(self, img):
        img = self.fn(img)
        self.out.append(np.array(img))
        return img


class BlurSpy(object):
    """ImageFilter with a GaussianBlur that notes its radius."""

    def __init__(self, real):
        self.real = real
        self.radii = []

    def GaussianBlur(self, radius):
        self.radii.append(radius)
        return self.real.GaussianBlur(radius=radius)


def build_views(T):
    def tail():
        return [Tap(T.RandomHorizontalFlip()),
                T.NormalizeImage(scale=1.0 / 255.0, mean=list(CU.MEAN), std=list(CU.STD), order='hwc'), T.ToCHWImage()]
    crop = [T.MAERandCropImage(S, scale=[0.2, 1.0], interpolation='bicubic', backend='pil') for _ in range(2)]
    j1, j2 = PilColorJitter(0.7), PilColorJitter(1.0)
    v1 = [Tap(crop[0]), Tap(j1), Tap(T.RandomGrayscale(p=0.3)), Tap(T.SimCLRGaussianBlur(sigma=[.1, 2.], p=0.6))] + tail()
    v2 = [Tap(crop[1]), Tap(T.RandomApply([j2], p=0.7)), Tap(T.RandomGrayscale(p=0.3)), Tap(T.BYOLSolarize(p=0.5))] + tail()
    return T.TwoViewsTransform(T.Compose(v1), T.Compose(v2)), (v1, v2), (j1, j2), crop


def observe_box(T, crop, H, W):
    """The box the crop is about to choose: the crop alone on an image whose pixels encode their position; the
    generators are put back afterwards."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    coded = np.stack([yy, xx, np.zeros_like(yy)], axis=2).astype(np.uint8)
    state = (random.getstate(), np.random.get_state())
    resize, crop._resize_func = crop._resize_func, lambda img, size: img
    piece = np.asarray(crop(Image.fromarray(coded)))
    crop._resize_func = resize
    random.setstate(state[0])
    np.random.set_state(state[1])
    return piece[0, 0, 0], piece[0, 0, 1], piece.shape[0], piece.shape[1]


def run_call(T, src, spy):
    """One pass over the batch, image by image, through the reference's TwoViewsTransform -> {key: array}."""
    two, views, jits, crops = build_views.cache
    n = src.shape[0]
    out = {}
    for v in (1, 2):
        out['box_%d' % v] = np.zeros((n, 4), np.int32)
        out['jit_codes_%d' % v] = np.zeros((n, 4), np.int32)
        out['jit_vals_%d' % v] = np.zeros((n, 4), np.float64)
        for k in ('gray', 'sol', 'flip'):
            out['%s_%d' % (k, v)] = np.zeros(n, np.uint8)
        out['blur_%d' % v] = -np.ones(n, np.float64)
        out['stages_%d' % v] = np.zeros((5, n, S, S, 3), np.uint8)
        out['f32_%d' % v] = np.zeros((n, 3, S, S), np.float32)
    H, W = src.shape[1:3]
    # (view 2's box can only be observed when view 1 has consumed its draws: its crop is hooked for the time of a call)
    for b in range(n):
        for taps in views:
            for t in taps[:5]:
                t.out = []
        for j in jits:
            j.log = []
        spy.radii = []
        out['box_1'][b] = observe_box(T, crops[0], H, W)
        inner2 = views[1][0].fn

        def crop2(img, _b=b, _inner=inner2):
            out['box_2'][_b] = observe_box(T, crops[1], H, W)
            return _inner(img)
        views[1][0].fn = crop2
        im1, im2 = two(Image.fromarray(src[b]))
        views[1][0].fn = inner2
        for v, (taps, j, im) in enumerate(zip(views, jits, (im1, im2)), start=1):
            st = [t.out[0] for t in taps[:5]]
            assert all(a.shape == (S, S, 3) and a.dtype == np.uint8 for a in st)
            out['stages_%d' % v][:, b] = st
            out['f32_%d' % v][b] = im
            ops = j.log[0] if j.log else []
            assert len(j.log) <= 1
            for k, (code, val) in enumerate(ops):
                out['jit_codes_%d' % v][b, k] = code
                out['jit_vals_%d' % v][b, k] = val
            if not ops:
                assert np.array_equal(st[1], st[0])
            out['gray_%d' % v][b] = not np.array_equal(st[2], st[1])     # (no block-noise image is gray already)
            if v == 1:
                assert len(spy.radii) <= 1
                if spy.radii:
                    out['blur_1'][b] = spy.radii[0]
                else:
                    assert np.array_equal(st[3], st[2])
            else:
                out['sol_2'][b] = not np.array_equal(st[3], st[2])
            out['flip_%d' % v][b] = not np.array_equal(st[4], st[3])
            assert np.array_equal(st[4], st[3][:, ::-1] if out['flip_%d' % v][b] else st[3])
            top, left, h, w = out['box_%d' % v][b]
            assert np.array_equal(st[0], np.asarray(Image.fromarray(src[b, top:top + h, left:left + w]).resize(
                (S, S), Image.BICUBIC)))
    assert out['f32_1'].dtype == np.float32
    return out


def check_coverage(o):
    codes = np.concatenate([o['jit_codes_1'], o['jit_codes_2']])
    vals = np.concatenate([o['jit_vals_1'], o['jit_vals_2']])
    n_ops = (codes != 0).sum(axis=1)
    has = {c: (codes == c).any(axis=1) for c in (VU.OP_BRIGHTNESS, VU.OP_CONTRAST, VU.OP_SATURATION, VU.OP_HUE)}
    for c, m in has.items():
        assert m.any() and not m.all(), 'op %d must be applied and skipped' % c
    for k in ('gray_1', 'gray_2', 'sol_2', 'flip_1', 'flip_2'):
        assert 0 < o[k].sum() < len(o[k]), k + ': both values are needed'
    assert (o['blur_1'] < 0).any() and (o['blur_1'] >= 0).any(), 'a blurred and a non-blurred sample are needed'
    pos = [int(np.argmax(codes[i] == VU.OP_CONTRAST)) for i in np.nonzero(has[VU.OP_CONTRAST])[0]]
    last = [int(n_ops[i]) - 1 for i in np.nonzero(has[VU.OP_CONTRAST])[0]]
    assert 0 in pos, 'contrast first'
    assert any(p == l and p > 0 for p, l in zip(pos, last)), 'contrast last'
    assert any(0 < p < l for p, l in zip(pos, last)), 'contrast in the middle'
    stages = np.concatenate([o['stages_1'], o['stages_2']], axis=1)
    big = [i for i in range(len(codes)) if any(c in (VU.OP_BRIGHTNESS, VU.OP_CONTRAST, VU.OP_SATURATION) and v > 1
                                               for c, v in zip(codes[i], vals[i]))]
    assert any((stages[1, i] == 0).sum() > (stages[0, i] == 0).sum() and
               (stages[1, i] == 255).sum() > (stages[0, i] == 255).sum() for i in big), 'a factor > 1 saturating both ends'
    hue = vals[codes == VU.OP_HUE]
    assert (hue >= 128).any() and ((hue > 0) & (hue < 128)).any(), 'a negative and a positive hue shift'
    rs = [VU.box_weights(r)[0] for r in o['blur_1'] if r >= 0]
    assert 0 in rs and 1 in rs, 'box radii 0 and 1'
    none = [(n_ops[:B][i] == 0 and not o['gray_1'][i] and o['blur_1'][i] < 0) for i in range(B)] + \
           [(n_ops[B:][i] == 0 and not o['gray_2'][i] and not o['sol_2'][i]) for i in range(B)]
    assert any(none), 'a sample with no op at all'


def generate(T, seed):
    spy = BlurSpy(T.ImageFilter.real if isinstance(T.ImageFilter, BlurSpy) else T.ImageFilter)
    T.ImageFilter = spy
    build_views.cache = build_views(T)
    src = CU.block_noise(700 + SEED, B, *HW)
    random.seed(seed)
    np.random.seed(seed)
    out = {'src': src}
    for suffix in ('', '_second'):
        for k, v in run_call(T, src, spy).items():
            if suffix and k.startswith('f32_'):
                continue                           # (the second call keeps its decisions and final uint8 images only)
            out[k + suffix] = v[4] if suffix and k.startswith('stages_') else v
    check_coverage(out)
    assert not np.array_equal(out['box_1'], out['box_1_second'])
    return out


def main():
    T = load_reference_transforms()
    out = generate(T, SEED)
    path = os.path.join(HERE, 'view_aug_small.npz')
    np.savez_compressed(path + '.tmp.npz', **out)
    size = os.path.getsize(path + '.tmp.npz')
    if size >= 256 * 1024:
        os.remove(path + '.tmp.npz')
        raise AssertionError('%d bytes: too large' % size)
    os.replace(path + '.tmp.npz', path)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    assert ref_runner.available(), 'needs the reference tree'
    main()
