"""Generate tests/golden/crop_resize_small.npz by EXECUTING THE REFERENCE's own file under the paddle shim:
passl/data/preprocess/basic_transforms.py — RandCropImage, MAERandCropImage, RandFlipImage, RandomHorizontalFlip,
NormalizeImage, ToCHWImage — on PIL images (Pillow does the resampling).

    python tests/golden/make_golden_crop_resize.py

The file imports cv2 (not installed), three names of paddle.vision.transforms and passl.utils.logger at its top and uses
none of them on this path: empty stand-in modules are put into sys.modules here, for the time of this script.

Cases (tests/crop_resize_util.py:GOLDEN_CASES), random.seed(5) and np.random.seed(5) before each:
  a  MAERandCropImage(32, scale=[0.2, 1], 'bicubic', 'pil') + RandomHorizontalFlip + NormalizeImage(order='hwc') +
     ToCHWImage on 8 uint8 images of 40 x 56; a SECOND consecutive call on the same images too (the streams continue)
  b  RandCropImage(32, scale=[0.08, 1], 'bicubic', 'pil') + RandFlipImage + the same tail on 8 images of 64 x 48
  c  one 96 x 96 image cropped whole, to 32 (a 3 x down-scale, 13 taps)
Stored per case: src uint8 [B, H, W, 3], table int32 [B, 8] = (top, left, h, w, flip, 0, 0, 0) as the classes chose them
(observed at the crop and the flip, not restated), u8 uint8 [B, 32, 32, 3] (resized, flipped), f32 [B, 3, 32, 32].
Nothing is written when a random case lacks an up-scaled axis, a down-scaled axis, a box touching a border, either flip
value or a box with h != w, or when no output pixel of it saturates at 0 and at 255."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import crop_resize_util as CU                      # noqa: E402
from oracle import paddle_shim, ref_runner         # noqa: E402

S = 32


class _Anything(types.ModuleType):
    """A stand-in module: every attribute exists and is a class of no content."""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (object,), {})


def load_reference_transforms():
    paddle_shim.install()
    for name in ('cv2', 'paddle.vision.transforms', 'passl', 'passl.utils', 'passl.utils.logger'):
        if name not in sys.modules:
            sys.modules[name] = _Anything(name)
    sys.modules['passl.utils'].logger = sys.modules['passl.utils.logger']
    path = os.path.join(ref_runner.REF_ROOT, 'passl', 'data', 'preprocess', 'basic_transforms.py')
    spec = importlib.util.spec_from_file_location('_ref_basic_transforms', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(T, crop, flip, src):
    """One call of the composed pipeline, sample by sample -> (table, u8, f32).  The box is observed by running the crop
    on an image whose pixels encode their own position (the same draws: the generators are restored in between); the
    flip by comparing the flip's output with its input."""
    norm = T.NormalizeImage(scale=1.0 / 255.0, mean=list(CU.MEAN), std=list(CU.STD), order='hwc')
    chw = T.ToCHWImage()
    B, H, W, _ = src.shape
    table = np.zeros((B, 8), dtype=np.int32)
    u8 = np.zeros((B, S, S, 3), dtype=np.uint8)
    f32 = np.zeros((B, 3, S, S), dtype=np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    coded = np.stack([yy, xx, np.zeros_like(yy)], axis=2).astype(np.uint8)       # H, W < 256
    for b in range(B):
        state = (random.getstate(), np.random.get_state())
        resize, crop._resize_func = crop._resize_func, lambda img, size: img      # the crop alone, on the coded image
        piece = np.asarray(crop(Image.fromarray(coded) if isinstance(crop, T.MAERandCropImage) else coded))
        crop._resize_func = resize
        random.setstate(state[0])
        np.random.set_state(state[1])
        table[b, :4] = (piece[0, 0, 0], piece[0, 0, 1], piece.shape[0], piece.shape[1])
        # the real thing (MAERandCropImage crops PIL images, RandCropImage slices arrays: basic_transforms.py:417, :661)
        img = crop(Image.fromarray(src[b]) if isinstance(crop, T.MAERandCropImage) else src[b])
        assert isinstance(img, Image.Image) and img.size == (S, S)
        resized = np.asarray(img)
        top, left, h, w = table[b, :4]
        assert np.array_equal(resized, np.asarray(Image.fromarray(src[b, top:top + h, left:left + w]).resize(
            (S, S), Image.BICUBIC)))
        if flip is not None:
            img = flip(img)
            flipped = np.asarray(img)
            table[b, 4] = 0 if np.array_equal(flipped, resized) else 1
            assert np.array_equal(flipped, resized[:, ::-1] if table[b, 4] else resized)
        u8[b] = np.asarray(img)
        f32[b] = chw(norm(img))
    assert f32.dtype == np.float32
    return table, u8, f32


def check_coverage(name, table, u8, H, W):
    t = table
    up = (t[:, 2] < S) | (t[:, 3] < S)
    down = (t[:, 2] > S) | (t[:, 3] > S)
    border = (t[:, 0] == 0) | (t[:, 1] == 0) | (t[:, 0] + t[:, 2] == H) | (t[:, 1] + t[:, 3] == W)
    print('case %s: up-scaled %d, down-scaled %d, an axis equal %d, border %d, flipped %d, h != w %d, pixels at 0 / 255: '
          '%d / %d' % (name, up.sum(), down.sum(), ((t[:, 2] == S) | (t[:, 3] == S)).sum(), border.sum(), t[:, 4].sum(),
                       (t[:, 2] != t[:, 3]).sum(), (u8 == 0).sum(), (u8 == 255).sum()))
    assert up.any() and down.any(), 'an up-scaled and a down-scaled sample are needed'
    assert border.any(), 'no box touches a border'
    assert 0 < t[:, 4].sum() < len(t), 'both flip values are needed'
    assert (t[:, 2] != t[:, 3]).any(), 'no box with h != w'
    assert (u8 == 0).any() and (u8 == 255).any(), 'no output pixel saturates'


def main():
    T = load_reference_transforms()
    out = {}
    for name, c in sorted(CU.GOLDEN_CASES.items()):
        H, W = c['hw']
        src = CU.golden_sources(name)
        random.seed(c['seed'])
        np.random.seed(c['seed'])
        crop = getattr(T, c['crop'])(S, scale=c['scale'], interpolation='bicubic', backend='pil')
        flip = getattr(T, c['flip'])()
        calls = ['', '_second'] if name == 'a' else ['']
        for suffix in calls:
            table, u8, f32 = run_case(T, crop, flip, src)
            check_coverage(name + suffix, table, u8, H, W)
            out['table_%s%s' % (name, suffix)] = table
            out['u8_%s%s' % (name, suffix)] = u8
            out['f32_%s%s' % (name, suffix)] = f32
        out['src_' + name] = src
        if name == 'a':
            assert [tuple(r) for r in out['table_a'][:, :5].tolist()] == CU.CASE_A_TABLE, out['table_a']
            assert not np.array_equal(out['table_a'], out['table_a_second'])
    # (c): the whole 96 x 96 image to 32 through the same classes: a scale of [1, 1] and a ratio of [1, 1] give the full box
    src = CU.golden_sources('c')
    random.seed(5)
    np.random.seed(5)
    crop = T.MAERandCropImage(S, scale=[1.0, 1.0], ratio=[1.0, 1.0], interpolation='bicubic', backend='pil')
    table, u8, f32 = run_case(T, crop, None, src)
    assert table[0].tolist() == [0, 0, 96, 96, 0, 0, 0, 0]
    out.update(src_c=src, table_c=table, u8_c=u8, f32_c=f32)
    path = os.path.join(HERE, 'crop_resize_small.npz')
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
