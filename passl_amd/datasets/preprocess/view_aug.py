"""The colour stage of the contrastive recipes on a device-resident uint8 batch, and the two views of one image —
reference passl/data/preprocess/basic_transforms.py: TwoViewsTransform (:88-98), ColorJitter (:770-787), RandomApply
(:859-869), RandomGrayscale (:872-906), SimCLRGaussianBlur (:909-926), BYOLSolarize (:929-944), as ``base_transform1/2``
of tasks/ssl/mocov3/configs/mocov3_vit_base_patch16_224_pt_in1k_4n32c_dp_fp16o1.yaml compose them; also
passl_v110/datasets/preprocess/transforms.py: GaussianBlur(_PIL=True) (:175-186).

The reference runs these per sample on the host, through Pillow.  Here the decisions are drawn on the host IN THE
REFERENCE'S ORDER AND FROM THE REFERENCE'S GENERATORS — per sample the whole of view 1 (crop, colour entries, flip), then
the whole of view 2, as a single-worker loader would consume the global streams —

    RandomApply(p)                 np.random.rand(); skipped when p < x
    ColorJitter(p, ...)            random.random() < p, then the inner rule below
    RandomGrayscale(p)             np.random.rand() < p
    SimCLRGaussianBlur(sigma, p)   random.random() < p, then random.uniform(sigma[0], sigma[1])
    GaussianBlur(sigma, _PIL=True) np.random.uniform(sigma[0], sigma[1])
    BYOLSolarize(p)                random.random() < p

and travel as device tables: the crop's int32 [B, 8] (crop.py; its flip column stays 0 here) and the operations' int32
[B, 24] (include/passl_hip.h).  The kernels of csrc/view_aug.hip compute Pillow's 8-bit arithmetic bit for bit.

ColorJitter's inner rule is a RESTATED ASSUMPTION: the class inherits paddle.vision.transforms.ColorJitter, which is not
part of the reference tree.  The entries present, in the order brightness, contrast, saturation, hue — a value v gives
the range [max(0, 1 - v), 1 + v], hue [-v, v], an entry whose range collapses to its centre is absent — are shuffled by
``random.shuffle``; each then draws ``random.uniform(lo, hi)``; the hue shift is int(trunc(f * 255)) mod 256.

Refused with NotImplementedError: the v110 ``GaussianBlur(_PIL=False)`` (cv2), ``RandomResizedCrop`` (crop.py says why),
``ToTensor`` / ``Normalize`` (paddle's: they divide by 255 where NormalizeImage multiplies by fp32(1/255), so the floats
differ), any other name, more than one blur or more than one contrast entry per view, and a contrast entry behind a
blur (its mean would have to be taken over the blurred image)."""
import math
import random

import numpy as np
import torch

from ...hip import ops
from .crop import (MAERandCropImage, NormalizeImage, RandCropImage, RandFlipImage, RandomHorizontalFlip, ToCHWImage)

OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_GRAY, OP_SOLARIZE = range(7)
OP_BLUR = 7                       # host side only: it becomes the row's (r, ww, fw, split), never an op code
MAX_OPS = 8
ROW = ops.VIEW_ROW
_f32 = np.float32


def box_weights(radius):
    """ImageFilter.GaussianBlur(radius) -> (r, ww, fw) of its box passes, in fp32 / integers as Pillow computes them."""
    rad = _f32(radius)
    s2 = _f32(_f32(rad * rad) / _f32(3))
    L = _f32(np.sqrt(_f32(_f32(_f32(12) * s2) + _f32(1))))
    l = _f32(np.floor(_f32(_f32(L - _f32(1)) / _f32(2))))
    num = _f32(_f32(_f32(_f32(2) * l) + _f32(1)) * _f32(_f32(l * _f32(l + _f32(1))) - _f32(_f32(3) * s2)))
    den = _f32(_f32(6) * _f32(s2 - _f32(_f32(l + _f32(1)) * _f32(l + _f32(1)))))
    fr = _f32(l + _f32(num / den))
    r = int(fr)
    ww = int(_f32(_f32(1 << 24) / _f32(_f32(fr * _f32(2)) + _f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def _range(value, name, center, lo_bound, hi_bound, clip_zero):
    if isinstance(value, (list, tuple)):
        if len(value) != 2 or not lo_bound <= value[0] <= value[1] <= hi_bound:
            raise ValueError('ColorJitter(%s=%r): two values inside [%s, %s] expected' % (name, value, lo_bound, hi_bound))
        rng = [float(value[0]), float(value[1])]
    else:
        if value < 0:
            raise ValueError('ColorJitter(%s=%r): a non-negative value expected' % (name, value))
        rng = [center - value, center + value]
        if clip_zero:
            rng[0] = max(rng[0], 0)
        if not lo_bound <= rng[0] <= rng[1] <= hi_bound:
            raise ValueError('ColorJitter(%s=%r): outside [%s, %s]' % (name, value, lo_bound, hi_bound))
    return None if rng[0] == rng[1] == center else rng


class ColorJitter(object):
    """The reference's arguments and defaults (p first, then paddle.vision's brightness, contrast, saturation, hue).
    ``rng``: a ``random.Random``; None = the global ``random``, which is what the reference uses."""

    def __init__(self, p=1.0, brightness=0, contrast=0, saturation=0, hue=0, rng=None):
        self.p = p
        self.entries = []
        for code, name, v in ((OP_BRIGHTNESS, 'brightness', brightness), (OP_CONTRAST, 'contrast', contrast),
                              (OP_SATURATION, 'saturation', saturation)):
            r = _range(v, name, 1, 0, float('inf'), True)
            if r is not None:
                self.entries.append((code, r[0], r[1]))
        r = _range(hue, 'hue', 0, -0.5, 0.5, False)
        if r is not None:
            self.entries.append((OP_HUE, r[0], r[1]))
        self.rng = rng

    def draw(self):
        rnd = random if self.rng is None else self.rng
        if not rnd.random() < self.p:
            return []
        order = list(self.entries)
        rnd.shuffle(order)
        out = []
        for code, lo, hi in order:
            f = rnd.uniform(lo, hi)
            out.append((code, int(math.trunc(f * 255)) % 256 if code == OP_HUE else f))
        return out


class RandomGrayscale(object):
    def __init__(self, p=0.1, np_rng=None):
        self.p = p
        self.np_rng = np_rng

    def draw(self):
        return [(OP_GRAY, 0)] if (np.random if self.np_rng is None else self.np_rng).rand() < self.p else []


class SimCLRGaussianBlur(object):
    def __init__(self, sigma=[.1, 2.], p=1.0, rng=None):
        self.p = p
        self.sigma = sigma
        self.rng = rng

    def draw(self):
        rnd = random if self.rng is None else self.rng
        if rnd.random() < self.p:
            return [(OP_BLUR, rnd.uniform(self.sigma[0], self.sigma[1]))]
        return []


class GaussianBlur(object):
    """passl_v110's class: always applied (a RandomApply decides around it), the radius from ``np.random.uniform``."""

    def __init__(self, sigma=[.1, 2.], _PIL=False, np_rng=None):
        if not _PIL:
            raise NotImplementedError('GaussianBlur(_PIL=False) blurs through cv2.GaussianBlur with a 23 x 23 kernel, which '
                                      "is not built: only Pillow's ImageFilter.GaussianBlur is (_PIL=True, or "
                                      'SimCLRGaussianBlur)')
        self.sigma = sigma
        self.np_rng = np_rng

    def draw(self):
        return [(OP_BLUR, (np.random if self.np_rng is None else self.np_rng).uniform(self.sigma[0], self.sigma[1]))]


class BYOLSolarize(object):
    def __init__(self, p=1.0, rng=None):
        self.p = p
        self.rng = rng

    def draw(self):
        return [(OP_SOLARIZE, 0)] if (random if self.rng is None else self.rng).random() < self.p else []


class RandomApply(object):
    """``transforms``: built colour entries, or their config entries (build_view_pipeline builds those)."""

    def __init__(self, transforms, p=0.5, np_rng=None):
        self.transforms = list(transforms)
        self.p = p
        self.np_rng = np_rng

    def draw(self):
        if self.p < (np.random if self.np_rng is None else self.np_rng).rand():
            return []
        out = []
        for t in self.transforms:
            out += t.draw()
        return out


_COLOUR = (ColorJitter, RandomGrayscale, SimCLRGaussianBlur, GaussianBlur, BYOLSolarize, RandomApply)


def _may_emit(t, code):
    if isinstance(t, RandomApply):
        return sum(_may_emit(u, code) for u in t.transforms)
    if isinstance(t, ColorJitter):
        return int(any(e[0] == code for e in t.entries))
    if isinstance(t, (SimCLRGaussianBlur, GaussianBlur)):
        return int(code == OP_BLUR)
    return 0


class DeviceViewPipeline(object):
    """One view: crop -> colour entries -> (flip) -> normalise + HWC -> CHW of a resident uint8 batch [B, Hs, Ws, 3], out
    of place.  Launches: crop_resize_u8; view_gray_sum when some sample has a contrast entry; view_pointwise; and, only
    when some sample of the batch blurs, gaussian_blur_u8 and a second view_pointwise.  ``step`` counts the calls."""

    def __init__(self, crop, ops, flip, normalize):
        assert isinstance(crop, RandCropImage) and isinstance(normalize, NormalizeImage)
        assert flip is None or isinstance(flip, (RandFlipImage, RandomHorizontalFlip))
        assert all(isinstance(t, _COLOUR) for t in ops)
        if sum(_may_emit(t, OP_BLUR) for t in ops) > 1 or sum(_may_emit(t, OP_CONTRAST) for t in ops) > 1:
            raise NotImplementedError('a view with more than one blur or more than one contrast entry is not built')
        seen_blur = False
        for t in ops:
            if seen_blur and _may_emit(t, OP_CONTRAST):
                raise NotImplementedError('a contrast entry behind a blur is not built: its mean would be taken over the '
                                          'blurred image')
            seen_blur = seen_blur or bool(_may_emit(t, OP_BLUR))
        self.crop, self.ops, self.flip, self.normalize = crop, list(ops), flip, normalize
        self.size = crop.size
        self.step = 0

    def draw_sample(self, Hs, Ws):
        """((top, left, h, w), [(code, value)], flip) of one sample of this view: the crop's draws, the colour entries'
        in order, the flip's."""
        box = self.crop.draw(Hs, Ws)
        ops_ = []
        for t in self.ops:
            ops_ += t.draw()
        return box, ops_, bool(self.flip.draw()) if self.flip is not None else False

    @staticmethod
    def encode(samples):
        """[(box, ops, flip)] -> (crop table int32 [B, 8], operation table int32 [B, 24])."""
        B = len(samples)
        crop = np.zeros((B, 8), dtype=np.int32)
        table = np.zeros((B, ROW), dtype=np.int32)
        for b, (box, ops_, flip) in enumerate(samples):
            crop[b, :4] = box
            codes = [(c, v) for c, v in ops_ if c != OP_BLUR]
            blurs = [i for i, (c, _v) in enumerate(ops_) if c == OP_BLUR]
            if len(blurs) > 1 or len(codes) > MAX_OPS:
                raise ValueError('sample %d: %d blurs and %d operations do not fit a row (1, %d)'
                                 % (b, len(blurs), len(codes), MAX_OPS))
            table[b, 0], table[b, 1], table[b, 2], table[b, 5], table[b, 6] = len(codes), int(flip), -1, len(codes), -1
            if blurs:
                table[b, 2:5] = box_weights(ops_[blurs[0]][1])
                table[b, 5] = blurs[0]                       # the operations in front of the blur
            for k, (c, v) in enumerate(codes):
                table[b, 8 + k] = c
                if c == OP_HUE:
                    table[b, 16 + k] = int(v)
                elif c in (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION):
                    table[b, 16 + k] = np.array([v], dtype=np.float32).view(np.int32)[0]
                if c == OP_CONTRAST:
                    table[b, 6] = k
        return crop, table

    @staticmethod
    def validate(table):
        """ValueError unless every row of the int32 [B, 24] table is well formed: 0 <= n <= 8, a flip of 0 or 1, known op
        codes and zeros behind them, finite factors, hue shifts in [0, 256), 0 <= split <= n, r within the built envelope
        with the weights of a box pass (or r = -1, split = n and no weights), and the index of the one contrast entry, in
        front of split."""
        t = np.asarray(table)
        if t.ndim != 2 or t.shape[1] != ROW or t.dtype != np.int32:
            raise ValueError('operation table: int32 [B, %d] expected, got %s %s' % (ROW, t.dtype, t.shape))
        for b in range(t.shape[0]):
            row = t[b].astype(np.int64)
            n, flip, r, ww, fw, split, ci = (int(v) for v in row[:7])
            codes, values = row[8:16], t[b, 16:24]
            ok = 0 <= n <= MAX_OPS and flip in (0, 1) and 0 <= split <= n and row[7] == 0
            ok = ok and all(OP_BRIGHTNESS <= c <= OP_SOLARIZE for c in codes[:max(n, 0)]) and not codes[max(n, 0):].any()
            if ok:
                where = [k for k in range(n) if codes[k] == OP_CONTRAST]
                ok = (ci == -1 and not where) or (where == [ci] and ci < split)
                for k in range(n):
                    if codes[k] in (OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION):
                        ok = ok and bool(np.isfinite(values[k:k + 1].view(np.float32)[0]))
                    elif codes[k] == OP_HUE:
                        ok = ok and 0 <= values[k] < 256
            if ok and r == -1:
                ok = split == n and ww == 0 and fw == 0
            elif ok:
                ok = 0 <= r <= ops.BLUR_R_MAX and ww > 0 and fw >= 0 and 0 <= (1 << 24) - (2 * r + 1) * ww - 2 * fw <= 1
            if not ok:
                raise ValueError('operation table: row %d = %s is not well formed (or its blur radius is outside the '
                                 'built envelope, r <= %d)' % (b, t[b].tolist(), ops.BLUR_R_MAX))

    def __call__(self, x, samples=None):
        """x uint8 [B, Hs, Ws, 3] on the device -> fp32 [B, 3, size, size] (a new tensor).  ``samples``: what draw_sample
        returned for every sample (TwoViewsTransform draws both views sample by sample); None: drawn here.  Both tables
        go through pinned memory in one non-blocking copy, so the host never waits for the stream."""
        from .crop import DeviceCropPipeline
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError('DeviceViewPipeline: a uint8 [B, H, W, 3] batch expected, got %s %s'
                             % (x.dtype, tuple(x.shape)))
        B, Hs, Ws, _ = x.shape
        if samples is None:
            samples = [self.draw_sample(Hs, Ws) for _ in range(B)]
        crop_t, table = self.encode(samples)
        DeviceCropPipeline.validate(crop_t, Hs, Ws)
        self.validate(table)
        x = x.contiguous()
        host = torch.empty((B * (8 + ROW),), dtype=torch.int32, pin_memory=x.is_cuda)
        host.numpy()[:B * 8] = crop_t.reshape(-1)
        host.numpy()[B * 8:] = table.reshape(-1)
        dev = host.to(x.device, non_blocking=True)
        n = self.normalize
        out = run_view(x, dev[:B * 8].view(B, 8), dev[B * 8:].view(B, ROW), self.size, (n.mean, n.std, n.scale),
                       contrast=bool((table[:, 6] >= 0).any()), r_max=int(table[:, 2].max()) if B else -1)
        self.step += 1
        return out


def run_view(x, crop_t, table, size, normalize, contrast, r_max):
    """The launches of one view.  ``contrast``: some sample has a contrast entry; ``r_max``: the largest blur r of the
    table (< 0: no sample blurs) — both known on the host, which drew the table."""
    u8 = ops.crop_resize_u8(x, crop_t, size)
    sums = ops.view_gray_sum(u8, table) if contrast else None
    if r_max < 0:
        return ops.view_pointwise(u8, table, sums, 0, normalize)
    u8 = ops.view_pointwise(u8, table, sums, 1, None)
    u8 = ops.gaussian_blur_u8(u8, table, r_max)
    return ops.view_pointwise(u8, table, None, 2, normalize)


class TwoViewsTransform(object):
    """Two views of ONE resident batch: per sample the whole of view 1 is drawn, then the whole of view 2 (the reference
    calls base_transform1(x), then base_transform2(x), image by image).  The loader's ``batch_transform`` of a
    SyntheticRawTwoView source: x uint8 [B, Hs, Ws, 3] -> (x_q, x_k), fp32 [B, 3, S, S] each."""

    def __init__(self, base_transform1, base_transform2):
        assert isinstance(base_transform1, DeviceViewPipeline) and isinstance(base_transform2, DeviceViewPipeline)
        self.base_transform1, self.base_transform2 = base_transform1, base_transform2
        self.step = 0

    def draw(self, B, Hs, Ws):
        s1, s2 = [], []
        for _ in range(B):
            s1.append(self.base_transform1.draw_sample(Hs, Ws))
            s2.append(self.base_transform2.draw_sample(Hs, Ws))
        return s1, s2

    def __call__(self, x):
        s1, s2 = self.draw(x.shape[0], x.shape[1], x.shape[2])
        out = (self.base_transform1(x, s1), self.base_transform2(x, s2))
        self.step += 1
        return out


_CLASSES = {c.__name__: c for c in (RandCropImage, MAERandCropImage, RandFlipImage, RandomHorizontalFlip, NormalizeImage,
                                    ToCHWImage) + _COLOUR}
_REFUSED = {
    'RandomResizedCrop': "the v110 configs' class is paddle.vision's, which is not part of the reference tree, and the v2 "
                         'class draws randint(0, height - h + 1), so its box can leave the image; write RandCropImage or '
                         'MAERandCropImage',
    'ToTensor': "paddle's ToTensor divides by 255 where NormalizeImage multiplies by fp32(1/255): write NormalizeImage "
                'and ToCHWImage',
    'Normalize': "paddle's Normalize follows ToTensor's division by 255, which rounds differently from NormalizeImage: "
                 'write NormalizeImage and ToCHWImage',
}


def _entries(cfg):
    """A transform list in either schema -> [(name, kwargs)]: v2 ``- Name: {kwargs}`` / ``- Name:``, v110
    ``- {name: Name, **kwargs}``."""
    out = []
    for e in (cfg or []):
        e = dict(e)
        if 'name' in e:
            out.append((e.pop('name'), e))
        elif len(e) == 1:
            (name, kw), = e.items()
            out.append((name, dict(kw or {})))
        else:
            raise ValueError('transform entry %r: one {Name: arguments} or {name: Name, ...} expected' % (e,))
    return out


def _build(name, kw):
    if name in _REFUSED:
        raise NotImplementedError('%s is not built: %s' % (name, _REFUSED[name]))
    if name not in _CLASSES:
        raise NotImplementedError('transform %r of a raw two-view source is not built (built: %s)'
                                  % (name, ', '.join(_CLASSES)))
    if name == 'RandomApply':
        inner = [_build(n, k) for n, k in _entries(kw.pop('transforms', None))]
        if not all(isinstance(t, _COLOUR) for t in inner):
            raise NotImplementedError('RandomApply: only colour entries can stand inside it')
        return RandomApply(inner, **kw)
    return _CLASSES[name](**kw)


def build_view_pipeline(transform_cfg):
    """One ``base_transform`` list -> DeviceViewPipeline.  Every entry is honoured or refused: the list must read crop,
    colour entries, optional flip, then NormalizeImage and ToCHWImage (in the order NormalizeImage's ``order`` says)."""
    entries = _entries(transform_cfg)
    built = [_build(n, k) for n, k in entries]
    kinds = ['crop' if isinstance(t, RandCropImage) else 'flip' if isinstance(t, (RandFlipImage, RandomHorizontalFlip))
             else 'norm' if isinstance(t, NormalizeImage) else 'chw' if isinstance(t, ToCHWImage) else 'colour'
             for t in built]
    norm = next((t for t in built if isinstance(t, NormalizeImage)), None)
    tail = ['norm', 'chw'] if norm is None or norm.order == 'hwc' else ['chw', 'norm']
    shape = [k for k in kinds if k != 'colour']
    colour = [i for i, k in enumerate(kinds) if k == 'colour']
    contiguous = not colour or colour == list(range(1, 1 + len(colour)))
    if shape not in (['crop'] + tail, ['crop', 'flip'] + tail) or not contiguous:
        raise ValueError('a view must read: crop, colour entries, optional flip, then NormalizeImage and ToCHWImage '
                         "(NormalizeImage first with order='hwc', last with order='chw'); got %r" % ([n for n, _ in entries],))
    flip = next((t for t in built if isinstance(t, (RandFlipImage, RandomHorizontalFlip))), None)
    return DeviceViewPipeline(built[0], [built[i] for i in colour], flip, norm)


def build_two_views(transform_cfg):
    """The ``transform`` block of a SyntheticRawTwoView source, ``[{TwoViewsTransform: {base_transform1: [...],
    base_transform2: [...]}}]`` -> TwoViewsTransform."""
    entries = _entries(transform_cfg)
    if len(entries) != 1 or entries[0][0] != 'TwoViewsTransform' or \
            sorted(entries[0][1]) != ['base_transform1', 'base_transform2']:
        raise ValueError('the transform of a raw two-view source must be one TwoViewsTransform with base_transform1 and '
                         'base_transform2; got %r' % ([n for n, _ in entries],))
    kw = entries[0][1]
    return TwoViewsTransform(build_view_pipeline(kw['base_transform1']), build_view_pipeline(kw['base_transform2']))
