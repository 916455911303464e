"""The front of the image pipeline on a device-resident uint8 batch — reference passl/data/preprocess/basic_transforms.py:
RandCropImage (:373-419; also passl_v110/datasets/preprocess/transforms.py:322), MAERandCropImage (:635-662),
RandFlipImage (:665-693), RandomHorizontalFlip (:696-704), NormalizeImage (:707-753), ToCHWImage (:756-767), as
tasks/ssl/mae/main_linprobe.py:188-196 composes them.

The reference runs these per sample on the host, through Pillow.  Here a step is one launch of csrc/crop_resize.hip
(``ops.crop_resize_norm``): the per-sample parameters are drawn on the host IN THE REFERENCE'S ORDER AND FROM THE
REFERENCE'S GENERATORS — for the samples in order, the crop's draws and then the flip's draw, as a single-worker loader
would consume the global streams —

    RandCropImage          random.uniform x 2 (aspect, area), random.randint x 2 (left, top)
    MAERandCropImage       np.random.uniform x 2 (area, log aspect), random.randint x 2 (left, top)
    RandFlipImage          random.randint(0, 1)
    RandomHorizontalFlip   np.random.rand()

and travel as a device table int32 [B, 8] = (top, left, h, w, flip, 0, 0, 0).  The kernel crops, resamples (Pillow's
8-bit bicubic, bit for bit), flips, normalises and writes fp32 NCHW; the uint8 batch is never written.

Refused with NotImplementedError, because the kernel computes Pillow's bicubic and nothing else: ``backend='cv2'`` (the
classes' default), every interpolation but 'bicubic' ('random' included), vertical flips, ``channel_num=4``,
``output_fp16``, and the name ``RandomResizedCrop`` (the v110 one is paddle.vision's class, not in the reference tree;
the v2 one draws ``randint(0, height - h + 1)``, so its box can leave the image)."""
import math
import random

import numpy as np
import torch

from ...hip import ops

_RATIO = (3. / 4., 4. / 3.)


def _square(size):
    if isinstance(size, (list, tuple)):
        if len(size) == 1:
            return int(size[0])
        if len(size) != 2 or int(size[0]) != int(size[1]):
            raise NotImplementedError('crop size %r: only square outputs are built' % (size,))
        return int(size[0])
    return int(size)


class RandCropImage(object):
    """The reference's arguments and defaults.  ``rng`` / ``np_rng``: a ``random.Random`` / ``np.random.RandomState``;
    None = the global ``random`` / ``np.random``, which is what the reference uses."""

    def __init__(self, size, scale=None, ratio=None, interpolation=None, backend='cv2', rng=None, np_rng=None):
        name = type(self).__name__
        if str(backend).lower() != 'pil':
            raise NotImplementedError("%s(backend=%r): only backend='pil' is built — the kernel computes Pillow's 8-bit "
                                      "bicubic resampling, cv2's differs in every pixel" % (name, backend))
        if interpolation == 'random' or isinstance(interpolation, (list, tuple)):
            raise NotImplementedError("%s(interpolation=%r): a per-sample choice of filter is not built, only 'bicubic'"
                                      % (name, interpolation))
        if not isinstance(interpolation, str) or interpolation.lower() != 'bicubic':
            raise NotImplementedError("%s(interpolation=%r): only 'bicubic' is built" % (name, interpolation))
        self.size = _square(size)
        self.scale = [0.08, 1.0] if scale is None else list(scale)
        self.ratio = list(_RATIO) if ratio is None else list(ratio)
        self.rng, self.np_rng = rng, np_rng

    def draw(self, Hs, Ws):
        """(top, left, h, w) of one sample; basic_transforms.py:398-415."""
        rnd = random if self.rng is None else self.rng
        aspect_ratio = math.sqrt(rnd.uniform(*self.ratio))
        w = 1. * aspect_ratio
        h = 1. / aspect_ratio
        bound = min((float(Ws) / Hs) / (w ** 2), (float(Hs) / Ws) / (h ** 2))
        scale_max = min(self.scale[1], bound)
        scale_min = min(self.scale[0], bound)
        target_size = math.sqrt(Ws * Hs * rnd.uniform(scale_min, scale_max))
        w = int(target_size * w)
        h = int(target_size * h)
        left = rnd.randint(0, Ws - w)
        top = rnd.randint(0, Hs - h)
        return top, left, h, w


class MAERandCropImage(RandCropImage):
    def draw(self, Hs, Ws):
        """basic_transforms.py:648-659: no rejection loop; the box is cut to the image."""
        rnd = random if self.rng is None else self.rng
        nrnd = np.random if self.np_rng is None else self.np_rng
        target_area = Ws * Hs * nrnd.uniform(*self.scale)
        log_ratio = tuple(math.log(x) for x in self.ratio)
        aspect_ratio = math.exp(nrnd.uniform(*log_ratio))
        w = min(int(round(math.sqrt(target_area * aspect_ratio))), Ws)
        h = min(int(round(math.sqrt(target_area / aspect_ratio))), Hs)
        left = rnd.randint(0, Ws - w)
        top = rnd.randint(0, Hs - h)
        return top, left, h, w


class RandFlipImage(object):
    def __init__(self, flip_code=1, rng=None):
        assert flip_code in [-1, 0, 1], 'flip_code should be a value in [-1, 0, 1]'
        if flip_code != 1:
            raise NotImplementedError('RandFlipImage(flip_code=%r): only the horizontal flip (flip_code=1) is built'
                                      % (flip_code,))
        self.flip_code = flip_code
        self.rng = rng

    def draw(self):
        return (random if self.rng is None else self.rng).randint(0, 1) == 1


class RandomHorizontalFlip(object):
    def __init__(self, p=0.5, np_rng=None):
        self.p = p
        self.np_rng = np_rng

    def draw(self):
        return bool((np.random if self.np_rng is None else self.np_rng).rand() < self.p)


class NormalizeImage(object):
    """(float32(v) * scale - mean[c]) / std[c]; ``order`` says on which side of ToCHWImage the entry stands and does not
    change a value."""

    def __init__(self, scale=None, mean=None, std=None, order='chw', output_fp16=False, channel_num=3):
        if isinstance(scale, str):
            scale = eval(scale)                              # the reference's configs write '1.0/255.0'
        assert channel_num in [3, 4], 'channel number of input image should be set to 3 or 4.'
        if channel_num != 3:
            raise NotImplementedError('NormalizeImage(channel_num=4): the zero-padded fourth channel is not built')
        if output_fp16:
            raise NotImplementedError('NormalizeImage(output_fp16=True): the kernel writes fp32')
        if order not in ('chw', 'hwc'):
            raise ValueError("NormalizeImage(order=%r): 'chw' or 'hwc'" % (order,))
        self.scale = float(np.float32(scale if scale is not None else 1.0 / 255.0))
        self.order = order
        self.mean = [float(v) for v in (mean if mean is not None else [0.485, 0.456, 0.406])]
        self.std = [float(v) for v in (std if std is not None else [0.229, 0.224, 0.225])]
        if len(self.mean) != 3 or len(self.std) != 3 or any(np.float32(v) == 0 for v in self.std):
            raise ValueError('NormalizeImage: three means and three non-zero stds expected')


class ToCHWImage(object):
    pass


class DeviceCropPipeline(object):
    """crop -> (flip) -> normalise + HWC -> CHW of a resident uint8 batch [B, Hs, Ws, 3], one launch, out of place.
    ``step`` counts the calls."""

    def __init__(self, crop, flip, normalize):
        assert isinstance(crop, RandCropImage) and isinstance(normalize, NormalizeImage)
        assert flip is None or isinstance(flip, (RandFlipImage, RandomHorizontalFlip))
        self.crop, self.flip, self.normalize = crop, flip, normalize
        self.size = crop.size
        self.step = 0

    def draw(self, B, Hs, Ws):
        """The table of one step, np.int32 [B, 8] = (top, left, h, w, flip, 0, 0, 0): sample by sample, the crop's draws
        and then the flip's; drawn on the host without touching a device."""
        table = np.zeros((B, 8), dtype=np.int32)
        for b in range(B):
            table[b, :4] = self.crop.draw(Hs, Ws)
            if self.flip is not None:
                table[b, 4] = self.flip.draw()
        return table

    @staticmethod
    def validate(table, Hs, Ws):
        """ValueError unless every row of the int32 [B, 8] table is a non-empty box inside an Hs x Ws image, a flip of
        0 or 1 and three zeros."""
        t = np.asarray(table)
        if t.ndim != 2 or t.shape[1] != 8 or t.dtype != np.int32:
            raise ValueError('crop table: int32 [B, 8] expected, got %s %s' % (t.dtype, t.shape))
        t = t.astype(np.int64)
        bad = (t[:, :2] < 0).any(axis=1) | (t[:, 2:4] < 1).any(axis=1) | (t[:, 0] + t[:, 2] > Hs) | \
            (t[:, 1] + t[:, 3] > Ws) | (t[:, 4] < 0) | (t[:, 4] > 1) | (t[:, 5:] != 0).any(axis=1)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError('crop table: row %d = %s is no box of the %d x %d image' % (i, t[i].tolist(), Hs, Ws))

    def __call__(self, x):
        """x uint8 [B, Hs, Ws, 3] on the device -> fp32 [B, 3, size, size] (a new tensor).  One launch; the table goes
        through pinned memory with a non-blocking copy, so the host never waits for the stream."""
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise ValueError('DeviceCropPipeline: a uint8 [B, H, W, 3] batch expected, got %s %s'
                             % (x.dtype, tuple(x.shape)))
        B, Hs, Ws, _ = x.shape
        table = self.draw(B, Hs, Ws)
        self.validate(table, Hs, Ws)
        x = x.contiguous()
        host = torch.empty((B, 8), dtype=torch.int32, pin_memory=x.is_cuda)
        host.numpy()[...] = table
        dev = host.to(x.device, non_blocking=True)
        n = self.normalize
        out = ops.crop_resize_norm(x, dev, self.size, n.mean, n.std, n.scale)
        self.step += 1
        return out


class ChainedBatchTransform(object):
    """The loader's ``batch_transform`` when more than one stage runs on the resident batch: the stages in order, each
    out of place (crop -> RandomErasing: the reference's per-sample order)."""

    def __init__(self, stages):
        self.stages = list(stages)

    def __call__(self, x):
        for fn in self.stages:
            x = fn(x)
        return x


_CLASSES = {c.__name__: c for c in (RandCropImage, MAERandCropImage, RandFlipImage, RandomHorizontalFlip,
                                    NormalizeImage, ToCHWImage)}


def build_crop_pipeline(transforms_cfg):
    """The ``transforms`` list of a raw (uint8) source -> DeviceCropPipeline.  Every entry is honoured or refused: the
    list must read crop, optional flip, NormalizeImage and ToCHWImage (in the order NormalizeImage's ``order`` says),
    optionally followed by ``RandomErasing`` (built by build_random_erasing, not here)."""
    entries = [dict(t) for t in (transforms_cfg or [])]
    names = [e.get('name') for e in entries]
    if 'RandomResizedCrop' in names:
        raise NotImplementedError(
            "RandomResizedCrop is not built: the v110 configs' class is paddle.vision's, which is not part of the "
            "reference tree, and the v2 class draws randint(0, height - h + 1), so its box can leave the image; write "
            'RandCropImage or MAERandCropImage')
    if names and names[-1] == 'RandomErasing':
        entries, names = entries[:-1], names[:-1]
    unknown = [n for n in names if n not in _CLASSES]
    if unknown:
        raise NotImplementedError('transforms %r of a raw source are not built (built: %s, then RandomErasing)'
                                  % (unknown, ', '.join(_CLASSES)))
    built = [_CLASSES[e.pop('name')](**e) for e in entries]
    kinds = ['crop' if isinstance(t, RandCropImage) else 'flip' if isinstance(t, (RandFlipImage, RandomHorizontalFlip))
             else 'norm' if isinstance(t, NormalizeImage) else 'chw' for t in built]
    norm = next((t for t in built if isinstance(t, NormalizeImage)), None)
    tail = ['norm', 'chw'] if norm is None or norm.order == 'hwc' else ['chw', 'norm']
    if kinds not in (['crop'] + tail, ['crop', 'flip'] + tail):
        raise ValueError('transforms of a raw source must read: crop, optional flip, then NormalizeImage and ToCHWImage '
                         "(NormalizeImage first with order='hwc', last with order='chw'); got %r" % (names,))
    return DeviceCropPipeline(built[0], built[1] if kinds[1] == 'flip' else None, norm)
