"""The numpy restatement that DEFINES passl_hip_crop_resize_norm (csrc/crop_resize.hip), and the restated parameter
draws of the reference's crop / flip classes (passl/data/preprocess/basic_transforms.py).  Shared by the CPU and GPU tests
and by tests/golden/make_golden_crop_resize.py; nothing here imports the package.

Result definition: Pillow's 8-bit ``Image.resize((S, S), BICUBIC)`` of the cropped image, flipped left-right when
``flip`` is set, then ``(float32(v) * scale - mean[c]) / std[c]`` in fp32, laid out CHW.

Resampling arithmetic (Pillow, src/libImaging/Resample.c), per axis with ``n_in`` crop pixels and ``n_out`` outputs:
    scale = n_in / n_out;  fs = max(1, scale);  support = 2 fs
    per output i:  center = (i + 0.5) scale
                   lo = max(int(center - support + 0.5), 0);  hi = min(int(center + support + 0.5), n_in)
                   w_k = bicubic((k + lo - center + 0.5) / fs)  for k < hi - lo      (a = -0.5; 1 / fs is formed first)
                   w_k /= sum_k w_k                                                   (summed in k order, in double)
                   K_k = int(w_k 2^22 + 0.5)  if w_k >= 0 else  int(w_k 2^22 - 0.5)  (truncation)
    pass: clip((sum_k K_k p[lo + k] + 2^21) >> 22, 0, 255), the shift arithmetic
Horizontal pass first (to uint8), the vertical pass on those uint8 values.  Taps are clamped to the CROP."""
import math
import random

import numpy as np

PRECISION_BITS = 22
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SCALE = 1.0 / 255.0

# the golden cases: name -> (class, source (H, W), B, S, crop scale, seed)
GOLDEN_CASES = {
    'a': dict(crop='MAERandCropImage', flip='RandomHorizontalFlip', hw=(40, 56), B=8, S=32, scale=[0.2, 1.0], seed=5),
    'b': dict(crop='RandCropImage', flip='RandFlipImage', hw=(64, 48), B=8, S=32, scale=[0.08, 1.0], seed=5),
}
# the boxes of case (a), first call: (top, left, h, w, flip)
CASE_A_TABLE = [(4, 19, 26, 32, 1), (0, 5, 40, 46, 0), (0, 13, 40, 43, 1), (0, 15, 32, 25, 0), (0, 5, 39, 32, 0),
                (7, 11, 31, 30, 1), (1, 7, 39, 41, 0), (1, 17, 32, 29, 1)]
RATIO = (3. / 4., 4. / 3.)


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(n_in, n_out):
    """-> lo int64 [n_out], count int64 [n_out], K int64 [n_out, ksize] (zero past count)."""
    scale = n_in / n_out
    fs = max(1.0, scale)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    lo = np.zeros(n_out, dtype=np.int64)
    cnt = np.zeros(n_out, dtype=np.int64)
    K = np.zeros((n_out, ksize), dtype=np.int64)
    for i in range(n_out):
        center = (i + 0.5) * scale
        a = max(int(center - support + 0.5), 0)
        b = min(int(center + support + 0.5), n_in)
        w = [bicubic((k + a - center + 0.5) * ss) for k in range(b - a)]
        ww = 0.0
        for v in w:
            ww += v
        for k, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            K[i, k] = int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5))
        lo[i], cnt[i] = a, b - a
    return lo, cnt, K


def _resample_axis0(img, n_out):
    """img uint8 [n_in, ...] -> uint8 [n_out, ...] along axis 0."""
    lo, cnt, K = coefficients(img.shape[0], n_out)
    out = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    wide = img.astype(np.int64)
    for i in range(n_out):
        acc = np.tensordot(K[i, :cnt[i]], wide[lo[i]:lo[i] + cnt[i]], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8(img, S):
    """img uint8 [h, w, C] -> uint8 [S, S, C]: the horizontal pass, then the vertical pass on its uint8 result."""
    hor = _resample_axis0(np.ascontiguousarray(img.transpose(1, 0, 2)), S).transpose(1, 0, 2)
    return _resample_axis0(np.ascontiguousarray(hor), S)


def clamp_box(row, Hs, Ws):
    """What the kernel makes of a table row: top / left into the source, then 1 <= h <= Hs - top, 1 <= w <= Ws - left."""
    top, left, h, w = (int(v) for v in row[:4])
    top, left = min(max(top, 0), Hs - 1), min(max(left, 0), Ws - 1)
    return top, left, min(max(h, 1), Hs - top), min(max(w, 1), Ws - left)


def normalise(u8, scale=SCALE, mean=MEAN, std=STD):
    """uint8 [..., 3] -> fp32 [..., 3] as NormalizeImage(order='hwc') computes it."""
    scale = np.float32(scale)
    mean = np.array(mean).reshape(1, 1, 3).astype('float32')
    std = np.array(std).reshape(1, 1, 3).astype('float32')
    return ((u8.astype('float32') * scale - mean) / std).astype('float32')


def crop_resize_norm_ref(src, table, S, scale=SCALE, mean=MEAN, std=STD):
    """src uint8 [B, Hs, Ws, 3], table int [B, >= 5] -> (uint8 [B, S, S, 3] after the flip, fp32 [B, 3, S, S])."""
    B, Hs, Ws, _ = src.shape
    u8 = np.empty((B, S, S, 3), dtype=np.uint8)
    for b in range(B):
        top, left, h, w = clamp_box(table[b], Hs, Ws)
        r = resize_u8(src[b, top:top + h, left:left + w], S)
        u8[b] = r[:, ::-1] if int(table[b][4]) else r
    f = np.stack([normalise(u8[b], scale, mean, std).transpose(2, 0, 1) for b in range(B)])
    return u8, np.ascontiguousarray(f)


# ---------------------------------------------------------------------------------------------- the draws, restated
def draw_mae_rand_crop(Hs, Ws, scale, ratio=RATIO):
    """MAERandCropImage.__call__: np.random.uniform x 2 (area, log aspect), random.randint x 2 (left, top)."""
    area = Ws * Hs * np.random.uniform(*scale)
    aspect = math.exp(np.random.uniform(*tuple(math.log(x) for x in ratio)))
    w = min(int(round(math.sqrt(area * aspect))), Ws)
    h = min(int(round(math.sqrt(area / aspect))), Hs)
    left = random.randint(0, Ws - w)
    top = random.randint(0, Hs - h)
    return top, left, h, w


def draw_rand_crop(Hs, Ws, scale, ratio=RATIO):
    """RandCropImage.__call__: random.uniform x 2 (aspect, area), random.randint x 2 (left, top)."""
    aspect = math.sqrt(random.uniform(*ratio))
    w, h = 1. * aspect, 1. / aspect
    bound = min((float(Ws) / Hs) / (w ** 2), (float(Hs) / Ws) / (h ** 2))
    smax, smin = min(scale[1], bound), min(scale[0], bound)
    size = math.sqrt(Ws * Hs * random.uniform(smin, smax))
    w, h = int(size * w), int(size * h)
    left = random.randint(0, Ws - w)
    top = random.randint(0, Hs - h)
    return top, left, h, w


def draw_table(crop, flip, B, Hs, Ws, scale, p=0.5):
    """int32 [B, 8] = (top, left, h, w, flip, 0, 0, 0), sample by sample: the crop's draws, then the flip's draw
    (RandFlipImage: random.randint(0, 1) == 1; RandomHorizontalFlip: np.random.rand() < p) — from the global generators,
    as a single-worker loader of the reference would consume them."""
    t = np.zeros((B, 8), dtype=np.int32)
    for b in range(B):
        t[b, :4] = (draw_mae_rand_crop if crop == 'MAERandCropImage' else draw_rand_crop)(Hs, Ws, scale)
        t[b, 4] = (random.randint(0, 1) == 1) if flip == 'RandFlipImage' else (np.random.rand() < p)
    return t


def block_noise(seed, B, H, W):
    """uint8 [B, H, W, 3]: uniform random bytes, constant over 2 x 2 blocks (a quarter of the entropy to store; the
    resampled images still take every value and overshoot to 0 and 255 at the block edges)."""
    q = np.random.RandomState(seed).randint(0, 256, size=(B, (H + 1) // 2, (W + 1) // 2, 3)).astype(np.uint8)
    return np.ascontiguousarray(q.repeat(2, axis=1).repeat(2, axis=2)[:, :H, :W])


def golden_sources(name):
    """The uint8 source images of a golden case: a generator of its own, so the global streams stay untouched."""
    if name == 'c':
        return block_noise(303, 1, 96, 96)
    c = GOLDEN_CASES[name]
    return block_noise(100 + c['seed'], c['B'], *c['hw'])
