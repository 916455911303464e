"""The numpy restatement that DEFINES the colour stage of the two-view pipeline (csrc/view_aug.hip, csrc/view_aug_pixel.h)
and the restated draws of the reference's classes (passl/data/preprocess/basic_transforms.py: ColorJitter, RandomGrayscale,
SimCLRGaussianBlur, BYOLSolarize, RandomApply, TwoViewsTransform).  Shared by the CPU and GPU tests and by
tests/golden/make_golden_view_aug.py; nothing here imports the package.

All of it is Pillow's 8-bit arithmetic on a uint8 [H, W, 3] image:
  blend(deg, img, f)   Image.blend as ImageEnhance uses it: a = float32(f); t = float32(deg) + a * float32(img - deg), the
                       product and the sum each rounded to fp32; inside 0 <= f <= 1 (uint8)(int)t, outside 0 for t <= 0,
                       255 for t >= 255, truncation in between
  gray                 (19595 R + 38470 G + 7471 B + 0x8000) >> 16                                        (convert('L'))
  brightness(f)        blend(0, img, f)
  saturation(f)        blend(gray, img, f)
  contrast(f)          blend(m, img, f), m = int(mean(gray) + 0.5) = (2 sum + N) // (2 N) over the CURRENT image
  hue(shift)           RGB -> HSV (Convert.c), H = (H + shift) mod 256, HSV -> RGB
  grayscale            R = G = B = gray
  solarise             v < 128 ? v : 255 - v
  gaussian_blur(rad)   three box blurs per axis (BoxBlur.c), box radius and weights in fp32 / uint32
An operation list is a list of (code, value): OP_* below; the value is the factor, the hue shift (an int in [0, 256)) or,
for OP_BLUR, the radius."""
import math
import random

import numpy as np

OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_GRAY, OP_SOLARIZE, OP_BLUR = range(8)
f32 = np.float32


# ---------------------------------------------------------------------------------------------- point-wise arithmetic
def gray(img):
    """uint8 [..., 3] -> uint8 [...]."""
    w = img.astype(np.int64)
    return ((19595 * w[..., 0] + 38470 * w[..., 1] + 7471 * w[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """deg, img uint8 (broadcastable) -> uint8."""
    a = f32(f)
    d = deg.astype(np.int32)
    diff = (img.astype(np.int32) - d).astype(np.float32)
    t = d.astype(np.float32) + (a * diff).astype(np.float32)             # two fp32 roundings, no fma
    t = t.astype(np.float32)
    if 0.0 <= float(a) <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    return out.astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(gray(img)[..., None], img, f)


def contrast_mean(img):
    g = gray(img).astype(np.int64)
    return int((2 * int(g.sum()) + g.size) // (2 * g.size))


def contrast(img, f, m=None):
    m = contrast_mean(img) if m is None else m
    return blend(np.full_like(img, m), img, f)


def rgb2hsv(img):
    """uint8 [..., 3] -> uint8 [..., 3] as Pillow's convert('HSV')."""
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    mx = np.maximum(np.maximum(r, g), b)
    mn = np.minimum(np.minimum(r, g), b)
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(np.float32)
    s = cr / np.where(flat, 1, mx).astype(np.float32)                    # fp32
    rc = (mx - r).astype(np.float32) / cr
    gc = (mx - g).astype(np.float32) / cr
    bc = (mx - b).astype(np.float32) / cr
    h_r = (bc - gc).astype(np.float32)
    h_g = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32)
    h_b = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H = np.where(flat, 0, H)
    S = np.where(flat, 0, S)
    return np.stack([H, S, mx], axis=-1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), -np.floor(-x + 0.5))


def hsv2rgb(hsv):
    """uint8 [..., 3] -> uint8 [..., 3] as Pillow's HSV -> RGB conversion."""
    H, S, V = (hsv[..., i].astype(np.int32) for i in range(3))
    h = (H.astype(np.float64) * 6.0 / 255.0).astype(np.float32)
    fs = (S.astype(np.float64) / 255.0).astype(np.float32)
    i = np.floor(h)
    f = (h - i).astype(np.float32).astype(np.float64)
    fs = fs.astype(np.float64)
    v = V.astype(np.float64)
    p = _round_away((v * (1.0 - fs)).astype(np.float32).astype(np.float64)).astype(np.int32)
    q = _round_away((v * (1.0 - fs * f)).astype(np.float32).astype(np.float64)).astype(np.int32)
    t = _round_away((v * (1.0 - fs * (1.0 - f))).astype(np.float32).astype(np.float64)).astype(np.int32)
    p, q, t = (np.clip(x, 0, 255) for x in (p, q, t))
    k = i.astype(np.int32) % 6
    R = np.choose(k, [V, q, p, p, t, V])
    G = np.choose(k, [t, V, V, q, p, p])
    B = np.choose(k, [p, p, t, V, V, q])
    grey = S == 0
    out = np.stack([np.where(grey, V, R), np.where(grey, V, G), np.where(grey, V, B)], axis=-1)
    return out.astype(np.uint8)


def hue(img, shift):
    hsv = rgb2hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) % 256).astype(np.uint8)
    return hsv2rgb(hsv)


def grayscale(img):
    g = gray(img)
    return np.stack([g, g, g], axis=-1)


def solarize(img):
    return np.where(img < 128, img, 255 - img).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- Gaussian blur
def box_radius(radius):
    """ImageFilter.GaussianBlur's box radius for three passes, in fp32."""
    r = f32(radius)
    s2 = f32(f32(r * r) / f32(3))
    L = f32(np.sqrt(f32(f32(f32(12) * s2) + f32(1))))
    l = f32(np.floor(f32(f32(L - f32(1)) / f32(2))))
    num = f32(f32(f32(f32(2) * l) + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    den = f32(f32(6) * f32(s2 - f32(f32(l + f32(1)) * f32(l + f32(1)))))
    return f32(l + f32(num / den))


def box_weights(radius):
    """-> (r, ww, fw) of one box pass; (0, 0, 0) with a box radius of exactly 0 (Pillow skips the blur)."""
    fr = box_radius(radius)
    r = int(fr)
    ww = int(f32(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _box_pass_axis1(img, r, ww, fw):
    """img uint8 [H, W, C]: one pass along axis 1, every index clamped to the line."""
    W = img.shape[1]
    wide = img.astype(np.int64)
    x = np.arange(W)
    acc = np.zeros_like(wide)
    for k in range(-r, r + 1):
        acc += wide[:, np.clip(x + k, 0, W - 1)]
    far = wide[:, np.clip(x - r - 1, 0, W - 1)] + wide[:, np.clip(x + r + 1, 0, W - 1)]
    return ((ww * acc + fw * far + (1 << 23)) >> 24).astype(np.uint8)


def box_blur(img, r, ww, fw):
    for _ in range(3):
        img = _box_pass_axis1(img, r, ww, fw)
    img = np.ascontiguousarray(img.transpose(1, 0, 2))
    for _ in range(3):
        img = _box_pass_axis1(img, r, ww, fw)
    return np.ascontiguousarray(img.transpose(1, 0, 2))


def gaussian_blur(img, radius):
    return box_blur(img, *box_weights(radius))


# ---------------------------------------------------------------------------------------------- operation lists
def apply_ops(img, ops, stages=None):
    """img uint8 [H, W, 3]; ops: [(code, value)] applied in order.  ``stages``: a list that receives the image after each
    operation."""
    for code, v in ops:
        if code == OP_BRIGHTNESS:
            img = brightness(img, v)
        elif code == OP_CONTRAST:
            img = contrast(img, v)
        elif code == OP_SATURATION:
            img = saturation(img, v)
        elif code == OP_HUE:
            img = hue(img, v)
        elif code == OP_GRAY:
            img = grayscale(img)
        elif code == OP_SOLARIZE:
            img = solarize(img)
        elif code == OP_BLUR:
            img = gaussian_blur(img, v)
        elif code != OP_NONE:
            raise ValueError('op code %r' % (code,))
        if stages is not None:
            stages.append(img)
    return img


def view_ref(u8, ops, flip, scale, mean, std):
    """One sample: resized uint8 [S, S, 3] -> (uint8 [S, S, 3] after the ops and the flip, fp32 [3, S, S])."""
    out = apply_ops(u8, ops)
    if flip:
        out = out[:, ::-1]
    out = np.ascontiguousarray(out)
    m = np.array(mean).reshape(1, 1, 3).astype('float32')
    s = np.array(std).reshape(1, 1, 3).astype('float32')
    f = ((out.astype('float32') * np.float32(scale) - m) / s).astype('float32')
    return out, np.ascontiguousarray(f.transpose(2, 0, 1))


# ---------------------------------------------------------------------------------------------- the draws, restated
def hue_shift(f):
    """paddle.vision's adjust_hue on a PIL image: np.uint8(f * 255) added to H with wrap-around."""
    return int(math.trunc(f * 255)) % 256


def jitter_entries(brightness=0, contrast=0, saturation=0, hue=0):
    """ASSUMPTION (the class's base, paddle.vision.transforms.ColorJitter, is not in the reference tree): the entries
    present, in the order brightness, contrast, saturation, hue: a value v gives [max(0, 1 - v), 1 + v], hue [-v, v];
    an entry whose range collapses to its centre is absent."""
    out = []
    for code, v in ((OP_BRIGHTNESS, brightness), (OP_CONTRAST, contrast), (OP_SATURATION, saturation)):
        lo, hi = max(0.0, 1.0 - v), 1.0 + v
        if not lo == hi == 1.0:
            out.append((code, lo, hi))
    if hue != 0:
        out.append((OP_HUE, -hue, hue))
    return out


def draw_color_jitter(p, entries):
    """ColorJitter.__call__: random.random() < p, then random.shuffle of the entries, a random.uniform each."""
    if not random.random() < p:
        return []
    order = list(entries)
    random.shuffle(order)
    ops = []
    for code, lo, hi in order:
        f = random.uniform(lo, hi)
        ops.append((code, hue_shift(f) if code == OP_HUE else f))
    return ops


# ---------------------------------------------------------------------------------------------- the golden file
def golden_samples(z, view, suffix=''):
    """tests/golden/view_aug_small.npz -> [(box, ops, flip)] of one view of one call, from the OBSERVED decisions: the
    jitter's list, then grayscale, then the blur (view 1) or the solarisation (view 2)."""
    v = '_%d%s' % (view, suffix)
    out = []
    for b in range(len(z['box' + v])):
        ops = [(int(c), int(x) if c == OP_HUE else float(x))
               for c, x in zip(z['jit_codes' + v][b], z['jit_vals' + v][b]) if c != OP_NONE]
        if z['gray' + v][b]:
            ops.append((OP_GRAY, 0))
        if z['blur' + v][b] >= 0:
            ops.append((OP_BLUR, float(z['blur' + v][b])))
        if z['sol' + v][b]:
            ops.append((OP_SOLARIZE, 0))
        out.append((tuple(int(t) for t in z['box' + v][b]), ops, bool(z['flip' + v][b])))
    return out


def all_colours():
    """uint8 [4096, 4096, 3]: every colour once."""
    n = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(n >> 16) & 255, (n >> 8) & 255, n & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def contrast_mean_sum(img, ops):
    """What passl_hip_view_gray_sum writes for a sample: the sum of gray over the image after the operations in front of
    its contrast entry; 0 without one."""
    codes = [c for c, _v in ops if c != OP_BLUR]
    if OP_CONTRAST not in codes:
        return 0
    k = [c for c, _v in ops].index(OP_CONTRAST)
    return int(gray(apply_ops(img, ops[:k])).astype(np.int64).sum())
