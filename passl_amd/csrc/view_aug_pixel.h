// Per-pixel arithmetic of the colour stage (csrc/view_aug.hip): Pillow's 8-bit Image.blend, convert('L'), RGB <-> HSV
// (Convert.c) and ImageOps.solarize, restated in tests/view_aug_util.py.  __host__ __device__ and free of HIP headers, so a
// plain C++ program can run every function over all 2^24 colours without a GPU (tests/test_view_aug_host.py).
// Every translation unit that includes this compiles it without contraction: the blend's product and sum round to fp32
// one after the other.
#pragma once
#include <math.h>
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

#pragma clang fp contract(off)

namespace view_aug {

enum Op : int32_t {
  kOpNone = 0, kOpBrightness = 1, kOpContrast = 2, kOpSaturation = 3, kOpHue = 4, kOpGray = 5, kOpSolarize = 6,
  kOpCount = 7
};
constexpr int kMaxOps = 8;          // operations per sample
constexpr int kRow = 24;            // int32 per table row
// a table row: [0] n ops, [1] flip, [2] blur r (< 0: no blur), [3] ww, [4] fw, [5] split: ops [0, split) run before
// the blur and [split, n) after it, [6] index of the contrast entry (< 0: none), [7] 0, [8..16) op codes,
// [16..24) values: the fp32 factor's bits, or the hue shift

struct Rgb { int r, g, b; };

__host__ __device__ inline int gray_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__host__ __device__ inline int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// a / b rounded to nearest in fp32, on either side
__host__ __device__ inline float fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

__host__ __device__ inline int blend1(int deg, int v, float a, bool inside) {
  const float prod = a * (float)(v - deg);
  const float t = (float)deg + prod;
  if (inside) return (int)t & 255;                          // 0 <= t <= 255 there
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return clip255((int)t);
}

__host__ __device__ inline Rgb blend3(int dr, int dg, int db, Rgb p, float a) {
  const bool inside = a >= 0.0f && a <= 1.0f;
  return Rgb{blend1(dr, p.r, a, inside), blend1(dg, p.g, a, inside), blend1(db, p.b, a, inside)};
}

// (r, g, b) -> (H, S, V)
__host__ __device__ inline Rgb rgb2hsv(Rgb p) {
  const int mx = p.r > p.g ? (p.r > p.b ? p.r : p.b) : (p.g > p.b ? p.g : p.b);
  const int mn = p.r < p.g ? (p.r < p.b ? p.r : p.b) : (p.g < p.b ? p.g : p.b);
  if (mx == mn) return Rgb{0, 0, mx};
  const float cr = (float)(mx - mn);
  const float s = fdiv(cr, (float)mx);
  const float rc = fdiv((float)(mx - p.r), cr), gc = fdiv((float)(mx - p.g), cr), bc = fdiv((float)(mx - p.b), cr);
  float h;
  if (p.r == mx) h = bc - gc;
  else if (p.g == mx) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  double hd = (double)h / 6.0 + 1.0;                        // in [5/6, 11/6]
  if (hd >= 1.0) hd = hd - 1.0;                             // = fmod(hd, 1.0), exact
  h = (float)hd;
  return Rgb{clip255((int)((double)h * 255.0)), clip255((int)((double)s * 255.0)), mx};
}

__host__ __device__ inline int round_away(float x) { return (int)floor((double)x + 0.5); }   // x >= 0 here

// (H, S, V) -> (r, g, b)
__host__ __device__ inline Rgb hsv2rgb(Rgb q) {
  const int H = q.r, S = q.g, V = q.b;
  if (S == 0) return Rgb{V, V, V};
  const float h = (float)((double)H * 6.0 / 255.0);
  const double fs = (double)(float)((double)S / 255.0);
  const float fl = floorf(h);
  const double f = (double)(h - fl);
  const double v = (double)V;
  const int p = clip255(round_away((float)(v * (1.0 - fs))));
  const int qq = clip255(round_away((float)(v * (1.0 - fs * f))));
  const int t = clip255(round_away((float)(v * (1.0 - fs * (1.0 - f)))));
  switch ((int)fl % 6) {
    case 0: return Rgb{V, t, p};
    case 1: return Rgb{qq, V, p};
    case 2: return Rgb{p, V, t};
    case 3: return Rgb{p, qq, V};
    case 4: return Rgb{t, p, V};
    default: return Rgb{V, p, qq};
  }
}

__host__ __device__ inline float bits_to_float(int32_t v) {
  union { int32_t i; float f; } u;
  u.i = v;
  return u.f;
}

// one operation on one pixel; ``m``: the contrast entry's mean.  An unknown code leaves the pixel as it is.
__host__ __device__ inline Rgb apply_op(Rgb p, int32_t code, int32_t value, int m) {
  switch (code) {
    case kOpBrightness: return blend3(0, 0, 0, p, bits_to_float(value));
    case kOpContrast: return blend3(m, m, m, p, bits_to_float(value));
    case kOpSaturation: {
      const int g = gray_of(p.r, p.g, p.b);
      return blend3(g, g, g, p, bits_to_float(value));
    }
    case kOpHue: {
      Rgb hsv = rgb2hsv(p);
      hsv.r = (hsv.r + (value & 255)) & 255;
      return hsv2rgb(hsv);
    }
    case kOpGray: {
      const int g = gray_of(p.r, p.g, p.b);
      return Rgb{g, g, g};
    }
    case kOpSolarize: return Rgb{p.r < 128 ? p.r : 255 - p.r, p.g < 128 ? p.g : 255 - p.g, p.b < 128 ? p.b : 255 - p.b};
    default: return p;
  }
}

}  // namespace view_aug
