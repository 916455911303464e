// Random resized crop (bicubic), horizontal flip, NormalizeImage and HWC -> CHW of a device-resident uint8 batch, in
// one launch.
//
// Reference: the transform classes of passl/data/preprocess/basic_transforms.py that tasks/ssl/mae/main_linprobe.py
// :188-196 composes — RandCropImage / MAERandCropImage (:373-419, :635-662: crop, then `_pil_resize`), RandFlipImage /
// RandomHorizontalFlip (:665-704), NormalizeImage (:707-753), ToCHWImage (:756-767) — which run on the host, sample by
// sample, through Pillow.  Here the parameters are drawn on the host (passl_amd/datasets/preprocess/crop.py) and travel
// as a device table int32 [B][8] = (top, left, h, w, flip, 0, 0, 0); src uint8 [B][Hs][Ws][3] is never written; out is
// fp32 [B][3][S][S].
//
// RESULT: Pillow's 8-bit Image.resize((S, S), BICUBIC) of the crop src[b, top:top+h, left:left+w], flipped left-right
// when flip != 0, then lut[c][v] = (float(v) * scale - mean[c]) / std[c], every operation rounded to fp32 on its own
// (no fused multiply-add), as numpy computes NormalizeImage.__call__.
//
//   per axis, n_in crop pixels -> n_out = S outputs, all in IEEE double, no contraction (Pillow's Resample.c):
//     scale = n_in / n_out;  fs = max(1, scale);  support = 2 fs;  ss = 1 / fs
//     output i:  center = (i + 0.5) scale
//                lo = max((int)(center - support + 0.5), 0);  hi = min((int)(center + support + 0.5), n_in)
//                w_k = bicubic(((k + lo) - center + 0.5) ss), k < hi - lo, a = -0.5:
//                      |x| < 1: ((a + 2) x - (a + 3)) x x + 1;  |x| < 2: (((x - 5) x + 8) x - 4) a;  else 0
//                w_k /= (w_0 + w_1 + ...)                          summed in k order
//                K_k = (int)(w_k 2^22 + 0.5) for w_k >= 0, (int)(w_k 2^22 - 0.5) otherwise        (truncation)
//     a pass:    clip((2^21 + sum_k K_k p[lo + k]) >> 22, 0, 255) in 32-bit integers, the shift arithmetic
//   The horizontal pass runs first and rounds to uint8; the vertical pass runs on those uint8 values.  Taps are clamped
//   to the CROP, never to the source image: the reference crops first and resizes afterwards.
//
// One workgroup per (sample, band of kBand output rows).  Prologue: the S horizontal and the band's vertical coefficient
// rows in fp64 into LDS (add / mul / div only, so the integers equal the host's), the 3 x 256 normalisation table.
// Horizontal pass: the source rows the band's taps reach, resampled to uint8 [row][channel][S] in LDS.  Vertical pass and
// epilogue from LDS: a lane owns 4 consecutive outputs of one channel plane's row (one 16-byte store; single floats
// when S % 4 != 0 or out is not 16-byte aligned).  No atomics; stores are vector stores.
//
// ENVELOPE: 3 channels; one band's LDS image must fit 64 KiB:
//     4 S (KH + 2) + 4 kBand (KV + 2) + 3072 + 3 S NR <= 65536,   r = max(1, Hs / S), rw = max(1, Ws / S),
//     KH = 2 ceil(2 rw) + 1, KV = 2 ceil(2 r) + 1, NR = ceil((kBand - 1) r) + 2 ceil(2 r) + 3
// i.e. the SOURCE over the output (a crop is never larger) up to 3.0 at S = 256, 3.4 at S = 224, 1.8 at S = 384;
// PASSL_EUNSUPPORTED beyond.  The library cannot read the table on the host: the kernel clamps every box to the source
// (top, left into it, then 1 <= h <= Hs - top, 1 <= w <= Ws - left), and every LDS index to its carve, so no access
// leaves a tensor whatever the table holds.  Nothing here assumes that the crop is the whole resampled source: an
// output window (Resize + CenterCrop) would add an offset to `i` in axis_coeffs.
//
// passl_hip_crop_resize_u8 is the same crop and resample ending in the uint8 HWC image (crop_resize_u8_kernel): the input
// of the colour stage of view_aug.hip.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kBand = 16;
constexpr int kPrec = 22;
constexpr int kLdsMax = 65536;

struct CropGeom {
  int Hs, Ws, S, KH, KV, NR, bands;
  float mean[3], stdv[3], scale;
};

__host__ __device__ inline double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// the coefficient row of output i: K[0 .. cnt), taps lo .. lo + cnt of the n_in crop pixels; cnt <= cap (the carve)
__host__ __device__ inline void axis_coeffs(int n_in, int n_out, int i, int cap, int32_t* K, int32_t& lo, int32_t& cnt) {
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)i + 0.5) * scale;
  int a = (int)(center - support + 0.5);
  if (a < 0) a = 0;
  int e = (int)(center + support + 0.5);
  if (e > n_in) e = n_in;
  int n = e - a;
  if (n > cap) n = cap;
  double ww = 0.0;
  for (int k = 0; k < n; ++k) ww += bicubic(((double)(k + a) - center + 0.5) * ss);
  for (int k = 0; k < n; ++k) {
    double w = bicubic(((double)(k + a) - center + 0.5) * ss);
    if (ww != 0.0) w = w / ww;
    K[k] = w < 0.0 ? (int32_t)(-0.5 + w * (double)(1 << kPrec)) : (int32_t)(0.5 + w * (double)(1 << kPrec));
  }
  lo = a;
  cnt = n;
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kPrec, 0), 255); }

struct Carve {                     // byte offsets into the dynamic LDS, each a multiple of 16
  int hk, hlo, hcnt, vk, vlo, vcnt, lut, rows, total;
};

__host__ __device__ inline int up16(int v) { return (v + 15) & ~15; }

__host__ __device__ inline Carve carve(const CropGeom& g) {
  Carve c;
  c.hk = 0;
  c.hlo = c.hk + up16(4 * g.S * g.KH);
  c.hcnt = c.hlo + up16(4 * g.S);
  c.vk = c.hcnt + up16(4 * g.S);
  c.vlo = c.vk + up16(4 * kBand * g.KV);
  c.vcnt = c.vlo + up16(4 * kBand);
  c.lut = c.vcnt + up16(4 * kBand);
  c.rows = c.lut + 4 * 768;
  c.total = c.rows + up16(3 * g.S * g.NR);
  return c;
}

template <int VEC>
__global__ void __launch_bounds__(kThreads) crop_resize_norm_kernel(const uint8_t* __restrict__ src, float* __restrict__ out,
                                                                    const int32_t* __restrict__ table, CropGeom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Carve cv = carve(g);
  int32_t* hk = reinterpret_cast<int32_t*>(smem + cv.hk);
  int32_t* hlo = reinterpret_cast<int32_t*>(smem + cv.hlo);
  int32_t* hcnt = reinterpret_cast<int32_t*>(smem + cv.hcnt);
  int32_t* vk = reinterpret_cast<int32_t*>(smem + cv.vk);
  int32_t* vlo = reinterpret_cast<int32_t*>(smem + cv.vlo);
  int32_t* vcnt = reinterpret_cast<int32_t*>(smem + cv.vcnt);
  float* lut = reinterpret_cast<float*>(smem + cv.lut);
  uint8_t* rows = reinterpret_cast<uint8_t*>(smem + cv.rows);

  const int tid = threadIdx.x;
  const int S = g.S;
  const int b = blockIdx.x / g.bands;                        // uniform over the workgroup
  const int y0 = (blockIdx.x - b * g.bands) * kBand;
  const int ny = min(kBand, S - y0);
  // the box, clamped to the source: 0 <= top < Hs, 1 <= h <= Hs - top, likewise left / w, whatever the table holds
  const int32_t* t = table + (int64_t)b * 8;
  const int top = min(max(t[0], 0), g.Hs - 1), left = min(max(t[1], 0), g.Ws - 1);
  const int h = min(max(t[2], 1), g.Hs - top), w = min(max(t[3], 1), g.Ws - left);
  const bool flip = t[4] != 0;

  for (int i = tid; i < S; i += kThreads) axis_coeffs(w, S, i, g.KH, hk + i * g.KH, hlo[i], hcnt[i]);
  if (tid >= kThreads - kBand) {                             // (the last lanes: the first ones carry a second column at S > 240)
    const int i = tid - (kThreads - kBand);
    if (i < ny) axis_coeffs(h, S, y0 + i, g.KV, vk + i * g.KV, vlo[i], vcnt[i]);
  }
  for (int i = tid; i < 768; i += kThreads) {
    const int c = i >> 8;
    lut[i] = __fdiv_rn(__fsub_rn(__fmul_rn((float)(i & 255), g.scale), g.mean[c]), g.stdv[c]);
  }
  __syncthreads();

  // the crop rows [row_lo, row_lo + nr) feed this band (lo and lo + cnt do not decrease with the output row)
  const int row_lo = vlo[0];
  const int nr = min(vlo[ny - 1] + vcnt[ny - 1] - row_lo, g.NR);
  const uint8_t* crop = src + (((int64_t)b * g.Hs + top + row_lo) * g.Ws + left) * 3;
  const int per_row = 3 * S;
  for (int i = tid; i < nr * per_row; i += kThreads) {
    const int r = i / per_row;
    const int rem = i - r * per_row;
    const int x = rem / 3, c = rem - x * 3;
    const uint8_t* p = crop + ((int64_t)r * g.Ws + hlo[x]) * 3 + c;
    const int32_t* K = hk + x * g.KH;
    const int n = hcnt[x];
    int acc = 1 << (kPrec - 1);
    for (int k = 0; k < n; ++k) acc += K[k] * (int)p[3 * k];
    rows[(r * 3 + c) * S + x] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  const int xv = S / VEC;                                    // lanes per output row
  float* plane = out + (int64_t)b * 3 * S * S;
  for (int i = tid; i < 3 * ny * xv; i += kThreads) {
    const int c = i / (ny * xv);
    const int rem = i - c * (ny * xv);
    const int y = rem / xv, x = (rem - y * xv) * VEC;
    const int32_t* K = vk + y * g.KV;
    const int n = vcnt[y];
    const int base = vlo[y] - row_lo;
    const float* l = lut + c * 256;
    float* q = plane + ((int64_t)c * S + y0 + y) * S + x;
    if constexpr (VEC == 4) {
      const int xs = flip ? S - 4 - x : x;                   // a multiple of 4: S % 4 == 0
      int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int k = 0; k < n; ++k) {
        const int r = max(min(base + k, nr - 1), 0);
        const uint32_t v = *reinterpret_cast<const uint32_t*>(rows + (r * 3 + c) * S + xs);
        const int kk = K[k];
        a0 += kk * (int)(v & 255u);
        a1 += kk * (int)((v >> 8) & 255u);
        a2 += kk * (int)((v >> 16) & 255u);
        a3 += kk * (int)(v >> 24);
      }
      const f32x4 o = flip ? f32x4{l[clip8(a3)], l[clip8(a2)], l[clip8(a1)], l[clip8(a0)]}
                           : f32x4{l[clip8(a0)], l[clip8(a1)], l[clip8(a2)], l[clip8(a3)]};
      *reinterpret_cast<f32x4*>(q) = o;
    } else {
      const int xs = flip ? S - 1 - x : x;
      int acc = 1 << (kPrec - 1);
      for (int k = 0; k < n; ++k) acc += K[k] * (int)rows[(max(min(base + k, nr - 1), 0) * 3 + c) * S + xs];
      *q = l[clip8(acc)];
    }
  }
}

// The same band, ending in the resized uint8 HWC image (flipped when the table says so) instead of flip + normalise +
// fp32 NCHW: coefficients, carve, clamps and both passes as above, no normalisation table.  (A body shared by both
// kernels through an inlined template changed the register allocation of crop_resize_norm_kernel, so the band loop is
// written twice and axis_coeffs / carve / clip8 / crop_geom are what the two share.)
__global__ void __launch_bounds__(kThreads) crop_resize_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out,
                                                                  const int32_t* __restrict__ table, CropGeom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Carve cv = carve(g);
  int32_t* hk = reinterpret_cast<int32_t*>(smem + cv.hk);
  int32_t* hlo = reinterpret_cast<int32_t*>(smem + cv.hlo);
  int32_t* hcnt = reinterpret_cast<int32_t*>(smem + cv.hcnt);
  int32_t* vk = reinterpret_cast<int32_t*>(smem + cv.vk);
  int32_t* vlo = reinterpret_cast<int32_t*>(smem + cv.vlo);
  int32_t* vcnt = reinterpret_cast<int32_t*>(smem + cv.vcnt);
  uint8_t* rows = reinterpret_cast<uint8_t*>(smem + cv.rows);

  const int tid = threadIdx.x;
  const int S = g.S;
  const int b = blockIdx.x / g.bands;                        // uniform over the workgroup
  const int y0 = (blockIdx.x - b * g.bands) * kBand;
  const int ny = min(kBand, S - y0);
  // the box, clamped to the source: 0 <= top < Hs, 1 <= h <= Hs - top, likewise left / w, whatever the table holds
  const int32_t* t = table + (int64_t)b * 8;
  const int top = min(max(t[0], 0), g.Hs - 1), left = min(max(t[1], 0), g.Ws - 1);
  const int h = min(max(t[2], 1), g.Hs - top), w = min(max(t[3], 1), g.Ws - left);
  const bool flip = t[4] != 0;

  for (int i = tid; i < S; i += kThreads) axis_coeffs(w, S, i, g.KH, hk + i * g.KH, hlo[i], hcnt[i]);
  if (tid >= kThreads - kBand) {                             // (the last lanes: the first ones carry a second column at S > 240)
    const int i = tid - (kThreads - kBand);
    if (i < ny) axis_coeffs(h, S, y0 + i, g.KV, vk + i * g.KV, vlo[i], vcnt[i]);
  }
  __syncthreads();

  // the crop rows [row_lo, row_lo + nr) feed this band (lo and lo + cnt do not decrease with the output row)
  const int row_lo = vlo[0];
  const int nr = min(vlo[ny - 1] + vcnt[ny - 1] - row_lo, g.NR);
  const uint8_t* crop = src + (((int64_t)b * g.Hs + top + row_lo) * g.Ws + left) * 3;
  const int per_row = 3 * S;
  for (int i = tid; i < nr * per_row; i += kThreads) {
    const int r = i / per_row;
    const int rem = i - r * per_row;
    const int x = rem / 3, c = rem - x * 3;
    const uint8_t* p = crop + ((int64_t)r * g.Ws + hlo[x]) * 3 + c;
    const int32_t* K = hk + x * g.KH;
    const int n = hcnt[x];
    int acc = 1 << (kPrec - 1);
    for (int k = 0; k < n; ++k) acc += K[k] * (int)p[3 * k];
    rows[(r * 3 + c) * S + x] = (uint8_t)clip8(acc);
  }
  __syncthreads();

  uint8_t* image = out + ((int64_t)b * S + y0) * S * 3;
  for (int i = tid; i < ny * per_row; i += kThreads) {
    const int y = i / per_row;
    const int rem = i - y * per_row;
    const int x = rem / 3, c = rem - x * 3;
    const int32_t* K = vk + y * g.KV;
    const int n = vcnt[y];
    const int base = vlo[y] - row_lo;
    const int xs = flip ? S - 1 - x : x;
    int acc = 1 << (kPrec - 1);
    for (int k = 0; k < n; ++k) acc += K[k] * (int)rows[(max(min(base + k, nr - 1), 0) * 3 + c) * S + xs];
    image[i] = (uint8_t)clip8(acc);
  }
}

// the launch geometry of both entry points; PASSL_OK, or the status to return
int crop_geom(int B, int Hs, int Ws, int S, CropGeom& g, Carve& cv) {
  // the carve's capacities, from the SOURCE extent: a crop is never larger.  ceil() of the exact rationals, in integers.
  auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  const int64_t sup_h = Hs > S ? ceil_div(2ll * Hs, S) : 2, sup_w = Ws > S ? ceil_div(2ll * Ws, S) : 2;
  const int64_t KH = 2 * sup_w + 1, KV = 2 * sup_h + 1;
  const int64_t NR = (Hs > S ? ceil_div((int64_t)(kBand - 1) * Hs, S) : kBand - 1) + 2 * sup_h + 3;
  const int64_t bands = ceil_div(S, kBand);
  const int64_t lds = 4ll * S * (KH + 2) + 4ll * kBand * (KV + 2) + 3072 + 3ll * S * NR + 8 * 16;
  if (lds > kLdsMax || bands * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  g.Hs = Hs; g.Ws = Ws; g.S = S; g.KH = (int)KH; g.KV = (int)KV; g.NR = (int)NR; g.bands = (int)bands;
  cv = carve(g);
  return cv.total > kLdsMax ? PASSL_EUNSUPPORTED : PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_crop_resize_norm(const uint8_t* src, float* out, const int32_t* table, int B, int Hs, int Ws,
                                          int S, const float* mean_std_scale, passl_stream_t stream) {
  if (!src || !out || !table || !mean_std_scale || B < 0 || Hs <= 0 || Ws <= 0 || S <= 0) return PASSL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(out) & 3u) || (reinterpret_cast<uintptr_t>(table) & 3u)) return PASSL_EINVAL;
  if ((int64_t)Hs * Ws * 3 >= (1ll << 31) || (int64_t)S * S * 3 >= (1ll << 31)) return PASSL_EINVAL;
  for (int c = 0; c < 3; ++c)
    if (!(mean_std_scale[3 + c] != 0.0f)) return PASSL_EINVAL;      // (a zero or NaN std)
  if (B == 0) return PASSL_OK;
  CropGeom g;
  Carve cv;
  if (const int rc = crop_geom(B, Hs, Ws, S, g, cv)) return rc;
  for (int c = 0; c < 3; ++c) {
    g.mean[c] = mean_std_scale[c];
    g.stdv[c] = mean_std_scale[3 + c];
  }
  g.scale = mean_std_scale[6];
  const dim3 grid((unsigned)(g.bands * B));
  if ((S & 3) == 0 && aligned16(out))
    hipLaunchKernelGGL((crop_resize_norm_kernel<4>), grid, dim3(kThreads), (size_t)cv.total, as_stream(stream), src, out,
                       table, g);
  else
    hipLaunchKernelGGL((crop_resize_norm_kernel<1>), grid, dim3(kThreads), (size_t)cv.total, as_stream(stream), src, out,
                       table, g);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_crop_resize_u8(const uint8_t* src, uint8_t* out, const int32_t* table, int B, int Hs, int Ws, int S,
                                        passl_stream_t stream) {
  if (!src || !out || !table || B < 0 || Hs <= 0 || Ws <= 0 || S <= 0) return PASSL_EINVAL;
  if (reinterpret_cast<uintptr_t>(table) & 3u) return PASSL_EINVAL;
  if ((int64_t)Hs * Ws * 3 >= (1ll << 31) || (int64_t)S * S * 3 >= (1ll << 31)) return PASSL_EINVAL;
  if (B == 0) return PASSL_OK;
  CropGeom g;
  Carve cv;
  if (const int rc = crop_geom(B, Hs, Ws, S, g, cv)) return rc;
  for (int c = 0; c < 3; ++c) g.mean[c] = 0.0f, g.stdv[c] = 1.0f;
  g.scale = 1.0f;
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((unsigned)(g.bands * B)), dim3(kThreads), (size_t)cv.total,
                     as_stream(stream), src, out, table, g);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
