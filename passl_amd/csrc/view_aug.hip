// The colour stage of the two-view pipeline on a device-resident uint8 batch: ColorJitter (brightness, contrast,
// saturation, hue), RandomGrayscale, BYOLSolarize and SimCLRGaussianBlur of passl/data/preprocess/basic_transforms.py
// (:770-787, :872-944), which the reference runs on the host through Pillow, sample by sample; then the tail of
// crop_resize.hip: flip, NormalizeImage, HWC -> CHW.
//
// img uint8 [B][H][W][3] is what passl_hip_crop_resize_u8 wrote.  The per-sample decisions are drawn on the host
// (passl_amd/datasets/preprocess/view_aug.py) and travel as a device table int32 [B][24] (view_aug_pixel.h):
//   [0] n ops (<= 8)   [1] flip   [2] blur r (< 0: none)   [3] ww   [4] fw   [5] split   [6] contrast entry's index (< 0: none)
//   [8..16) op codes   [16..24) values (a factor's fp32 bits, the hue shift)
// Ops [0, split) run before the sample's blur and [split, n) after it; split = n without a blur.
//
// RESULT: Pillow's 8-bit arithmetic, bit for bit (tests/view_aug_util.py restates it):
//   view_gray_sum   sums[b] = sum of gray over the image after ops [0, contrast index); 0 without a contrast entry.
//                   One workgroup per sample, integer partial sums through LDS: exact, order-free, no atomics.
//   view_pointwise  the ops of one part of every sample's list, pixel by pixel; the contrast mean is
//                   (2 sums[b] + N) / (2 N).  Output uint8 HWC, or flipped + normalised fp32 NCHW through the 3 x 256 table
//                   (16-byte stores when W % 4 == 0 and out is 16-byte aligned, single floats otherwise).
//   gaussian_blur   three box passes along x, then three along y, each rounding to uint8, every tap clamped to the image
//                   at every pass: out[x] = (ww sum_{|k| <= r} p[x + k] + fw (p[x - r - 1] + p[x + r + 1]) + 2^23) >> 24.
//                   One workgroup per 32 x 32 tile: the tile and a halo of 3 (kBlurRMax + 1) pixels in LDS, all six passes
//                   from LDS between two buffers.  A tile position holds the value of the image position it is clamped to, so
//                   the clamp at every pass is the clamp of that position's taps; what a pass cannot compute (its taps leave
//                   the tile) is confined to the outer (r + 1) ring per pass and never reaches the 32 x 32 interior.
//                   Samples with r < 0 are copied.  (r, ww, fw) come from the host: no float arithmetic here.
// The library cannot read the table on the host: every count, index and radius is clamped in the kernel, an unknown op
// code is a no-op, so no access leaves a tensor whatever the table holds.  Plain vector loads and stores only.
#include "common.h"
#include "view_aug_pixel.h"

#pragma clang fp contract(off)

namespace {

using namespace view_aug;

constexpr int kThreads = 256;
constexpr int kIter = 8;               // work items of a lane in the pointwise kernel
constexpr int kSumThreads = 1024;
constexpr int kBlurRMax = 1;
constexpr int kTile = 32;
constexpr int kHalo = 3 * (kBlurRMax + 1);
constexpr int kExt = kTile + 2 * kHalo;

struct Row {                           // a table row, clamped
  int n, flip, r, split, ci;
  uint32_t ww, fw;
};

__device__ __forceinline__ Row read_row(const int32_t* __restrict__ t) {
  Row w;
  w.n = min(max(t[0], 0), kMaxOps);
  w.flip = t[1] != 0;
  w.r = min(t[2], kBlurRMax);
  w.ww = (uint32_t)t[3];
  w.fw = (uint32_t)t[4];
  w.split = min(max(t[5], 0), w.n);
  w.ci = t[6] < w.n ? t[6] : -1;
  return w;
}

template <int VEC>
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ p, Rgb (&px)[VEC]) {
  if constexpr (VEC == 4) {            // 12 bytes, 4-byte aligned
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint32_t a = q[0], b = q[1], c = q[2];
    px[0] = Rgb{(int)(a & 255u), (int)((a >> 8) & 255u), (int)((a >> 16) & 255u)};
    px[1] = Rgb{(int)(a >> 24), (int)(b & 255u), (int)((b >> 8) & 255u)};
    px[2] = Rgb{(int)((b >> 16) & 255u), (int)(b >> 24), (int)(c & 255u)};
    px[3] = Rgb{(int)((c >> 8) & 255u), (int)((c >> 16) & 255u), (int)(c >> 24)};
  } else {
    px[0] = Rgb{(int)p[0], (int)p[1], (int)p[2]};
  }
}

__device__ __forceinline__ Rgb run_ops(Rgb p, const int32_t* __restrict__ t, int from, int to, int m) {
  for (int k = from; k < to; ++k) p = apply_op(p, t[8 + k], t[16 + k], m);
  return p;
}

// ---------------------------------------------------------------------------------------------- gray sum
template <int VEC>
__global__ void __launch_bounds__(kSumThreads) view_gray_sum_kernel(const uint8_t* __restrict__ img,
                                                                    const int32_t* __restrict__ table,
                                                                    unsigned long long* __restrict__ sums, int HW) {
  __shared__ unsigned long long part[kSumThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* t = table + (int64_t)b * kRow;
  const Row w = read_row(t);
  if (w.ci < 0) {                                            // uniform over the workgroup
    if (tid == 0) sums[b] = 0ull;
    return;
  }
  const uint8_t* base = img + (int64_t)b * HW * 3;
  unsigned long long acc = 0ull;
  for (int i = tid * VEC; i < HW; i += kSumThreads * VEC) {  // HW % VEC == 0
    Rgb px[VEC];
    load_px<VEC>(base + (int64_t)i * 3, px);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const Rgb q = run_ops(px[j], t, 0, w.ci, 0);
      acc += (unsigned long long)gray_of(q.r, q.g, q.b);
    }
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = kSumThreads / 2; s > 0; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  if (tid == 0) sums[b] = part[0];
}

// ---------------------------------------------------------------------------------------------- pointwise
struct NormConsts {
  float mean[3], stdv[3], scale;
};

template <int VEC, bool F32OUT>
__global__ void __launch_bounds__(kThreads) view_pointwise_kernel(const uint8_t* __restrict__ img,
                                                                  const int32_t* __restrict__ table,
                                                                  const unsigned long long* __restrict__ sums,
                                                                  uint8_t* __restrict__ out8, float* __restrict__ out,
                                                                  int H, int W, int chunks, int part, NormConsts nc) {
  __shared__ float lut[768];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks;                         // uniform over the workgroup
  const int chunk = blockIdx.x - b * chunks;
  const int32_t* t = table + (int64_t)b * kRow;
  const Row w = read_row(t);
  const int from = part == 2 ? w.split : 0, to = part == 1 ? w.split : w.n;
  int m = 0;
  if (sums && w.ci >= 0) {
    const unsigned long long N = (unsigned long long)H * (unsigned long long)W;
    m = (int)min((2ull * sums[b] + N) / (2ull * N), 255ull);
  }
  if constexpr (F32OUT) {
    for (int i = tid; i < 768; i += kThreads) {
      const int c = i >> 8;
      lut[i] = __fdiv_rn(__fsub_rn(__fmul_rn((float)(i & 255), nc.scale), nc.mean[c]), nc.stdv[c]);
    }
    __syncthreads();
  }
  const int xv = W / VEC;                                    // work items per row (W % VEC == 0)
  const int items = H * xv;
  const int HW = H * W;
  const uint8_t* base = img + (int64_t)b * HW * 3;
  const int end = min(items, (chunk + 1) * (kThreads * kIter));
  for (int j = chunk * (kThreads * kIter) + tid; j < end; j += kThreads) {
    const int y = j / xv, x = (j - y * xv) * VEC;
    const bool flip = F32OUT && w.flip;
    const int xs = flip ? W - VEC - x : x;
    Rgb px[VEC];
    load_px<VEC>(base + ((int64_t)y * W + xs) * 3, px);
#pragma unroll
    for (int k = 0; k < VEC; ++k) px[k] = run_ops(px[k], t, from, to, m);
    if constexpr (F32OUT) {
      float* q = out + (int64_t)b * 3 * HW + (int64_t)y * W + x;
      if constexpr (VEC == 4) {
        const int i0 = flip ? 3 : 0, i1 = flip ? 2 : 1, i2 = flip ? 1 : 2, i3 = flip ? 0 : 3;
        *reinterpret_cast<f32x4*>(q) = f32x4{lut[px[i0].r], lut[px[i1].r], lut[px[i2].r], lut[px[i3].r]};
        *reinterpret_cast<f32x4*>(q + HW) =
            f32x4{lut[256 + px[i0].g], lut[256 + px[i1].g], lut[256 + px[i2].g], lut[256 + px[i3].g]};
        *reinterpret_cast<f32x4*>(q + 2 * (int64_t)HW) =
            f32x4{lut[512 + px[i0].b], lut[512 + px[i1].b], lut[512 + px[i2].b], lut[512 + px[i3].b]};
      } else {
        q[0] = lut[px[0].r];
        q[HW] = lut[256 + px[0].g];
        q[2 * (int64_t)HW] = lut[512 + px[0].b];
      }
    } else {
      uint8_t* q = out8 + ((int64_t)b * HW + (int64_t)y * W + x) * 3;
      if constexpr (VEC == 4) {
        uint32_t* o = reinterpret_cast<uint32_t*>(q);
        o[0] = (uint32_t)px[0].r | ((uint32_t)px[0].g << 8) | ((uint32_t)px[0].b << 16) | ((uint32_t)px[1].r << 24);
        o[1] = (uint32_t)px[1].g | ((uint32_t)px[1].b << 8) | ((uint32_t)px[2].r << 16) | ((uint32_t)px[2].g << 24);
        o[2] = (uint32_t)px[2].b | ((uint32_t)px[3].r << 8) | ((uint32_t)px[3].g << 16) | ((uint32_t)px[3].b << 24);
      } else {
        q[0] = (uint8_t)px[0].r;
        q[1] = (uint8_t)px[0].g;
        q[2] = (uint8_t)px[0].b;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- Gaussian blur
// one box pass over the whole extended tile: in -> out, along x (ALONG_X) or along y; origin = the image coordinate of
// tile position 0 along the pass's axis, n = the image's extent along it
template <bool ALONG_X>
__device__ __forceinline__ void box_pass(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int origin, int n, int r,
                                         uint32_t ww, uint32_t fw) {
  for (int i = threadIdx.x; i < kExt * kExt * 3; i += kThreads) {
    const int pix = i / 3, c = i - pix * 3;
    const int ey = pix / kExt, ex = pix - ey * kExt;
    const int e = ALONG_X ? ex : ey;
    const int ic = min(max(origin + e, 0), n - 1);           // the image position this tile position stands for
    auto tap = [&](int k) -> uint32_t {
      const int p = min(max(ic + k, 0), n - 1);
      const int te = min(max(p - origin, 0), kExt - 1);
      return (uint32_t)in[((ALONG_X ? ey * kExt + te : te * kExt + ex)) * 3 + c];
    };
    uint32_t acc = 0;
    for (int k = -r; k <= r; ++k) acc += tap(k);
    const uint32_t edge = tap(-r - 1) + tap(r + 1);
    out[i] = (uint8_t)((ww * acc + fw * edge + (1u << 23)) >> 24);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) gaussian_blur_u8_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out,
                                                                    const int32_t* __restrict__ table, int H, int W,
                                                                    int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) uint8_t bufa[kExt * kExt * 3];
  __shared__ __attribute__((aligned(16))) uint8_t bufb[kExt * kExt * 3];
  const int tid = threadIdx.x;
  const int per = tiles_x * tiles_y;
  const int b = blockIdx.x / per;                            // uniform over the workgroup
  const int tl = blockIdx.x - b * per;
  const int ty = tl / tiles_x, tx = tl - ty * tiles_x;
  const int y0 = ty * kTile, x0 = tx * kTile;
  const Row w = read_row(table + (int64_t)b * kRow);
  const uint8_t* src = img + (int64_t)b * H * W * 3;
  uint8_t* dst = out + (int64_t)b * H * W * 3;
  const int th = min(kTile, H - y0), tw = min(kTile, W - x0);
  if (w.r < 0) {                                             // not blurred: the tile as it is
    for (int i = tid; i < th * tw * 3; i += kThreads) {
      const int y = i / (tw * 3), rem = i - y * (tw * 3);
      const int64_t at = ((int64_t)(y0 + y) * W + x0) * 3 + rem;
      dst[at] = src[at];
    }
    return;
  }
  const int oy = y0 - kHalo, ox = x0 - kHalo;
  for (int i = tid; i < kExt * kExt * 3; i += kThreads) {
    const int pix = i / 3, c = i - pix * 3;
    const int ey = pix / kExt, ex = pix - ey * kExt;
    const int iy = min(max(oy + ey, 0), H - 1), ix = min(max(ox + ex, 0), W - 1);
    bufa[i] = src[((int64_t)iy * W + ix) * 3 + c];
  }
  __syncthreads();
  box_pass<true>(bufa, bufb, ox, W, w.r, w.ww, w.fw);
  box_pass<true>(bufb, bufa, ox, W, w.r, w.ww, w.fw);
  box_pass<true>(bufa, bufb, ox, W, w.r, w.ww, w.fw);
  box_pass<false>(bufb, bufa, oy, H, w.r, w.ww, w.fw);
  box_pass<false>(bufa, bufb, oy, H, w.r, w.ww, w.fw);
  box_pass<false>(bufb, bufa, oy, H, w.r, w.ww, w.fw);
  for (int i = tid; i < th * tw * 3; i += kThreads) {
    const int y = i / (tw * 3), rem = i - y * (tw * 3);
    const int x = rem / 3, c = rem - x * 3;
    dst[((int64_t)(y0 + y) * W + x0 + x) * 3 + c] = bufa[((kHalo + y) * kExt + kHalo + x) * 3 + c];
  }
}

bool bad_image(int B, int H, int W) { return B < 0 || H <= 0 || W <= 0 || (int64_t)H * W * 3 >= (1ll << 31); }

}  // namespace

extern "C" int passl_hip_view_gray_sum(const uint8_t* img, const int32_t* table, uint64_t* sums, int B, int H, int W,
                                       passl_stream_t stream) {
  if (!img || !table || !sums || bad_image(B, H, W)) return PASSL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(table) & 3u) || (reinterpret_cast<uintptr_t>(sums) & 7u)) return PASSL_EINVAL;
  if (B == 0) return PASSL_OK;
  const int HW = H * W;
  unsigned long long* s = reinterpret_cast<unsigned long long*>(sums);
  if ((HW & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3u) == 0)
    hipLaunchKernelGGL((view_gray_sum_kernel<4>), dim3((unsigned)B), dim3(kSumThreads), 0, as_stream(stream), img, table, s,
                       HW);
  else
    hipLaunchKernelGGL((view_gray_sum_kernel<1>), dim3((unsigned)B), dim3(kSumThreads), 0, as_stream(stream), img, table, s,
                       HW);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_view_pointwise(const uint8_t* img, const int32_t* table, const uint64_t* sums, uint8_t* out_u8,
                                        float* out_f32, int B, int H, int W, int part, const float* mean_std_scale,
                                        passl_stream_t stream) {
  if (!img || !table || bad_image(B, H, W) || part < 0 || part > 2) return PASSL_EINVAL;
  if ((out_u8 != nullptr) == (out_f32 != nullptr)) return PASSL_EINVAL;          // exactly one output
  if ((reinterpret_cast<uintptr_t>(table) & 3u) || (reinterpret_cast<uintptr_t>(sums) & 7u) ||
      (reinterpret_cast<uintptr_t>(out_f32) & 3u))
    return PASSL_EINVAL;
  NormConsts nc = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 1.f};
  if (out_f32) {
    if (!mean_std_scale) return PASSL_EINVAL;
    for (int c = 0; c < 3; ++c) {
      if (!(mean_std_scale[3 + c] != 0.0f)) return PASSL_EINVAL;                 // (a zero or NaN std)
      nc.mean[c] = mean_std_scale[c];
      nc.stdv[c] = mean_std_scale[3 + c];
    }
    nc.scale = mean_std_scale[6];
  }
  if (B == 0) return PASSL_OK;
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3u) == 0 &&
                   (out_f32 ? aligned16(out_f32) : (reinterpret_cast<uintptr_t>(out_u8) & 3u) == 0);
  const int64_t items = (int64_t)H * (vec ? W / 4 : W);
  const int64_t chunks = (items + kThreads * kIter - 1) / (kThreads * kIter);
  if (chunks * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const dim3 grid((unsigned)(chunks * B)), block(kThreads);
  const unsigned long long* s = reinterpret_cast<const unsigned long long*>(sums);
#define PASSL_VIEW_LAUNCH(V, F)                                                                                       \
  hipLaunchKernelGGL((view_pointwise_kernel<V, F>), grid, block, 0, as_stream(stream), img, table, s, out_u8, out_f32, H, \
                     W, (int)chunks, part, nc)
  if (out_f32) {
    if (vec) PASSL_VIEW_LAUNCH(4, true);
    else PASSL_VIEW_LAUNCH(1, true);
  } else {
    if (vec) PASSL_VIEW_LAUNCH(4, false);
    else PASSL_VIEW_LAUNCH(1, false);
  }
#undef PASSL_VIEW_LAUNCH
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_gaussian_blur_u8(const uint8_t* img, uint8_t* out, const int32_t* table, int B, int H, int W,
                                          int r_max, passl_stream_t stream) {
  if (!img || !out || !table || img == out || bad_image(B, H, W)) return PASSL_EINVAL;
  if (reinterpret_cast<uintptr_t>(table) & 3u) return PASSL_EINVAL;
  if (r_max > kBlurRMax) return PASSL_EUNSUPPORTED;
  if (B == 0) return PASSL_OK;
  const int64_t tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  if (tiles_x * tiles_y * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  hipLaunchKernelGGL(gaussian_blur_u8_kernel, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(kThreads), 0, as_stream(stream),
                     img, out, table, H, W, (int)tiles_x, (int)tiles_y);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
