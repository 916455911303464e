// Random erasing of a device-resident batch.
//
// Reference: class RandomErasing, passl_v110/datasets/preprocess/random_erasing.py:34-115 (after timm), which erases on
// the host, sample by sample: box parameters from Python's `random`, the 'pixel' fill from np.random.normal.  Here the
// boxes are drawn on the host (passl_amd/datasets/preprocess/random_erasing.py) and travel as a device table
// int32 [B][4] = (top, left, h, w); h == 0 or w == 0: the sample is not erased.
//
// ONE box per sample is the whole interface: the reference erases at most one box whatever max_count is — `_erase`
// returns after its first successful box (:89-103), the drawn count only divides the target area.
//
//   mode 0 ('const')  fill = 0.0f
//   mode 1 ('pixel')  fill = a standard normal defined BY POSITION, not by thread layout.  e = (c*H + y)*W + x, the
//                     element's index inside its sample; g = e >> 2;
//                     (w0..w3) = Philox4x32-10(counter (g, b, step_lo, step_hi), key (seed_lo, seed_hi));
//                     u0 = (float(w0 >> 8) + 1) 2^-24 in (0, 1], u1 = float(w1 >> 8) 2^-24 in [0, 1), u2 / u3 likewise
//                     from w2 / w3; r01 = sqrtf(-2 logf(u0)), r23 = sqrtf(-2 logf(u2));
//                     z = (r01 cos 2 pi u1, r01 sin 2 pi u1, r23 cos 2 pi u3, r23 sin 2 pi u3); element e gets z[e & 3].
//                     Precise logf / sqrtf / sincospif.  A value depends on (seed, step, b, e) only.
//   ('rand', one colour per box, is not built: the reference class raises on it for any box whose width is not 3.)
//
// out != x: out of place, one pass in the tile form of mixup.hip / drop_path.hip — a workgroup owns kU * 256 consecutive
// chunks of ONE sample (its box is one uniform load), a lane issues its kU loads back to back; out = x outside the box,
// the fill inside; x is never written.  out == x: in place, only box elements are stored and x is not loaded (x and out
// may alias, so neither carries __restrict__).  Chunks are 16 bytes when C*H*W % 4 == 0 and both pointers are 16-byte
// aligned — a chunk is then exactly one Philox group — single floats otherwise.  A chunk may cross a row end or a border
// of the box (W % 4 != 0): its elements are walked.  Philox, logf and sincospif run only for elements inside a box.
// The library cannot read the table on the host: the kernel clamps every box to the image, so no access leaves the
// tensor whatever the table holds.
#include <math.h>
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;

struct EraseGeom {
  int H, W;
  uint32_t k0, k1, s_lo, s_hi;
};

// one half of a group's Box-Muller quadruple: (r cos, r sin) from the radius word wr and the angle word wa
__device__ __forceinline__ void normal_pair(uint32_t wr, uint32_t wa, float& c, float& s) {
  const float ur = ((float)(wr >> 8) + 1.0f) * 0x1p-24f;     // (0, 1]
  const float ua = (float)(wa >> 8) * 0x1p-24f;              // [0, 1)
  const float r = sqrtf(-2.0f * logf(ur));
  float sn, cs;
  sincospif(2.0f * ua, &sn, &cs);
  c = r * cs;
  s = r * sn;
}

// VEC = 4: per = chunks of one sample (C*H*W / 4), chunk i is Philox group i.  VEC = 1: per = C*H*W, element i lies in
// group i >> 2.  tiles = workgroups per sample.
template <int VEC, int MODE, bool INPLACE>
__global__ void __launch_bounds__(kThreads) random_erase_kernel(const float* x, float* out,
                                                                const int32_t* __restrict__ boxes, int per, int tiles,
                                                                EraseGeom gm) {
  const int b = blockIdx.x / tiles;                          // uniform over the workgroup
  const int first = (blockIdx.x - b * tiles) * (kThreads * kU) + threadIdx.x;
  const int64_t off = (int64_t)b * per * VEC;
  // the box, clamped to the image: 0 <= yl <= yh <= H, 0 <= xl <= xh <= W whatever the table holds
  const int32_t* bx = boxes + (int64_t)b * 4;
  const int top = bx[0], left = bx[1], bh = bx[2], bw = bx[3];
  const int yl = min(max(top, 0), gm.H), xl = min(max(left, 0), gm.W);
  const int yh = yl + min(max(bh, 0), gm.H - yl), xh = xl + min(max(bw, 0), gm.W - xl);
  const bool empty = yh == yl || xh == xl;
  if (INPLACE && empty) return;
  float v[kU][VEC];
  if (!INPLACE) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {                           // branch-free: a lane past the end re-reads the last chunk
      const int i = first + u * kThreads;
      const float* p = x + off + (int64_t)(i < per ? i : per - 1) * VEC;
      if constexpr (VEC == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[u][0] = a[0]; v[u][1] = a[1]; v[u][2] = a[2]; v[u][3] = a[3];
      } else {
        v[u][0] = *p;
      }
    }
  }
  const unsigned hw = (unsigned)(gm.H * gm.W);
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (i >= per) break;
    bool in[VEC];
    bool any = false, all = true;
    if (!empty) {
      const unsigned e = (unsigned)i * VEC;                  // < C*H*W < 2^31 (checked by the caller)
      const unsigned idx = e % hw;
      int yy = (int)(idx / (unsigned)gm.W);
      int xx = (int)(idx - (unsigned)yy * (unsigned)gm.W);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        in[k] = yy >= yl && yy < yh && xx >= xl && xx < xh;
        any |= in[k];
        all &= in[k];
        if (++xx == gm.W) {
          xx = 0;
          if (++yy == gm.H) yy = 0;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) in[k] = false;
      all = false;
    }
    if (any) {
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (MODE == 1) {
        uint32_t c0 = (uint32_t)(VEC == 4 ? i : i >> 2), c1 = (uint32_t)b, c2 = gm.s_lo, c3 = gm.s_hi;
        philox4x32_10(c0, c1, c2, c3, gm.k0, gm.k1);
        if constexpr (VEC == 4) {
          if (in[0] || in[1]) normal_pair(c0, c1, z[0], z[1]);
          if (in[2] || in[3]) normal_pair(c2, c3, z[2], z[3]);
        } else {
          const int k = i & 3;                               // one element: its half of the quadruple only
          float c, s;
          if (k < 2) normal_pair(c0, c1, c, s); else normal_pair(c2, c3, c, s);
          z[0] = (k & 1) ? s : c;
        }
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (in[k]) v[u][k] = z[k];
    }
    float* q = out + off + (int64_t)i * VEC;
    if (!INPLACE || all) {
      if constexpr (VEC == 4)
        *reinterpret_cast<f32x4*>(q) = f32x4{v[u][0], v[u][1], v[u][2], v[u][3]};
      else
        *q = v[u][0];
    } else if (any) {
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        if (in[k]) q[k] = v[u][k];
    }
  }
}

template <int VEC>
void launch_random_erase(const float* x, float* out, const int32_t* boxes, int B, int per, int mode,
                         const EraseGeom& gm, hipStream_t st) {
  const int tiles = (per + kThreads * kU - 1) / (kThreads * kU);
  const dim3 grid((unsigned)(tiles * B));
#define PASSL_ERASE_LAUNCH(MODE, INPLACE)                                                                       \
  hipLaunchKernelGGL((random_erase_kernel<VEC, MODE, INPLACE>), grid, dim3(kThreads), 0, st, x, out, boxes, per, \
                     tiles, gm)
  if (x == out) {
    if (mode == 0) PASSL_ERASE_LAUNCH(0, true); else PASSL_ERASE_LAUNCH(1, true);
  } else {
    if (mode == 0) PASSL_ERASE_LAUNCH(0, false); else PASSL_ERASE_LAUNCH(1, false);
  }
#undef PASSL_ERASE_LAUNCH
}

}  // namespace

extern "C" int passl_hip_random_erase(const float* x, float* out, const int32_t* boxes, int B, int C, int H, int W,
                                      int mode, int64_t seed, int64_t step, passl_stream_t stream) {
  if (!x || !out || !boxes || B < 0 || C <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return PASSL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u) ||
      (reinterpret_cast<uintptr_t>(boxes) & 3u))
    return PASSL_EINVAL;
  const int64_t E = (int64_t)C * H * W;                      // elements of one sample
  if (E >= (1ll << 31)) return PASSL_EINVAL;
  if (B == 0) return PASSL_OK;
  const bool vec = (E & 3) == 0 && aligned16(x) && aligned16(out);
  const int64_t per = vec ? E / 4 : E;
  const int64_t tiles = (per + kThreads * kU - 1) / (kThreads * kU);
  if (E > 0x7fffffffll - 4 * kThreads * kU || tiles * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const uint64_t sd = (uint64_t)seed, sp = (uint64_t)step;
  const EraseGeom gm{H, W, (uint32_t)sd, (uint32_t)(sd >> 32), (uint32_t)sp, (uint32_t)(sp >> 32)};
  if (vec)
    launch_random_erase<4>(x, out, boxes, B, (int)per, mode, gm, as_stream(stream));
  else
    launch_random_erase<1>(x, out, boxes, B, (int)per, mode, gm, as_stream(stream));
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
