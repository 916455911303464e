// Mixup / CutMix of a device-resident batch, the mixed target, and cross-entropy over soft targets.
//
// Reference: class Mixup, passl_v110/datasets/preprocess/mixup.py:108-276 (_mix_batch :248-264, mixup_target :29-37),
// which mixes on the host; SoftTargetCrossEntropy, tasks/ssl/mae/util/loss.py:44-47 = passl/loss/celoss.py:48-49.
//
//   batch_mix     out[b] = fl(fl(x[b] lam) + fl(x[B-1-b] (1-lam)))            (mode 0, mixup.py:261-263)
//                 out[b] = x[B-1-b] inside the box, x[b] elsewhere            (mode 1, mixup.py:259)
//   mixup_target  t[i]   = lam smooth(onehot(y[i])) + (1-lam) smooth(onehot(y[N-1-i]))
//   soft_ce       loss   = mean_i (lse_i T_i - sum_j t_ij s_ij), T_i = sum_j t_ij;  ds = g/N (softmax T - t)
//
// batch_mix is an HBM-bound streaming kernel in the tile form of drop_path.hip.  A lane owns chunk e of sample b AND of
// its partner B-1-b (b < B/2; the middle sample of an odd batch is its own partner): both chunks are loaded once and
// both results stored, so a launch reads and writes every byte of the batch exactly once — the bytes of a copy, over two
// read and two write streams.  A workgroup owns kU * 256 consecutive chunks of one pair; a lane issues its 2 * kU loads
// back to back.  Chunks are 16 bytes when every sample starts on a 16-byte boundary (C*H*W % 4 == 0: every image size the
// models take), single floats otherwise.
// The cross-entropy keeps the form of clas.hip: one wave per row, per-row terms summed in one fixed order, no atomics.
#include <math.h>
#include "common.h"
#include "terms_finish.h"

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;

template <int VEC> struct Chunk;
template <> struct Chunk<4> {
  __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
  }
  __device__ static __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
};
template <> struct Chunk<1> {
  __device__ static __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
  __device__ static __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};

struct MixBox {
  int H, W, yl, yh, xl, xh;
};

// per = chunks of one sample (C*H*W / VEC); tiles = workgroups per pair
template <int VEC, int MODE>
__global__ void __launch_bounds__(kThreads) batch_mix_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                             int B, int per, int tiles, float lam, float oml,
                                                             MixBox box) {
  const int b = blockIdx.x / tiles;
  const int bp = B - 1 - b;                                  // uniform over the workgroup
  const int first = (blockIdx.x - b * tiles) * (kThreads * kU) + threadIdx.x;
  const int64_t off = (int64_t)b * per * VEC, offp = (int64_t)bp * per * VEC;
  float p[kU][VEC], q[kU][VEC];
#pragma unroll
  for (int u = 0; u < kU; ++u) {                             // branch-free: a lane past the end re-reads the last chunk
    const int i = first + u * kThreads;
    const int64_t e = (int64_t)(i < per ? i : per - 1) * VEC;
    Chunk<VEC>::load(x + off + e, p[u]);
    Chunk<VEC>::load(x + offp + e, q[u]);
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (MODE == 0) {
#pragma clang fp contract(off)                               // two rounded products and a rounded sum: no FMA
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float a = p[u][k], c = q[u][k];
        const float a_lam = a * lam, c_oml = c * oml;
        const float c_lam = c * lam, a_oml = a * oml;
        p[u][k] = a_lam + c_oml;
        q[u][k] = c_lam + a_oml;
      }
    } else {
      // position of the chunk's first element inside its channel plane, then walked element by element (a chunk may
      // cross a row end or a border of the box)
      const unsigned hw = (unsigned)(box.H * box.W);
      const unsigned e = (unsigned)(i < per ? i : per - 1) * VEC;      // < C*H*W < 2^31 (checked by the caller)
      const unsigned idx = e % hw;
      int yy = (int)(idx / (unsigned)box.W);
      int xx = (int)(idx - (unsigned)yy * (unsigned)box.W);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool in = yy >= box.yl && yy < box.yh && xx >= box.xl && xx < box.xh;
        const float a = p[u][k], c = q[u][k];
        p[u][k] = in ? c : a;
        q[u][k] = in ? a : c;
        if (++xx == box.W) {
          xx = 0;
          if (++yy == box.H) yy = 0;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (i >= per) break;
    Chunk<VEC>::store(out + off + (int64_t)i * VEC, p[u]);
    if (bp != b) Chunk<VEC>::store(out + offp + (int64_t)i * VEC, q[u]);
  }
}

// one thread per 4 consecutive elements of the flat [N*C] target; a chunk may cross a row end
__global__ void __launch_bounds__(kThreads) mixup_target_kernel(const int64_t* __restrict__ labels,
                                                                float* __restrict__ target, int N, int C, float lam,
                                                                float eps) {
  const int64_t total = (int64_t)N * C;
  const int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e0 >= total) return;
  const float off_v = eps / (float)C;
  const float on_v = 1.0f - eps + off_v;
  const float oml = 1.0f - lam;
  int i = (int)(e0 / C), j = (int)(e0 - (int64_t)i * C);
  int64_t y1 = labels[i], y2 = labels[N - 1 - i];
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool ok = y1 >= 0 && y1 < C && y2 >= 0 && y2 < C;
    const float t = (y1 == j ? on_v : off_v) * lam + (y2 == j ? on_v : off_v) * oml;
    v[k] = ok ? t : NAN;
    if (++j == C && k < 3) {
      j = 0;
      if (++i < N) {
        y1 = labels[i];
        y2 = labels[N - 1 - i];
      }
    }
  }
  if (e0 + 4 <= total) {
    Chunk<4>::store(target + e0, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e0 + k < total) target[e0 + k] = v[k];
  }
}

// (value, index) maximum, the lowest index on ties
__device__ __forceinline__ void wave_argmax(float& v, int& idx) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
}

// One wave per row; a lane reads chunks lane, lane + 64, ... of the row.  Pass 1: the row maximum of the scores and the
// arg-max of the target ("the label").  Pass 2: sum-exp, T = sum t, sum t s, and the label's rank as in clas.hip.
template <int VEC>
__global__ void __launch_bounds__(kThreads) soft_ce_fwd_kernel(const float* __restrict__ s,
                                                               const float* __restrict__ t, int N, int C,
                                                               float* __restrict__ lse, float* __restrict__ tsum,
                                                               float* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* r = s + (int64_t)row * C;
  const float* tr = t + (int64_t)row * C;
  const int chunks = C / VEC;
  float m = -INFINITY, tbest = -INFINITY;
  int lab = 0x7fffffff;
  for (int c = lane; c < chunks; c += 64) {
    float sv[VEC], tv[VEC];
    Chunk<VEC>::load(r + c * VEC, sv);
    Chunk<VEC>::load(tr + c * VEC, tv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      m = fmaxf(m, sv[k]);
      if (tv[k] > tbest) {                                   // ascending j within a lane: the first maximum stays
        tbest = tv[k];
        lab = c * VEC + k;
      }
    }
  }
  m = wave_max(m);
  wave_argmax(tbest, lab);
  const bool ok = lab >= 0 && lab < C;                       // false only for a row without any comparable target
  const float sl = ok ? r[lab] : 0.f;
  float z = 0.f, T = 0.f, dot = 0.f, cnt = 0.f;
  for (int c = lane; c < chunks; c += 64) {
    float sv[VEC], tv[VEC];
    Chunk<VEC>::load(r + c * VEC, sv);
    Chunk<VEC>::load(tr + c * VEC, tv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int j = c * VEC + k;
      z += __expf(sv[k] - m);
      T += tv[k];
      dot += tv[k] * sv[k];
      cnt += (sv[k] > sl || (sv[k] == sl && j < lab)) ? 1.f : 0.f;
    }
  }
  z = wave_sum(z);
  T = wave_sum(T);
  dot = wave_sum(dot);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    const float l = m + __logf(z);
    lse[row] = l;
    tsum[row] = T;
    const float invN = 1.0f / (float)N;
    terms[row] = (l * T - dot) * invN;                       // [3][N]: loss term, top-1 hit, top-5 hit
    terms[N + row] = (ok && cnt < 0.5f) ? 100.0f * invN : 0.f;
    terms[2 * N + row] = (ok && cnt < 4.5f) ? 100.0f * invN : 0.f;
  }
}

// ds[i][j] = g/N (exp(s_ij - lse_i) T_i - t_ij); a chunk lies inside one row (C % VEC == 0)
template <int VEC>
__global__ void __launch_bounds__(kThreads) soft_ce_bwd_kernel(const float* __restrict__ s,
                                                               const float* __restrict__ t,
                                                               const float* __restrict__ lse,
                                                               const float* __restrict__ tsum,
                                                               const float* __restrict__ gloss, int N, int C,
                                                               float* __restrict__ ds) {
  const int64_t chunks = (int64_t)N * C / VEC;
  const float k = *gloss / (float)N;
  for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * kThreads) {
    const int64_t e = c * VEC;
    const int i = (int)(e / C);
    const float l = lse[i], T = tsum[i];
    float sv[VEC], tv[VEC];
    Chunk<VEC>::load(s + e, sv);
    Chunk<VEC>::load(t + e, tv);
#pragma unroll
    for (int q = 0; q < VEC; ++q) sv[q] = k * (__expf(sv[q] - l) * T - tv[q]);
    Chunk<VEC>::store(ds + e, sv);
  }
}

template <int VEC>
void launch_batch_mix(const float* x, float* out, int B, int per, int mode, float lam, float oml, const MixBox& box,
                      hipStream_t st) {
  const int tiles = (per + kThreads * kU - 1) / (kThreads * kU);
  const dim3 grid((unsigned)(tiles * ((B + 1) / 2)));
  if (mode == 0)
    hipLaunchKernelGGL((batch_mix_kernel<VEC, 0>), grid, dim3(kThreads), 0, st, x, out, B, per, tiles, lam, oml, box);
  else
    hipLaunchKernelGGL((batch_mix_kernel<VEC, 1>), grid, dim3(kThreads), 0, st, x, out, B, per, tiles, lam, oml, box);
}

}  // namespace

extern "C" int passl_hip_batch_mix(const float* x, float* out, int B, int C, int H, int W, float lam,
                                   float one_minus_lam, int yl, int yh, int xl, int xh, int mode,
                                   passl_stream_t stream) {
  if (!x || !out || x == out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return PASSL_EINVAL;
  if (yl < 0 || yl > yh || yh > H || xl < 0 || xl > xh || xh > W) return PASSL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return PASSL_EINVAL;
  const int64_t E = (int64_t)C * H * W;                      // elements of one sample
  const bool vec = (E & 3) == 0 && aligned16(x) && aligned16(out);
  const int64_t per = vec ? E / 4 : E;
  const int64_t tiles = (per + kThreads * kU - 1) / (kThreads * kU);
  if (E > 0x7fffffffll - 4 * kThreads * kU || tiles * ((B + 1) / 2) > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const MixBox box{H, W, yl, yh, xl, xh};
  if (vec)
    launch_batch_mix<4>(x, out, B, (int)per, mode, lam, one_minus_lam, box, as_stream(stream));
  else
    launch_batch_mix<1>(x, out, B, (int)per, mode, lam, one_minus_lam, box, as_stream(stream));
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_mixup_target(const int64_t* labels, float* target, int N, int C, float lam, float eps,
                                      passl_stream_t stream) {
  if (!labels || !target || N <= 0 || C <= 0 || !aligned16(target)) return PASSL_EINVAL;
  if (!(lam >= 0.0f && lam <= 1.0f) || !(eps >= 0.0f && eps <= 1.0f)) return PASSL_EINVAL;
  const int64_t threads = ((int64_t)N * C + 3) / 4;
  const int64_t g = (threads + kThreads - 1) / kThreads;
  if (g > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  hipLaunchKernelGGL(mixup_target_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream), labels, target, N, C,
                     lam, eps);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

// ws: 3 * N floats (per-row loss term and top-1 / top-5 hits, summed in a fixed order)
extern "C" int passl_hip_soft_ce_fwd(const float* scores, const float* target, int N, int C, float* lse, float* tsum,
                                     float* out, float* ws, int64_t ws_floats, passl_stream_t stream) {
  if (!scores || !target || !lse || !tsum || !out || !ws || N <= 0 || C <= 0 || ws_floats < 3 * (int64_t)N)
    return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  if ((C & 3) == 0 && aligned16(scores) && aligned16(target))
    hipLaunchKernelGGL(soft_ce_fwd_kernel<4>, dim3((N + 3) / 4), dim3(kThreads), 0, st, scores, target, N, C, lse, tsum,
                       ws);
  else
    hipLaunchKernelGGL(soft_ce_fwd_kernel<1>, dim3((N + 3) / 4), dim3(kThreads), 0, st, scores, target, N, C, lse, tsum,
                       ws);
  hipLaunchKernelGGL(terms_finish_kernel<3>, dim3(1), dim3(192), 0, st, ws, N, out);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_soft_ce_bwd(const float* scores, const float* target, const float* lse, const float* tsum,
                                     const float* gloss, int N, int C, float* dscores, passl_stream_t stream) {
  if (!scores || !target || !lse || !tsum || !gloss || !dscores || N <= 0 || C <= 0) return PASSL_EINVAL;
  const bool vec = (C & 3) == 0 && aligned16(scores) && aligned16(target) && aligned16(dscores);
  int64_t g = ((int64_t)N * C / (vec ? 4 : 1) + kThreads - 1) / kThreads;
  if (g > 256 * 8) g = 256 * 8;
  if (vec)
    hipLaunchKernelGGL(soft_ce_bwd_kernel<4>, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream), scores, target,
                       lse, tsum, gloss, N, C, dscores);
  else
    hipLaunchKernelGGL(soft_ce_bwd_kernel<1>, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream), scores, target,
                       lse, tsum, gloss, N, C, dscores);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
