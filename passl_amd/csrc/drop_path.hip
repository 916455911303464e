// Stochastic depth (DropPath, passl_v110/modeling/backbones/mae.py:32-50 and its two uses per Block :186-187) over
// token rows [B*T][C]: sample b owns rows b*T .. (b+1)*T-1 and is kept or dropped as a whole.
//
//   draw:  keep[slot][b] = floor(keep_prob[slot] + u) with u from Philox4x32-10; seed by value, the step counter in
//          device memory, read and advanced by the launch itself: the launch's argument bytes never change, so a step
//          plan (plan.h) that replays it draws a fresh table every time.
//   add:   out = residual + keep[b] * (branch / keep_prob)        (rows of a dropped sample: residual copied, branch
//          not read)
//   bwd:   dbranch = keep[b] * (dy / keep_prob)                    (rows of a dropped sample: zeros, dy not read)
//
// add / bwd are HBM-bound streaming kernels in the tile form of bn.hip: a workgroup owns kU * 256 consecutive
// 8-element chunks OF ONE SAMPLE (so keep[b] is one uniform load per workgroup and the dropped / kept decision is a
// uniform branch), a lane issues its kU loads back to back, 16-byte loads and stores throughout.
// Algorithmic bytes per activation (bf16): add 6 (4 for a dropped sample), bwd 4 (2 for a dropped sample).
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;

// ---- word 0 of Philox4x32-10 (philox.h)
__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                     uint32_t k0, uint32_t k1) {
  philox4x32_10(c0, c1, c2, c3, k0, k1);
  return c0;
}

// one workgroup: every element is drawn with the value *step had when the launch began; after the barrier (all reads
// of *step are done) one thread leaves *step + 1 behind
__global__ void __launch_bounds__(kThreads) drop_path_draw_kernel(float* __restrict__ keep,
                                                                  const float* __restrict__ keep_prob, int slots,
                                                                  int B, uint64_t seed, uint64_t* step) {
  const uint64_t s = *step;
  const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int n = slots * B;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int slot = i / B, b = i - slot * B;
    const uint32_t x0 = philox4x32_10_x0((uint32_t)b, (uint32_t)slot, s_lo, s_hi, k0, k1);
    const float u = (float)(x0 >> 8) * 0x1p-24f;             // [0, 1), 24 bits: exact in fp32
    keep[i] = (keep_prob[slot] + u >= 1.0f) ? 1.0f : 0.0f;   // floor(keep_prob + rand), the sum rounded to fp32
  }
  __syncthreads();
  if (threadIdx.x == 0) *step = s + 1;
}

// chunk = 8 elements; per = chunks of one sample (T * C/8); tiles = workgroups per sample
template <typename T>
__global__ void __launch_bounds__(kThreads) drop_path_add_kernel(const T* __restrict__ branch,
                                                                 const T* __restrict__ res,
                                                                 const float* __restrict__ keep, float keep_prob,
                                                                 T* __restrict__ out, int per, int tiles) {
  const int b = blockIdx.x / tiles;
  const int first = (blockIdx.x - b * tiles) * (kThreads * kU) + threadIdx.x;
  const int64_t off = (int64_t)b * per;
  const bool kept = keep[b] != 0.0f;                  // uniform over the workgroup
  float r[kU][8];
#pragma unroll
  for (int u = 0; u < kU; ++u) {                      // branch-free: a lane past the end re-reads the last chunk
    const int i = first + u * kThreads;
    ElemTraits<T>::load8(res + (off + (i < per ? i : per - 1)) * 8, r[u]);
  }
  if (kept) {
    float v[kU][8];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = first + u * kThreads;
      ElemTraits<T>::load8(branch + (off + (i < per ? i : per - 1)) * 8, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[u][e] += v[u][e] / keep_prob;    // IEEE division (no fast-math in the build)
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (i >= per) break;
    ElemTraits<T>::store8(out + (off + i) * 8, r[u]);
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) drop_path_bwd_kernel(const T* __restrict__ dy,
                                                                 const float* __restrict__ keep, float keep_prob,
                                                                 T* __restrict__ dbranch, int per, int tiles) {
  const int b = blockIdx.x / tiles;
  const int first = (blockIdx.x - b * tiles) * (kThreads * kU) + threadIdx.x;
  const int64_t off = (int64_t)b * per;
  const bool kept = keep[b] != 0.0f;
  float v[kU][8];
  if (kept) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = first + u * kThreads;
      ElemTraits<T>::load8(dy + (off + (i < per ? i : per - 1)) * 8, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = v[u][e] / keep_prob;
    }
  } else {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.0f;
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (i >= per) break;
    ElemTraits<T>::store8(dbranch + (off + i) * 8, v[u]);
  }
}

// shape checks shared by add / bwd: -> chunks per sample and workgroups per sample, or a status
static int stream_geometry(int B, int T, int C, float keep_prob, int* per, int* tiles) {
  if (B <= 0 || T <= 0 || C <= 0 || (C & 7) || !(keep_prob > 0.0f && keep_prob <= 1.0f)) return PASSL_EINVAL;
  const int64_t p = (int64_t)T * (C >> 3);
  const int64_t t = (p + kThreads * kU - 1) / (kThreads * kU);
  if (p > 0x7fffffffll - kThreads * kU || t * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  *per = (int)p;
  *tiles = (int)t;
  return PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_drop_path_draw(float* keep, const float* keep_prob, int slots, int B, int64_t seed,
                                        int64_t* step, passl_stream_t stream) {
  if (!keep || !keep_prob || !step || slots <= 0 || B <= 0 || (reinterpret_cast<uintptr_t>(step) & 7))
    return PASSL_EINVAL;
  if ((int64_t)slots * B > (1 << 24)) return PASSL_EUNSUPPORTED;      // one workgroup: a table, not an activation
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), keep, keep_prob, slots, B,
                     (uint64_t)seed, reinterpret_cast<uint64_t*>(step));
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_drop_path_add(const void* branch, const void* residual, const float* keep, float keep_prob,
                                       void* out, int B, int T, int C, int dtype, passl_stream_t stream) {
  if (!branch || !residual || !keep || !out || !aligned16(branch) || !aligned16(residual) || !aligned16(out))
    return PASSL_EINVAL;
  int per = 0, tiles = 0;
  const int rc = stream_geometry(B, T, C, keep_prob, &per, &tiles);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(drop_path_add_kernel<T>, dim3((unsigned)(tiles * B)), dim3(kThreads), 0,
                                                 as_stream(stream), reinterpret_cast<const T*>(branch),
                                                 reinterpret_cast<const T*>(residual), keep, keep_prob,
                                                 reinterpret_cast<T*>(out), per, tiles);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_drop_path_bwd(const void* dy, const float* keep, float keep_prob, void* dbranch, int B, int T,
                                       int C, int dtype, passl_stream_t stream) {
  if (!dy || !keep || !dbranch || !aligned16(dy) || !aligned16(dbranch)) return PASSL_EINVAL;
  int per = 0, tiles = 0;
  const int rc = stream_geometry(B, T, C, keep_prob, &per, &tiles);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(drop_path_bwd_kernel<T>, dim3((unsigned)(tiles * B)), dim3(kThreads), 0,
                                                 as_stream(stream), reinterpret_cast<const T*>(dy), keep, keep_prob,
                                                 reinterpret_cast<T*>(dbranch), per, tiles);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
