// Element-wise dropout, paddle.nn.Dropout(p) in its default `upscale_in_train` mode [Paddle-semantics]:
//   training  out = kept ? x * factor : 0,  factor = float32(1 / (1 - float32(p)));   evaluation: identity (no launch).
// Reference call sites: passl/models/vision_transformer.py  Mlp :106-112 (after the activation and after fc2),
// Attention :153-155 (proj_drop), VisionTransformer :300, 358 (pos_drop).
//
// The mask is DEFINED BY POSITION (Paddle's generator cannot be reproduced; random erasing's 'pixel' mode does the
// same): chunk k = elements 8k .. 8k+7 of the tensor at dropout site `site` takes the four words x[0..3] of
// Philox4x32-10 on counter (k, site, step_lo, step_hi) and key (seed_lo, seed_hi); element e of the chunk owns the 16
// bits  r = (x[e >> 1] >> (16 * (e & 1))) & 0xFFFF  and is kept iff r >= thr, thr = floor(p * 65536 + 0.5) computed by
// the caller.  One Philox call per chunk, no mask tensor: the backward recomputes the mask from the same four numbers.
//
// `step` lives in device memory and is READ by every launch, never taken by value: a step plan (plan.h) that replays
// these launches with unchanged argument bytes draws fresh masks, because the one-thread advance launch at the head of
// the pass has moved the counter.
//
//   dropout           out = mask * (in * factor)                       (on dy: the backward of all of these sites)
//   dropout_add       out = residual + mask * (branch * factor)        (the product rounded to fp32 before the add)
//   gelu_dropout_fwd  out = mask * (gelu(x) * factor)
//   gelu_dropout_bwd  dx  = (mask * (dy * factor)) * gelu'(x)
//
// Tile form of eltwise.h / drop_path.hip: a workgroup owns kU * 256 consecutive chunks, a lane issues its kU loads back
// to back (a lane past the end re-reads the last chunk), 16-byte loads and stores; fp32 arithmetic, one rounding to
// `dtype`.  Algorithmic bytes per element (bf16): dropout 4, dropout_add 6, gelu_dropout_fwd 4, gelu_dropout_bwd 6 —
// what the launches they replace or extend move; the cost on top is ~40 32-bit multiplies per chunk.
#include "common.h"
#include "gelu_op.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kU = 4;
constexpr int64_t kMaxElems = 1ll << 35;      // chunk index = one 32-bit counter word

enum Mode { kPlain, kAdd, kGeluFwd, kGeluBwd };

// a * b rounded to fp32 before anything is done with it: never the multiplier of an fma (as attention.hip)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// a: the tensor that is scaled and masked (in / branch / x of the GELU / dy); b: residual (kAdd) or x (kGeluBwd)
template <typename T, int MODE>
__global__ void __launch_bounds__(kThreads) dropout_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                           T* __restrict__ out, int64_t nchunks, uint32_t thr,
                                                           float factor, uint64_t seed,
                                                           const uint64_t* __restrict__ step, uint32_t site) {
  constexpr bool kTwo = MODE == kAdd || MODE == kGeluBwd;
  const uint64_t s = *step;
  const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t base = (int64_t)blockIdx.x * (kThreads * kU) + threadIdx.x;
  float v[kU][8], w[kTwo ? kU : 1][8];
#pragma unroll
  for (int u = 0; u < kU; ++u) {                      // branch-free: a lane past the end re-reads the last chunk
    const int64_t i = base + u * kThreads;
    const int64_t ic = i < nchunks ? i : nchunks - 1;
    ElemTraits<T>::load8(a + ic * 8, v[u]);
    if (kTwo) ElemTraits<T>::load8(b + ic * 8, w[kTwo ? u : 0]);
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t i = base + u * kThreads;
    if (i >= nchunks) break;
    uint32_t x[4] = {(uint32_t)i, site, s_lo, s_hi};
    philox4x32_10(x[0], x[1], x[2], x[3], k0, k1);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool kept = ((x[e >> 1] >> (16 * (e & 1))) & 0xFFFFu) >= thr;
      const float in = MODE == kGeluFwd ? GeluOp::fwd(v[u][e]) : v[u][e];
      const float m = kept ? mul_rn(in, factor) : 0.0f;
      if (MODE == kAdd) o[e] = w[kTwo ? u : 0][e] + m;
      else if (MODE == kGeluBwd) o[e] = m * GeluOp::grad(w[kTwo ? u : 0][e]);
      else o[e] = m;
    }
    ElemTraits<T>::store8(out + i * 8, o);
  }
}

__global__ void dropout_advance_kernel(uint64_t* step) { *step = *step + 1; }

// n elements, a multiple of 8; every pointer 16-byte aligned, step 8-byte aligned.  b is read only by kAdd / kGeluBwd.
template <int MODE>
int launch_dropout(const void* a, const void* b, void* out, int64_t n, int thr, float factor, int64_t seed,
                   const int64_t* step, int site, int dtype, passl_stream_t stream) {
  constexpr bool kTwo = MODE == kAdd || MODE == kGeluBwd;
  if (!a || (kTwo && !b) || !out || !step || n <= 0 || (n & 7) || thr < 0 || thr > 65535 || !(factor > 0.0f) ||
      site < 0 || !aligned16(a) || (kTwo && !aligned16(b)) || !aligned16(out) ||
      (reinterpret_cast<uintptr_t>(step) & 7))
    return PASSL_EINVAL;
  if (n > kMaxElems) return PASSL_EUNSUPPORTED;
  const int64_t nchunks = n >> 3;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((dropout_kernel<T, MODE>),
                                                 dim3((unsigned)((nchunks + kThreads * kU - 1) / (kThreads * kU))),
                                                 dim3(kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(a),
                                                 reinterpret_cast<const T*>(b), reinterpret_cast<T*>(out), nchunks,
                                                 (uint32_t)thr, factor, (uint64_t)seed,
                                                 reinterpret_cast<const uint64_t*>(step), (uint32_t)site);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_dropout_advance(int64_t* step, passl_stream_t stream) {
  if (!step || (reinterpret_cast<uintptr_t>(step) & 7)) return PASSL_EINVAL;
  hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, as_stream(stream),
                     reinterpret_cast<uint64_t*>(step));
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_dropout(const void* in, void* out, int64_t n, int thr, float factor, int64_t seed,
                                 const int64_t* step, int site, int dtype, passl_stream_t stream) {
  return launch_dropout<kPlain>(in, nullptr, out, n, thr, factor, seed, step, site, dtype, stream);
}

extern "C" int passl_hip_dropout_add(const void* branch, const void* residual, void* out, int64_t n, int thr,
                                     float factor, int64_t seed, const int64_t* step, int site, int dtype,
                                     passl_stream_t stream) {
  return launch_dropout<kAdd>(branch, residual, out, n, thr, factor, seed, step, site, dtype, stream);
}

extern "C" int passl_hip_gelu_dropout_fwd(const void* x, void* out, int64_t n, int thr, float factor, int64_t seed,
                                          const int64_t* step, int site, int dtype, passl_stream_t stream) {
  return launch_dropout<kGeluFwd>(x, nullptr, out, n, thr, factor, seed, step, site, dtype, stream);
}

extern "C" int passl_hip_gelu_dropout_bwd(const void* dy, const void* x, void* dx, int64_t n, int thr, float factor,
                                          int64_t seed, const int64_t* step, int site, int dtype,
                                          passl_stream_t stream) {
  return launch_dropout<kGeluBwd>(dy, x, dx, n, thr, factor, seed, step, site, dtype, stream);
}
