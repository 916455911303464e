// Adan over a flat fp32 arena for gfx950 (passl/optimizer/adan.py:117-148 with is_vanilla=False; arXiv 2208.06677):
// one launch updates the parameters and the four state vectors from the gradient.  HBM-bound streaming: six vectors
// read, five written (44 B per element), one float4 of each buffer per lane, grid-stride with the AdamW grid rule.
// No atomics, no LDS: an element is touched by exactly one lane.
//
//   gg   = g*gs;  if clip: gg *= coef
//   diff = first ? 0 : gg - pre
//   m    = b1*m + (1-b1)*gg
//   d    = b2*d + (1-b2)*diff
//   u    = gg + b2*diff
//   s    = b3*s + (1-b3)*(u*u)
//   den  = sqrt(s)/sqrt(1-b3^t) + eps
//   upd  = (m/(1-b1^t) + b2*d/(1-b2^t)) / den
//   prox (default): p = (p - lr*upd) / (1 + lr*wd)        no_prox: p = p*(1 - lr*wd) - lr*upd
//   pre  = gg
//
// The step-dependent scalars come from DEVICE memory, hyper = {lr, b1^t, b2^t, b3^t, first, 0, 0, 0}: a recorded step
// plan or a HIP graph replays correctly whichever step it was recorded at.  `first` (1.0 at t == 1) stands for the
// reference creating its state with pre_grad = grad.clone(): the difference is exactly zero, whatever pre holds.
#include <cstdio>
#include <cstdlib>

#include "common.h"

namespace {

constexpr int kThreads = 256;

// The segment lookup of adamw_segments_kernel (vit.hip), restated here: lifting it into a shared header changed the
// register allocation and load order of the AdamW kernels, which stay as they are.  seg_end: ascending exclusive end
// offsets in elements, the last one n.  A workgroup tile starts at a wave-uniform offset: its segment is found by a
// binary search through uniform loads of the table, resumed from the segment of the block's previous tile (offsets
// ascend); a lane then steps forward while its own float4 lies beyond that segment — no step at all unless a boundary
// falls inside the tile.  Neither cursor leaves [0, n_seg) whatever the table holds.
__device__ __forceinline__ int seg_cursor_tile(const int64_t* __restrict__ seg_end, int n_seg, int s0, int64_t first) {
  int hi = n_seg - 1;
  while (s0 < hi) {                                     // first segment with first < seg_end[s]
    const int mid = (s0 + hi) >> 1;
    if (first < seg_end[mid]) hi = mid; else s0 = mid + 1;
  }
  return s0;
}
__device__ __forceinline__ int seg_cursor_lane(const int64_t* __restrict__ seg_end, int n_seg, int s, int64_t elem) {
  while (s + 1 < n_seg && elem >= seg_end[s]) ++s;
  return s;
}

// What is configuration, by value: the same for every step.  omb = 1 - beta, see adan_config.
struct AdanConfig {
  float b1, b2, b3, omb1, omb2, omb3, eps, gs;
  int no_prox;
};

// The element rule, stated ONCE: the flat and the grouped kernel both call this, so a segment updated with
// (lr*scale, wd_s) gets the bits the flat kernel gives a buffer of its own with those two values.
template <bool kClip>
__device__ __forceinline__ void adan_update(float* __restrict__ pp, const float* __restrict__ gp,
                                            float* __restrict__ mp, float* __restrict__ dp, float* __restrict__ sp,
                                            float* __restrict__ prep, int count, float lr, float wd, float b1p,
                                            float b2p, float b3p, bool first, const AdanConfig& c, float coef) {
  // every operation rounded on its own, in the order written: what the compiler may fuse into a multiply-add depends on
  // the code around the call (loop-invariant scalars in the flat walk, per-lane ones in the grouped walk), and the two
  // walks must give equal bits.  The kernel is HBM-bound; the extra VALU instructions are not seen.
#pragma clang fp contract(off)
  const float bc1 = 1.f - b1p;
  const float bc2 = 1.f - b2p;
  const float bc3 = sqrtf(1.f - b3p);
  const float lw = lr * wd;
#pragma unroll
  for (int e = 0; e < count; ++e) {
    float gg = gp[e] * c.gs;
    if (kClip) gg *= coef;
    const float diff = first ? 0.f : gg - prep[e];
    mp[e] = c.b1 * mp[e] + c.omb1 * gg;
    dp[e] = c.b2 * dp[e] + c.omb2 * diff;
    const float u = gg + c.b2 * diff;
    sp[e] = c.b3 * sp[e] + c.omb3 * (u * u);
    const float den = sqrtf(sp[e]) / bc3 + c.eps;
    const float upd = (mp[e] / bc1 + c.b2 * dp[e] / bc2) / den;
    if (c.no_prox) pp[e] = pp[e] * (1.f - lw) - lr * upd;
    else pp[e] = (pp[e] - lr * upd) / (1.f + lw);
    prep[e] = gg;
  }
}

// One float4 of each of the six buffers through adan_update: the body of both walks below.
template <bool kClip>
__device__ __forceinline__ void adan_update4(float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ m, float* __restrict__ d, float* __restrict__ s,
                                             float* __restrict__ pre, int64_t i, float lr, float wd, float b1p,
                                             float b2p, float b3p, bool first, const AdanConfig& c, float coef) {
  float4 pv = reinterpret_cast<float4*>(p)[i];
  const float4 gv = reinterpret_cast<const float4*>(g)[i];
  float4 mv = reinterpret_cast<float4*>(m)[i];
  float4 dv = reinterpret_cast<float4*>(d)[i];
  float4 sv = reinterpret_cast<float4*>(s)[i];
  float4 qv = reinterpret_cast<float4*>(pre)[i];
  adan_update<kClip>(&pv.x, &gv.x, &mv.x, &dv.x, &sv.x, &qv.x, 4, lr, wd, b1p, b2p, b3p, first, c, coef);
  reinterpret_cast<float4*>(p)[i] = pv;
  reinterpret_cast<float4*>(m)[i] = mv;
  reinterpret_cast<float4*>(d)[i] = dv;
  reinterpret_cast<float4*>(s)[i] = sv;
  reinterpret_cast<float4*>(pre)[i] = qv;
}

// The flat grid-stride walk: one weight decay.  kClip: the gradient times ONE coefficient that
// grad_clip_finalize_kernel (flat.hip) left in device memory at coef_p.  n % 4 == 0.
template <bool kClip>
__global__ void __launch_bounds__(kThreads) adan_flat_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ d,
    float* __restrict__ s, float* __restrict__ pre, int64_t n, const float* __restrict__ hyper, float wd,
    AdanConfig c, const float* __restrict__ coef_p) {
  const float lr = hyper[0], b1p = hyper[1], b2p = hyper[2], b3p = hyper[3];
  const bool first = hyper[4] != 0.f;
  const float coef = kClip ? coef_p[0] : 1.f;
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nv; i += stride)
    adan_update4<kClip>(p, g, m, d, s, pre, i, lr, wd, b1p, b2p, b3p, first, c, coef);
}

// ... with a learning-rate multiplier and a weight decay per SEGMENT of the buffer: the table and the lookup of
// adamw_segments_kernel (vit.hip).  A float4 lies in one segment; the data accesses are bounded by n
// whatever the table holds.  kClip: clip = the {norm, coef} table of grad_clip_finalize_kernel, seg_set[s] the set of
// segment s (outside [0, n_sets): coefficient 1 — a parameter excluded from clipping).
template <bool kClip>
__global__ void __launch_bounds__(kThreads) adan_segments_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ d,
    float* __restrict__ s, float* __restrict__ pre, int64_t n, const int64_t* __restrict__ seg_end,
    const float* __restrict__ seg_lr_scale, const float* __restrict__ seg_wd, int n_seg,
    const float* __restrict__ hyper, AdanConfig c, const int32_t* __restrict__ seg_set,
    const float* __restrict__ clip, int n_sets) {
  const float lr = hyper[0], b1p = hyper[1], b2p = hyper[2], b3p = hyper[3];
  const bool first = hyper[4] != 0.f;
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int s0 = 0;
  for (int64_t tile = (int64_t)blockIdx.x * kThreads; tile < nv; tile += stride) {
    s0 = seg_cursor_tile(seg_end, n_seg, s0, tile << 2);        // first element of the tile: uniform
    const int64_t i = tile + threadIdx.x;
    if (i >= nv) continue;
    const int sg = seg_cursor_lane(seg_end, n_seg, s0, i << 2);
    const float lr_s = lr * seg_lr_scale[sg];
    const float wd_s = seg_wd[sg];
    float coef = 1.f;
    if constexpr (kClip) {
      const int set = seg_set[sg];
      if (set >= 0 && set < n_sets) coef = clip[2 * set + 1];
    }
    adan_update4<kClip>(p, g, m, d, s, pre, i, lr_s, wd_s, b1p, b2p, b3p, first, c, coef);
  }
}

}  // namespace

// What the four entry points ask of their common arguments, and their grid (the AdamW rule: one thread per float4,
// capped at 2048 workgroups — the walks are grid-stride).
static inline bool adan_args_ok(const float* p, const float* g, const float* m, const float* d, const float* s,
                                const float* pre, int64_t n, const float* hyper) {
  return p && g && m && d && s && pre && hyper && n >= 0 && !(n & 3) && aligned16(p) && aligned16(g) &&
         aligned16(m) && aligned16(d) && aligned16(s) && aligned16(pre) &&
         !(reinterpret_cast<uintptr_t>(hyper) & 3u);
}
// 1 - beta as the reference forms it: in DOUBLE from the caller's decimal, rounded to fp32 once (0.02f for beta = 0.98).
// beta arrives here as a float, and 1.f - 0.98f misses 0.02f by 1e-6 relative — fifty ulp in exp_avg at the first step.
// The caller's decimal is the shortest one that rounds to the float (what repr() prints for it); a beta that has no
// decimal of nine digits or fewer takes 1.f - beta.  Host code, three betas per launch, no allocation.
static float one_minus(float b) {
  char buf[32];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)b);
    const double v = strtod(buf, nullptr);
    if ((float)v == b) return (float)(1.0 - v);
  }
  return 1.f - b;
}
static AdanConfig adan_config(float beta1, float beta2, float beta3, float epsilon, float grad_scale, int no_prox) {
  return {beta1, beta2, beta3, one_minus(beta1), one_minus(beta2), one_minus(beta3), epsilon, grad_scale,
          no_prox ? 1 : 0};
}
static inline unsigned adan_grid(int64_t n) {
  int64_t b = ((n >> 2) + kThreads - 1) / kThreads;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (unsigned)b;
}

template <bool kClip>
static int adan_flat(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                     const float* hyper, const float* coef, float beta1, float beta2, float beta3, float epsilon,
                     float weight_decay, int no_prox, float grad_scale, passl_stream_t stream) {
  if (!adan_args_ok(p, g, m, d, s, pre, n, hyper)) return PASSL_EINVAL;
  if (n == 0) return PASSL_OK;
  const AdanConfig c = adan_config(beta1, beta2, beta3, epsilon, grad_scale, no_prox);
  hipLaunchKernelGGL(adan_flat_kernel<kClip>, dim3(adan_grid(n)), dim3(kThreads), 0, as_stream(stream), p, g, m, d, s,
                     pre, n, hyper, weight_decay, c, coef);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_adan_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                                  const float* hyper, float beta1, float beta2, float beta3, float epsilon,
                                  float weight_decay, int no_prox, float grad_scale, passl_stream_t stream) {
  return adan_flat<false>(p, g, m, d, s, pre, n, hyper, nullptr, beta1, beta2, beta3, epsilon, weight_decay, no_prox,
                          grad_scale, stream);
}

extern "C" int passl_hip_adan_clip_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                                       const float* hyper, const float* coef, float beta1, float beta2, float beta3,
                                       float epsilon, float weight_decay, int no_prox, float grad_scale,
                                       passl_stream_t stream) {
  if (!coef || (reinterpret_cast<uintptr_t>(coef) & 3u)) return PASSL_EINVAL;
  return adan_flat<true>(p, g, m, d, s, pre, n, hyper, coef, beta1, beta2, beta3, epsilon, weight_decay, no_prox,
                         grad_scale, stream);
}

template <bool kClip>
static int adan_segments(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                         const int64_t* seg_end, const float* seg_lr_scale, const float* seg_wd,
                         const int32_t* seg_set, int n_seg, const float* hyper, const float* clip, int n_sets,
                         float beta1, float beta2, float beta3, float epsilon, int no_prox, float grad_scale,
                         passl_stream_t stream) {
  if (!adan_args_ok(p, g, m, d, s, pre, n, hyper) || !seg_end || !seg_lr_scale || !seg_wd || n_seg <= 0 ||
      (reinterpret_cast<uintptr_t>(seg_end) & 7u) || (reinterpret_cast<uintptr_t>(seg_lr_scale) & 3u) ||
      (reinterpret_cast<uintptr_t>(seg_wd) & 3u))
    return PASSL_EINVAL;
  if (n == 0) return PASSL_OK;
  const AdanConfig c = adan_config(beta1, beta2, beta3, epsilon, grad_scale, no_prox);
  hipLaunchKernelGGL(adan_segments_kernel<kClip>, dim3(adan_grid(n)), dim3(kThreads), 0, as_stream(stream), p, g, m, d,
                     s, pre, n, seg_end, seg_lr_scale, seg_wd, n_seg, hyper, c, seg_set, clip, n_sets);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_adan_groups_dev(float* p, const float* g, float* m, float* d, float* s, float* pre,
                                         int64_t n, const int64_t* seg_end, const float* seg_lr_scale,
                                         const float* seg_wd, int n_seg, const float* hyper, float beta1, float beta2,
                                         float beta3, float epsilon, int no_prox, float grad_scale,
                                         passl_stream_t stream) {
  return adan_segments<false>(p, g, m, d, s, pre, n, seg_end, seg_lr_scale, seg_wd, nullptr, n_seg, hyper, nullptr, 0,
                              beta1, beta2, beta3, epsilon, no_prox, grad_scale, stream);
}

extern "C" int passl_hip_adan_groups_clip_dev(float* p, const float* g, float* m, float* d, float* s, float* pre,
                                              int64_t n, const int64_t* seg_end, const float* seg_lr_scale,
                                              const float* seg_wd, const int32_t* seg_set, int n_seg,
                                              const float* hyper, const float* clip, int n_sets, float beta1,
                                              float beta2, float beta3, float epsilon, int no_prox, float grad_scale,
                                              passl_stream_t stream) {
  if (!clip || !seg_set || n_sets <= 0 || (reinterpret_cast<uintptr_t>(seg_set) & 3u) ||
      (reinterpret_cast<uintptr_t>(clip) & 3u))
    return PASSL_EINVAL;
  return adan_segments<true>(p, g, m, d, s, pre, n, seg_end, seg_lr_scale, seg_wd, seg_set, n_seg, hyper, clip, n_sets,
                             beta1, beta2, beta3, epsilon, no_prox, grad_scale, stream);
}
