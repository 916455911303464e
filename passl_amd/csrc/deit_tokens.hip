// Token assembly with one or two learnable prefix rows (DeiT: cls_token, and dist_token for the distilled class).
//
// Reference: DistilledVisionTransformer.forward_features, passl/models/deit.py:238-247:
//   x = concat(cls_token.expand(B), dist_token.expand(B), patch_embed(x)) + pos_embed
// and its gradients.  The token assembly of csrc/vit.hip (mae_gather) carries one prefix row; this pair carries NP = 1
// or 2 and no keep-gather.  Both are streaming launches, 8 elements a thread:
//   forward   out[b, t] = (t < NP ? prefix_t : x[b, t - NP]) + pos[t]          one launch over [B, NP + L, C]
//   backward  dx[b, t - NP] = dout[b, t]  (t >= NP)                            the first blocks of one launch
//             dprefix_t[c] += sum_b dout[b, t, c]                              its last blocks: a thread per 8 channels
//                                                                              of a prefix row, images in order
// dpos[t] = sum_b dout[b, t] is the library's column sum (passl_hip_colsum_acc) over dout seen as [B, (NP + L) C].
// No atomics: every output element has one writer and a fixed order of sums.
//
// The distilled class returns (head(x) + head_dist(x_dist)) / 2 (deit.py:255-259) on fp32 logits: mean2 forms it in one
// launch, one rounding (of the sum; the halving is exact), and its backward hands dy / 2 to both heads.
#include "common.h"

namespace deit {

constexpr int kThreads = 256;
constexpr int kMaxPrefix = 2;

template <typename T>
__global__ void __launch_bounds__(kThreads) prefix_tokens_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ p0, const float* __restrict__ p1, const float* __restrict__ pos,
    T* __restrict__ out, int64_t n8, int L, int NP, int c8) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n8) return;
  const int cp = (int)(i % c8);
  const int64_t row = i / c8, b = row / (L + NP);
  const int t = (int)(row % (L + NP));
  float a[8], p[8];
  if (t < NP) ElemTraits<float>::load8((t == 0 ? p0 : p1) + cp * 8, a);
  else ElemTraits<T>::load8(x + ((b * L + t - NP) * c8 + cp) * 8, a);
  ElemTraits<float>::load8(pos + ((int64_t)t * c8 + cp) * 8, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += p[e];
  ElemTraits<T>::store8(out + i * 8, a);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) prefix_tokens_bwd_kernel(
    const T* __restrict__ dout, T* __restrict__ dx, float* __restrict__ dp0, float* __restrict__ dp1, int64_t n8,
    int copy_blocks, int B, int L, int NP, int c8) {
  if ((int)blockIdx.x < copy_blocks) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;     // over dx [B, L, C]
    if (i >= n8) return;
    const int cp = (int)(i % c8);
    const int64_t row = i / c8, b = row / L;
    const int t = (int)(row % L);
    float a[8];
    ElemTraits<T>::load8(dout + ((b * (L + NP) + NP + t) * c8 + cp) * 8, a);
    ElemTraits<T>::store8(dx + i * 8, a);
    return;
  }
  const int j = ((int)blockIdx.x - copy_blocks) * kThreads + threadIdx.x;   // over [NP, C / 8]
  if (j >= NP * c8) return;
  const int t = j / c8, cp = j % c8;
  float* dst = (t == 0 ? dp0 : dp1) + cp * 8;
  float s[8];
  ElemTraits<float>::load8(dst, s);
  for (int b = 0; b < B; ++b) {
    float a[8];
    ElemTraits<T>::load8(dout + (((int64_t)b * (L + NP) + t) * c8 + cp) * 8, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += a[e];
  }
  ElemTraits<float>::store8(dst, s);
}

// out = (a + b) / 2, or with b == nullptr a / 2 (the backward)
__global__ void __launch_bounds__(kThreads) mean2_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  out[i] = (b ? a[i] + b[i] : a[i]) * 0.5f;
}

// PASSL_OK, or the status the entry points return without launching; *n8 = rows * C / 8
int check_shape(int B, int L, int NP, int C, int dtype, int64_t rows, int64_t* n8) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8 || NP < 1 || NP > kMaxPrefix) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  *n8 = rows * (C / 8);
  return (*n8 + kThreads - 1) / kThreads + kMaxPrefix * C > INT32_MAX ? PASSL_EUNSUPPORTED : PASSL_OK;
}

}  // namespace deit

extern "C" int passl_hip_prefix_tokens_fwd(const void* x, const float* prefix0, const float* prefix1, const float* pos,
                                           void* out, int B, int L, int NP, int C, int dtype, passl_stream_t stream) {
  if (!x || !prefix0 || !pos || !out || (NP == 2 && !prefix1)) return PASSL_EINVAL;
  int64_t n8;
  const int rc = deit::check_shape(B, L, NP, C, dtype, (int64_t)B * (L + NP), &n8);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(x) && aligned16(prefix0) && aligned16(prefix1) && aligned16(pos) && aligned16(out))) return PASSL_EINVAL;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(deit::prefix_tokens_fwd_kernel<T>, dim3((unsigned)((n8 + deit::kThreads - 1) / deit::kThreads)),
                       dim3(deit::kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(x), prefix0, prefix1, pos,
                       reinterpret_cast<T*>(out), n8, L, NP, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_prefix_tokens_bwd(const void* dout, void* dx, float* dprefix0, float* dprefix1, int B, int L,
                                           int NP, int C, int dtype, passl_stream_t stream) {
  if (!dout || !dx || !dprefix0 || (NP == 2 && !dprefix1)) return PASSL_EINVAL;
  int64_t n8;
  const int rc = deit::check_shape(B, L, NP, C, dtype, (int64_t)B * L, &n8);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(dout) && aligned16(dx) && aligned16(dprefix0) && aligned16(dprefix1))) return PASSL_EINVAL;
  const int copy_blocks = (int)((n8 + deit::kThreads - 1) / deit::kThreads);
  const int sum_blocks = (NP * (C / 8) + deit::kThreads - 1) / deit::kThreads;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(deit::prefix_tokens_bwd_kernel<T>, dim3((unsigned)(copy_blocks + sum_blocks)), dim3(deit::kThreads),
                       0, as_stream(stream), reinterpret_cast<const T*>(dout), reinterpret_cast<T*>(dx), dprefix0,
                       dprefix1, n8, copy_blocks, B, L, NP, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_mean2(const float* a, const float* b, float* out, int64_t n, passl_stream_t stream) {
  if (!a || !out || n <= 0) return PASSL_EINVAL;
  if ((n + deit::kThreads - 1) / deit::kThreads > INT32_MAX) return PASSL_EUNSUPPORTED;
  hipLaunchKernelGGL(deit::mean2_kernel, dim3((unsigned)((n + deit::kThreads - 1) / deit::kThreads)), dim3(deit::kThreads),
                     0, as_stream(stream), a, b, out, n);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}
