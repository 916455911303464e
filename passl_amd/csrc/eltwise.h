// Streaming unary activations (vit.hip: GELU, tanh; clip.hip: QuickGELU): one kernel template and one
// launcher over an operator struct `Op` with  static __device__ float fwd(float x)  and  grad(float x).
// The operators stay in the files that cite their reference call sites.  Everything here assumes a
// 256-thread block.
#pragma once
#include "common.h"

namespace {

// Tile form (as the BatchNorm streaming kernels, bn.hip): a workgroup owns U x 256 consecutive 16-byte
// chunks, a lane the chunks base + u * 256; all loads are issued back to back, branch-free (a lane past
// the end re-reads the last chunk), no loop.
constexpr int kEltU = 4;

// out = Op::fwd(x), or with BWD  out = dy * Op::grad(x)
template <typename T, typename Op, bool BWD>
__global__ void __launch_bounds__(256) unary_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                    T* __restrict__ out, int64_t nchunks) {
  const int64_t base = (int64_t)blockIdx.x * (256 * kEltU) + threadIdx.x;
  float v[kEltU][8], d[kEltU][8];
#pragma unroll
  for (int u = 0; u < kEltU; ++u) {
    const int64_t i = base + u * 256;
    const int64_t ic = i < nchunks ? i : nchunks - 1;
    ElemTraits<T>::load8(x + ic * 8, v[u]);
    if (BWD) ElemTraits<T>::load8(dy + ic * 8, d[u]);
  }
#pragma unroll
  for (int u = 0; u < kEltU; ++u) {
    const int64_t i = base + u * 256;
    if (i >= nchunks) break;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = BWD ? d[u][e] * Op::grad(v[u][e]) : Op::fwd(v[u][e]);
    ElemTraits<T>::store8(out + i * 8, o);
  }
}

// n elements, a multiple of 8; every pointer 16-byte aligned.  dy is read only with BWD.
template <typename Op, bool BWD>
int launch_unary(const void* x, const void* dy, void* out, int64_t n, int dtype, passl_stream_t stream) {
  if (!x || (BWD && !dy) || !out || n <= 0 || (n & 7) || !aligned16(x) || (BWD && !aligned16(dy)) ||
      !aligned16(out))
    return PASSL_EINVAL;
  const int64_t nchunks = n >> 3;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((unary_kernel<T, Op, BWD>),
                                                 dim3((unsigned)((nchunks + 256 * kEltU - 1) / (256 * kEltU))),
                                                 dim3(256), 0, as_stream(stream), reinterpret_cast<const T*>(x),
                                                 reinterpret_cast<const T*>(dy), reinterpret_cast<T*>(out),
                                                 nchunks);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

}  // namespace
