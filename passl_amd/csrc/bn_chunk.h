// The per-chunk (8 channels of one row) arithmetic of the BatchNorm streaming kernels, in ONE place: bn.hip's apply /
// backward-apply kernels and the A-operand prologue of igemm_kernel (conv_igemm.hip) call these, so both sides compile
// the same fp32 expression — operand order and contraction included — and round to bf16 through the same pack2bf
// (ElemTraits<T>::store8 there, epi::pack8 here).  Values produced on either side are bit-identical.
#pragma once
#include "common.h"

namespace bnc {

// v = v * scale + shift
__device__ __forceinline__ void affine8(float (&v)[8], const float (&sc)[8], const float (&sh)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + sh[e];
}

__device__ __forceinline__ void relu8(float (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
}

// o = cA * g + cB * v + cC  (BatchNorm backward: g the masked output gradient, v the layer's input), evaluated as
// fma(cA, g, cB * v) + cC.  The contraction is spelled out: left to the compiler, which of the two products is fused
// into the sum depends on the code around the expression, and the two callers would round differently.
__device__ __forceinline__ void bwd8(float (&o)[8], const float (&g)[8], const float (&v)[8], const float (&cA)[8],
                                     const float (&cB)[8], const float (&cC)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = __fmaf_rn(cA[e], g[e], cB[e] * v[e]) + cC[e];
}

}  // namespace bnc
