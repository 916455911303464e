// The exact (erf) GELU and its derivative, stated once: the streaming GELU launches (vit.hip) and the GELU + dropout
// launches (dropout.hip) evaluate these two functions and nothing else.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  return cdf + x * 0.39894228040143268f * __expf(-0.5f * x * x);
}

// operator of the streaming unary kernel (eltwise.h)
struct GeluOp {
  __device__ static __forceinline__ float fwd(float x) { return gelu_f(x); }
  __device__ static __forceinline__ float grad(float x) { return gelu_grad_f(x); }
};

}  // namespace
