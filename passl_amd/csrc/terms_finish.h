// The fixed-order end of the classification losses (clas.hip, mixup.hip): the row kernel leaves kRows
// arrays of N per-row terms, one wave adds each.  Launched as dim3(1), dim3(64 * kRows).
#pragma once
#include "common.h"

namespace {

// out[k] = sum_i terms[k][i] in one fixed order (wave k)
template <int kRows>
__global__ void __launch_bounds__(64 * kRows) terms_finish_kernel(const float* __restrict__ terms, int N,
                                                                  float* __restrict__ out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float a = 0.f;
  for (int i = lane; i < N; i += 64) a += terms[(int64_t)w * N + i];
  a = wave_sum(a);
  if (lane == 0) out[w] = a;
}

}  // namespace
