// Operand policy of the exact-fp32-MFMA attention kernels (attention_core.h lists what a policy supplies); shared by
// attention.hip and window_attention.hip, whose staging differs only in the row map it hands to stage.
//
// LDS holds fp32 rows [T_pad][d + 4] (bf16 inputs are converted when staged); every product is
// v_mfma_f32_16x16x4_f32, one tile per accumulate step.
#pragma once
#include "attention_core.h"

namespace af32 {

// a * b rounded to fp32 before anything is done with it: never the multiplier of an fma
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

template <typename T, int DH_>
struct F32Ops {
  using elem_t = T;
  using lds_t = float;
  static constexpr int DH = DH_, P = DH + 4, kStep = 1, kMaxTiles = 13, kMaxRows = 16 * kMaxTiles;
  typedef float Own[DH / 4];         // DH/4 consecutive channels [l4*DH/4, ...) of row l15
  static constexpr int fwd_waves_per_eu(int) { return 0; }
  static constexpr bool kAccumByLane = false;
  static constexpr bool kSelectProb = true;      // one wave per SIMD at T = 197: nothing else hides an MFMA chain

  template <int NTH, class Rows>
  __device__ static __forceinline__ void stage(const T* __restrict__ base, int64_t rs, const Rows& rows, int Tn,
                                               int Tpad, float* lds) {
    for (int i = threadIdx.x; i < Tpad * (DH / 4); i += NTH) {
      const int r = i / (DH / 4), c = (i % (DH / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < Tn) {
        const T* p = base + (int64_t)rows.row(r) * rs + c;
        v = make_float4(ElemTraits<T>::ld(p), ElemTraits<T>::ld(p + 1), ElemTraits<T>::ld(p + 2),
                        ElemTraits<T>::ld(p + 3));
      }
      *reinterpret_cast<float4*>(lds + r * P + c) = v;
    }
  }

  __device__ static __forceinline__ void load_own(const T* __restrict__ p, bool valid, int l4, Own& reg) {
#pragma unroll
    for (int v = 0; v < DH / 4; ++v) reg[v] = valid ? ElemTraits<T>::ld(p + l4 * (DH / 4) + v) : 0.f;
  }

  __device__ static __forceinline__ f32x4 dot(const float* lds, int tile, const Own& own, int l15, int l4) {
    float swept[DH / 4];
#pragma unroll
    for (int v = 0; v < DH / 16; ++v) {
      const float4 t = *reinterpret_cast<const float4*>(lds + (tile * 16 + l15) * P + l4 * (DH / 4) + v * 4);
      swept[v * 4] = t.x; swept[v * 4 + 1] = t.y; swept[v * 4 + 2] = t.z; swept[v * 4 + 3] = t.w;
    }
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DH / 4; ++ks)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(swept[ks], own[ks], acc, 0, 0, 0);
    return acc;
  }

  __device__ static __forceinline__ void accum(const float (&c)[1][4], const float* lds, int t0, int l15, int l4,
                                               f32x4 (&o)[DH / 16]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* rp = lds + (t0 * 16 + l4 * 4 + r) * P + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd)
        o[jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[0][r], rp[jd * 16], o[jd], 0, 0, 0);
    }
  }

  __device__ static __forceinline__ float dot_own(const Own& a, const Own& b) {
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < DH / 4; ++v) d += a[v] * b[v];
    return d;
  }

  static constexpr int kRowVec = 1;
  __device__ static __forceinline__ void lds_vec(const float* p, float (&v)[1]) { v[0] = *p; }
  __device__ static __forceinline__ void glb_vec(const T* p, float (&v)[1]) { v[0] = ElemTraits<T>::ld(p); }

  // The recomputation rounds s * scale before it subtracts lse, as the forward did before it formed lse: fused
  // into one fma it keeps the product's rounding error, |s| 2^-24, as a relative error of every P (a lone key's P
  // is then not 1).  The bf16-MFMA policy does not: its P is rounded to bf16 before it is used.
  __device__ static __forceinline__ float prob(float s, float scale, float l) { return __expf(mul_rn(s, scale) - l); }
};

}  // namespace af32
