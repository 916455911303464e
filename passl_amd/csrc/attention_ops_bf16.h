// Operand policy of the bf16-MFMA attention kernels (attention_core.h lists what a policy supplies); shared by
// attention_bf16.hip, which describes the operand layout, and window_attention.hip, whose staging differs only in the
// row map it hands to stage.
#pragma once
#include "attention_core.h"

namespace abf {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
#define ABF_LDS3(p) ((__attribute__((address_space(3))) bf16x4_t*)(p))

template <int DH_>
struct Bf16Ops {
  using elem_t = bf16_t;
  using lds_t = bf16_t;
  // T <= 208 -> 13 tiles, padded to an even count
  static constexpr int DH = DH_, P = DH + 8, kStep = 2, kMaxTiles = 14, kMaxRows = 16 * kMaxTiles;
  typedef bf16x8_t Own[DH / 32];     // channels [32 s + 8 l4, +8) for s < DH/32
  // the 8-wave forward is capped at 128 VGPRs: two workgroups per CU
  static constexpr int fwd_waves_per_eu(int NW) { return NW == 8 ? 4 : 1; }
  static constexpr bool kAccumByLane = true;
  static constexpr bool kSelectProb = false;     // the select costs the 8-wave d = 64 dQ sweep 6 VGPRs: 5 waves, not 6

  template <int NTH, class Rows>
  __device__ static __forceinline__ void stage(const bf16_t* __restrict__ base, int64_t rs, const Rows& rows, int Tn,
                                               int Tpad, bf16_t* lds) {
    constexpr int CH = DH / 8;
    for (int i = threadIdx.x; i < Tpad * CH; i += NTH) {
      const int r = i / CH, c = (i % CH) * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r < Tn) v = *reinterpret_cast<const uint4*>(base + (int64_t)rows.row(r) * rs + c);
      *reinterpret_cast<uint4*>(lds + r * P + c) = v;
    }
  }

  __device__ static __forceinline__ void load_own(const bf16_t* __restrict__ p, bool valid, int l4, Own& f) {
#pragma unroll
    for (int s = 0; s < DH / 32; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (valid) v = *reinterpret_cast<const uint4*>(p + 32 * s + 8 * l4);
      f[s] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  __device__ static __forceinline__ f32x4 dot(const bf16_t* lds, int tile, const Own& own, int l15, int l4) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DH / 32; ++s) {
      const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(lds + (tile * 16 + l15) * P + 32 * s + 8 * l4);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, own[s], acc, 0, 0, 0);
    }
    return acc;
  }

  __device__ static __forceinline__ void accum(const float (&c)[2][4], const bf16_t* lds, int t0, int lane,
                                               f32x4 (&o)[DH / 16]) {
    const uint4 v = make_uint4(pack2bf(c[0][0], c[0][1]), pack2bf(c[0][2], c[0][3]), pack2bf(c[1][0], c[1][1]),
                               pack2bf(c[1][2], c[1][3]));
    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, v);
    const int j = lane & 15, l4 = lane >> 4;
    const bf16_t* base = lds + (t0 * 16 + 4 * l4 + (j >> 2)) * P + 4 * (j & 3);
#pragma unroll
    for (int jd = 0; jd < DH / 16; ++jd) {
      const bf16x4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(ABF_LDS3(base + jd * 16));
      const bf16x4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(ABF_LDS3(base + 16 * P + jd * 16));
      bf16x8_t b;
      b[0] = b0[0]; b[1] = b0[1]; b[2] = b0[2]; b[3] = b0[3];
      b[4] = b1[0]; b[5] = b1[1]; b[6] = b1[2]; b[7] = b1[3];
      o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, o[jd], 0, 0, 0);
    }
  }

  __device__ static __forceinline__ float dot_own(const Own& a, const Own& b) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < DH / 32; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) d += (float)a[s][e] * (float)b[s][e];
    return d;
  }

  static constexpr int kRowVec = 8;
  __device__ static __forceinline__ void lds_vec(const bf16_t* p, float (&v)[8]) { ElemTraits<bf16_t>::load8(p, v); }
  __device__ static __forceinline__ void glb_vec(const bf16_t* p, float (&v)[8]) { ElemTraits<bf16_t>::load8(p, v); }

  // s * scale - l may contract to one fma (F32Ops::prob of attention.hip says why that path rounds the product)
  __device__ static __forceinline__ float prob(float s, float scale, float l) { return __expf(s * scale - l); }
};

}  // namespace abf
