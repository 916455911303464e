// Fused short-sequence attention, bf16-MFMA operands; used when the activations are bf16 (entered from
// attention.hip).  attention_core.h has the algorithm, the reference call sites, the limits and the kernels
// themselves; this file supplies their operand policy Bf16Ops and picks the number of waves.
//
// The operands stay bf16:
//   * LDS holds bf16 rows [T_pad32][d + 8] (16-byte padded pitch): half the footprint of the fp32
//     staging, 2 workgroups per CU;
//   * scores S^T = K Q^T and dP^T = V dO^T: v_mfma_f32_16x16x32_bf16, A-operand = one ds_read_b128
//     per 32 channels of the swept row, B-operand = the own row's 16-byte global loads;
//   * P V, dS K, P^T dO, dS^T Q: the lane's 2 x 4 fp32 coefficients of a PAIR of tiles are packed
//     to one bf16x8 A-operand (k-slot e < 4 <-> row 4*l4 + e of the first tile, e >= 4 <-> the
//     second); the B-operand comes from the row-major LDS tile through two ds_read_b64_tr_b16
//     (transposing reads: a 16-lane group fetches a [4 rows][16 channels] block and lane i
//     receives channel i of the 4 rows) — no transposed copy of V / K / dO / Q is ever made.
// Softmax statistics, exp, delta and all accumulators are fp32; P and dS are rounded to bf16 only
// as MFMA operands.  8x fewer MFMA issue slots than the exact-fp32 kernels.
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

  template <int NTH>
  __device__ static __forceinline__ void stage(const bf16_t* __restrict__ base, int64_t rs, int Tn, int Tpad,
                                               bf16_t* lds) {
    constexpr int CH = DH / 8;
    for (int i = threadIdx.x; i < Tpad * CH; i += NTH) {
      const int r = i / CH, c = (i % CH) * 8;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r < Tn) v = *reinterpret_cast<const uint4*>(base + (int64_t)r * rs + c);
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

// NW = waves per workgroup: a head with >= 8 row tiles (T > 112) gets 8 waves — its K / V staging (64 KB at
// T = 197, d = 64) allows only 2 workgroups per CU, and 8 waves per CU cannot hide the global-load latency of the
// per-tile query fragments; shorter sequences keep 4 (more workgroups per CU fit anyway).
// option attn_waves = 4 / 8 forces the workgroup size (A/B runs); default: 8 waves from 8 row tiles on
inline bool eight_waves(int Tn, bool backward) {
  const int forced = passl_opt(Opt::attn_waves);
  if (forced == 4) return false;
  if (forced == 8) return true;
  // measured (profiles/r03_attention_waves.txt; repeat with tools/attention_bench.py --time --waves 4|8): the forward
  // gains from 8 waves at every benchmark shape (faster staging even when half the waves have no row tile), the
  // backward only from 8 row tiles on
  return backward ? (Tn + 15) / 16 >= 8 : true;
}

}  // namespace abf

// entry points used by attention.hip (shapes already validated there); 16-byte aligned rows required
int passl_attn_bf16_fwd(const void* qkv, void* out, float* lse, int B, int Tn, int H, int DH, float scale,
                        int causal, hipStream_t st) {
  const bool wide = abf::eight_waves(Tn, false);
  return attn::by_head_dim(DH, [&](auto dh) {
    using Ops = abf::Bf16Ops<decltype(dh)::value>;
    return wide ? attn::launch_fwd<Ops, 8>(qkv, out, lse, B, Tn, H, scale, causal, st)
                : attn::launch_fwd<Ops, 4>(qkv, out, lse, B, Tn, H, scale, causal, st);
  });
}

int passl_attn_bf16_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                        int B, int Tn, int H, int DH, float scale, int causal, hipStream_t st) {
  const bool wide = abf::eight_waves(Tn, true);
  return attn::by_head_dim(DH, [&](auto dh) {
    using Ops = abf::Bf16Ops<decltype(dh)::value>;
    return wide ? attn::launch_bwd<Ops, 8>(qkv, out, dout, lse, dqkv, B, Tn, H, scale, causal, st)
                : attn::launch_bwd<Ops, 4>(qkv, out, dout, lse, dqkv, B, Tn, H, scale, causal, st);
  });
}
