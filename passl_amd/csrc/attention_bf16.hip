// Fused short-sequence attention, bf16-MFMA operands; used when the activations are bf16 (entered from
// attention.hip).  attention_core.h has the algorithm, the reference call sites, the limits and the kernels
// themselves, attention_ops_bf16.h their operand policy Bf16Ops (shared with window_attention.hip); this file picks the
// number of waves.
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
#include "attention_ops_bf16.h"

namespace abf {

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
