// Fused short-sequence attention, exact-fp32-MFMA operands, and the two entry points of the C ABI.
// attention_core.h has the algorithm, the reference call sites, the limits and the kernels themselves,
// attention_ops_f32.h their operand policy F32Ops (shared with window_attention.hip); this file checks shapes and picks
// the path.
//
// LDS holds fp32 rows [T_pad][d + 4] (bf16 inputs are converted when staged); every product is
// v_mfma_f32_16x16x4_f32, one tile per accumulate step.  These kernels serve fp32 activations (the parity dtype)
// and bf16 activations that are not 16-byte aligned or are routed here by option attn_f32mfma; aligned bf16
// activations take the bf16-MFMA kernels of attention_bf16.hip.
#include "attention_core.h"
#include "attention_ops_f32.h"

// attention_bf16.hip: bf16-MFMA kernels for bf16 activations
int passl_attn_bf16_fwd(const void* qkv, void* out, float* lse, int B, int Tn, int H, int DH, float scale,
                        int causal, hipStream_t st);
int passl_attn_bf16_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                        int B, int Tn, int H, int DH, float scale, int causal, hipStream_t st);

using af32::F32Ops;

namespace {

// option attn_f32mfma = 1 routes bf16 activations through the exact-fp32-MFMA kernels (A/B runs)
bool use_bf16_mfma() { return !passl_opt(Opt::attn_f32mfma); }

constexpr int kWaves = 4;

bool shape_ok(int B, int Tn, int H, int DH) {
  return B > 0 && H > 0 && Tn > 0 && Tn <= attn::kMaxTokens && (DH == 32 || DH == 64);
}

}  // namespace

extern "C" int passl_hip_attention_fwd(const void* qkv, void* out, float* lse, int B, int T_, int H,
                                       int DH, float scale, int causal, int dtype, passl_stream_t stream) {
  if (!qkv || !out || !lse) return PASSL_EINVAL;
  if (!shape_ok(B, T_, H, DH)) return PASSL_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && use_bf16_mfma() && aligned16(qkv) && aligned16(out))
    return passl_attn_bf16_fwd(qkv, out, lse, B, T_, H, DH, scale, causal, st);
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return attn::launch_fwd<F32Ops<T, decltype(dh)::value>, kWaves>(qkv, out, lse, B, T_, H, scale, causal, st);
  });)
}

extern "C" int passl_hip_attention_bwd(const void* qkv, const void* out, const void* dout,
                                       const float* lse, void* dqkv, int B, int T_, int H, int DH,
                                       float scale, int causal, int dtype, passl_stream_t stream) {
  if (!qkv || !out || !dout || !lse || !dqkv) return PASSL_EINVAL;
  if (!shape_ok(B, T_, H, DH)) return PASSL_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && use_bf16_mfma() && aligned16(qkv) && aligned16(out) && aligned16(dout) &&
      aligned16(dqkv))
    return passl_attn_bf16_bwd(qkv, out, dout, lse, dqkv, B, T_, H, DH, scale, causal, st);
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return attn::launch_bwd<F32Ops<T, decltype(dh)::value>, kWaves>(qkv, out, dout, lse, dqkv, B, T_, H, scale, causal,
                                                                     st);
  });)
}
