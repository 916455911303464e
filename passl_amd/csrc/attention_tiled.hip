// Key-tiled (flash-style) multi-head self-attention for sequences of up to 1024 tokens on gfx950, and the two entry
// points of the C ABI.  attention_core.h keeps a head's whole K and V in LDS and stops at 208 tokens; these kernels
// stream blocks of kBlock = 64 swept rows through LDS instead, so the footprint does not grow with T.
//
// Reference: Attention.forward, passl/models/vision_transformer.py:142-156 (= passl/models/deit.py through its
// import):  softmax(q k^T * d^-0.5) v  per (image, head), q/k/v sliced from the fused qkv projection [B, T, 3, H, d]
// at 577 / 578 tokens (DeiT at 384 pixels).  No causal flag and no key bias: nothing beyond 208 tokens needs them.
//
// The operand policies are those of the dense kernels, unchanged: F32Ops (attention_ops_f32.h, exact-fp32 MFMA) for
// fp32 activations and for bf16 activations that are not 16-byte aligned, Bf16Ops (attention_ops_bf16.h) for aligned
// bf16.  Their stage / dot / accum see one block of 64 rows [kBlock][Ops::P] where the dense kernels hand them the
// whole head.  The tiling of a wave is that of attention_core.h: a wave owns 16 query rows (16 key columns), a lane
// holds 4 scores of ONE own row per 16-wide tile.
//
// Forward.  One workgroup of NW waves per (image, head, block of 16 NW query rows); the K and V blocks of the head
// pass through LDS one after the other (single buffer: several workgroups per CU overlap one's staging with another's
// MFMAs).  Online softmax in fp32 per own row: running max m, running sum z, accumulator o.  Per block
//   m' = max(m, block max),  alpha = exp(m - m'),  p = exp(s - m'),  z = z alpha + sum p,  o = o alpha + p V,
// and out = o / z, lse = m + log z at the end.  p is the operand of p V (the bf16 policy rounds it there, and only
// there); alpha and 1 / z belong to the row of lane l15 and are fetched by shuffle for the accumulator's rows 4 l4 + r.
//
// Backward = the two sweeps of attention_core.h with a block loop inside:
//   dQ:      own query rows against streamed K and V blocks;
//   dK, dV:  own key columns against streamed Q and dO blocks, with lse and delta_i = dO_i . O_i of the block's rows
//            in LDS (delta is formed again by every workgroup: no workspace).
// P is recomputed from the saved lse by Ops::prob.  No atomics, no scratch, no workspace: every output element has
// one writer and a fixed order of sums, two launches give the same bits.
//
// Limits: d in {32, 64}, 1 <= T <= 1024.
#include "attention_core.h"
#include "attention_ops_bf16.h"
#include "attention_ops_f32.h"

namespace atile {

using attn::kNeg;
using attn::qkv_off;
using attn::SameRows;
using attn::shx;

constexpr int kMaxTokens = 1024;
constexpr int kBlock = 64;             // swept rows per LDS block: 4 tiles, whole accumulate steps of both policies
constexpr int kTiles = kBlock / 16;

// two [kBlock][P] operand blocks; `stats`: plus lse[kBlock] and delta[kBlock] of the dK / dV sweep
template <class Ops>
constexpr int lds_bytes(bool stats) {
  return 2 * kBlock * Ops::P * (int)sizeof(typename Ops::lds_t) + (stats ? 2 * kBlock * 4 : 0);
}

#define ATILE_ACCUM(c, lds, t0, o)                                    \
  do {                                                                \
    if constexpr (Ops::kAccumByLane) Ops::accum(c, lds, t0, lane, o); \
    else Ops::accum(c, lds, t0, l15, l4, o);                          \
  } while (0)

// workgroup -> (image, head, own block)
__device__ __forceinline__ void decode(int nob, int H, int& b, int& h, int& ob) {
  ob = blockIdx.x % nob;
  const int bh = blockIdx.x / nob;
  b = bh / H;
  h = bh % H;
}

// ------------------------------------------------------------------ forward
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) tiled_fwd_kernel(
    const typename Ops::elem_t* __restrict__ qkv, typename Ops::elem_t* __restrict__ out, float* __restrict__ lse,
    int Tn, int H, int nob, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + kBlock * P;
  const int64_t rs = (int64_t)3 * H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int row0 = (ob * NW + wave) * 16, row = row0 + l15;
  typename Ops::Own q;
  Ops::load_own(qkv + qkv_off<DH>(b, row < Tn ? row : 0, 0, h, Tn, H), row < Tn, l4, q);
  float m = kNeg, z = 0.f;
  f32x4 o[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Tn; k0 += kBlock) {
    const int n = min(kBlock, Tn - k0);            // keys of this block; the rows beyond are staged as zeros
    __syncthreads();                               // the previous block has been read by every wave
    Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, k0, 1, h, Tn, H), rs, SameRows{}, n, kBlock, Ks);
    Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, k0, 2, h, Tn, H), rs, SameRows{}, n, kBlock, Vs);
    __syncthreads();
    float s[kTiles][4];
    float bm = kNeg;
#pragma unroll
    for (int ct = 0; ct < kTiles; ++ct) {
      const f32x4 a = Ops::dot(Ks, ct, q, l15, l4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[ct][r] = (ct * 16 + l4 * 4 + r < n) ? a[r] * scale : kNeg;   // a padding key is not a key with score 0
        bm = fmaxf(bm, s[ct][r]);
      }
    }
    bm = fmaxf(bm, shx(bm, 16));
    bm = fmaxf(bm, shx(bm, 32));
    const float mn = fmaxf(m, bm);
    const float alpha = __expf(m - mn);            // 0 at the first block (m = kNeg), 1 while the max stands
    m = mn;
    float bz = 0.f;
#pragma unroll
    for (int ct = 0; ct < kTiles; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) { s[ct][r] = __expf(s[ct][r] - m); bz += s[ct][r]; }
    bz += shx(bz, 16);
    bz += shx(bz, 32);
    z = z * alpha + bz;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ar = __shfl(alpha, 4 * l4 + r, 64);                  // the accumulator's row 4 l4 + r
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) o[jd][r] *= ar;
    }
#pragma unroll
    for (int cp = 0; cp < kTiles / kStep; ++cp) {
      float p[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) p[u][r] = s[kStep * cp + u][r];
      ATILE_ACCUM(p, Vs, kStep * cp, o);
    }
  }
  if (row < Tn && l4 == 0) lse[((int64_t)b * H + h) * Tn + row] = m + __logf(z);
  const float inv = 1.0f / z;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * l4 + r, 64);
    const int orow = row0 + l4 * 4 + r;
    if (orow < Tn) {
      T* op = out + (((int64_t)b * Tn + orow) * H + h) * DH + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, o[jd][r] * ir);
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 1: dQ
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) tiled_bwd_q_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dqkv, int Tn, int H, int nob, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + kBlock * P;
  const int64_t rs = (int64_t)3 * H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int row0 = (ob * NW + wave) * 16, row = row0 + l15;
  const bool rv = row < Tn;
  const int rr = rv ? row : 0;
  typename Ops::Own q, dor;
  float delta;
  {
    typename Ops::Own orw;
    Ops::load_own(qkv + qkv_off<DH>(b, rr, 0, h, Tn, H), rv, l4, q);
    const int64_t oo = (((int64_t)b * Tn + rr) * H + h) * DH;
    Ops::load_own(dout + oo, rv, l4, dor);
    Ops::load_own(out + oo, rv, l4, orw);
    delta = Ops::dot_own(dor, orw);
  }
  delta += shx(delta, 16);
  delta += shx(delta, 32);
  const float l = rv ? lse[((int64_t)b * H + h) * Tn + row] : 0.f;
  f32x4 dq[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) dq[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Tn; k0 += kBlock) {
    const int n = min(kBlock, Tn - k0);
    __syncthreads();
    Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, k0, 1, h, Tn, H), rs, SameRows{}, n, kBlock, Ks);
    Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, k0, 2, h, Tn, H), rs, SameRows{}, n, kBlock, Vs);
    __syncthreads();
#pragma unroll
    for (int cp = 0; cp < kTiles / kStep; ++cp) {
      float ds[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int ct = kStep * cp + u;
        const f32x4 s = Ops::dot(Ks, ct, q, l15, l4), dp = Ops::dot(Vs, ct, dor, l15, l4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool cv = rv && (ct * 16 + l4 * 4 + r < n);
          const float e = Ops::prob(s[r], scale, l);
          const float p = cv ? e : 0.f;
          ds[u][r] = p * (dp[r] - delta) * scale;
        }
      }
      ATILE_ACCUM(ds, Ks, kStep * cp, dq);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = row0 + l4 * 4 + r;
    if (orow < Tn) {
      T* op = dqkv + qkv_off<DH>(b, orow, 0, h, Tn, H) + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, dq[jd][r]);
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 2: dK, dV
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) tiled_bwd_kv_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dqkv, int Tn, int H, int nob, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  constexpr int kPart = DH / 4;                                  // channels of a row's delta per thread: 4 threads a row
  static_assert(kPart % Ops::kRowVec == 0, "a quarter row is whole vectors");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Qs = reinterpret_cast<L*>(smem);
  L* Ds = Qs + kBlock * P;                                       // dO
  float* Ls = reinterpret_cast<float*>(Qs + 2 * kBlock * P);     // lse[kBlock]
  float* Dl = Ls + kBlock;                                       // delta[kBlock]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int col0 = (ob * NW + wave) * 16, col = col0 + l15;
  const bool cv = col < Tn;
  typename Ops::Own kown, vown;
  Ops::load_own(qkv + qkv_off<DH>(b, cv ? col : 0, 1, h, Tn, H), cv, l4, kown);
  Ops::load_own(qkv + qkv_off<DH>(b, cv ? col : 0, 2, h, Tn, H), cv, l4, vown);
  f32x4 dk[DH / 16], dv[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) { dk[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int st_row = threadIdx.x >> 2, st_part = threadIdx.x & 3;  // delta prologue: threads 0 .. 4 kBlock - 1
  for (int r0 = 0; r0 < Tn; r0 += kBlock) {
    const int n = min(kBlock, Tn - r0);
    // this thread's quarter of an O row, in flight while the block is staged
    float ov[kPart];
    float lv = 0.f;
    const bool sv = st_row < n;                                  // st_row < kBlock follows: n <= kBlock
    if (sv) {
      constexpr int V = Ops::kRowVec;
      const T* op = out + (((int64_t)b * Tn + r0 + st_row) * H + h) * DH + st_part * kPart;
#pragma unroll
      for (int c = 0; c < kPart; c += V) {
        float t[V];
        Ops::glb_vec(op + c, t);
#pragma unroll
        for (int e = 0; e < V; ++e) ov[c + e] = t[e];
      }
      if (st_part == 0) lv = lse[((int64_t)b * H + h) * Tn + r0 + st_row];
    } else {
#pragma unroll
      for (int c = 0; c < kPart; ++c) ov[c] = 0.f;
    }
    __syncthreads();
    Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, r0, 0, h, Tn, H), (int64_t)3 * H * DH, SameRows{}, n, kBlock, Qs);
    Ops::template stage<NW * 64>(dout + (((int64_t)b * Tn + r0) * H + h) * DH, (int64_t)H * DH, SameRows{}, n, kBlock, Ds);
    __syncthreads();
    if (threadIdx.x < 4 * kBlock) {                              // whole waves: the shuffles stay among active lanes
      constexpr int V = Ops::kRowVec;
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < kPart; c += V) {
        float a[V];
        Ops::lds_vec(Ds + st_row * P + st_part * kPart + c, a);  // zero rows beyond n
#pragma unroll
        for (int e = 0; e < V; ++e) d += a[e] * ov[c + e];
      }
      d += shx(d, 1);
      d += shx(d, 2);
      if (st_part == 0) { Ls[st_row] = lv; Dl[st_row] = d; }
    }
    __syncthreads();
#pragma unroll
    for (int rp = 0; rp < kTiles / kStep; ++rp) {
      float p[kStep][4], ds[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int rt = kStep * rp + u;
        const f32x4 s = Ops::dot(Qs, rt, kown, l15, l4), dp = Ops::dot(Ds, rt, vown, l15, l4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = rt * 16 + l4 * 4 + r;
          const bool ok = cv && lr < n;
          p[u][r] = ok ? Ops::prob(s[r], scale, Ls[lr]) : 0.f;
          ds[u][r] = p[u][r] * (dp[r] - Dl[lr]) * scale;
        }
      }
      ATILE_ACCUM(p, Ds, kStep * rp, dv);
      ATILE_ACCUM(ds, Qs, kStep * rp, dk);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ocol = col0 + l4 * 4 + r;
    if (ocol < Tn) {
      T* kp = dqkv + qkv_off<DH>(b, ocol, 1, h, Tn, H) + l15;
      T* vp = dqkv + qkv_off<DH>(b, ocol, 2, h, Tn, H) + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) {
        ElemTraits<T>::st(kp + jd * 16, dk[jd][r]);
        ElemTraits<T>::st(vp + jd * 16, dv[jd][r]);
      }
    }
  }
}

#undef ATILE_ACCUM

// ------------------------------------------------------------------ launches
// workgroups of a sweep: (image, head, block of 16 NW own rows)
template <int NW>
int own_blocks(int Tn) { return (Tn + 16 * NW - 1) / (16 * NW); }

template <class Ops, int NW>
int launch_fwd(const void* qkv, void* out, float* lse, int B, int Tn, int H, float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int nob = own_blocks<NW>(Tn);
  return attn::launch_sweep<&tiled_fwd_kernel<Ops, NW>, NW>(B * H * nob, lds_bytes<Ops>(false), lds_bytes<Ops>(true), st,
                                                            reinterpret_cast<const T*>(qkv), reinterpret_cast<T*>(out),
                                                            lse, Tn, H, nob, scale);
}

template <class Ops, int NW>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int Tn, int H,
               float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int nob = own_blocks<NW>(Tn);
  const T *q = reinterpret_cast<const T*>(qkv), *o = reinterpret_cast<const T*>(out), *d = reinterpret_cast<const T*>(dout);
  const int rc = attn::launch_sweep<&tiled_bwd_q_kernel<Ops, NW>, NW>(B * H * nob, lds_bytes<Ops>(false),
                                                                      lds_bytes<Ops>(true), st, q, o, d, lse,
                                                                      reinterpret_cast<T*>(dqkv), Tn, H, nob, scale);
  if (rc != PASSL_OK) return rc;
  return attn::launch_sweep<&tiled_bwd_kv_kernel<Ops, NW>, NW>(B * H * nob, lds_bytes<Ops>(true), lds_bytes<Ops>(true), st,
                                                               q, o, d, lse, reinterpret_cast<T*>(dqkv), Tn, H, nob, scale);
}

// waves per workgroup: the bf16 policy's MFMAs are short next to the staging of a block, so 128 own rows share one
// staged block; the exact-fp32 policy keeps 4 waves (its dQ and dK / dV sweeps hold more registers per wave)
constexpr int kWavesBf16 = 8, kWavesF32 = 4;
static_assert(4 * kBlock <= kWavesF32 * 64, "the delta prologue of the dK / dV sweep needs 4 threads per block row");

// PASSL_OK, or the status the entry points return without launching
int check_shape(int B, int Tn, int H, int DH) {
  if (B <= 0 || H <= 0 || Tn <= 0 || Tn > kMaxTokens || (DH != 32 && DH != 64)) return PASSL_EUNSUPPORTED;
  if ((int64_t)B * H * own_blocks<kWavesF32>(Tn) > INT32_MAX) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

}  // namespace atile

extern "C" int passl_hip_attention_tiled_fwd(const void* qkv, void* out, float* lse, int B, int T_, int H, int DH,
                                             float scale, int dtype, passl_stream_t stream) {
  if (!qkv || !out || !lse) return PASSL_EINVAL;
  const int rc = atile::check_shape(B, T_, H, DH);
  if (rc != PASSL_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && aligned16(qkv) && aligned16(out))
    return attn::by_head_dim(DH, [&](auto dh) {
      return atile::launch_fwd<abf::Bf16Ops<decltype(dh)::value>, atile::kWavesBf16>(qkv, out, lse, B, T_, H, scale, st);
    });
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return atile::launch_fwd<af32::F32Ops<T, decltype(dh)::value>, atile::kWavesF32>(qkv, out, lse, B, T_, H, scale, st);
  });)
}

extern "C" int passl_hip_attention_tiled_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                                             void* dqkv, int B, int T_, int H, int DH, float scale, int dtype,
                                             passl_stream_t stream) {
  if (!qkv || !out || !dout || !lse || !dqkv) return PASSL_EINVAL;
  const int rc = atile::check_shape(B, T_, H, DH);
  if (rc != PASSL_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv))
    return attn::by_head_dim(DH, [&](auto dh) {
      return atile::launch_bwd<abf::Bf16Ops<decltype(dh)::value>, atile::kWavesBf16>(qkv, out, dout, lse, dqkv, B, T_, H,
                                                                                      scale, st);
    });
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return atile::launch_bwd<af32::F32Ops<T, decltype(dh)::value>, atile::kWavesF32>(qkv, out, dout, lse, dqkv, B, T_, H,
                                                                                      scale, st);
  });)
}
