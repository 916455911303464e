// Key-tiled multi-head CROSS-attention on gfx950: q, k and v are three tensors and the number of queries differs from
// the number of keys.  The two entry points of the C ABI and their three kernels.
//
// Reference: CAECrossAttention.forward, passl/models/cae.py:244-257: q = Linear_q(x_q), k = Linear_k(LN_k(x_kv + pos)),
// v = Linear_v(LN_v(x_kv)), softmax(q k^T * d^-0.5) v per (image, head), at Tq = 75 masked-patch queries against
// Tk = 196 keys in the latent regressor of CAE pre-training.  No causal flag, no key bias.
//
// The kernels are those of attention_tiled.hip with separate operands and lengths: q, out, dout, dq are
// [B, Tq, H, d], k, v, dk, dv are [B, Tk, H, d] (row stride H d where the fused qkv has 3 H d), lse is fp32 [B, H, Tq].
// The operand policies are the dense kernels', unchanged: F32Ops (attention_ops_f32.h, exact-fp32 MFMA) for fp32
// activations and for bf16 activations that are not 16-byte aligned, Bf16Ops (attention_ops_bf16.h) for aligned bf16.
// A wave owns 16 query rows (16 key columns), a lane holds 4 scores of ONE own row per 16-wide tile; blocks of
// kBlock = 64 swept rows pass through LDS.
//
// Forward.  One workgroup of NW waves per (image, head, block of 16 NW query rows); the head's Tk keys and values are
// streamed under the fp32 online softmax of attention_tiled.hip (running max m, running sum z, accumulator o rescaled
// when the max rises; out = o / z, lse = m + log z).  A padding key of the last block is not a key.
// Backward = two sweeps:
//   dQ:      own query rows (Tq of them) against streamed K and V blocks (Tk rows);
//   dK, dV:  own key columns (Tk of them) against streamed Q and dO blocks (Tq rows), with lse and
//            delta_i = dO_i . O_i of the block's query rows in LDS.
// P is recomputed from the saved lse by Ops::prob.  No atomics, no scratch, no workspace: every output element has one
// writer and a fixed order of sums, two launches give the same bits.  With Tq = Tk and q, k, v the slices of one qkv the
// arithmetic of a row is attention_tiled.hip's, operation for operation.
//
// Waves per workgroup: attention_tiled.hip's, 8 for the bf16 policy (128 own rows share a staged block) and 4 for the
// exact-fp32 policy.  A wave whose 16 own rows lie beyond the end still stages and sweeps; a 5-wave workgroup (80 rows:
// the 75 queries of CAE with nothing idle) was built and measured against this one at Tq = 75, Tk = 196 and lost (forward
// 37.9 against 36.3 us, backward 141.5 against 104.0 us: its dK / dV sweep stages every Q / dO block for a third
// workgroup), so it is not kept.  A row's result does not depend on the number of waves.
//
// Limits: d in {32, 64}, 1 <= Tq <= 1024, 1 <= Tk <= 1024.
#include "attention_core.h"
#include "attention_ops_bf16.h"
#include "attention_ops_f32.h"

namespace xattn {

using attn::kNeg;
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

#define XATTN_ACCUM(c, lds, t0, o)                                    \
  do {                                                                \
    if constexpr (Ops::kAccumByLane) Ops::accum(c, lds, t0, lane, o); \
    else Ops::accum(c, lds, t0, l15, l4, o);                          \
  } while (0)

// element (b, t, h, 0) of a token tensor [B, Tn, H, DH]
template <int DH>
__device__ __forceinline__ int64_t tok_off(int b, int t, int h, int Tn, int H) {
  return (((int64_t)b * Tn + t) * H + h) * DH;
}

// workgroup -> (image, head, own block)
__device__ __forceinline__ void decode(int nob, int H, int& b, int& h, int& ob) {
  ob = blockIdx.x % nob;
  const int bh = blockIdx.x / nob;
  b = bh / H;
  h = bh % H;
}

// ------------------------------------------------------------------ forward
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) cross_fwd_kernel(
    const typename Ops::elem_t* __restrict__ qp, const typename Ops::elem_t* __restrict__ kp,
    const typename Ops::elem_t* __restrict__ vp, typename Ops::elem_t* __restrict__ out, float* __restrict__ lse,
    int Tq, int Tk, int H, int nob, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + kBlock * P;
  const int64_t rs = (int64_t)H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int row0 = (ob * NW + wave) * 16, row = row0 + l15;
  typename Ops::Own q;
  Ops::load_own(qp + tok_off<DH>(b, row < Tq ? row : 0, h, Tq, H), row < Tq, l4, q);
  float m = kNeg, z = 0.f;
  f32x4 o[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Tk; k0 += kBlock) {
    const int n = min(kBlock, Tk - k0);            // keys of this block; the rows beyond are staged as zeros
    __syncthreads();                               // the previous block has been read by every wave
    Ops::template stage<NW * 64>(kp + tok_off<DH>(b, k0, h, Tk, H), rs, SameRows{}, n, kBlock, Ks);
    Ops::template stage<NW * 64>(vp + tok_off<DH>(b, k0, h, Tk, H), rs, SameRows{}, n, kBlock, Vs);
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
      XATTN_ACCUM(p, Vs, kStep * cp, o);
    }
  }
  if (row < Tq && l4 == 0) lse[((int64_t)b * H + h) * Tq + row] = m + __logf(z);
  const float inv = 1.0f / z;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float ir = __shfl(inv, 4 * l4 + r, 64);
    const int orow = row0 + l4 * 4 + r;
    if (orow < Tq) {
      T* op = out + tok_off<DH>(b, orow, h, Tq, H) + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, o[jd][r] * ir);
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 1: dQ
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) cross_bwd_q_kernel(
    const typename Ops::elem_t* __restrict__ qp, const typename Ops::elem_t* __restrict__ kp,
    const typename Ops::elem_t* __restrict__ vp, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dqp, int Tq, int Tk, int H, int nob, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + kBlock * P;
  const int64_t rs = (int64_t)H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int row0 = (ob * NW + wave) * 16, row = row0 + l15;
  const bool rv = row < Tq;
  const int rr = rv ? row : 0;
  typename Ops::Own q, dor;
  float delta;
  {
    typename Ops::Own orw;
    const int64_t oo = tok_off<DH>(b, rr, h, Tq, H);
    Ops::load_own(qp + oo, rv, l4, q);
    Ops::load_own(dout + oo, rv, l4, dor);
    Ops::load_own(out + oo, rv, l4, orw);
    delta = Ops::dot_own(dor, orw);
  }
  delta += shx(delta, 16);
  delta += shx(delta, 32);
  const float l = rv ? lse[((int64_t)b * H + h) * Tq + row] : 0.f;
  f32x4 dq[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) dq[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < Tk; k0 += kBlock) {
    const int n = min(kBlock, Tk - k0);
    __syncthreads();
    Ops::template stage<NW * 64>(kp + tok_off<DH>(b, k0, h, Tk, H), rs, SameRows{}, n, kBlock, Ks);
    Ops::template stage<NW * 64>(vp + tok_off<DH>(b, k0, h, Tk, H), rs, SameRows{}, n, kBlock, Vs);
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
      XATTN_ACCUM(ds, Ks, kStep * cp, dq);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = row0 + l4 * 4 + r;
    if (orow < Tq) {
      T* op = dqp + tok_off<DH>(b, orow, h, Tq, H) + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, dq[jd][r]);
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 2: dK, dV
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) cross_bwd_kv_kernel(
    const typename Ops::elem_t* __restrict__ qp, const typename Ops::elem_t* __restrict__ kp,
    const typename Ops::elem_t* __restrict__ vp, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dkp, typename Ops::elem_t* __restrict__ dvp, int Tq, int Tk, int H, int nob,
    float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  constexpr int kPart = DH / 4;                                  // channels of a row's delta per thread: 4 threads a row
  static_assert(kPart % Ops::kRowVec == 0, "a quarter row is whole vectors");
  static_assert(4 * kBlock <= NW * 64, "the delta prologue needs 4 threads per block row");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int b, h, ob;
  decode(nob, H, b, h, ob);
  L* Qs = reinterpret_cast<L*>(smem);
  L* Ds = Qs + kBlock * P;                                       // dO
  float* Ls = reinterpret_cast<float*>(Qs + 2 * kBlock * P);     // lse[kBlock]
  float* Dl = Ls + kBlock;                                       // delta[kBlock]
  const int64_t rs = (int64_t)H * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int col0 = (ob * NW + wave) * 16, col = col0 + l15;
  const bool cv = col < Tk;
  typename Ops::Own kown, vown;
  Ops::load_own(kp + tok_off<DH>(b, cv ? col : 0, h, Tk, H), cv, l4, kown);
  Ops::load_own(vp + tok_off<DH>(b, cv ? col : 0, h, Tk, H), cv, l4, vown);
  f32x4 dk[DH / 16], dv[DH / 16];
#pragma unroll
  for (int jd = 0; jd < DH / 16; ++jd) { dk[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int st_row = threadIdx.x >> 2, st_part = threadIdx.x & 3;  // delta prologue: threads 0 .. 4 kBlock - 1
  for (int r0 = 0; r0 < Tq; r0 += kBlock) {                      // the swept side is the queries
    const int n = min(kBlock, Tq - r0);
    // this thread's quarter of an O row, in flight while the block is staged
    float ov[kPart];
    float lv = 0.f;
    const bool sv = st_row < n;                                  // st_row < kBlock follows: n <= kBlock
    if (sv) {
      constexpr int V = Ops::kRowVec;
      const T* op = out + tok_off<DH>(b, r0 + st_row, h, Tq, H) + st_part * kPart;
#pragma unroll
      for (int c = 0; c < kPart; c += V) {
        float t[V];
        Ops::glb_vec(op + c, t);
#pragma unroll
        for (int e = 0; e < V; ++e) ov[c + e] = t[e];
      }
      if (st_part == 0) lv = lse[((int64_t)b * H + h) * Tq + r0 + st_row];
    } else {
#pragma unroll
      for (int c = 0; c < kPart; ++c) ov[c] = 0.f;
    }
    __syncthreads();
    Ops::template stage<NW * 64>(qp + tok_off<DH>(b, r0, h, Tq, H), rs, SameRows{}, n, kBlock, Qs);
    Ops::template stage<NW * 64>(dout + tok_off<DH>(b, r0, h, Tq, H), rs, SameRows{}, n, kBlock, Ds);
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
      XATTN_ACCUM(p, Ds, kStep * rp, dv);
      XATTN_ACCUM(ds, Qs, kStep * rp, dk);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ocol = col0 + l4 * 4 + r;
    if (ocol < Tk) {
      T* ko = dkp + tok_off<DH>(b, ocol, h, Tk, H) + l15;
      T* vo = dvp + tok_off<DH>(b, ocol, h, Tk, H) + l15;
#pragma unroll
      for (int jd = 0; jd < DH / 16; ++jd) {
        ElemTraits<T>::st(ko + jd * 16, dk[jd][r]);
        ElemTraits<T>::st(vo + jd * 16, dv[jd][r]);
      }
    }
  }
}

#undef XATTN_ACCUM

// ------------------------------------------------------------------ launches
// workgroups of a sweep over `rows` own rows: (image, head, block of 16 NW own rows)
constexpr int own_blocks(int rows, int nw) { return (rows + 16 * nw - 1) / (16 * nw); }

template <class Ops, int NW>
int launch_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int Tq, int Tk, int H,
               float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int nob = own_blocks(Tq, NW);
  return attn::launch_sweep<&cross_fwd_kernel<Ops, NW>, NW>(
      B * H * nob, lds_bytes<Ops>(false), lds_bytes<Ops>(true), st, reinterpret_cast<const T*>(q),
      reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), reinterpret_cast<T*>(out), lse, Tq, Tk, H, nob, scale);
}

template <class Ops, int NW>
int launch_bwd_q(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                 void* dq, int B, int Tq, int Tk, int H, float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int nob = own_blocks(Tq, NW);
  return attn::launch_sweep<&cross_bwd_q_kernel<Ops, NW>, NW>(
      B * H * nob, lds_bytes<Ops>(false), lds_bytes<Ops>(true), st, reinterpret_cast<const T*>(q),
      reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), reinterpret_cast<const T*>(out),
      reinterpret_cast<const T*>(dout), lse, reinterpret_cast<T*>(dq), Tq, Tk, H, nob, scale);
}

template <class Ops, int NW>
int launch_bwd_kv(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse,
                  void* dk, void* dv, int B, int Tq, int Tk, int H, float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int nob = own_blocks(Tk, NW);
  return attn::launch_sweep<&cross_bwd_kv_kernel<Ops, NW>, NW>(
      B * H * nob, lds_bytes<Ops>(true), lds_bytes<Ops>(true), st, reinterpret_cast<const T*>(q),
      reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), reinterpret_cast<const T*>(out),
      reinterpret_cast<const T*>(dout), lse, reinterpret_cast<T*>(dk), reinterpret_cast<T*>(dv), Tq, Tk, H, nob, scale);
}

// waves per workgroup (see the head of the file)
constexpr int kWavesBf16 = 8, kWavesF32 = 4;

// PASSL_OK, or the status the entry points return without launching
int check_shape(int B, int Tq, int Tk, int H, int DH) {
  if (B <= 0 || H <= 0 || Tq <= 0 || Tq > kMaxTokens || Tk <= 0 || Tk > kMaxTokens || (DH != 32 && DH != 64))
    return PASSL_EUNSUPPORTED;
  if ((int64_t)B * H * own_blocks(Tq > Tk ? Tq : Tk, kWavesF32) > INT32_MAX) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

}  // namespace xattn

extern "C" int passl_hip_cross_attention_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B,
                                             int Tq, int Tk, int H, int DH, float scale, int dtype,
                                             passl_stream_t stream) {
  if (!q || !k || !v || !out || !lse) return PASSL_EINVAL;
  const int rc = xattn::check_shape(B, Tq, Tk, H, DH);
  if (rc != PASSL_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out))
    return attn::by_head_dim(DH, [&](auto dh) {
      return xattn::launch_fwd<abf::Bf16Ops<decltype(dh)::value>, xattn::kWavesBf16>(q, k, v, out, lse, B, Tq, Tk, H,
                                                                                     scale, st);
    });
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return xattn::launch_fwd<af32::F32Ops<T, decltype(dh)::value>, xattn::kWavesF32>(q, k, v, out, lse, B, Tq, Tk, H,
                                                                                     scale, st);
  });)
}

extern "C" int passl_hip_cross_attention_bwd(const void* q, const void* k, const void* v, const void* out,
                                             const void* dout, const float* lse, void* dq, void* dk, void* dv, int B,
                                             int Tq, int Tk, int H, int DH, float scale, int dtype,
                                             passl_stream_t stream) {
  if (!q || !k || !v || !out || !dout || !lse || !dq || !dk || !dv) return PASSL_EINVAL;
  const int rc = xattn::check_shape(B, Tq, Tk, H, DH);
  if (rc != PASSL_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (dtype == PASSL_BF16 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) &&
      aligned16(dq) && aligned16(dk) && aligned16(dv))
    return attn::by_head_dim(DH, [&](auto dh) {
      using Ops = abf::Bf16Ops<decltype(dh)::value>;
      const int r1 = xattn::launch_bwd_q<Ops, xattn::kWavesBf16>(q, k, v, out, dout, lse, dq, B, Tq, Tk, H, scale, st);
      if (r1 != PASSL_OK) return r1;
      return xattn::launch_bwd_kv<Ops, xattn::kWavesBf16>(q, k, v, out, dout, lse, dk, dv, B, Tq, Tk, H, scale, st);
    });
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    using Ops = af32::F32Ops<T, decltype(dh)::value>;
    const int r1 = xattn::launch_bwd_q<Ops, xattn::kWavesF32>(q, k, v, out, dout, lse, dq, B, Tq, Tk, H, scale, st);
    if (r1 != PASSL_OK) return r1;
    return xattn::launch_bwd_kv<Ops, xattn::kWavesF32>(q, k, v, out, dout, lse, dk, dv, B, Tq, Tk, H, scale, st);
  });)
}
