// Fused multi-head self-attention for short ViT sequences (MAE: 50 / 197 tokens) on gfx950: the three kernels and
// their launches, written once over an operand policy `Ops` (attention.hip: exact-fp32 MFMA, attention_bf16.hip:
// bf16 MFMA) and the number of waves per workgroup `NW`.
//
// Reference: Attention.forward, passl_v110/modeling/backbones/mae.py:141-155 (= passl/models/
// vision_transformer.py:142-156):  softmax(q k^T * d^-0.5) v  per (image, head), q/k/v sliced from
// the fused qkv projection [B, T, 3, H, d].  The T x T score matrix never reaches HBM.
//
// One workgroup per (image, head).  The whole K and V (backward sweep 2: Q and dO) of the head live in LDS as
// Ops::lds_t [T_pad][Ops::P]; a wave owns 16 query rows (or 16 key columns) at a time.  Scores come from a
// "swapped" MFMA (A-operand = swept tile, B-operand = own tile) so that a lane holds 4 scores of ONE own row per
// 16-wide tile: row max / sum are in-lane plus two wave shuffles (lanes l, l^16, l^32 share a row).  The probability
// tile is then already in the A-operand layout of the second MFMA (P x V, dS x K, P^T x dO, dS^T x Q), which takes
// Ops::kStep tiles at a time.
// Backward = two sweeps: own query rows x swept keys -> dQ;  own key columns x swept queries -> dK, dV (P is
// recomputed from the saved row log-sum-exp by Ops::prob; delta_i = dO_i . O_i).
// `causal` (CLIP text tower, passl_v110/modeling/backbones/clip.py:284-286: additive triu(-inf, 1)
// mask): key j is visible to query i iff j <= i; fully masked tiles are skipped.
// Limits: d in {32, 64}, T <= 208 (13 tiles) — the MAE pre-training shapes; larger T takes the
// KV-tiled (flash-style) variant of attention_tiled.hip.
//
// Ops supplies
//   elem_t, lds_t        element type in memory and in LDS
//   DH, P                head dimension and LDS row pitch (in lds_t)
//   kStep                tiles per accumulate step (1 or 2); T_pad is a multiple of 16 * kStep
//   kMaxTiles, kMaxRows  tile count padded to a multiple of kStep, and 16 * kMaxTiles
//   Own                  a lane's fragment of an own row (an array type)
//   fwd_waves_per_eu(NW) second argument of the forward's __launch_bounds__ (0 = none)
//   kAccumByLane         accum takes the whole lane, not (l15, l4)
//   kSelectProb          dQ sweep: form prob for every lane and select (the tile stays one basic block and the
//                        MFMA chains of its two scores interleave) rather than branch around it
//   stage<NTH>           rows rows.row(0 .. Tn - 1) of a strided matrix -> LDS [Tpad][P]; rows >= Tn are zero.  `rows` maps
//                        a token to its row: SameRows here, the window's row numbers in window_attention.hip
//   load_own             fragment of an own row from global memory, zero when invalid
//   dot                  acc[r] = own[row l15] . swept[row tile*16 + 4*l4 + r]
//   accum                o[own = 4*l4' + r'][d = jd*16 + l15] += sum over the 16 * kStep rows of tiles [t0, t0 + kStep)
//                        of coef(own l15, row) * M[row][d];  c[u][r] = the lane's coefficient for row 4*l4 + r of tile
//                        t0 + u.  Called with (l15, l4), or with the whole lane if kAccumByLane (see ATTN_ACCUM)
//   dot_own              the lane's share of own_a . own_b
//   kRowVec, lds_vec,    the delta prologue of the dK / dV sweep reads kRowVec channels of a dO row in LDS and of an O row
//   glb_vec              in memory at a time, as fp32
//   prob(s, scale, l)    exp(s * scale - l)
#pragma once
#include <type_traits>
#include "common.h"
#include "options.h"

namespace attn {

constexpr float kNeg = -1e30f;
constexpr int kMaxTokens = 208;        // 13 tiles

__device__ __forceinline__ float shx(float v, int m) { return __shfl_xor(v, m, 64); }

// element (b, t, which, h, 0) of qkv [B, T, 3, H, DH]
template <int DH>
__device__ __forceinline__ int64_t qkv_off(int b, int t, int which, int h, int Tn, int H) {
  return ((((int64_t)b * Tn + t) * 3 + which) * H + h) * DH;
}

// Tn rounded up to whole accumulate steps
template <class Ops>
__host__ __device__ __forceinline__ int pad_rows(int Tn) {
  constexpr int SH = Ops::kStep > 1 ? 5 : 4;
  return ((Tn + (1 << SH) - 1) >> SH) << SH;
}

// dynamic LDS of a launch at Tn tokens; `stats`: plus lse[Tpad] and delta[Tpad] of the dK / dV sweep
template <class Ops>
constexpr int lds_bytes(int Tpad, bool stats) {
  return 2 * Tpad * Ops::P * (int)sizeof(typename Ops::lds_t) + (stats ? 2 * Tpad * 4 : 0);
}
// the cap set for every kernel of a policy: the dK / dV sweep's, the largest
template <class Ops>
constexpr int max_lds() { return lds_bytes<Ops>(Ops::kMaxRows, true); }

// the row map of tokens that lie where they are counted
struct SameRows {
  __device__ __forceinline__ int row(int t) const { return t; }
};

// Ops::accum, handed the kernel's `lane` or its `l15`, `l4`, whichever the policy's address arithmetic is written in:
// naming the other one as well, even unused, reorders the instructions of every kernel of that policy
#define ATTN_ACCUM(c, lds, t0, o)                                     \
  do {                                                                \
    if constexpr (Ops::kAccumByLane) Ops::accum(c, lds, t0, lane, o); \
    else Ops::accum(c, lds, t0, l15, l4, o);                          \
  } while (0)

// ------------------------------------------------------------------ forward
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64, Ops::fwd_waves_per_eu(NW)) attn_fwd_kernel(
    const typename Ops::elem_t* __restrict__ qkv, typename Ops::elem_t* __restrict__ out, float* __restrict__ lse,
    int Tn, int H, float scale, int causal) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep, kMaxTiles = Ops::kMaxTiles;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + Tpad * P;
  const int64_t rs = (int64_t)3 * H * DH;
  Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, 0, 1, h, Tn, H), rs, SameRows{}, Tn, Tpad, Ks);
  Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, 0, 2, h, Tn, H), rs, SameRows{}, Tn, Tpad, Vs);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (int rb = wave; rb < nt; rb += NW) {
    const int row = rb * 16 + l15;
    typename Ops::Own q;
    Ops::load_own(qkv + qkv_off<DH>(b, row < Tn ? row : 0, 0, h, Tn, H), row < Tn, l4, q);
    float s[kMaxTiles][4];
    float m = kNeg;
    const int ntc = causal ? rb + 1 : nt;        // causal: key tiles beyond the diagonal are all masked
    const int lim = causal ? min(row, Tn - 1) : Tn - 1;   // last visible key of this query row
#pragma unroll
    for (int ct = 0; ct < kMaxTiles; ++ct) {
      if (ct < ntc) {
        const f32x4 a = Ops::dot(Ks, ct, q, l15, l4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[ct][r] = (ct * 16 + l4 * 4 + r <= lim) ? a[r] * scale : kNeg;
          m = fmaxf(m, s[ct][r]);
        }
      } else if constexpr (kStep > 1) {          // the slot may be the second tile of a step
#pragma unroll
        for (int r = 0; r < 4; ++r) s[ct][r] = kNeg;
      }
    }
    m = fmaxf(m, shx(m, 16));
    m = fmaxf(m, shx(m, 32));
    float z = 0.f;
#pragma unroll
    for (int ct = 0; ct < kMaxTiles; ++ct)
      if (ct < ntc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[ct][r] = __expf(s[ct][r] - m); z += s[ct][r]; }
      } else if constexpr (kStep > 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[ct][r] = 0.f;
      }
    z += shx(z, 16);
    z += shx(z, 32);
    const float inv = 1.0f / z;
    f32x4 o[DH / 16];
#pragma unroll
    for (int jd = 0; jd < DH / 16; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cp = 0; cp < kMaxTiles / kStep; ++cp)
      if (kStep * cp < ntc) {
        float p[kStep][4];
#pragma unroll
        for (int u = 0; u < kStep; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) p[u][r] = s[kStep * cp + u][r] * inv;
        ATTN_ACCUM(p, Vs, kStep * cp, o);
      }
    if (row < Tn && l4 == 0) lse[((int64_t)b * H + h) * Tn + row] = m + __logf(z);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = rb * 16 + l4 * 4 + r;
      if (orow < Tn) {
        T* op = out + (((int64_t)b * Tn + orow) * H + h) * DH + l15;
#pragma unroll
        for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, o[jd][r]);
      }
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 1: dQ
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) attn_bwd_q_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dqkv, int Tn, int H, float scale, int causal) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + Tpad * P;
  const int64_t rs = (int64_t)3 * H * DH;
  Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, 0, 1, h, Tn, H), rs, SameRows{}, Tn, Tpad, Ks);
  Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, 0, 2, h, Tn, H), rs, SameRows{}, Tn, Tpad, Vs);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (int rb = wave; rb < nt; rb += NW) {
    const int row = rb * 16 + l15;
    const bool rv = row < Tn;
    const int rr = rv ? row : 0;
    typename Ops::Own q, dor, orw;
    Ops::load_own(qkv + qkv_off<DH>(b, rr, 0, h, Tn, H), rv, l4, q);
    const int64_t oo = (((int64_t)b * Tn + rr) * H + h) * DH;
    Ops::load_own(dout + oo, rv, l4, dor);
    Ops::load_own(out + oo, rv, l4, orw);
    float delta = Ops::dot_own(dor, orw);
    delta += shx(delta, 16);
    delta += shx(delta, 32);
    const float l = rv ? lse[((int64_t)b * H + h) * Tn + row] : 0.f;
    f32x4 dq[DH / 16];
#pragma unroll
    for (int jd = 0; jd < DH / 16; ++jd) dq[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntc = causal ? rb + 1 : nt;
    const int lim = causal ? min(row, Tn - 1) : Tn - 1;
    for (int cp = 0; kStep * cp < ntc; ++cp) {
      float ds[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int ct = kStep * cp + u;
        if (kStep == 1 || ct < ntc) {
          const f32x4 s = Ops::dot(Ks, ct, q, l15, l4), dp = Ops::dot(Vs, ct, dor, l15, l4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool cv = rv && (ct * 16 + l4 * 4 + r <= lim);
            float p;
            if constexpr (Ops::kSelectProb) {
              const float e = Ops::prob(s[r], scale, l);
              p = cv ? e : 0.f;
            } else {
              p = cv ? Ops::prob(s[r], scale, l) : 0.f;
            }
            ds[u][r] = p * (dp[r] - delta) * scale;
          }
        } else {                                 // no second tile in the last step
#pragma unroll
          for (int r = 0; r < 4; ++r) ds[u][r] = 0.f;
        }
      }
      ATTN_ACCUM(ds, Ks, kStep * cp, dq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = rb * 16 + l4 * 4 + r;
      if (orow < Tn) {
        T* op = dqkv + qkv_off<DH>(b, orow, 0, h, Tn, H) + l15;
#pragma unroll
        for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, dq[jd][r]);
      }
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 2: dK, dV
template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64) attn_bwd_kv_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const typename Ops::elem_t* __restrict__ out,
    const typename Ops::elem_t* __restrict__ dout, const float* __restrict__ lse,
    typename Ops::elem_t* __restrict__ dqkv, int Tn, int H, float scale, int causal) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  L* Qs = reinterpret_cast<L*>(smem);
  L* Ds = Qs + Tpad * P;                                         // dO
  float* Ls = reinterpret_cast<float*>(Qs + 2 * Tpad * P);       // lse[Tpad]
  float* Dl = Ls + Tpad;                                         // delta[Tpad]
  Ops::template stage<NW * 64>(qkv + qkv_off<DH>(b, 0, 0, h, Tn, H), (int64_t)3 * H * DH, SameRows{}, Tn, Tpad, Qs);
  Ops::template stage<NW * 64>(dout + (((int64_t)b * Tn) * H + h) * DH, (int64_t)H * DH, SameRows{}, Tn, Tpad, Ds);
  __syncthreads();
  for (int t = threadIdx.x; t < Tpad; t += NW * 64) {
    float d = 0.f, l = 0.f;
    if (t < Tn) {
      constexpr int V = Ops::kRowVec;                          // delta_t = dO_t . O_t
      const T* op = out + (((int64_t)b * Tn + t) * H + h) * DH;
#pragma unroll
      for (int c = 0; c < DH; c += V) {
        float a[V], o[V];
        Ops::lds_vec(Ds + t * P + c, a);
        Ops::glb_vec(op + c, o);
#pragma unroll
        for (int e = 0; e < V; ++e) d += a[e] * o[e];
      }
      l = lse[((int64_t)b * H + h) * Tn + t];
    }
    Ls[t] = l;
    Dl[t] = d;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int ntp = Tpad >> 4;                                     // a multiple of kStep
  for (int cb = wave; cb < nt; cb += NW) {
    const int col = cb * 16 + l15;
    const bool cv = col < Tn;
    typename Ops::Own kown, vown;
    Ops::load_own(qkv + qkv_off<DH>(b, cv ? col : 0, 1, h, Tn, H), cv, l4, kown);
    Ops::load_own(qkv + qkv_off<DH>(b, cv ? col : 0, 2, h, Tn, H), cv, l4, vown);
    f32x4 dk[DH / 16], dv[DH / 16];
#pragma unroll
    for (int jd = 0; jd < DH / 16; ++jd) { dk[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int rp = causal ? (cb >> (kStep - 1)) : 0; kStep * rp < ntp; ++rp) {   // causal: rows before the key see nothing
      float p[kStep][4], ds[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int rt = kStep * rp + u;
        const f32x4 s = Ops::dot(Qs, rt, kown, l15, l4), dp = Ops::dot(Ds, rt, vown, l15, l4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + l4 * 4 + r;
          const bool ok = cv && row < Tn && (!causal || row >= col);
          p[u][r] = ok ? Ops::prob(s[r], scale, Ls[row]) : 0.f;
          ds[u][r] = p[u][r] * (dp[r] - Dl[row]) * scale;
        }
      }
      ATTN_ACCUM(p, Ds, kStep * rp, dv);
      ATTN_ACCUM(ds, Qs, kStep * rp, dk);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ocol = cb * 16 + l4 * 4 + r;
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
}

// ------------------------------------------------------------------ launches
// one sweep: `groups` workgroups of NW waves with `lds` bytes of dynamic LDS; the kernel's cap is raised to `cap` once
template <auto Kernel, int NW, class... A>
int launch_sweep(int groups, int lds, int cap, hipStream_t st, A... a) {
  static bool capped = false;
  if (!capped) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    capped = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(groups), dim3(NW * 64), lds, st, a...);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

template <class Ops, int NW>
int launch_fwd(const void* qkv, void* out, float* lse, int B, int Tn, int H, float scale, int causal,
               hipStream_t st) {
  using T = typename Ops::elem_t;
  return launch_sweep<&attn_fwd_kernel<Ops, NW>, NW>(B * H, lds_bytes<Ops>(pad_rows<Ops>(Tn), false), max_lds<Ops>(), st,
                                                    reinterpret_cast<const T*>(qkv), reinterpret_cast<T*>(out), lse, Tn,
                                                    H, scale, causal);
}

template <class Ops, int NW>
int launch_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B,
               int Tn, int H, float scale, int causal, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int Tpad = pad_rows<Ops>(Tn);
  const T *q = reinterpret_cast<const T*>(qkv), *o = reinterpret_cast<const T*>(out), *d = reinterpret_cast<const T*>(dout);
  const int rc = launch_sweep<&attn_bwd_q_kernel<Ops, NW>, NW>(B * H, lds_bytes<Ops>(Tpad, false), max_lds<Ops>(), st, q, o,
                                                                d, lse, reinterpret_cast<T*>(dqkv), Tn, H, scale, causal);
  if (rc != PASSL_OK) return rc;
  return launch_sweep<&attn_bwd_kv_kernel<Ops, NW>, NW>(B * H, lds_bytes<Ops>(Tpad, true), max_lds<Ops>(), st, q, o, d, lse,
                                                         reinterpret_cast<T*>(dqkv), Tn, H, scale, causal);
}

// f(std::integral_constant<int, DH>) for the two head dimensions the kernels are built for
template <typename F>
int by_head_dim(int DH, F f) {
  return DH == 64 ? f(std::integral_constant<int, 64>{}) : f(std::integral_constant<int, 32>{});
}

#undef ATTN_ACCUM

}  // namespace attn
