// Swin Transformer kernels for gfx950: shifted-window attention with a relative-position bias, and patch merging.
//
// Reference: WindowAttention.forward, passl/models/swin_transformer.py:112-200, and the roll / window_partition /
// attn_mask / window_reverse / roll of SwinTransformerBlock.forward :291-340; PatchMerging.forward :343-384.
//
// Window attention.  The kernels are the three of attention_core.h (same operand policies and, through a row map, the
// same Ops::stage; same MFMA tiling, same softmax in registers; launched by attn::launch_sweep) with two changes.  They
// are a second copy of the sweeps and not a policy of the first: DESIGN 33 has what was tried and what it did to the
// dense kernels' code.
//   * Tokens are addressed, not moved.  qkv [B, Hp*Wp, 3, nH, DH] is the projection of the unshifted, unpartitioned
//     map.  Token i = (iy, ix) of window (wy, wx) is row ((wy ws + iy + shift) mod Hp) Wp + ((wx ws + ix + shift) mod Wp)
//     of its image: roll(-shift), window_partition, window_reverse and roll(+shift) never run.  A window's row numbers
//     are computed once into LDS; staging, the own-row loads and the stores go through them.
//   * score = (q . k) scale + table[(iy - jy + ws - 1)(2 ws - 1) + (ix - jx + ws - 1), h] + mask, all fp32.  With a
//     shift, mask = -100 where the region labels of i and j differ (label = 3 r(y, Hp) + r(x, Wp) of the position in
//     the shifted map, r(y, n) = 0 below n - ws, 1 below n - shift, else 2).  Each token carries one word in LDS,
//     code = iy (2 ws - 1) + ix in the low half and its label in the high half: the bias index of a pair is
//     code_q - code_k + const, the mask one compare.  The head's table column lies in LDS.
//     The forward and both backward sweeps form the score by the same rounded operations (score()), so the
//     recomputed P = exp(score - lse) is the forward's.
// Table gradient: dtable[r, h] = sum of dS = P (dP - delta) over every image, window and pair with index r, taken from
// the fp32 dS before it is rounded to an MFMA operand.  No atomics: the dQ sweep runs as `slabs` workgroups per head,
// workgroup s walks windows s, s + slabs, ... and keeps the dS tiles of its waves in registers across them, then
// writes one dense [T, T] partial.  Two small launches add the partials in slab order and fold [nH, T, T] into
// the table, each bin in a fixed pair order: two runs give the same bits.
// NT = compile-time bound on the number of 16-row tiles (4, 9 = ws up to 12, 13 = ws up to 14), NW = waves per workgroup: a wave owns at most
// ceil(NT / NW) row tiles, which bounds the registers of the kept dS tiles.
//
// Patch merging: out[b, y, x, k C + c] = in[b, 2 y + (k & 1), 2 x + (k >> 1), c], a bijection moved in 16-byte pieces.
#include <type_traits>
#include "attention_core.h"
#include "attention_ops_f32.h"
#include "attention_ops_bf16.h"

namespace wattn {

using attn::kNeg;
using attn::pad_rows;
using attn::shx;

constexpr int kMaxWindow = 14;          // T = 196 <= attn::kMaxTokens
constexpr float kMask = -100.f;

struct Geo {
  int Hp, Wp, ws, shift, nH, nWx, nW;   // nWx windows per row of windows, nW per image
};

// NT tiles rounded up to whole accumulate steps
template <class Ops>
constexpr int padded_tiles(int NT) { return (NT + Ops::kStep - 1) / Ops::kStep * Ops::kStep; }

// main region of attention_core.h, then rows[Tpad], tok[Tpad], table column [(2 ws - 1)^2]
template <class Ops>
constexpr int lds_total(int Tpad, bool stats, int ws) {
  return attn::lds_bytes<Ops>(Tpad, stats) + 2 * Tpad * 4 + (2 * ws - 1) * (2 * ws - 1) * 4;
}

// (a * scale) + bm with both roundings: the forward and the backward sweeps must agree bit for bit
__device__ __forceinline__ float score(float a, float scale, float bm) {
#pragma clang fp contract(off)
  return a * scale + bm;
}

__device__ __forceinline__ int region(int y, int n, int ws, int shift) { return y < n - ws ? 0 : (y < n - shift ? 1 : 2); }

// bias + mask of (query word tq, key word tk); k0 = (ws - 1)(2 ws - 1) + ws - 1
__device__ __forceinline__ float bias_mask(int tq, int tk, int k0, const float* tb) {
  return tb[(tq & 0xffff) - (tk & 0xffff) + k0] + ((tq >> 16) != (tk >> 16) ? kMask : 0.f);
}

template <int NTH>
__device__ __forceinline__ void load_table(const float* __restrict__ table, const Geo& g, int h, float* tb) {
  const int nb = (2 * g.ws - 1) * (2 * g.ws - 1);
  for (int i = threadIdx.x; i < nb; i += NTH) tb[i] = table[(int64_t)i * g.nH + h];
}

// rows[t] = row of token t in its image (0 for t >= Tn), tok[t] = code | label << 16
template <int NTH>
__device__ __forceinline__ void window_tokens(const Geo& g, int w, int Tn, int Tpad, int* rows, int* tok) {
  const int wy = w / g.nWx, wx = w % g.nWx, D = 2 * g.ws - 1;
  for (int t = threadIdx.x; t < Tpad; t += NTH) {
    int ri = 0, tk = 0;
    if (t < Tn) {
      const int iy = t / g.ws, ix = t % g.ws;
      const int y = wy * g.ws + iy, x = wx * g.ws + ix;
      int gy = y + g.shift, gx = x + g.shift;
      if (gy >= g.Hp) gy -= g.Hp;
      if (gx >= g.Wp) gx -= g.Wp;
      ri = gy * g.Wp + gx;
      const int label = g.shift > 0 ? 3 * region(y, g.Hp, g.ws, g.shift) + region(x, g.Wp, g.ws, g.shift) : 0;
      tk = (iy * D + ix) | (label << 16);
    }
    rows[t] = ri;
    tok[t] = tk;
  }
}

// Ops::stage's row map of a window: token t lies in row rows[t] of its image
struct Rows {
  const int* rows;
  __device__ __forceinline__ int row(int t) const { return rows[t]; }
};

template <class Ops, class Coef>
__device__ __forceinline__ void accum(const Coef& c, const typename Ops::lds_t* lds, int t0, int lane,
                                      f32x4 (&o)[Ops::DH / 16]) {
  if constexpr (Ops::kAccumByLane) Ops::accum(c, lds, t0, lane, o);
  else Ops::accum(c, lds, t0, lane & 15, lane >> 4, o);
}

// ------------------------------------------------------------------ forward: one workgroup per (window, head)
template <class Ops, int NW, int NT>
__global__ void __launch_bounds__(NW * 64) wattn_fwd_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const float* __restrict__ table,
    typename Ops::elem_t* __restrict__ out, float* __restrict__ lse, Geo g, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep, NTP = padded_tiles<Ops>(NT);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int h = blockIdx.x % g.nH, win = blockIdx.x / g.nH;
  const int b = win / g.nW, w = win % g.nW;
  const int Tn = g.ws * g.ws, nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  const int k0 = (g.ws - 1) * (2 * g.ws - 1) + g.ws - 1;
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + Tpad * P;
  int* rows = reinterpret_cast<int*>(smem + attn::lds_bytes<Ops>(Tpad, false));
  int* tok = rows + Tpad;
  float* tb = reinterpret_cast<float*>(tok + Tpad);
  window_tokens<NW * 64>(g, w, Tn, Tpad, rows, tok);
  load_table<NW * 64>(table, g, h, tb);
  __syncthreads();
  const int64_t rs = (int64_t)3 * g.nH * DH;
  const int64_t Limg = (int64_t)g.Hp * g.Wp;
  const T* img = qkv + (int64_t)b * Limg * rs + h * DH;
  Ops::template stage<NW * 64>(img + g.nH * DH, rs, Rows{rows}, Tn, Tpad, Ks);
  Ops::template stage<NW * 64>(img + 2 * g.nH * DH, rs, Rows{rows}, Tn, Tpad, Vs);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (int rb = wave; rb < nt; rb += NW) {
    const int row = rb * 16 + l15;
    typename Ops::Own q;
    Ops::load_own(img + (int64_t)rows[row] * rs, row < Tn, l4, q);
    const int tq = tok[row];
    float s[NTP][4];
    float m = kNeg;
#pragma unroll
    for (int ct = 0; ct < NTP; ++ct) {
      if (ct < nt) {
        const f32x4 a = Ops::dot(Ks, ct, q, l15, l4);
        const int4 tk = *reinterpret_cast<const int4*>(tok + ct * 16 + l4 * 4);
        const int tks[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[ct][r] = (ct * 16 + l4 * 4 + r < Tn) ? score(a[r], scale, bias_mask(tq, tks[r], k0, tb)) : kNeg;
          m = fmaxf(m, s[ct][r]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[ct][r] = kNeg;
      }
    }
    m = fmaxf(m, shx(m, 16));
    m = fmaxf(m, shx(m, 32));
    float z = 0.f;
#pragma unroll
    for (int ct = 0; ct < NTP; ++ct)
      if (ct < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[ct][r] = __expf(s[ct][r] - m); z += s[ct][r]; }
      } else {
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
    for (int cp = 0; cp < NTP / kStep; ++cp)
      if (kStep * cp < nt) {
        float p[kStep][4];
#pragma unroll
        for (int u = 0; u < kStep; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) p[u][r] = s[kStep * cp + u][r] * inv;
        accum<Ops>(p, Vs, kStep * cp, lane, o);
      }
    if (row < Tn && l4 == 0) lse[(int64_t)blockIdx.x * Tn + row] = m + __logf(z);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = rb * 16 + l4 * 4 + r;
      if (orow < Tn) {
        T* op = out + ((b * Limg + rows[orow]) * g.nH + h) * DH + l15;
#pragma unroll
        for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, o[jd][r]);
      }
    }
  }
}

// ------------------------------------------------------------------ backward, sweep 1: dQ and the dS partial
// grid = slabs * nH; workgroup (s, h) walks windows s, s + slabs, ... of head h
template <class Ops, int NW, int NT>
__global__ void __launch_bounds__(NW * 64) wattn_bwd_q_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const float* __restrict__ table,
    const typename Ops::elem_t* __restrict__ out, const typename Ops::elem_t* __restrict__ dout,
    const float* __restrict__ lse, typename Ops::elem_t* __restrict__ dqkv, float* __restrict__ part, Geo g,
    int windows, int slabs, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep, NTP = padded_tiles<Ops>(NT);
  constexpr int RB = (NT + NW - 1) / NW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int h = blockIdx.x % g.nH, slab = blockIdx.x / g.nH;
  const int Tn = g.ws * g.ws, nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  const int k0 = (g.ws - 1) * (2 * g.ws - 1) + g.ws - 1;
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + Tpad * P;
  int* rows = reinterpret_cast<int*>(smem + attn::lds_bytes<Ops>(Tpad, false));
  int* tok = rows + Tpad;
  float* tb = reinterpret_cast<float*>(tok + Tpad);
  load_table<NW * 64>(table, g, h, tb);
  const int64_t rs = (int64_t)3 * g.nH * DH;
  const int64_t Limg = (int64_t)g.Hp * g.Wp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  float acc[RB][NT][4];
#pragma unroll
  for (int k = 0; k < RB; ++k)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[k][ct][r] = 0.f;
  for (int win = slab; win < windows; win += slabs) {
    const int b = win / g.nW, w = win % g.nW;
    __syncthreads();                               // the waves are done with the window before
    window_tokens<NW * 64>(g, w, Tn, Tpad, rows, tok);
    __syncthreads();
    const T* img = qkv + (int64_t)b * Limg * rs + h * DH;
    Ops::template stage<NW * 64>(img + g.nH * DH, rs, Rows{rows}, Tn, Tpad, Ks);
    Ops::template stage<NW * 64>(img + 2 * g.nH * DH, rs, Rows{rows}, Tn, Tpad, Vs);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RB; ++k) {
      const int rb = wave + k * NW;
      if (rb < nt) {
        const int row = rb * 16 + l15;
        const bool rv = row < Tn;
        typename Ops::Own q, dor, orw;
        Ops::load_own(img + (int64_t)rows[row] * rs, rv, l4, q);
        const int64_t oo = ((b * Limg + rows[row]) * g.nH + h) * DH;
        Ops::load_own(dout + oo, rv, l4, dor);
        Ops::load_own(out + oo, rv, l4, orw);
        float delta = Ops::dot_own(dor, orw);
        delta += shx(delta, 16);
        delta += shx(delta, 32);
        const float l = rv ? lse[((int64_t)win * g.nH + h) * Tn + row] : 0.f;
        const int tq = tok[row];
        f32x4 dq[DH / 16];
#pragma unroll
        for (int jd = 0; jd < DH / 16; ++jd) dq[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cp = 0; cp < NTP / kStep; ++cp)
          if (kStep * cp < nt) {
            float ds[kStep][4];
#pragma unroll
            for (int u = 0; u < kStep; ++u) {
              const int ct = kStep * cp + u;
              if (ct < NT && (kStep == 1 || ct < nt)) {
                const f32x4 s = Ops::dot(Ks, ct, q, l15, l4), dp = Ops::dot(Vs, ct, dor, l15, l4);
                const int4 tk = *reinterpret_cast<const int4*>(tok + ct * 16 + l4 * 4);
                const int tks[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const bool cv = rv && (ct * 16 + l4 * 4 + r < Tn);
                  const float e = __expf(score(s[r], scale, bias_mask(tq, tks[r], k0, tb)) - l);
                  const float d = (cv ? e : 0.f) * (dp[r] - delta);
                  acc[k][ct][r] += d;              // fp32 dS: the table's gradient
                  ds[u][r] = d * scale;
                }
              } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) ds[u][r] = 0.f;
              }
            }
            accum<Ops>(ds, Ks, kStep * cp, lane, dq);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int orow = rb * 16 + l4 * 4 + r;
          if (orow < Tn) {
            T* op = dqkv + (b * Limg + rows[orow]) * rs + h * DH + l15;
#pragma unroll
            for (int jd = 0; jd < DH / 16; ++jd) ElemTraits<T>::st(op + jd * 16, dq[jd][r]);
          }
        }
      }
    }
  }
  float* pp = part + ((int64_t)slab * g.nH + h) * Tn * Tn;
#pragma unroll
  for (int k = 0; k < RB; ++k) {
    const int row = (wave + k * NW) * 16 + l15;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = ct * 16 + l4 * 4 + r;
        if (row < Tn && col < Tn) pp[row * Tn + col] = acc[k][ct][r];
      }
  }
}

// ------------------------------------------------------------------ backward, sweep 2: dK, dV per (window, head)
template <class Ops, int NW, int NT>
__global__ void __launch_bounds__(NW * 64) wattn_bwd_kv_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const float* __restrict__ table,
    const typename Ops::elem_t* __restrict__ out, const typename Ops::elem_t* __restrict__ dout,
    const float* __restrict__ lse, typename Ops::elem_t* __restrict__ dqkv, Geo g, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int h = blockIdx.x % g.nH, win = blockIdx.x / g.nH;
  const int b = win / g.nW, w = win % g.nW;
  const int Tn = g.ws * g.ws, nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  const int k0 = (g.ws - 1) * (2 * g.ws - 1) + g.ws - 1;
  L* Qs = reinterpret_cast<L*>(smem);
  L* Ds = Qs + Tpad * P;                                         // dO
  float* Ls = reinterpret_cast<float*>(Qs + 2 * Tpad * P);       // lse[Tpad]
  float* Dl = Ls + Tpad;                                         // delta[Tpad]
  int* rows = reinterpret_cast<int*>(smem + attn::lds_bytes<Ops>(Tpad, true));
  int* tok = rows + Tpad;
  float* tb = reinterpret_cast<float*>(tok + Tpad);
  window_tokens<NW * 64>(g, w, Tn, Tpad, rows, tok);
  load_table<NW * 64>(table, g, h, tb);
  __syncthreads();
  const int64_t rs = (int64_t)3 * g.nH * DH, os = (int64_t)g.nH * DH;
  const int64_t Limg = (int64_t)g.Hp * g.Wp;
  const T* img = qkv + (int64_t)b * Limg * rs + h * DH;
  const T* oimg = out + (int64_t)b * Limg * os + h * DH;
  Ops::template stage<NW * 64>(img, rs, Rows{rows}, Tn, Tpad, Qs);
  Ops::template stage<NW * 64>(dout + (int64_t)b * Limg * os + h * DH, os, Rows{rows}, Tn, Tpad, Ds);
  __syncthreads();
  for (int t = threadIdx.x; t < Tpad; t += NW * 64) {
    float d = 0.f, l = 0.f;
    if (t < Tn) {
      constexpr int V = Ops::kRowVec;                          // delta_t = dO_t . O_t
      const T* op = oimg + (int64_t)rows[t] * os;
#pragma unroll
      for (int c = 0; c < DH; c += V) {
        float a[V], o[V];
        Ops::lds_vec(Ds + t * P + c, a);
        Ops::glb_vec(op + c, o);
#pragma unroll
        for (int e = 0; e < V; ++e) d += a[e] * o[e];
      }
      l = lse[(int64_t)blockIdx.x * Tn + t];
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
    Ops::load_own(img + (int64_t)rows[col] * rs + g.nH * DH, cv, l4, kown);
    Ops::load_own(img + (int64_t)rows[col] * rs + 2 * g.nH * DH, cv, l4, vown);
    const int tkey = tok[col];
    f32x4 dk[DH / 16], dv[DH / 16];
#pragma unroll
    for (int jd = 0; jd < DH / 16; ++jd) { dk[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int rp = 0; kStep * rp < ntp; ++rp) {
      float p[kStep][4], ds[kStep][4];
#pragma unroll
      for (int u = 0; u < kStep; ++u) {
        const int rt = kStep * rp + u;
        const f32x4 s = Ops::dot(Qs, rt, kown, l15, l4), dp = Ops::dot(Ds, rt, vown, l15, l4);
        const int4 tq = *reinterpret_cast<const int4*>(tok + rt * 16 + l4 * 4);
        const int tqs[4] = {tq.x, tq.y, tq.z, tq.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + l4 * 4 + r;
          const bool ok = cv && row < Tn;
          const float e = __expf(score(s[r], scale, bias_mask(tqs[r], tkey, k0, tb)) - Ls[row]);
          p[u][r] = ok ? e : 0.f;
          ds[u][r] = p[u][r] * (dp[r] - Dl[row]) * scale;
        }
      }
      accum<Ops>(p, Ds, kStep * rp, lane, dv);
      accum<Ops>(ds, Qs, kStep * rp, lane, dk);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ocol = cb * 16 + l4 * 4 + r;
      if (ocol < Tn) {
        T* kp = dqkv + (b * Limg + rows[ocol]) * rs + g.nH * DH + h * DH + l15;
        T* vp = kp + g.nH * DH;
#pragma unroll
        for (int jd = 0; jd < DH / 16; ++jd) {
          ElemTraits<T>::st(kp + jd * 16, dk[jd][r]);
          ElemTraits<T>::st(vp + jd * 16, dv[jd][r]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ table gradient: slabs -> [nH, T, T] -> bins
// part[0] += part[1] + part[2] + ... in slab order, one thread per element
__global__ void __launch_bounds__(256) wattn_slab_sum_kernel(float* __restrict__ part, int64_t n, int slabs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = part[i];
  for (int s = 1; s < slabs; ++s) a += part[(int64_t)s * n + i];
  part[i] = a;
}

// dtable[r, h] = sum of dense[h, i, j] over the pairs with index r, keys in row-major order; one thread per bin
__global__ void __launch_bounds__(256) wattn_table_fold_kernel(const float* __restrict__ dense,
                                                               float* __restrict__ dtable, int ws, int nH) {
  const int D = 2 * ws - 1, Tn = ws * ws;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= D * D * nH) return;
  const int r = idx / nH, h = idx % nH;
  const int dy = r / D - (ws - 1), dx = r % D - (ws - 1);       // iy - jy, ix - jx
  const float* dh = dense + (int64_t)h * Tn * Tn;
  float a = 0.f;
  for (int jy = max(0, -dy); jy < min(ws, ws - dy); ++jy)
    for (int jx = max(0, -dx); jx < min(ws, ws - dx); ++jx)
      a += dh[((jy + dy) * ws + jx + dx) * Tn + jy * ws + jx];
  dtable[idx] = a;
}

// ------------------------------------------------------------------ launches
// workgroups per head of the dQ sweep: enough to fill the device, and at least two windows each where there are two
inline int table_slabs(int windows, int nH) { return PASSL_WINDOW_ATTENTION_SLABS(windows, nH); }

template <class Ops, int NW, int NT>
int launch_fwd(const void* qkv, const float* table, void* out, float* lse, int B, const Geo& g, float scale,
               hipStream_t st) {
  using T = typename Ops::elem_t;
  return attn::launch_sweep<&wattn_fwd_kernel<Ops, NW, NT>, NW>(
      B * g.nW * g.nH, lds_total<Ops>(pad_rows<Ops>(g.ws * g.ws), false, g.ws),
      lds_total<Ops>(padded_tiles<Ops>(NT) * 16, true, kMaxWindow), st, reinterpret_cast<const T*>(qkv), table,
      reinterpret_cast<T*>(out), lse, g, scale);
}

template <class Ops, int NW, int NT>
int launch_bwd(const void* qkv, const float* table, const void* out, const void* dout, const float* lse, void* dqkv,
               float* dtable, float* ws, int B, const Geo& g, float scale, hipStream_t st) {
  using T = typename Ops::elem_t;
  const int Tn = g.ws * g.ws, Tpad = pad_rows<Ops>(Tn), cap = lds_total<Ops>(padded_tiles<Ops>(NT) * 16, true, kMaxWindow);
  const int windows = B * g.nW, slabs = table_slabs(windows, g.nH);
  const T *q = reinterpret_cast<const T*>(qkv), *o = reinterpret_cast<const T*>(out), *d = reinterpret_cast<const T*>(dout);
  int rc = attn::launch_sweep<&wattn_bwd_q_kernel<Ops, NW, NT>, NW>(
      slabs * g.nH, lds_total<Ops>(Tpad, false, g.ws), cap, st, q, table, o, d, lse, reinterpret_cast<T*>(dqkv), ws, g,
      windows, slabs, scale);
  if (rc != PASSL_OK) return rc;
  rc = attn::launch_sweep<&wattn_bwd_kv_kernel<Ops, NW, NT>, NW>(
      windows * g.nH, lds_total<Ops>(Tpad, true, g.ws), cap, st, q, table, o, d, lse, reinterpret_cast<T*>(dqkv), g, scale);
  if (rc != PASSL_OK) return rc;
  const int64_t n = (int64_t)g.nH * Tn * Tn;
  if (slabs > 1) {
    hipLaunchKernelGGL(wattn_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, n, slabs);
    PASSL_RETURN_IF_LAUNCH_FAILED();
  }
  const int bins = (2 * g.ws - 1) * (2 * g.ws - 1) * g.nH;
  hipLaunchKernelGGL(wattn_table_fold_kernel, dim3((bins + 255) / 256), dim3(256), 0, st, ws, dtable, g.ws, g.nH);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

// f(NW, NT) for the tile count of T tokens: 4 waves own one row tile each up to T = 64, 8 waves two beyond
template <class Ops, typename F>
int by_tiles(int Tn, F f) {
  const int nt = (Tn + 15) >> 4;
  if (nt <= 4) return f(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
  if (nt <= 9) return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 9>{});
  return f(std::integral_constant<int, 8>{}, std::integral_constant<int, 13>{});
}

// PASSL_OK, or the status the entry points return without launching
int check_shape(int B, int Hp, int Wp, int ws, int shift, int nH, int DH, int dtype, Geo* g) {
  if (B <= 0 || Hp <= 0 || Wp <= 0 || nH <= 0 || ws <= 0 || shift < 0) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  if (ws > kMaxWindow || (DH != 32 && DH != 64)) return PASSL_EUNSUPPORTED;
  if (Hp % ws || Wp % ws || shift >= ws) return PASSL_EINVAL;
  if (shift > 0 && (Hp < Wp ? Hp : Wp) <= ws) return PASSL_EINVAL;
  const int64_t groups = (int64_t)B * (Hp / ws) * (Wp / ws) * nH;
  if (groups > INT32_MAX || (int64_t)Hp * Wp > INT32_MAX) return PASSL_EUNSUPPORTED;
  *g = Geo{Hp, Wp, ws, shift, nH, Wp / ws, (Hp / ws) * (Wp / ws)};
  return PASSL_OK;
}

// ------------------------------------------------------------------ patch merging
// FWD: y[b, oy, ox, k C + c] = x[b, 2 oy + (k & 1), 2 ox + (k >> 1), c]; !FWD: the same pairs, copied back
template <bool FWD>
__global__ void __launch_bounds__(256) patch_merge_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          int64_t n, int H, int W, int cv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // 16-byte piece of the merged tensor
  if (i >= n) return;
  const int c = (int)(i % cv);
  int64_t t = i / cv;
  const int k = (int)(t & 3);
  t >>= 2;
  const int W2 = W >> 1, H2 = H >> 1;
  const int ox = (int)(t % W2);
  t /= W2;
  const int oy = (int)(t % H2);
  const int64_t b = t / H2;
  const int64_t j = ((b * H + 2 * oy + (k & 1)) * W + 2 * ox + (k >> 1)) * cv + c;
  if (FWD) dst[i] = src[j];
  else dst[j] = src[i];
}

template <bool FWD>
int patch_merge(const void* src, void* dst, int B, int H, int W, int C, int dtype, hipStream_t st) {
  if (!src || !dst) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (H & 1) || (W & 1) || C % 8) return PASSL_EINVAL;
  if (!aligned16(src) || !aligned16(dst)) return PASSL_EINVAL;
  const int cv = C / (dtype == PASSL_BF16 ? 8 : 4);
  const int64_t n = (int64_t)B * H * W * cv;
  if ((n + 255) / 256 > INT32_MAX) return PASSL_EUNSUPPORTED;
  hipLaunchKernelGGL(patch_merge_kernel<FWD>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n, H, W, cv);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

}  // namespace wattn

// fp32 activations: exact-fp32 MFMA; bf16 activations: bf16 MFMA (16-byte aligned rows, as every arena tensor has)
#define WATTN_DISPATCH(dtype, DH, Tn, ...)                                                        \
  if ((dtype) == PASSL_BF16) {                                                                    \
    return attn::by_head_dim(DH, [&](auto dh) {                                                   \
      using Ops = abf::Bf16Ops<decltype(dh)::value>;                                              \
      return wattn::by_tiles<Ops>(Tn, [&](auto nw, auto ntl) {                                    \
        constexpr int NW = decltype(nw)::value, NT = decltype(ntl)::value;                        \
        __VA_ARGS__                                                                               \
      });                                                                                         \
    });                                                                                           \
  }                                                                                               \
  return attn::by_head_dim(DH, [&](auto dh) {                                                     \
    using Ops = af32::F32Ops<float, decltype(dh)::value>;                                         \
    return wattn::by_tiles<Ops>(Tn, [&](auto nw, auto ntl) {                                      \
      constexpr int NW = decltype(nw)::value, NT = decltype(ntl)::value;                          \
      __VA_ARGS__                                                                                 \
    });                                                                                           \
  });

extern "C" int passl_hip_window_attention_fwd(const void* qkv, const float* table, void* out, float* lse, int B,
                                              int Hp, int Wp, int ws, int shift, int nH, int DH, float scale,
                                              int dtype, passl_stream_t stream) {
  if (!qkv || !table || !out || !lse) return PASSL_EINVAL;
  wattn::Geo g;
  const int rc = wattn::check_shape(B, Hp, Wp, ws, shift, nH, DH, dtype, &g);
  if (rc != PASSL_OK) return rc;
  if (dtype == PASSL_BF16 && !(aligned16(qkv) && aligned16(out))) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  WATTN_DISPATCH(dtype, DH, ws * ws, return (wattn::launch_fwd<Ops, NW, NT>(qkv, table, out, lse, B, g, scale, st));)
}

extern "C" int passl_hip_window_attention_bwd(const void* qkv, const float* table, const void* out,
                                              const void* dout, const float* lse, void* dqkv, float* dtable,
                                              float* ws_buf, int64_t ws_floats, int B, int Hp, int Wp, int ws,
                                              int shift, int nH, int DH, float scale, int dtype,
                                              passl_stream_t stream) {
  if (!qkv || !table || !out || !dout || !lse || !dqkv || !dtable || !ws_buf) return PASSL_EINVAL;
  wattn::Geo g;
  const int rc = wattn::check_shape(B, Hp, Wp, ws, shift, nH, DH, dtype, &g);
  if (rc != PASSL_OK) return rc;
  if (dtype == PASSL_BF16 && !(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv)))
    return PASSL_EINVAL;
  const int64_t Tn = ws * ws;
  if (ws_floats < (int64_t)wattn::table_slabs(B * g.nW, nH) * nH * Tn * Tn) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  WATTN_DISPATCH(dtype, DH, ws * ws, return (wattn::launch_bwd<Ops, NW, NT>(qkv, table, out, dout, lse, dqkv, dtable,
                                                                            ws_buf, B, g, scale, st));)
}

extern "C" int passl_hip_patch_merge(const void* x, void* y, int B, int H, int W, int C, int dtype,
                                     passl_stream_t stream) {
  return wattn::patch_merge<true>(x, y, B, H, W, C, dtype, as_stream(stream));
}

extern "C" int passl_hip_patch_merge_bwd(const void* dy, void* dx, int B, int H, int W, int C, int dtype,
                                         passl_stream_t stream) {
  return wattn::patch_merge<false>(dy, dx, B, H, W, C, dtype, as_stream(stream));
}
