// CaiT attention kernels for gfx950: talking-heads self-attention and class attention, head dimension 48.
//
// Reference: TalkingHeadAttn.forward, passl/models/cait.py:137-185, and ClassAttn.forward :46-88.
//
// Talking heads.  Per image, with S_h = (q_h k_h^T) scale:
//   A_g = sum_h S_h wl[h, g] + bl[g],  P_g = softmax_j A_g,  R_g = sum_h P_h ww[h, g] + bw[g],  O_g = R_g v_g.
// Every (query, key) pair couples all H heads twice, so a workgroup owns 16 query rows (dK / dV sweep: 16 key columns)
// of ALL heads of one image: wave h is head h (block = H waves).  A workgroup alternates between two layouts:
//   * MFMA phases, wave = head: S_h, dR_h = dO_h v_h^T (scores) and R_h v_h, dS_h k_h, ... (products) on
//     v_mfma_f32_16x16x4_f32, the "swapped" tiling of attention_core.h (a lane holds 4 keys of one own row).  The swept
//     operand (K, V, Q, dO tiles) is read from memory in operand layout; nothing but scores lies in LDS.
//   * pair phases, wave = row, lane = key: a thread reads the H scores of its (row, key) pair from LDS, runs both head
//     mixes and the softmax in fp32 registers and writes the H coefficients back in place.
// Both dtypes compute in fp32 from the stored values (bf16 is widened when loaded, exact): the only roundings of the
// bf16 path are those of the stored out, dq, dk, dv.  The fp32 path is "exact" in the project's sense.
// The forward holds the whole score row of a block, X[H][16][T_pad + 4] fp32 (104 KiB at H = 8, T_pad = 208).  The
// backward recomputes P = exp(A - lse) pointwise, so it walks the swept axis in chunks of 64 and needs X and Y =
// dR only per chunk.  delta_h[i] = sum_j P_h dP_h needs the whole row before dA: the dQ sweep makes two passes over
// the keys (pass A: delta, dww, dbw; pass B: dA, dwl, dbl, dS, dQ) and recomputes S and dR in the second.
// A is formed by mix() from S = mul_rn(q . k, scale) in all three kernels: same operations, same order, contraction
// off, so the recomputed P is the forward's.
// Small gradients: every workgroup of the dQ sweep writes one partial [144] (shuffle tree, then waves in order) and a
// last launch adds the partials of a bin in a fixed order.  No atomics, no scratch; two launches give the same bits.
//
// Class attention: one wave per (image, head); lane = key for the scores, lane = channel for the output.  The
// backward reads k and v once: dq = scale (sum_j P_j dP_j k_j - delta sum_j P_j k_j).
#include "attention_core.h"
#include "attention_ops_f32.h"

namespace cait {

using af32::mul_rn;
using attn::kNeg;

constexpr int DH = 48, kMaxH = 8, kChunk = 64, kCP = kChunk + 4;
constexpr int kMix = 144;          // wl[8][8], ww[8][8], bl[8], bw[8], zero beyond H
constexpr int kPart = 144;         // dwl[8][8], dbl[8], dww[8][8], dbw[8] of one workgroup
constexpr int kWl = 0, kWw = 64, kBl = 128, kBw = 136;

template <typename T> struct Vec12;
template <> struct Vec12<float> {
  __device__ static __forceinline__ void ld(const float* p, bool ok, float (&f)[12]) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) t = *reinterpret_cast<const float4*>(p + 4 * v);
      f[4 * v] = t.x; f[4 * v + 1] = t.y; f[4 * v + 2] = t.z; f[4 * v + 3] = t.w;
    }
  }
  __device__ static __forceinline__ void st(float* p, const float (&f)[12]) {
#pragma unroll
    for (int v = 0; v < 3; ++v)
      *reinterpret_cast<float4*>(p + 4 * v) = make_float4(f[4 * v], f[4 * v + 1], f[4 * v + 2], f[4 * v + 3]);
  }
};
template <> struct Vec12<bf16_t> {   // 8-byte pieces: a head's 48 channels start on a 32-byte boundary
  __device__ static __forceinline__ void ld(const bf16_t* p, bool ok, float (&f)[12]) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      uint2 t = make_uint2(0u, 0u);
      if (ok) t = *reinterpret_cast<const uint2*>(p + 4 * v);
      f[4 * v] = __uint_as_float(t.x << 16); f[4 * v + 1] = __uint_as_float(t.x & 0xffff0000u);
      f[4 * v + 2] = __uint_as_float(t.y << 16); f[4 * v + 3] = __uint_as_float(t.y & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ void st(bf16_t* p, const float (&f)[12]) {
#pragma unroll
    for (int v = 0; v < 3; ++v)
      *reinterpret_cast<uint2*>(p + 4 * v) = make_uint2(pack2bf(f[4 * v], f[4 * v + 1]), pack2bf(f[4 * v + 2], f[4 * v + 3]));
  }
};

// acc[r] = own[row l15] . swept[row 4 l4 + r]; a lane holds channels [12 l4, 12 l4 + 12) of both
__device__ __forceinline__ f32x4 dot12(const float (&swept)[12], const float (&own)[12]) {
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 12; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(swept[ks], own[ks], acc, 0, 0, 0);
  return acc;
}

// the two Linears over the head axis in LDS, padded to 8 x 8 with zeros
__device__ __forceinline__ void load_mix(const float* __restrict__ wl, const float* __restrict__ bl,
                                         const float* __restrict__ ww, const float* __restrict__ bw, int H, float* W) {
  for (int t = threadIdx.x; t < kMix; t += blockDim.x) {
    float v = 0.f;
    if (t < 128) {
      const int h = (t >> 3) & 7, g = t & 7;
      if (h < H && g < H) v = (t < 64 ? wl : ww)[h * H + g];
    } else {
      const int g = t & 7;
      if (g < H) v = (t < kBw ? bl : bw)[g];
    }
    W[t] = v;
  }
}

// y[g] = sum_h x[h] w[h, g] + b[g], heads in order, every product and sum rounded: the three kernels agree bit for bit
__device__ __forceinline__ void mix(const float (&x)[8], const float* w, const float* b, float (&y)[8]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    float a = x[0] * w[g];
#pragma unroll
    for (int h = 1; h < 8; ++h) a = a + x[h] * w[h * 8 + g];
    y[g] = a + b[g];
  }
}

// y[h] = sum_g x[g] w[h, g]: the transposed mix of the backward
__device__ __forceinline__ void mix_t(const float (&x)[8], const float* w, float (&y)[8]) {
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) a += x[g] * w[h * 8 + g];
    y[h] = a;
  }
}

// 0 the compiler cannot see through: the dQ sweep loads its own rows again in every chunk.  Hoisted out of the chunk
// loops they cost 24 registers next to the 72 sums of the small gradients, and the kernel spills.
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// ------------------------------------------------------------------ forward: one workgroup per (image, 16 query rows)
template <typename T>
__global__ void __launch_bounds__(512) th_fwd_kernel(
    const T* __restrict__ qkv, const float* __restrict__ wl, const float* __restrict__ bl,
    const float* __restrict__ ww, const float* __restrict__ bw, T* __restrict__ out, float* __restrict__ lse, int Tn,
    int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* W = reinterpret_cast<float*>(smem);
  float* X = W + kMix;                                   // [H][16][P]
  const int nt = (Tn + 15) >> 4, Tpad = nt * 16, P = Tpad + 4;
  const int b = blockIdx.x / nt, rb = blockIdx.x % nt;
  const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  load_mix(wl, bl, ww, bw, H, W);
  const int64_t rs = (int64_t)3 * H * DH;
  const T* img = qkv + (int64_t)b * Tn * rs + h * DH;    // q of token t at img + t rs, k + H DH, v + 2 H DH
  {
    const int row = rb * 16 + l15;
    float q[12];
    Vec12<T>::ld(img + (int64_t)(row < Tn ? row : 0) * rs + l4 * 12, row < Tn, q);
    float* xr = X + (h * 16 + l15) * P + l4 * 4;
    for (int ct = 0; ct < nt; ++ct) {
      const int kr = ct * 16 + l15;
      float kf[12];
      Vec12<T>::ld(img + H * DH + (int64_t)(kr < Tn ? kr : 0) * rs + l4 * 12, kr < Tn, kf);
      const f32x4 a = dot12(kf, q);
      st4(xr + ct * 16, mul_rn(a[0], scale), mul_rn(a[1], scale), mul_rn(a[2], scale), mul_rn(a[3], scale));
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int i = h; i < 16; i += NW) {                     // pair phase: this wave's rows, lane = key
    const int row = rb * 16 + i;
    if (row >= Tn) continue;
    float a[4][8], m[8], z[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) { m[g] = kNeg; z[g] = 0.f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      const bool valid = j < Tn;
      float s[8];
#pragma unroll
      for (int hh = 0; hh < 8; ++hh) s[hh] = (valid && hh < H) ? X[(hh * 16 + i) * P + j] : 0.f;
      mix(s, W + kWl, W + kBl, a[k]);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        if (!valid) a[k][g] = kNeg;
        m[g] = fmaxf(m[g], a[k][g]);
      }
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) m[g] = wave_max(m[g]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool valid = lane + 64 * k < Tn;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        a[k][g] = valid ? __expf(a[k][g] - m[g]) : 0.f;
        z[g] += a[k][g];
      }
    }
    float inv[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      z[g] = wave_sum(z[g]);
      inv[g] = 1.0f / z[g];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = lane + 64 * k;
      const bool valid = j < Tn;
      float p[8], r[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) p[g] = a[k][g] * inv[g];
      mix(p, W + kWw, W + kBw, r);
      if (j < Tpad) {
#pragma unroll
        for (int g = 0; g < 8; ++g)
          if (g < H) X[(g * 16 + i) * P + j] = valid ? r[g] : 0.f;   // a padded key contributes nothing
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < 8; ++g)
        if (g < H) lse[((int64_t)b * H + g) * Tn + row] = m[g] + __logf(z[g]);
    }
  }
  __syncthreads();
  f32x4 o[3];
#pragma unroll
  for (int jd = 0; jd < 3; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xr = X + (h * 16 + l15) * P + l4 * 4;
  for (int ct = 0; ct < nt; ++ct) {
    const float4 c4 = *reinterpret_cast<const float4*>(xr + ct * 16);
    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vr = ct * 16 + l4 * 4 + r;
      const bool ok = vr < Tn;
      const T* vp = img + 2 * H * DH + (int64_t)(ok ? vr : 0) * rs + l15;
#pragma unroll
      for (int jd = 0; jd < 3; ++jd)
        o[jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(c[r], ok ? ElemTraits<T>::ld(vp + jd * 16) : 0.f, o[jd], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = rb * 16 + l4 * 4 + r;
    if (orow < Tn) {
      T* op = out + (((int64_t)b * Tn + orow) * H + h) * DH + l15;
#pragma unroll
      for (int jd = 0; jd < 3; ++jd) ElemTraits<T>::st(op + jd * 16, o[jd][r]);
    }
  }
}

// ------------------------------------------------------------------ backward
// 64 + 8 per-thread sums -> this workgroup's partial dst[72]: shuffle tree, then the waves in order
__device__ __forceinline__ void reduce_part(const float (&aw)[64], const float (&ab)[8], float* red, float* dst,
                                            int wave, int lane, int NW) {
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const float v = wave_sum(aw[k]);
    if (lane == 0) red[wave * 72 + k] = v;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = wave_sum(ab[k]);
    if (lane == 0) red[wave * 72 + 64 + k] = v;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 72; t += blockDim.x) {
    float a = 0.f;
    for (int w = 0; w < NW; ++w) a += red[w * 72 + t];
    dst[t] = a;
  }
  __syncthreads();
}

// scores of a chunk of 64 swept rows against the wave's own rows: X = (own . a) scale, Y = own2 . b
// (one tile at a time: unrolled, the loads of four tiles in flight cost the dQ sweep its registers)
template <typename T>
__device__ __forceinline__ void chunk_scores(const T* __restrict__ a, int64_t as, const T* __restrict__ b2, int64_t bs,
                                             const float (&own)[12], const float (&own2)[12], int c, int nt, int Tn,
                                             float scale, int l15, int l4, float* xr, float* yr) {
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int ct = c * 4 + t;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, d = s;
    if (ct < nt) {
      const int sr = ct * 16 + l15;
      const bool ok = sr < Tn;
      float af[12], bf[12];
      Vec12<T>::ld(a + (int64_t)(ok ? sr : 0) * as + l4 * 12, ok, af);
      Vec12<T>::ld(b2 + (int64_t)(ok ? sr : 0) * bs + l4 * 12, ok, bf);
      s = dot12(af, own);
      d = dot12(bf, own2);
    }
    st4(xr + t * 16, mul_rn(s[0], scale), mul_rn(s[1], scale), mul_rn(s[2], scale), mul_rn(s[3], scale));
    st4(yr + t * 16, d[0], d[1], d[2], d[3]);
  }
}

// sweep 1, one workgroup per (image, 16 query rows), as two launches: each keeps 72 sums of small gradients per thread,
// and both passes in one kernel do not fit the registers of 8 waves.
//   kPassB = false: delta, and the partials of dww, dbw;  kPassB = true: dQ, and the partials of dwl, dbl
template <typename T, bool kPassB>
__global__ void __launch_bounds__(512) th_bwd_q_kernel(
    const T* __restrict__ qkv, const float* __restrict__ wl, const float* __restrict__ bl,
    const float* __restrict__ ww, const float* __restrict__ bw, const T* __restrict__ dout,
    const float* __restrict__ lse, T* __restrict__ dqkv, float* __restrict__ delta, float* __restrict__ part, int Tn,
    int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* W = reinterpret_cast<float*>(smem);
  float* red = W + kMix;                                 // [8][72]
  float* Dl = red + 8 * 72;                              // delta [16][8]
  float* X = Dl + 128;                                   // [H][16][kCP]
  float* Y = X + H * 16 * kCP;
  const int nt = (Tn + 15) >> 4, nch = (Tn + kChunk - 1) / kChunk;
  const int b = blockIdx.x / nt, rb = blockIdx.x % nt;
  const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  load_mix(wl, bl, ww, bw, H, W);
  for (int t = threadIdx.x; t < 128; t += blockDim.x) {
    const int row = rb * 16 + (t >> 3), g = t & 7;
    Dl[t] = (kPassB && g < H && row < Tn) ? delta[((int64_t)b * H + g) * Tn + row] : 0.f;
  }
  const int64_t rs = (int64_t)3 * H * DH, os = (int64_t)H * DH;
  const T* img = qkv + (int64_t)b * Tn * rs + h * DH;
  const T* dimg = dout + (int64_t)b * Tn * os + h * DH;
  float* mine = part + (int64_t)blockIdx.x * kPart;
  const int orow_ = rb * 16 + l15;
  const bool orv = orow_ < Tn;
  float* xr = X + (h * 16 + l15) * kCP + l4 * 4;
  float* yr = Y + (h * 16 + l15) * kCP + l4 * 4;
  float aw[64], ab[8];
#pragma unroll
  for (int k = 0; k < 64; ++k) aw[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) ab[k] = 0.f;
  __syncthreads();
  if constexpr (!kPassB) {
  for (int c = 0; c < nch; ++c) {
    {
      float q[12], dor[12];
      const int z = opaque_zero() + (orv ? orow_ : 0);
      Vec12<T>::ld(img + (int64_t)z * rs + l4 * 12, orv, q);
      Vec12<T>::ld(dimg + (int64_t)z * os + l4 * 12, orv, dor);
      chunk_scores<T>(img + H * DH, rs, img + 2 * H * DH, rs, q, dor, c, nt, Tn, scale, l15, l4, xr, yr);
    }
    __syncthreads();
#pragma unroll 1
    for (int i = h; i < 16; i += NW) {
      const int row = rb * 16 + i;
      if (row >= Tn) continue;
      const bool valid = c * kChunk + lane < Tn;
      float s[8], dr[8], a[8], p[8], dp[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        s[g] = g < H ? X[(g * 16 + i) * kCP + lane] : 0.f;
        dr[g] = g < H ? Y[(g * 16 + i) * kCP + lane] : 0.f;
      }
      mix(s, W + kWl, W + kBl, a);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float l = g < H ? lse[((int64_t)b * H + g) * Tn + row] : 0.f;
        p[g] = valid ? __expf(a[g] - l) : 0.f;
      }
      mix_t(dr, W + kWw, dp);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float d = wave_sum(p[g] * dp[g]);
        if (lane == 0) Dl[i * 8 + g] += d;
        ab[g] += valid ? dr[g] : 0.f;
#pragma unroll
        for (int hh = 0; hh < 8; ++hh) aw[hh * 8 + g] += p[hh] * dr[g];
      }
    }
    __syncthreads();
  }
  reduce_part(aw, ab, red, mine + 72, h, lane, NW);
  for (int t = threadIdx.x; t < 128; t += blockDim.x) {
    const int row = rb * 16 + (t >> 3), g = t & 7;
    if (g < H && row < Tn) delta[((int64_t)b * H + g) * Tn + row] = Dl[t];
  }
  } else {
  f32x4 dq[3];
#pragma unroll
  for (int jd = 0; jd < 3; ++jd) dq[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < nch; ++c) {
    {
      float q[12], dor[12];
      const int z = opaque_zero() + (orv ? orow_ : 0);
      Vec12<T>::ld(img + (int64_t)z * rs + l4 * 12, orv, q);
      Vec12<T>::ld(dimg + (int64_t)z * os + l4 * 12, orv, dor);
      chunk_scores<T>(img + H * DH, rs, img + 2 * H * DH, rs, q, dor, c, nt, Tn, scale, l15, l4, xr, yr);
    }
    __syncthreads();
#pragma unroll 1
    for (int i = h; i < 16; i += NW) {
      const int row = rb * 16 + i;
      if (row >= Tn) continue;
      const bool valid = c * kChunk + lane < Tn;
      float s[8], dr[8], a[8], p[8], dp[8], da[8], ds[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        s[g] = g < H ? X[(g * 16 + i) * kCP + lane] : 0.f;
        dr[g] = g < H ? Y[(g * 16 + i) * kCP + lane] : 0.f;
      }
      mix(s, W + kWl, W + kBl, a);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float l = g < H ? lse[((int64_t)b * H + g) * Tn + row] : 0.f;
        p[g] = valid ? __expf(a[g] - l) : 0.f;
      }
      mix_t(dr, W + kWw, dp);
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        da[g] = p[g] * (dp[g] - Dl[i * 8 + g]);
        ab[g] += da[g];
      }
#pragma unroll
      for (int hh = 0; hh < 8; ++hh)
#pragma unroll
        for (int g = 0; g < 8; ++g) aw[hh * 8 + g] += s[hh] * da[g];
      mix_t(da, W + kWl, ds);
#pragma unroll
      for (int g = 0; g < 8; ++g)
        if (g < H) X[(g * 16 + i) * kCP + lane] = ds[g] * scale;
    }
    __syncthreads();
#pragma unroll 2   // four tiles in flight spill
    for (int t = 0; t < 4; ++t) {
      const int ct = c * 4 + t;
      if (ct < nt) {
        const float4 c4 = *reinterpret_cast<const float4*>(xr + t * 16);
        const float cf[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kr = ct * 16 + l4 * 4 + r;
          const bool ok = kr < Tn;
          const T* kp = img + H * DH + (int64_t)(ok ? kr : 0) * rs + l15;
#pragma unroll
          for (int jd = 0; jd < 3; ++jd)
            dq[jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[r], ok ? ElemTraits<T>::ld(kp + jd * 16) : 0.f, dq[jd], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int orow = rb * 16 + l4 * 4 + r;
    if (orow < Tn) {
      T* op = dqkv + ((int64_t)b * Tn + orow) * rs + h * DH + l15;
#pragma unroll
      for (int jd = 0; jd < 3; ++jd) ElemTraits<T>::st(op + jd * 16, dq[jd][r]);
    }
  }
  reduce_part(aw, ab, red, mine, h, lane, NW);
  }
}

// sweep 2: dK, dV; one workgroup per (image, 16 key columns), query rows swept in chunks of 64
template <typename T>
__global__ void __launch_bounds__(512) th_bwd_kv_kernel(
    const T* __restrict__ qkv, const float* __restrict__ wl, const float* __restrict__ bl,
    const float* __restrict__ ww, const float* __restrict__ bw, const T* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta, T* __restrict__ dqkv, int Tn, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* W = reinterpret_cast<float*>(smem);
  float* Ls = W + kMix;                                  // lse [8][64] of the chunk
  float* Ds = Ls + 8 * kChunk;                           // delta [8][64]
  float* X = Ds + 8 * kChunk;                            // [H][16][kCP]
  float* Y = X + H * 16 * kCP;
  const int nt = (Tn + 15) >> 4, nch = (Tn + kChunk - 1) / kChunk;
  const int b = blockIdx.x / nt, cb = blockIdx.x % nt;
  const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  load_mix(wl, bl, ww, bw, H, W);
  const int64_t rs = (int64_t)3 * H * DH, os = (int64_t)H * DH;
  const T* img = qkv + (int64_t)b * Tn * rs + h * DH;
  const T* dimg = dout + (int64_t)b * Tn * os + h * DH;
  float kown[12], vown[12];
  {
    const int col = cb * 16 + l15;
    const bool cv = col < Tn;
    Vec12<T>::ld(img + H * DH + (int64_t)(cv ? col : 0) * rs + l4 * 12, cv, kown);
    Vec12<T>::ld(img + 2 * H * DH + (int64_t)(cv ? col : 0) * rs + l4 * 12, cv, vown);
  }
  float* xr = X + (h * 16 + l15) * kCP + l4 * 4;
  float* yr = Y + (h * 16 + l15) * kCP + l4 * 4;
  f32x4 dk[3], dv[3];
#pragma unroll
  for (int jd = 0; jd < 3; ++jd) { dk[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[jd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int c = 0; c < nch; ++c) {
    for (int t = threadIdx.x; t < 8 * kChunk; t += blockDim.x) {
      const int g = t >> 6, i = c * kChunk + (t & 63);
      const bool ok = g < H && i < Tn;
      Ls[t] = ok ? lse[((int64_t)b * H + g) * Tn + i] : 0.f;
      Ds[t] = ok ? delta[((int64_t)b * H + g) * Tn + i] : 0.f;
    }
    chunk_scores<T>(img, rs, dimg, os, kown, vown, c, nt, Tn, scale, l15, l4, xr, yr);
    __syncthreads();
#pragma unroll 1
    for (int jj = h; jj < 16; jj += NW) {                // pair phase: this wave's key columns, lane = query
      if (cb * 16 + jj >= Tn) continue;
      const bool valid = c * kChunk + lane < Tn;
      float s[8], dr[8], a[8], p[8], r[8], dp[8], da[8], ds[8];
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        s[g] = g < H ? X[(g * 16 + jj) * kCP + lane] : 0.f;
        dr[g] = g < H ? Y[(g * 16 + jj) * kCP + lane] : 0.f;
      }
      mix(s, W + kWl, W + kBl, a);
#pragma unroll
      for (int g = 0; g < 8; ++g) p[g] = valid ? __expf(a[g] - Ls[g * kChunk + lane]) : 0.f;
      mix(p, W + kWw, W + kBw, r);
      mix_t(dr, W + kWw, dp);
#pragma unroll
      for (int g = 0; g < 8; ++g) da[g] = p[g] * (dp[g] - Ds[g * kChunk + lane]);
      mix_t(da, W + kWl, ds);
#pragma unroll
      for (int g = 0; g < 8; ++g)
        if (g < H) {
          X[(g * 16 + jj) * kCP + lane] = valid ? r[g] : 0.f;
          Y[(g * 16 + jj) * kCP + lane] = ds[g] * scale;
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int rt = c * 4 + t;
      if (rt < nt) {
        const float4 r4 = *reinterpret_cast<const float4*>(xr + t * 16);
        const float4 s4 = *reinterpret_cast<const float4*>(yr + t * 16);
        const float cr[4] = {r4.x, r4.y, r4.z, r4.w}, cs[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = rt * 16 + l4 * 4 + r;
          const bool ok = i < Tn;
          const T* dp_ = dimg + (int64_t)(ok ? i : 0) * os + l15;
          const T* qp = img + (int64_t)(ok ? i : 0) * rs + l15;
#pragma unroll
          for (int jd = 0; jd < 3; ++jd) {
            dv[jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(cr[r], ok ? ElemTraits<T>::ld(dp_ + jd * 16) : 0.f, dv[jd], 0, 0, 0);
            dk[jd] = __builtin_amdgcn_mfma_f32_16x16x4f32(cs[r], ok ? ElemTraits<T>::ld(qp + jd * 16) : 0.f, dk[jd], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ocol = cb * 16 + l4 * 4 + r;
    if (ocol < Tn) {
      T* kp = dqkv + ((int64_t)b * Tn + ocol) * rs + H * DH + h * DH + l15;
      T* vp = kp + H * DH;
#pragma unroll
      for (int jd = 0; jd < 3; ++jd) {
        ElemTraits<T>::st(kp + jd * 16, dk[jd][r]);
        ElemTraits<T>::st(vp + jd * 16, dv[jd][r]);
      }
    }
  }
}

// one workgroup per bin of the partials: thread t adds workgroups t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(256) th_small_grads_kernel(const float* __restrict__ part, int nwg, int H,
                                                             float* __restrict__ dwl, float* __restrict__ dbl,
                                                             float* __restrict__ dww, float* __restrict__ dbw) {
  __shared__ float sh[256];
  const int bin = blockIdx.x, second = bin >= 72, k = bin % 72;
  float* dst;
  if (k < 64) {
    const int h = k >> 3, g = k & 7;
    if (h >= H || g >= H) return;
    dst = (second ? dww : dwl) + h * H + g;
  } else {
    if (k - 64 >= H) return;
    dst = (second ? dbw : dbl) + (k - 64);
  }
  float a = 0.f;
  for (int w = threadIdx.x; w < nwg; w += 256) a += part[(int64_t)w * kPart + bin];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = sh[0];
}

// ------------------------------------------------------------------ class attention: one wave per (image, head)
// q . k over the 48 channels, explicit fmas in channel order: the backward's score is the forward's
template <typename T>
__device__ __forceinline__ float dot48(const T* __restrict__ p, const float (&q)[48]) {
  float d = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float f[12];
    Vec12<T>::ld(p + 12 * c, true, f);
#pragma unroll
    for (int e = 0; e < 12; ++e) d = __fmaf_rn(f[e], q[12 * c + e], d);
  }
  return d;
}

template <typename T>
__device__ __forceinline__ void load48(const T* __restrict__ p, float (&q)[48]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float f[12];
    Vec12<T>::ld(p + 12 * c, true, f);
#pragma unroll
    for (int e = 0; e < 12; ++e) q[12 * c + e] = f[e];
  }
}

template <typename T>
__global__ void __launch_bounds__(64) cls_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                     const T* __restrict__ v, T* __restrict__ out,
                                                     float* __restrict__ lse, int Tn, int H, float scale) {
  __shared__ float ps[256];
  const int b = blockIdx.x / H, h = blockIdx.x % H, lane = threadIdx.x;
  const int64_t C = (int64_t)H * DH;
  float qf[48];
  load48(q + (int64_t)blockIdx.x * DH, qf);
  const T* kb = k + (int64_t)b * Tn * C + h * DH;
  const T* vb = v + (int64_t)b * Tn * C + h * DH;
  float s[4], m = kNeg;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = lane + 64 * it;
    s[it] = kNeg;
    if (j < Tn) s[it] = mul_rn(dot48(kb + j * C, qf), scale);
    m = fmaxf(m, s[it]);
  }
  m = wave_max(m);
  float z = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    s[it] = lane + 64 * it < Tn ? __expf(s[it] - m) : 0.f;
    z += s[it];
  }
  z = wave_sum(z);
  const float inv = 1.0f / z;
#pragma unroll
  for (int it = 0; it < 4; ++it) ps[lane + 64 * it] = s[it] * inv;
  __syncthreads();
  if (lane < DH) {
    float a = 0.f;
#pragma unroll 8
    for (int j = 0; j < Tn; ++j) a += ps[j] * ElemTraits<T>::ld(vb + j * C + lane);
    ElemTraits<T>::st(out + (int64_t)blockIdx.x * DH + lane, a);
  }
  if (lane == 0) lse[blockIdx.x] = m + __logf(z);
}

template <typename T>
__global__ void __launch_bounds__(64) cls_bwd_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                     const T* __restrict__ v, const T* __restrict__ dout,
                                                     const float* __restrict__ lse, T* __restrict__ dq,
                                                     T* __restrict__ dk, T* __restrict__ dv, int Tn, int H,
                                                     float scale) {
  const int b = blockIdx.x / H, h = blockIdx.x % H, lane = threadIdx.x;
  const int64_t C = (int64_t)H * DH;
  float qf[48], dof[48], A[48], Bk[48];
  load48(q + (int64_t)blockIdx.x * DH, qf);
  load48(dout + (int64_t)blockIdx.x * DH, dof);
#pragma unroll
  for (int d = 0; d < 48; ++d) { A[d] = 0.f; Bk[d] = 0.f; }
  const float l = lse[blockIdx.x];
  const int64_t base = (int64_t)b * Tn * C + h * DH;
  float p[4], dp[4], dlt = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = lane + 64 * it;
    p[it] = 0.f;
    dp[it] = 0.f;
    if (j < Tn) {
      const T* kp = k + base + j * C;
      const float pj = __expf(mul_rn(dot48(kp, qf), scale) - l);
      const float dpj = dot48(v + base + j * C, dof);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float kf[12], g[12];
        Vec12<T>::ld(kp + 12 * c, true, kf);
#pragma unroll
        for (int e = 0; e < 12; ++e) {
          A[12 * c + e] += pj * dpj * kf[e];
          Bk[12 * c + e] += pj * kf[e];
          g[e] = pj * dof[12 * c + e];
        }
        Vec12<T>::st(dv + base + j * C + 12 * c, g);
      }
      p[it] = pj;
      dp[it] = dpj;
      dlt += pj * dpj;
    }
  }
  dlt = wave_sum(dlt);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = lane + 64 * it;
    if (j < Tn) {
      const float ds = p[it] * (dp[it] - dlt) * scale;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float g[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) g[e] = ds * qf[12 * c + e];
        Vec12<T>::st(dk + base + j * C + 12 * c, g);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < 48; ++d) A[d] = scale * (wave_sum(A[d]) - dlt * wave_sum(Bk[d]));
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float g[12];
#pragma unroll
      for (int e = 0; e < 12; ++e) g[e] = A[12 * c + e];
      Vec12<T>::st(dq + (int64_t)blockIdx.x * DH + 12 * c, g);
    }
  }
}

// ------------------------------------------------------------------ token plumbing of the model, 8 elements a thread
// out[b, i] = x[b, i] + pos[i]: the position table over the patch rows (no class row yet)
template <typename T>
__global__ void __launch_bounds__(256) pos_add_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                      T* __restrict__ out, int64_t n8, int64_t lc8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  float a[8], p[8];
  ElemTraits<T>::load8(x + i * 8, a);
  ElemTraits<float>::load8(pos + (i % lc8) * 8, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += p[e];
  ElemTraits<T>::store8(out + i * 8, a);
}

// out [B, 1 + L, C]: row 0 of image b = c[b * cstride] (cstride 0: one class row for all), rows 1.. = x [B, L, C]
template <typename T>
__global__ void __launch_bounds__(256) cls_concat_kernel(const T* __restrict__ c, int64_t cstride,
                                                         const T* __restrict__ x, T* __restrict__ out, int64_t n8,
                                                         int L, int c8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int cp = (int)(i % c8);
  const int64_t row = i / c8, b = row / (L + 1);
  const int t = (int)(row % (L + 1));
  float a[8];
  if (t == 0) ElemTraits<T>::load8(c + b * cstride + cp * 8, a);
  else ElemTraits<T>::load8(x + ((b * L + t - 1) * c8 + cp) * 8, a);
  ElemTraits<T>::store8(out + i * 8, a);
}

// the inverse: dc[b] = dout[b, 0], dx[b, t] = dout[b, 1 + t] (+ add[b, t] when given: the patch rows' other consumer)
template <typename T>
__global__ void __launch_bounds__(256) cls_split_kernel(const T* __restrict__ dout, const T* __restrict__ add,
                                                        T* __restrict__ dc, T* __restrict__ dx, int64_t n8, int L,
                                                        int c8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const int cp = (int)(i % c8);
  const int64_t row = i / c8, b = row / (L + 1);
  const int t = (int)(row % (L + 1));
  float a[8];
  ElemTraits<T>::load8(dout + i * 8, a);
  if (t == 0) {
    ElemTraits<T>::store8(dc + (b * c8 + cp) * 8, a);
    return;
  }
  const int64_t o = ((b * L + t - 1) * c8 + cp) * 8;
  if (add) {
    float g[8];
    ElemTraits<T>::load8(add + o, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += g[e];
  }
  ElemTraits<T>::store8(dx + o, a);
}

// shapes of the three: positive, C a multiple of 8, the grid within 2^31 workgroups
int plumbing_shape(int B, int L, int C, int dtype, int64_t rows, int64_t* n8) {
  if (B <= 0 || L <= 0 || C <= 0 || C % 8) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  *n8 = rows * (C / 8);
  return (*n8 + 255) / 256 > INT32_MAX ? PASSL_EUNSUPPORTED : PASSL_OK;
}

// ------------------------------------------------------------------ launches
constexpr int fwd_lds(int Tn, int H) { return (kMix + H * 16 * ((Tn + 15) / 16 * 16 + 4)) * 4; }
constexpr int bwd_q_lds(int H) { return (kMix + 8 * 72 + 128 + 2 * H * 16 * kCP) * 4; }
constexpr int bwd_kv_lds(int H) { return (kMix + 16 * kChunk + 2 * H * 16 * kCP) * 4; }

template <auto Kernel, typename... A>
int launch(int groups, int threads, int lds, int cap, hipStream_t st, A... a) {
  static bool capped = false;
  if (!capped) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    capped = true;
  }
  hipLaunchKernelGGL(Kernel, dim3(groups), dim3(threads), lds, st, a...);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

// PASSL_OK, or the status the entry points return without launching
int check_shape(int B, int Tn, int H, int DHa, int dtype) {
  if (B <= 0 || Tn <= 0 || H <= 0 || DHa <= 0) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  if (DHa != DH || Tn > attn::kMaxTokens || H > kMaxH) return PASSL_EUNSUPPORTED;
  if ((int64_t)B * ((Tn + 15) / 16) > INT32_MAX || (int64_t)B * H > INT32_MAX) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

}  // namespace cait

extern "C" int passl_hip_talking_heads_attention_fwd(const void* qkv, const float* wl, const float* bl,
                                                     const float* ww, const float* bw, void* out, float* lse, int B,
                                                     int T_, int H, int DH, float scale, int dtype,
                                                     passl_stream_t stream) {
  if (!qkv || !wl || !bl || !ww || !bw || !out || !lse) return PASSL_EINVAL;
  const int rc = cait::check_shape(B, T_, H, DH, dtype);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(qkv) && aligned16(out))) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  const int groups = B * ((T_ + 15) / 16);
  PASSL_DISPATCH_DTYPE(dtype, return (cait::launch<&cait::th_fwd_kernel<T>>(
      groups, H * 64, cait::fwd_lds(T_, H), cait::fwd_lds(attn::kMaxTokens, cait::kMaxH), st,
      reinterpret_cast<const T*>(qkv), wl, bl, ww, bw, reinterpret_cast<T*>(out), lse, T_, H, scale));)
}

extern "C" int passl_hip_talking_heads_attention_bwd(const void* qkv, const float* wl, const float* bl,
                                                     const float* ww, const float* bw, const void* dout,
                                                     const float* lse, void* dqkv, float* dwl, float* dbl,
                                                     float* dww, float* dbw, float* ws_buf, int64_t ws_floats, int B,
                                                     int T_, int H, int DH, float scale, int dtype,
                                                     passl_stream_t stream) {
  if (!qkv || !wl || !bl || !ww || !bw || !dout || !lse || !dqkv || !dwl || !dbl || !dww || !dbw || !ws_buf)
    return PASSL_EINVAL;
  const int rc = cait::check_shape(B, T_, H, DH, dtype);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(qkv) && aligned16(dout) && aligned16(dqkv))) return PASSL_EINVAL;
  if (ws_floats < PASSL_TALKING_HEADS_ATTENTION_WS_FLOATS(B, T_, H)) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  const int groups = B * ((T_ + 15) / 16);
  float* delta = ws_buf;
  float* part = ws_buf + (int64_t)B * H * T_;
  PASSL_DISPATCH_DTYPE(dtype, {
    const T* q = reinterpret_cast<const T*>(qkv);
    const T* d = reinterpret_cast<const T*>(dout);
    int r = cait::launch<&cait::th_bwd_q_kernel<T, false>>(groups, H * 64, cait::bwd_q_lds(H),
                                                           cait::bwd_q_lds(cait::kMaxH), st, q, wl, bl, ww, bw, d, lse,
                                                           reinterpret_cast<T*>(dqkv), delta, part, T_, H, scale);
    if (r != PASSL_OK) return r;
    r = cait::launch<&cait::th_bwd_q_kernel<T, true>>(groups, H * 64, cait::bwd_q_lds(H), cait::bwd_q_lds(cait::kMaxH),
                                                      st, q, wl, bl, ww, bw, d, lse, reinterpret_cast<T*>(dqkv), delta,
                                                      part, T_, H, scale);
    if (r != PASSL_OK) return r;
    r = cait::launch<&cait::th_bwd_kv_kernel<T>>(groups, H * 64, cait::bwd_kv_lds(H), cait::bwd_kv_lds(cait::kMaxH), st,
                                                 q, wl, bl, ww, bw, d, lse, (const float*)delta,
                                                 reinterpret_cast<T*>(dqkv), T_, H, scale);
    if (r != PASSL_OK) return r;
  })
  hipLaunchKernelGGL(cait::th_small_grads_kernel, dim3(cait::kPart), dim3(256), 0, st, (const float*)part, groups, H,
                     dwl, dbl, dww, dbw);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_class_attention_fwd(const void* q, const void* k, const void* v, void* out, float* lse,
                                             int B, int T_, int H, int DH, float scale, int dtype,
                                             passl_stream_t stream) {
  if (!q || !k || !v || !out || !lse) return PASSL_EINVAL;
  const int rc = cait::check_shape(B, T_, H, DH, dtype);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out))) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cait::cls_fwd_kernel<T>, dim3(B * H), dim3(64), 0, st, reinterpret_cast<const T*>(q),
                       reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), reinterpret_cast<T*>(out), lse,
                       T_, H, scale);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_class_attention_bwd(const void* q, const void* k, const void* v, const void* dout,
                                             const float* lse, void* dq, void* dk, void* dv, int B, int T_, int H,
                                             int DH, float scale, int dtype, passl_stream_t stream) {
  if (!q || !k || !v || !dout || !lse || !dq || !dk || !dv) return PASSL_EINVAL;
  const int rc = cait::check_shape(B, T_, H, DH, dtype);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dout) && aligned16(dq) && aligned16(dk) &&
        aligned16(dv)))
    return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cait::cls_bwd_kernel<T>, dim3(B * H), dim3(64), 0, st, reinterpret_cast<const T*>(q),
                       reinterpret_cast<const T*>(k), reinterpret_cast<const T*>(v), reinterpret_cast<const T*>(dout),
                       lse, reinterpret_cast<T*>(dq), reinterpret_cast<T*>(dk), reinterpret_cast<T*>(dv), T_, H,
                       scale);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_cait_pos_add(const void* x, const float* pos, void* out, int B, int L, int C, int dtype,
                                      passl_stream_t stream) {
  if (!x || !pos || !out) return PASSL_EINVAL;
  int64_t n8;
  const int rc = cait::plumbing_shape(B, L, C, dtype, (int64_t)B * L, &n8);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(x) && aligned16(pos) && aligned16(out))) return PASSL_EINVAL;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cait::pos_add_kernel<T>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const T*>(x), pos, reinterpret_cast<T*>(out), n8, (int64_t)L * (C / 8));
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_cait_cls_concat(const void* c, int c_per_image, const void* x, void* out, int B, int L, int C,
                                         int dtype, passl_stream_t stream) {
  if (!c || !x || !out) return PASSL_EINVAL;
  int64_t n8;
  const int rc = cait::plumbing_shape(B, L, C, dtype, (int64_t)B * (L + 1), &n8);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(c) && aligned16(x) && aligned16(out))) return PASSL_EINVAL;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cait::cls_concat_kernel<T>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const T*>(c), (int64_t)(c_per_image ? C : 0), reinterpret_cast<const T*>(x),
                       reinterpret_cast<T*>(out), n8, L, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_cait_cls_split(const void* dout, const void* add, void* dc, void* dx, int B, int L, int C,
                                        int dtype, passl_stream_t stream) {
  if (!dout || !dc || !dx) return PASSL_EINVAL;
  int64_t n8;
  const int rc = cait::plumbing_shape(B, L, C, dtype, (int64_t)B * (L + 1), &n8);
  if (rc != PASSL_OK) return rc;
  if (!(aligned16(dout) && aligned16(add) && aligned16(dc) && aligned16(dx))) return PASSL_EINVAL;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cait::cls_split_kernel<T>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const T*>(dout), reinterpret_cast<const T*>(add), reinterpret_cast<T*>(dc),
                       reinterpret_cast<T*>(dx), n8, L, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}
