// Token merging (ToMe) for the ViT trunk on gfx950: bipartite soft matching, the size-weighted merge and its gradient,
// and proportional attention (a per-key additive term before the softmax).
//
// Reference: passl/models/utils/tome.py — bipartite_soft_matching :28-118, merge_wavg :121-133, ToMeAttention.forward
// :172-195 (metric = k.mean(1), attn + size.log() :183-185).
//
// tome_match, one workgroup per image, one launch, nothing returns to the host:
//   1. metric[t] = mean over heads of the K slice of qkv row t, fp32, heads added in ascending order; each row is
//      divided by its largest magnitude, then by the L2 norm of the result (two steps: neither a key of norm 1e20 nor
//      one of 1e-30 leaves fp32 range; an all-zero key stays zero and scores 0 against everybody).  LDS [T][DH + 4].
//   2. A = even tokens, B = odd tokens.  A wave owns A row i (kept in registers), its lanes the B rows j, j + 64:
//      score = a_i . b_j as DH sequential fmas; the lane's and then the wave's (max, arg-max), the lowest j on equal
//      scores.  The [|A|, |B|] score matrix exists only as one value per lane.  Row 0 (the class token) is -inf, idx 0.
//   3. rank_i = #{i' : max_i' > max_i, or max_i' == max_i and i' < i}: counting, no sort.  rank < r <=> merged.
//   4. dest: an unmerged A token's row is the number of unmerged A tokens before it (the class token stays row 0), B
//      token j's row is |A| - r + j, a merged A token's row is that of its arg-max B token.
// tome_merge_fwd: y[row] = sum over {t : dest[t] = row} of size[t] x[t] / sum of size[t].  A gather: every workgroup
//   threads the tokens of its image into per-row lists in LDS (head[row], next[t], ascending t), a wave walks the list of
//   an output row with its lanes over the channels, fp32 sums in ascending t, one rounding at the store.  No atomics,
//   no scratch: two runs give the same bits.  Also written: size_out and, when asked for, log(size_out), the key bias
//   of the next block's proportional attention.
// tome_merge_bwd: dx[t] = dy[dest[t]] * (size[t] / size_out[dest[t]]), one wave per input row.
// attention_fwd_keybias: attn_fwd_kernel of attention_core.h (same operand policies, same staging, same MFMA tiling and
//   softmax; no causal flag) with score = (q . k) scale + bias[b, j], each operation rounded, bias in LDS.  A second
//   copy and not a parameter of the first, so that the dense kernels' code stays as it is (DESIGN 33 has what a policy
//   parameter did to it).  With bias = 0 the output has the bits of passl_hip_attention_fwd.
#include <type_traits>
#include "attention_core.h"
#include "attention_ops_f32.h"
#include "attention_ops_bf16.h"

namespace tome {

using attn::kNeg;
using attn::pad_rows;
using attn::shx;

constexpr int kMaxTokens = attn::kMaxTokens;    // 208
constexpr int kMatchThreads = 1024;      // 16 waves: the K slice of an image is 300 KB of loads to keep in flight
constexpr int kMergeThreads = 256;

// ------------------------------------------------------------------ matching
// dynamic LDS: metric [T][DH + 4] fp32, nmax [NA] fp32, nidx [NA], merged [NA]
__host__ __device__ constexpr int match_lds(int T, int DH) { return (T * (DH + 4) + 3 * ((T + 1) / 2)) * 4; }

template <typename T, int DH>
__global__ void __launch_bounds__(kMatchThreads) tome_match_kernel(
    const T* __restrict__ qkv, int32_t* __restrict__ dest, float* __restrict__ node_max, int32_t* __restrict__ node_idx,
    int Tn, int H, int r) {
  constexpr int P = DH + 4, NW = kMatchThreads / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int NA = (Tn + 1) >> 1, NB = Tn >> 1;
  float* M = reinterpret_cast<float*>(smem);
  float* nmax = M + Tn * P;
  int* nidx = reinterpret_cast<int*>(nmax + NA);
  int* merged = nidx + NA;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // 1. mean over heads of K, 8 channels (16 or 32 bytes) per load
  const float invH = 1.0f / (float)H;
  for (int i = threadIdx.x; i < Tn * (DH / 8); i += kMatchThreads) {
    const int t = i / (DH / 8), d = (i % (DH / 8)) * 8;
    const T* p = qkv + attn::qkv_off<DH>(b, t, 1, 0, Tn, H) + d;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) {
      float v[8];
      ElemTraits<T>::load8(p + (int64_t)h * DH, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) M[t * P + d + e] = s[e] * invH;
  }
  __syncthreads();
  for (int t = wave; t < Tn; t += NW) {
    float v = lane < DH ? M[t * P + lane] : 0.f;       // DH <= 64: one channel per lane
    const float amax = wave_max(fabsf(v));
    if (amax > 0.f) {
      v = v / amax;
      const float ss = wave_sum(v * v);
      v = v / sqrtf(ss);
    } else {
      v = 0.f;
    }
    if (lane < DH) M[t * P + lane] = v;
  }
  __syncthreads();
  // 2. max and arg-max of every A row over the B rows
  for (int i = wave; i < NA; i += NW) {
    float best = -INFINITY;
    int bi = 0;
    if (i > 0) {                                        // i == 0: the class token is never merged
      float a[DH];
#pragma unroll
      for (int d = 0; d < DH; d += 4) {
        const float4 q = *reinterpret_cast<const float4*>(M + (2 * i) * P + d);
        a[d] = q.x; a[d + 1] = q.y; a[d + 2] = q.z; a[d + 3] = q.w;
      }
      for (int j = lane; j < NB; j += 64) {
        const float* bp = M + (2 * j + 1) * P;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
          const float4 q = *reinterpret_cast<const float4*>(bp + d);
          s = fmaf(a[d], q.x, s);
          s = fmaf(a[d + 1], q.y, s);
          s = fmaf(a[d + 2], q.z, s);
          s = fmaf(a[d + 3], q.w, s);
        }
        if (s > best) { best = s; bi = j; }             // ascending j: the lowest index of equal scores
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
    }
    if (lane == 0) { nmax[i] = best; nidx[i] = bi; }
  }
  __syncthreads();
  // 3. rank by counting
  for (int i = threadIdx.x; i < NA; i += kMatchThreads) {
    const float v = nmax[i];
    int rank = 0;
    for (int k = 0; k < NA; ++k) {
      const float u = nmax[k];
      rank += (u > v || (u == v && k < i)) ? 1 : 0;
    }
    merged[i] = rank < r ? 1 : 0;
    if (node_max) node_max[(int64_t)b * NA + i] = v;
    if (node_idx) node_idx[(int64_t)b * NA + i] = nidx[i];
  }
  __syncthreads();
  // 4. output rows
  int32_t* dp = dest + (int64_t)b * Tn;
  const int nunm = NA - r;
  for (int t = threadIdx.x; t < Tn; t += kMatchThreads) {
    int row;
    if (t & 1) {
      row = nunm + (t >> 1);
    } else {
      const int i = t >> 1;
      if (merged[i]) {
        row = nunm + nidx[i];
      } else {
        row = 0;
        for (int k = 0; k < i; ++k) row += 1 - merged[k];
      }
    }
    dp[t] = row;
  }
}

// ------------------------------------------------------------------ merge
// head[To] and next[Tn] in static LDS: the tokens of output row o are head[o], next[head[o]], ... in ascending order, -1 ends
// the list.  A dest outside [0, To) joins no list.
__device__ __forceinline__ void build_lists(const int32_t* __restrict__ dp, int Tn, int To, int* dst, int* head, int* next) {
  const int Tq = (Tn + 3) & ~3;                         // dst is read four entries at a time
  for (int t = threadIdx.x; t < Tq; t += kMergeThreads) {
    const int d = t < Tn ? dp[t] : -1;
    dst[t] = (d >= 0 && d < To) ? d : -1;
    head[t] = -1;                                       // To < Tn
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Tn; t += kMergeThreads) {
    const int d = dst[t];
    int nx = -1;
    bool first = true;
    if (d >= 0) {
      // one pass over the image's tokens (every lane reads the same words: LDS broadcasts): an earlier token with the
      // same row means t is not the head, the first later one is next[t]
#pragma unroll 4
      for (int k = 0; k < Tq; k += 4) {
        const int4 q = *reinterpret_cast<const int4*>(dst + k);
        const int e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool same = e[u] == d;
          first = first && !(same && k + u < t);
          nx = (same && k + u > t && nx < 0) ? k + u : nx;
        }
      }
      if (first) head[d] = t;
    }
    next[t] = nx;
  }
  __syncthreads();
}

// grid = B * slabs; workgroup (b, s) writes output rows s * 4 + wave, + 4 * slabs, ... of image b
template <typename T>
__global__ void __launch_bounds__(kMergeThreads) tome_merge_fwd_kernel(
    const T* __restrict__ x, const float* __restrict__ size, const int32_t* __restrict__ dest, T* __restrict__ y,
    float* __restrict__ size_out, float* __restrict__ logsize_out, int Tn, int To, int C, int slabs) {
  __shared__ __attribute__((aligned(16))) int dst[kMaxTokens], head[kMaxTokens], next[kMaxTokens];
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  build_lists(dest + (int64_t)b * Tn, Tn, To, dst, head, next);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* xb = x + (int64_t)b * Tn * C;
  const float* sb = size ? size + (int64_t)b * Tn : nullptr;
  for (int o = s * 4 + wave; o < To; o += 4 * slabs) {
    float wsum = 0.f;
    for (int t = head[o]; t >= 0; t = next[t]) wsum += sb ? sb[t] : 1.f;
    // two 8-channel pieces per lane and pass (C <= 1024: one pass), so that both loads of a source are in flight together
    for (int c0 = lane * 8; c0 < C; c0 += 1024) {
      const int c1 = c0 + 512;
      const bool two = c1 < C;
      float a0[8], a1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
      for (int t = head[o]; t >= 0; t = next[t]) {
        const float w = sb ? sb[t] : 1.f;
        float v0[8], v1[8];
        ElemTraits<T>::load8(xb + (int64_t)t * C + c0, v0);
        if (two) ElemTraits<T>::load8(xb + (int64_t)t * C + c1, v1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          a0[e] = fmaf(w, v0[e], a0[e]);
          if (two) a1[e] = fmaf(w, v1[e], a1[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) { a0[e] = a0[e] / wsum; a1[e] = a1[e] / wsum; }
      ElemTraits<T>::store8(y + ((int64_t)b * To + o) * C + c0, a0);
      if (two) ElemTraits<T>::store8(y + ((int64_t)b * To + o) * C + c1, a1);
    }
    if (lane == 0) {
      size_out[(int64_t)b * To + o] = wsum;
      if (logsize_out) logsize_out[(int64_t)b * To + o] = logf(wsum);
    }
  }
}

// one wave per input row; grid = ceil(B * Tn / 4)
template <typename T>
__global__ void __launch_bounds__(kMergeThreads) tome_merge_bwd_kernel(
    const T* __restrict__ dy, const float* __restrict__ size, const float* __restrict__ size_out,
    const int32_t* __restrict__ dest, T* __restrict__ dx, int64_t rows, int Tn, int To, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const int64_t b = row / Tn;
  const int d = dest[row];
  const bool ok = d >= 0 && d < To;
  const int64_t orow = b * To + (ok ? d : 0);
  const float f = ok ? (size ? size[row] : 1.f) / size_out[orow] : 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    float v[8];
    ElemTraits<T>::load8(dy + orow * C + c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ok ? v[e] * f : 0.f;
    ElemTraits<T>::store8(dx + row * C + c, v);
  }
}

// ------------------------------------------------------------------ proportional attention, forward
// (a * scale) + bias with both roundings, as the reference's `attn * scale + size.log()`
__device__ __forceinline__ float score(float a, float scale, float bias) {
#pragma clang fp contract(off)
  return a * scale + bias;
}

template <class Ops, class Coef>
__device__ __forceinline__ void accum(const Coef& c, const typename Ops::lds_t* lds, int t0, int lane,
                                      f32x4 (&o)[Ops::DH / 16]) {
  if constexpr (Ops::kAccumByLane) Ops::accum(c, lds, t0, lane, o);
  else Ops::accum(c, lds, t0, lane & 15, lane >> 4, o);
}

// main region of attention_core.h, then bias[Tpad]
template <class Ops>
constexpr int kb_lds(int Tpad) { return attn::lds_bytes<Ops>(Tpad, false) + Tpad * 4; }

template <class Ops, int NW>
__global__ void __launch_bounds__(NW * 64, Ops::fwd_waves_per_eu(NW)) attn_fwd_keybias_kernel(
    const typename Ops::elem_t* __restrict__ qkv, const float* __restrict__ kbias,
    typename Ops::elem_t* __restrict__ out, float* __restrict__ lse, int Tn, int H, float scale) {
  using T = typename Ops::elem_t;
  using L = typename Ops::lds_t;
  constexpr int DH = Ops::DH, P = Ops::P, kStep = Ops::kStep, kMaxTiles = Ops::kMaxTiles;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int nt = (Tn + 15) >> 4, Tpad = pad_rows<Ops>(Tn);
  L* Ks = reinterpret_cast<L*>(smem);
  L* Vs = Ks + Tpad * P;
  float* Bs = reinterpret_cast<float*>(smem + attn::lds_bytes<Ops>(Tpad, false));
  const int64_t rs = (int64_t)3 * H * DH;
  Ops::template stage<NW * 64>(qkv + attn::qkv_off<DH>(b, 0, 1, h, Tn, H), rs, attn::SameRows{}, Tn, Tpad, Ks);
  Ops::template stage<NW * 64>(qkv + attn::qkv_off<DH>(b, 0, 2, h, Tn, H), rs, attn::SameRows{}, Tn, Tpad, Vs);
  // a padded key carries kNeg in place of a bias: its K row is zero, so its score is kNeg, as in attn_fwd_kernel
  for (int t = threadIdx.x; t < Tpad; t += NW * 64) Bs[t] = t < Tn ? kbias[(int64_t)b * Tn + t] : kNeg;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  for (int rb = wave; rb < nt; rb += NW) {
    const int row = rb * 16 + l15;
    typename Ops::Own q;
    Ops::load_own(qkv + attn::qkv_off<DH>(b, row < Tn ? row : 0, 0, h, Tn, H), row < Tn, l4, q);
    float s[kMaxTiles][4];
    float m = kNeg;
#pragma unroll
    for (int ct = 0; ct < kMaxTiles; ++ct) {
      if (ct < nt) {
        const f32x4 a = Ops::dot(Ks, ct, q, l15, l4);
        const float4 kb = *reinterpret_cast<const float4*>(Bs + ct * 16 + l4 * 4);
        const float kbs[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[ct][r] = score(a[r], scale, kbs[r]);
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
      if (ct < nt) {
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
      if (kStep * cp < nt) {
        float p[kStep][4];
#pragma unroll
        for (int u = 0; u < kStep; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) p[u][r] = s[kStep * cp + u][r] * inv;
        accum<Ops>(p, Vs, kStep * cp, lane, o);
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

template <class Ops, int NW>
int launch_keybias(const void* qkv, const float* kbias, void* out, float* lse, int B, int Tn, int H, float scale,
                   hipStream_t st) {
  using T = typename Ops::elem_t;
  return attn::launch_sweep<&attn_fwd_keybias_kernel<Ops, NW>, NW>(
      B * H, kb_lds<Ops>(pad_rows<Ops>(Tn)), kb_lds<Ops>(Ops::kMaxRows), st, reinterpret_cast<const T*>(qkv), kbias,
      reinterpret_cast<T*>(out), lse, Tn, H, scale);
}

// the shapes the attention kernels take, and at least one A token besides the class token
bool match_shape_ok(int B, int Tn, int H, int DH) {
  return B > 0 && H > 0 && Tn >= 3 && Tn <= kMaxTokens && (DH == 32 || DH == 64);
}

// workgroups per image of the merge.  A wave walks its rows one after the other, so the loads in flight come from the
// number of waves; every workgroup reads dest and builds the image's lists again.  Measured at batch 128, C = 768
// (profiles/tome_kernels.txt): 8 per image beat 16 and 32 from about 85 tokens on, 16 beat 8 below.
inline int merge_slabs(int B, int To) {
  const bool few = To <= 64;
  int s = ((few ? 2048 : 1024) + B - 1) / B;
  const int cap = (To + 3) / 4, top = few ? 16 : 8;
  s = s < cap ? s : cap;
  s = s < top ? s : top;
  return s < 1 ? 1 : s;
}

}  // namespace tome

extern "C" int passl_hip_tome_match(const void* qkv, int32_t* dest, float* node_max, int32_t* node_idx, int B, int T_,
                                    int H, int DH, int r, int dtype, passl_stream_t stream) {
  if (!qkv || !dest) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  if (B <= 0 || H <= 0 || T_ <= 0 || r <= 0 || r > (T_ - 1) / 2) return PASSL_EINVAL;
  if (!tome::match_shape_ok(B, T_, H, DH)) return PASSL_EUNSUPPORTED;
  if (!aligned16(qkv)) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    constexpr int D = decltype(dh)::value;
    hipLaunchKernelGGL((tome::tome_match_kernel<T, D>), dim3(B), dim3(tome::kMatchThreads), tome::match_lds(T_, D), st,
                       reinterpret_cast<const T*>(qkv), dest, node_max, node_idx, T_, H, r);
    return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
  });)
}

namespace {

// PASSL_OK, or the status the two merge entries return without launching
int merge_shape(int B, int T_, int r, int C, int dtype) {
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  if (B <= 0 || T_ <= 0 || C <= 0 || r <= 0 || r >= T_ || C % 8) return PASSL_EINVAL;
  if (T_ > tome::kMaxTokens) return PASSL_EUNSUPPORTED;
  if ((int64_t)B * T_ > INT32_MAX) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_tome_merge_fwd(const void* x, const float* size, const int32_t* dest, void* y, float* size_out,
                                        float* logsize_out, int B, int T_, int r, int C, int dtype,
                                        passl_stream_t stream) {
  if (!x || !dest || !y || !size_out) return PASSL_EINVAL;
  const int rc = merge_shape(B, T_, r, C, dtype);
  if (rc != PASSL_OK) return rc;
  if (!aligned16(x) || !aligned16(y)) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  const int To = T_ - r, slabs = tome::merge_slabs(B, To);
  PASSL_DISPATCH_DTYPE(dtype,
    hipLaunchKernelGGL(tome::tome_merge_fwd_kernel<T>, dim3((unsigned)(B * slabs)), dim3(tome::kMergeThreads), 0, st,
                       reinterpret_cast<const T*>(x), size, dest, reinterpret_cast<T*>(y), size_out, logsize_out, T_,
                       To, C, slabs);)
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_tome_merge_bwd(const void* dy, const float* size, const float* size_out, const int32_t* dest,
                                        void* dx, int B, int T_, int r, int C, int dtype, passl_stream_t stream) {
  if (!dy || !size_out || !dest || !dx) return PASSL_EINVAL;
  const int rc = merge_shape(B, T_, r, C, dtype);
  if (rc != PASSL_OK) return rc;
  if (!aligned16(dy) || !aligned16(dx)) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  const int64_t rows = (int64_t)B * T_;
  PASSL_DISPATCH_DTYPE(dtype,
    hipLaunchKernelGGL(tome::tome_merge_bwd_kernel<T>, dim3((unsigned)((rows + 3) / 4)), dim3(tome::kMergeThreads), 0,
                       st, reinterpret_cast<const T*>(dy), size, size_out, dest, reinterpret_cast<T*>(dx), rows, T_,
                       T_ - r, C);)
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_attention_fwd_keybias(const void* qkv, const float* key_bias, void* out, float* lse, int B,
                                               int T_, int H, int DH, float scale, int dtype, passl_stream_t stream) {
  if (!qkv || !key_bias || !out || !lse) return PASSL_EINVAL;
  if (B <= 0 || H <= 0 || T_ <= 0 || T_ > attn::kMaxTokens || (DH != 32 && DH != 64)) return PASSL_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  // the routing of passl_hip_attention_fwd: aligned bf16 activations take the bf16-MFMA policy (8 waves unless option
  // attn_waves says 4), everything else the exact-fp32-MFMA policy
  if (dtype == PASSL_BF16 && !passl_opt(Opt::attn_f32mfma) && aligned16(qkv) && aligned16(out)) {
    const bool wide = passl_opt(Opt::attn_waves) != 4;
    return attn::by_head_dim(DH, [&](auto dh) {
      using Ops = abf::Bf16Ops<decltype(dh)::value>;
      return wide ? tome::launch_keybias<Ops, 8>(qkv, key_bias, out, lse, B, T_, H, scale, st)
                  : tome::launch_keybias<Ops, 4>(qkv, key_bias, out, lse, B, T_, H, scale, st);
    });
  }
  PASSL_DISPATCH_DTYPE(dtype, return attn::by_head_dim(DH, [&](auto dh) {
    return tome::launch_keybias<af32::F32Ops<T, decltype(dh)::value>, 4>(qkv, key_bias, out, lse, B, T_, H, scale, st);
  });)
}
