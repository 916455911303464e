// Streaming kernels of CAE pre-training (passl/models/cae.py, tasks/ssl/cae/engine_pretrain.py): the operands of the
// latent regressor's cross-attention, and the latent alignment loss.
//
// Token assembly.  Reference: CAERegressorDecoder / CAEPretrain.forward, cae.py:440-444, 811-815, 1009-1015:
//   pos_embed = self.pos_embed.expand(B); pos_masked = pos_embed[bool_masked_pos]; pos_unmasked = pos_embed[~mask]
//   q_in = x_masked + pos_masked;  v_in = concat(x_unmasked, x_masked);  k_in = v_in + concat(pos_unmasked, pos_masked)
// With the fixed sin-cos table pos fp32 [1 + L, C] (row 0 belongs to the class token) and the index tables of the mask
// the expanded position tensor and the concat copy never exist: one launch, a thread per 8 channels of a row of
// [B, Nu + Nm, C], reads its row of xu or xm and its row of the table once and stores up to three outputs.
// xu is [B, u0 + Nu, C] and is read from row u0 of every image: u0 = 1 skips the class row of the encoder's output
// (x_unmasked[:, 1:], cae.py:1017) without a copy; the backward gives those rows a zero gradient.
//   forward   row t < Nu:   v_in[b, t] = xu[b, t],        k_in[b, t] = xu[b, t] + pos[1 + ids_vis[b, t]]
//             row Nu + j:   v_in[b, Nu + j] = xm[b, j],   k_in[b, Nu + j] = q_in[b, j] = xm[b, j] + pos[1 + ids_msk[b, j]]
//   backward  dxu[b, t] = dk_in[b, t] + dv_in[b, t],      dxm[b, j] = (dq_in[b, j] + dk_in[b, Nu + j]) + dv_in[b, Nu + j]
// Sums in fp32, one rounding at the store.  The table is fixed: there is no dpos.  An index outside [0, L) is clamped,
// so no access leaves the table whatever the tables hold.
//
// MSE.  Reference: engine_pretrain.py:29-31, F.mse_loss(latent_pred.float(), latent_target.float(), 'mean'), the target
// being the teacher's rows after its class row (cae.py:984): pred [B, Tm, C], target [B, Tm + t0, C] read from row t0 of
// every image.  One wave per row forms sum_c (pred - target)^2 in fp32 into the workspace; one workgroup adds the rows
// in a fixed order and divides by B Tm C.  The backward is dpred = gloss 2 (pred - target) / (B Tm C).
#include "common.h"

namespace cae {

constexpr int kThreads = 256;

__device__ __forceinline__ int pos_row(const int32_t* __restrict__ ids, int64_t i, int L) {
  const int id = ids[i];
  return 1 + (id < 0 ? 0 : (id >= L ? L - 1 : id));
}

// rows [row_lo, Nu + Nm) of every image: row_lo = Nu when neither k_in nor v_in is wanted
template <typename T>
__global__ void __launch_bounds__(kThreads) tokens_assemble_kernel(
    const T* __restrict__ xu, const T* __restrict__ xm, const float* __restrict__ pos, const int32_t* __restrict__ ids_vis,
    const int32_t* __restrict__ ids_msk, T* __restrict__ q_in, T* __restrict__ k_in, T* __restrict__ v_in, int64_t n8,
    int row_lo, int u0, int Nu, int Nm, int L, int c8) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n8) return;
  const int rows = Nu + Nm - row_lo;
  const int cp = (int)(i % c8);
  const int64_t r = i / c8, b = r / rows;
  const int t = row_lo + (int)(r % rows);
  float a[8], p[8], s[8];
  int pr;
  if (t < Nu) {
    ElemTraits<T>::load8(xu + ((b * (u0 + Nu) + u0 + t) * c8 + cp) * 8, a);
    pr = pos_row(ids_vis, b * Nu + t, L);
  } else {
    ElemTraits<T>::load8(xm + ((b * Nm + t - Nu) * c8 + cp) * 8, a);
    pr = pos_row(ids_msk, b * Nm + t - Nu, L);
  }
  ElemTraits<float>::load8(pos + ((int64_t)pr * c8 + cp) * 8, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = a[e] + p[e];
  const int64_t o = ((b * (Nu + Nm) + t) * c8 + cp) * 8;
  if (v_in) ElemTraits<T>::store8(v_in + o, a);
  if (k_in) ElemTraits<T>::store8(k_in + o, s);
  if (q_in && t >= Nu) ElemTraits<T>::store8(q_in + ((b * Nm + t - Nu) * c8 + cp) * 8, s);
}

// over [B, Nu + Nm, C / 8]; a NULL gradient counts as zero
template <typename T>
__global__ void __launch_bounds__(kThreads) tokens_assemble_bwd_kernel(
    const T* __restrict__ dq_in, const T* __restrict__ dk_in, const T* __restrict__ dv_in, T* __restrict__ dxu,
    T* __restrict__ dxm, int64_t n8, int row_lo, int u0, int Nu, int Nm, int c8) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n8) return;
  const int rows = Nu + Nm - row_lo;
  const int cp = (int)(i % c8);
  const int64_t r = i / c8, b = r / rows;
  const int t = row_lo + (int)(r % rows);
  const int64_t o = ((b * (Nu + Nm) + t) * c8 + cp) * 8;
  float s[8], a[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  if (t >= Nu && dq_in) ElemTraits<T>::load8(dq_in + ((b * Nm + t - Nu) * c8 + cp) * 8, s);
  if (dk_in) {
    ElemTraits<T>::load8(dk_in + o, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += a[e];
  }
  if (dv_in) {
    ElemTraits<T>::load8(dv_in + o, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += a[e];
  }
  if (t < Nu) {
    ElemTraits<T>::store8(dxu + ((b * (u0 + Nu) + u0 + t) * c8 + cp) * 8, s);
    if (t == 0) {                                        // the skipped leading rows get a zero gradient
      const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int u = 0; u < u0; ++u) ElemTraits<T>::store8(dxu + ((b * (u0 + Nu) + u) * c8 + cp) * 8, z);
    }
  } else {
    ElemTraits<T>::store8(dxm + ((b * Nm + t - Nu) * c8 + cp) * 8, s);
  }
}

// ------------------------------------------------------------------ index tables of a 0/1 mask
// One wave per image walks the mask 64 patches at a time; a patch's place among the visible (masked) ones is the count
// of earlier visible (masked) patches: the running count plus the set bits below its lane in the ballot.  Ascending
// patch order on both sides, the order of the reference's boolean indexing.
//   ids_vis[b, k] = the k-th visible patch,  ids_msk[b, j] = the j-th masked patch,
//   rank[b, l]    = k for a visible patch, Nu + j for a masked one (mae_gather_bwd's ids_restore for the visible side).
// A mask whose count of ones is not L - Nu writes no entry outside the tables and leaves no entry unwritten (zeros).
__global__ void __launch_bounds__(kThreads) mask_ids_kernel(const float* __restrict__ mask, int32_t* __restrict__ ids_vis,
                                                            int32_t* __restrict__ ids_msk, int32_t* __restrict__ rank,
                                                            int B, int L, int Nu) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (b >= B) return;
  const int Nm = L - Nu;
  const unsigned long long below = (1ull << lane) - 1ull;
  int nv = 0, nm = 0;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    const bool valid = l < L;
    const bool m = valid && mask[(int64_t)b * L + l] != 0.f;
    const unsigned long long bm = __ballot(m), bv = __ballot(valid && !m);
    if (m) {
      const int j = nm + __popcll(bm & below);
      if (j < Nm) ids_msk[(int64_t)b * Nm + j] = l;
      rank[(int64_t)b * L + l] = Nu + j;
    } else if (valid) {
      const int k = nv + __popcll(bv & below);
      if (k < Nu) ids_vis[(int64_t)b * Nu + k] = l;
      rank[(int64_t)b * L + l] = k;
    }
    nm += __popcll(bm);
    nv += __popcll(bv);
  }
  for (int j = nm + lane; j < Nm; j += 64) ids_msk[(int64_t)b * Nm + j] = 0;
  for (int k = nv + lane; k < Nu; k += 64) ids_vis[(int64_t)b * Nu + k] = 0;
}

// ------------------------------------------------------------------ mse
// one wave per row of pred; BWD: dpred = g (pred - target), g = gloss 2 / n
template <typename T, bool BWD>
__global__ void __launch_bounds__(kThreads) mse_kernel(const T* __restrict__ pred, const T* __restrict__ target,
                                                       const float* __restrict__ gloss, float* __restrict__ terms,
                                                       T* __restrict__ dpred, int64_t rows, int Tm, int t0, int c8,
                                                       float two_over_n) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t b = row / Tm;
  const int t = (int)(row % Tm);
  const T* pr = pred + row * c8 * 8;
  const T* tr = target + (b * (Tm + t0) + t0 + t) * c8 * 8;
  const float g = BWD ? (gloss ? *gloss : 1.f) * two_over_n : 0.f;
  float acc = 0.f;
  for (int cp = lane; cp < c8; cp += 64) {
    float a[8], c[8];
    ElemTraits<T>::load8(pr + cp * 8, a);
    ElemTraits<T>::load8(tr + cp * 8, c);
    if (BWD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = g * (a[e] - c[e]);
      ElemTraits<T>::store8(dpred + (row * c8 + cp) * 8, a);
    } else {
      float q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = a[e] - c[e]; q[e] = d * d; }
      acc += ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
  }
  if (!BWD) {
    acc = wave_sum(acc);
    if (lane == 0) terms[row] = acc;
  }
}

// out[0] = (sum_i terms[i]) * inv_n in one fixed order: thread t adds t, t + 256, ...; wave shuffles; 4 wave sums in order
__global__ void __launch_bounds__(kThreads) mse_finish_kernel(const float* __restrict__ terms, int64_t n, float inv_n,
                                                              float* __restrict__ out) {
  __shared__ float part[kThreads / 64];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) a += terms[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((part[0] + part[1]) + (part[2] + part[3])) * inv_n;
}

inline bool dtype_ok(int dtype) { return dtype == PASSL_F32 || dtype == PASSL_BF16; }
inline int64_t blocks_for(int64_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace cae

extern "C" int passl_hip_cae_tokens_assemble(const void* xu, const void* xm, const float* pos, const int32_t* ids_vis,
                                             const int32_t* ids_msk, void* q_in, void* k_in, void* v_in, int B, int u0,
                                             int Nu, int Nm, int L, int C, int dtype, passl_stream_t stream) {
  if (!xm || !pos || !ids_msk || (!q_in && !k_in && !v_in)) return PASSL_EINVAL;
  if (B <= 0 || u0 < 0 || Nu < 0 || Nm <= 0 || L <= 0 || C <= 0 || C % 8) return PASSL_EINVAL;
  if (!cae::dtype_ok(dtype)) return PASSL_EUNSUPPORTED;
  const bool kv = k_in || v_in;
  if (kv && Nu > 0 && (!xu || !ids_vis)) return PASSL_EINVAL;
  if (!(aligned16(xu) && aligned16(xm) && aligned16(pos) && aligned16(q_in) && aligned16(k_in) && aligned16(v_in)))
    return PASSL_EINVAL;
  const int row_lo = kv ? 0 : Nu;
  const int64_t n8 = (int64_t)B * (Nu + Nm - row_lo) * (C / 8);
  if (cae::blocks_for(n8) > INT32_MAX) return PASSL_EUNSUPPORTED;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cae::tokens_assemble_kernel<T>, dim3((unsigned)cae::blocks_for(n8)), dim3(cae::kThreads), 0,
                       as_stream(stream), reinterpret_cast<const T*>(xu), reinterpret_cast<const T*>(xm), pos, ids_vis,
                       ids_msk, reinterpret_cast<T*>(q_in), reinterpret_cast<T*>(k_in), reinterpret_cast<T*>(v_in), n8,
                       row_lo, u0, Nu, Nm, L, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_cae_tokens_assemble_bwd(const void* dq_in, const void* dk_in, const void* dv_in, void* dxu,
                                                 void* dxm, int B, int u0, int Nu, int Nm, int C, int dtype,
                                                 passl_stream_t stream) {
  if (!dxm || (!dq_in && !dk_in && !dv_in)) return PASSL_EINVAL;
  if (B <= 0 || u0 < 0 || Nu < 0 || Nm <= 0 || C <= 0 || C % 8) return PASSL_EINVAL;
  if (dxu && Nu == 0) return PASSL_EINVAL;               // no visible row: nobody would write dxu's leading rows
  if (!cae::dtype_ok(dtype)) return PASSL_EUNSUPPORTED;
  if (!(aligned16(dq_in) && aligned16(dk_in) && aligned16(dv_in) && aligned16(dxu) && aligned16(dxm))) return PASSL_EINVAL;
  const int row_lo = dxu ? 0 : Nu;                       // without dxu only the masked rows are visited
  const int64_t n8 = (int64_t)B * (Nu + Nm - row_lo) * (C / 8);
  if (cae::blocks_for(n8) > INT32_MAX) return PASSL_EUNSUPPORTED;
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL(cae::tokens_assemble_bwd_kernel<T>, dim3((unsigned)cae::blocks_for(n8)), dim3(cae::kThreads), 0,
                       as_stream(stream), reinterpret_cast<const T*>(dq_in), reinterpret_cast<const T*>(dk_in),
                       reinterpret_cast<const T*>(dv_in), reinterpret_cast<T*>(dxu), reinterpret_cast<T*>(dxm), n8, row_lo,
                       u0, Nu, Nm, C / 8);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_cae_mask_ids(const float* mask, int32_t* ids_vis, int32_t* ids_msk, int32_t* rank, int B, int L,
                                      int Nu, passl_stream_t stream) {
  if (!mask || !ids_vis || !ids_msk || !rank || B <= 0 || L <= 0 || Nu <= 0 || Nu >= L) return PASSL_EINVAL;
  hipLaunchKernelGGL(cae::mask_ids_kernel, dim3((unsigned)((B + 3) / 4)), dim3(cae::kThreads), 0, as_stream(stream), mask,
                     ids_vis, ids_msk, rank, B, L, Nu);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_mse_fwd(const void* pred, const void* target, float* loss, int B, int Tm, int t0, int C,
                                 int dtype, float* ws, int64_t ws_floats, passl_stream_t stream) {
  if (!pred || !target || !loss || !ws || B <= 0 || Tm <= 0 || t0 < 0 || C <= 0 || C % 8) return PASSL_EINVAL;
  if (!cae::dtype_ok(dtype)) return PASSL_EUNSUPPORTED;
  const int64_t rows = (int64_t)B * Tm;
  if (ws_floats < rows || !aligned16(pred) || !aligned16(target)) return PASSL_EINVAL;
  if ((rows + 3) / 4 > INT32_MAX) return PASSL_EUNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const float inv_n = (float)(1.0 / ((double)rows * C));
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((cae::mse_kernel<T, false>), dim3((unsigned)((rows + 3) / 4)), dim3(cae::kThreads), 0, st,
                       reinterpret_cast<const T*>(pred), reinterpret_cast<const T*>(target), nullptr, ws, nullptr, rows,
                       Tm, t0, C / 8, 0.f);
  })
  hipLaunchKernelGGL(cae::mse_finish_kernel, dim3(1), dim3(cae::kThreads), 0, st, ws, rows, inv_n, loss);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

extern "C" int passl_hip_mse_bwd(const void* pred, const void* target, const float* gloss, void* dpred, int B, int Tm,
                                 int t0, int C, int dtype, passl_stream_t stream) {
  if (!pred || !target || !dpred || B <= 0 || Tm <= 0 || t0 < 0 || C <= 0 || C % 8) return PASSL_EINVAL;
  if (!cae::dtype_ok(dtype)) return PASSL_EUNSUPPORTED;
  const int64_t rows = (int64_t)B * Tm;
  if (!aligned16(pred) || !aligned16(target) || !aligned16(dpred)) return PASSL_EINVAL;
  if ((rows + 3) / 4 > INT32_MAX) return PASSL_EUNSUPPORTED;
  const float two_over_n = (float)(2.0 / ((double)rows * C));
  PASSL_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((cae::mse_kernel<T, true>), dim3((unsigned)((rows + 3) / 4)), dim3(cae::kThreads), 0,
                       as_stream(stream), reinterpret_cast<const T*>(pred), reinterpret_cast<const T*>(target), gloss,
                       nullptr, reinterpret_cast<T*>(dpred), rows, Tm, t0, C / 8, two_over_n);
  })
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}
