// Linear-probe head on gfx950: softmax cross-entropy with integer labels + top-1 / top-5 accuracy
// (forward and backward) over fp32 class scores [N][C].
//
// Reference: ClasHead.loss + accuracy, passl_v110/modeling/heads/clas_head.py:47-72
//   loss = mean_i (logsumexp(s_i) - s_i[label_i]);  acc_k = 100/N * #{i : label_i in top-k(s_i)}
// One wave per row (C = 1000: 16 scores per lane): row max / sum-exp by wave reductions; the
// label's rank = #{j : s_ij > s_i,label or (s_ij == s_i,label and j < label)} (ties resolve to the
// lower index, as a sorted top-k does), so no sort / top-k selection is materialised.
// A label outside [0, C) makes the loss NaN (the reference raises inside Paddle's kernel).
#include <math.h>
#include "common.h"
#include "terms_finish.h"

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) softmax_ce_fwd_kernel(const float* __restrict__ s,
                                                                  const int64_t* __restrict__ labels,
                                                                  int N, int C, float* __restrict__ lse,
                                                                  float* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* r = s + (int64_t)row * C;
  const int64_t lab = labels[row];
  const bool ok = lab >= 0 && lab < C;
  const float sl = ok ? r[lab] : 0.f;
  float m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, r[j]);
  m = wave_max(m);
  float z = 0.f, cnt = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float v = r[j];
    z += __expf(v - m);
    cnt += (v > sl || (v == sl && j < lab)) ? 1.f : 0.f;
  }
  z = wave_sum(z);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    const float l = m + __logf(z);
    lse[row] = l;
    const float invN = 1.0f / (float)N;
    terms[row] = ok ? (l - sl) * invN : NAN;               // [3][N]: loss term, top-1 hit, top-5 hit
    terms[N + row] = (ok && cnt < 0.5f) ? 100.0f * invN : 0.f;
    terms[2 * N + row] = (ok && cnt < 4.5f) ? 100.0f * invN : 0.f;
  }
}

// ds[i][j] = g/N (exp(s_ij - lse_i) - [j == label_i])
__global__ void __launch_bounds__(kThreads) softmax_ce_bwd_kernel(const float* __restrict__ s,
                                                                  const float* __restrict__ lse,
                                                                  const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ gloss, int N,
                                                                  int C, float* __restrict__ ds) {
  const int64_t total = (int64_t)N * C;
  const float k = *gloss / (float)N;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kThreads) {
    const int i = (int)(e / C), j = (int)(e % C);
    ds[e] = k * (__expf(s[e] - lse[i]) - (labels[i] == j ? 1.0f : 0.0f));
  }
}

// ---- ViTCELoss(type='sigmoid'), passl/loss/celoss.py:58-95: binary cross entropy with logits against the target
// t = onehot * (1 - eps) + eps, summed over the classes, mean over the rows.  The target is two numbers (t_on at the
// label, t_off elsewhere, rounded once by the caller): no dense target exists.
//   term(x, t) = max(x, 0) - x t + log1p(exp(-|x|));   d term / dx = sigmoid(x) - t
// One wave per row; a label outside [0, C) makes the row NaN (F.one_hot raises in the reference).
__global__ void __launch_bounds__(kThreads) sigmoid_ce_fwd_kernel(const float* __restrict__ s,
                                                                  const int64_t* __restrict__ labels, int N, int C,
                                                                  float t_on, float t_off,
                                                                  float* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* r = s + (int64_t)row * C;
  const int64_t lab = labels[row];
  float a = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float x = r[j];
    a += fmaxf(x, 0.f) - x * (j == lab ? t_on : t_off) + log1pf(expf(-fabsf(x)));
  }
  a = wave_sum(a);
  if (lane == 0) terms[row] = (lab >= 0 && lab < C) ? a / (float)N : NAN;
}

// ds[i][j] = (sigmoid(s_ij) - t_ij) * (g / N)
__global__ void __launch_bounds__(kThreads) sigmoid_ce_bwd_kernel(const float* __restrict__ s,
                                                                  const int64_t* __restrict__ labels,
                                                                  const float* __restrict__ gloss, int N, int C,
                                                                  float t_on, float t_off, float* __restrict__ ds) {
  const int64_t total = (int64_t)N * C;
  const float k = *gloss / (float)N;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kThreads) {
    const int i = (int)(e / C), j = (int)(e % C);
    const float sig = 1.0f / (1.0f + expf(-s[e]));
    ds[e] = (sig - (labels[i] == j ? t_on : t_off)) * k;
  }
}

}  // namespace

// ws: N floats (the rows' loss terms, each already divided by N; summed in a fixed order into out[0])
extern "C" int passl_hip_sigmoid_ce_fwd(const float* scores, const int64_t* labels, int N, int C, float t_on,
                                        float t_off, float* out, float* ws, int64_t ws_floats,
                                        passl_stream_t stream) {
  if (!scores || !labels || !out || !ws || N <= 0 || C <= 0 || ws_floats < (int64_t)N) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sigmoid_ce_fwd_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, st, scores, labels, N, C, t_on,
                     t_off, ws);
  hipLaunchKernelGGL(terms_finish_kernel<1>, dim3(1), dim3(64), 0, st, ws, N, out);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_sigmoid_ce_bwd(const float* scores, const int64_t* labels, const float* gloss, int N, int C,
                                        float t_on, float t_off, float* dscores, passl_stream_t stream) {
  if (!scores || !labels || !gloss || !dscores || N <= 0 || C <= 0) return PASSL_EINVAL;
  int64_t g = ((int64_t)N * C + kThreads - 1) / kThreads;
  if (g > 65535 * 4) g = 65535 * 4;
  hipLaunchKernelGGL(sigmoid_ce_bwd_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream), scores, labels,
                     gloss, N, C, t_on, t_off, dscores);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

// ws: 3 * N floats (per-row loss term and top-1 / top-5 hits, summed in a fixed order)
extern "C" int passl_hip_softmax_ce_fwd(const float* scores, const int64_t* labels, int N, int C,
                                        float* lse, float* out, float* ws, int64_t ws_floats,
                                        passl_stream_t stream) {
  if (!scores || !labels || !lse || !out || !ws || N <= 0 || C <= 0 || ws_floats < 3 * (int64_t)N)
    return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(softmax_ce_fwd_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, st, scores, labels, N,
                     C, lse, ws);
  hipLaunchKernelGGL(terms_finish_kernel<3>, dim3(1), dim3(192), 0, st, ws, N, out);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_softmax_ce_bwd(const float* scores, const float* lse, const int64_t* labels,
                                        const float* gloss, int N, int C, float* dscores,
                                        passl_stream_t stream) {
  if (!scores || !lse || !labels || !gloss || !dscores || N <= 0 || C <= 0) return PASSL_EINVAL;
  int64_t g = ((int64_t)N * C + kThreads - 1) / kThreads;
  if (g > 65535 * 4) g = 65535 * 4;
  hipLaunchKernelGGL(softmax_ce_bwd_kernel, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream),
                     scores, lse, labels, gloss, N, C, dscores);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
