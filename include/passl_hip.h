/*
 * passl_hip.h — C ABI of libpassl_hip.so: the MI355X (gfx950) kernels behind the
 * MoCo-v2 ResNet-50 data-parallel training step.
 *
 * PASSL (the reference) is 100 % Python and has NO FFI / operator boundary of its own:
 * every op on the hot path is a PaddlePaddle call made from Python
 * (SURVEY.md §8b).  This header therefore defines the boundary a maintainer would bind
 * (ctypes — see INTEGRATION.md); each entry point cites the reference call site whose
 * Paddle op(s) it replaces.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *   - every function enqueues work on `stream` (hipStream_t passed as void*) and returns
 *     immediately: no allocation, no host synchronisation, graph-capture safe
 *   - returns 0 on success, negative passl_status otherwise (argument errors are detected
 *     before anything is launched)
 *   - activations are NHWC ("channels-last"), channel count a multiple of 8;
 *     `dtype` selects the arithmetic/storage type of activations and packed weights:
 *     PASSL_F32 (exact-fp32 MFMA, parity runs) or PASSL_BF16 (bf16 storage, fp32 accumulate)
 *   - master parameters, gradients, optimizer state, BN statistics, q/k/queue are fp32
 */
#ifndef PASSL_HIP_H_
#define PASSL_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* passl_stream_t;

enum passl_status {
  PASSL_OK = 0,
  PASSL_EINVAL = -1,       /* bad argument (null pointer, misaligned, unsupported shape) */
  PASSL_ELAUNCH = -2,      /* hipLaunch failed */
  PASSL_EUNSUPPORTED = -3  /* dtype/shape combination not built */
};

enum passl_dtype { PASSL_F32 = 0, PASSL_BF16 = 1 };

/* The value passl_hip_abi_version() of a library built from THIS header returns: a caller compiled against another
 * layout of the descriptors below must not call it (tools/kbench and passl_amd/hip/lib.py check at start-up). */
#define PASSL_HIP_ABI_VERSION 16
int passl_hip_abi_version(void);
/* Tuning and diagnostic options: they choose kernels (defaults are tuned for MI355X; tests and A/B runs use them to
 * force a path).  Each option takes its default, then, once, on the first access to any option, the value of the
 * environment variable PASSL_<NAME in upper case> (igemm_ring: PASSL_IGEMM_RING) when that is set; a value that does not
 * parse or is not accepted is reported on stderr and the default kept.  passl_hip_set_option then sets a value,
 * passl_hip_get_option reads it back.  "any" = any int, a boolean is "!= 0".  The table: passl_amd/csrc/options.h.
 *   name                   values        default
 *   igemm_ring             any           1     the LDS-DMA ring conv kernel where it applies
 *   igemm_ring_min_nk      any           8     ... only for reductions of at least n 64-element K-tiles
 *   igemm_ring_min_tiles   any           1     ... and launches with at least n output tiles
 *   igemm_ring_bm          128|256       128   its row tile: 128 (4 waves, 2 LDS stages, two workgroups per CU) or
 *                                              256 (8 waves, 3 stages, one)
 *   igemm_ring_bk          32|64         64    its K-tile
 *   igemm_ring_stages32    3|4           4     ring depth of the BK = 32 form
 *   igemm_8p               0..2          1     the 256 x 256-tile 8-phase kernel: never / when its cost model prefers it
 *                                              to the ring kernel / whenever the launch is inside its envelope
 *   igemm_8p_min_nk        >= 1          8     ... (mode 1) only for reductions of at least n 64-element K-tiles
 *   igemm_8p_direct        any           1     ... its persistent form (stores from the accumulators)
 *   igemm_8p_dense         0..2          1     ... its matrix-operand form: off / persistent form / also the staged form
 *   igemm_8p_tk            >= 1          145   ... the cost model's constants (conv_igemm_8p.hip), in 0.01 us:
 *   igemm_8p_te            >= 1          1000        per K-tile / per tile (prologue + epilogue) of the staged form,
 *   igemm_8p_te_direct     >= 1          900         per tile of the persistent form,
 *   igemm_8p_ring_tk       >= 1          112         per K-tile / per tile of the ring kernel;
 *   igemm_8p_ring_te       >= 1          420
 *   igemm_8p_margin        >= 1          100         margin in %
 *   conv3x3_wave           any           1     the wave-per-patch kernel (conv3x3_wave.hip) for 3x3 / stride 1 / pad 1
 *                                              launches with 64 input and 64 output channels whose image sides are
 *                                              multiples of 8 (ResNet-50 stage 1, forward and data gradient)
 *   conv3x3_wave_rows      4|8           4     ... 4 x 8 patches on eight waves / 8 x 8 patches on four
 *   conv3x3_wave_modes     0..7          7     ... bit mask of the launches that take it: 1 plain / affine / ReLU,
 *                                              2 fused statistics, 4 BatchNorm-backward sums
 *   conv3x3_wave_dbg       any           0     ... ablation bits: 1 no statistics, 2 no epilogue, 4 no MFMA,
 *                                              8 no halo loads
 *   igemm_persist          any           0     persistent form of the register-staged kernel for dense 1x1 launches
 *                                              (bit-identical, measured slower: profiles/r06_negative_results.txt)
 *   igemm_persist_grid     >= 0          0     ... its grid, rounded down to a multiple of 8 (0: resident workgroups)
 *   igemm_nk1              any           24    register-staged kernel: K-tiles up to which the single-stage form runs
 *   igemm_lean             0|1           1     ... the 4-workgroup form of the single-K-tile dense launches
 *   igemm_dbg              0..63         0     ... ablation bits: 1 no stores, 2 no epilogue, 4 no A loads, 8 no MFMA,
 *                                              16 no statistics reduction, 32 no statistics arithmetic
 *   stem_kernel            any           1     the dedicated kernel of the bf16 stem convolution (conv_stem.hip)
 *   wgrad_dma              0|1           1     bf16 weight gradients through the LDS-DMA kernels
 *   wgrad_tile             any           0     ... their tile: by shape / 1 64x64, 2 64x128, 3 128x64, 4 128x128
 *   wgrad_pipe             any           2     ... the register double-buffered kernel: 0 off, 1 dense 128x128 shapes
 *                                              with 4 x 32-row stages, 2 every shape with 2 x 64-row stages
 *   wgrad_halo             0..2          2     spatially tiled 3x3 / stride 1 weight gradients (conv_wgrad_halo.inc):
 *                                              off / images whose sides are multiples of 8 / every such layer (the
 *                                              8 x 8 patches overhang, out-of-image pixels are fetched as zeros).  Its
 *                                              grid is one workgroup per 64 x 64 block of dw and slice: pass ~512 /
 *                                              blocks slices
 *   wgrad_halo_stages      2|3           2     ... its LDS stages
 *   wgrad_dbg              0|1           0     weight gradients: 1 skips the epilogue stores (ablation)
 *   bn_stream_unroll       0|2|4|8       4     BatchNorm streaming kernels: grid-stride / tile form of U chunks per lane
 *   stem_pool_form         0|1           1     passl_hip_bn_relu_maxpool_bwd_reduce: one 2048-item block per workgroup /
 *                                              workgroups that walk over their share of the items with the next
 *                                              item's loads in flight (tensors below 2^30 elements)
 *   stem_pool_wgs          1..65536      1024  ... workgroups of the latter.  Both stem_pool options change what
 *                                              passl_hip_bn_relu_maxpool_blocks returns: set them before sizing a slab
 *   attn_f32mfma           0|1           0     bf16 attention through the exact-fp32-MFMA kernels
 *   attn_waves             0|4|8         0     waves per workgroup of the bf16 attention kernels (0: by sequence length)
 * passl_hip_set_option returns PASSL_EINVAL for an unknown name or a value outside the option's values. */
int passl_hip_set_option(const char* name, int value);
/* The current value of an option; PASSL_EINVAL for an unknown name or a NULL `value`. */
int passl_hip_get_option(const char* name, int* value);
/* Which kernel the most recent passl_hip_conv_igemm call of this process launched: 0 = igemm_kernel
 * (register-staged), 1 = igemm_ring_kernel, 2 = stem_kernel, 3 = igemm_8p_kernel, 4 = conv3x3_wave_kernel; -1
 * before the first call.
 * Diagnostics for tests and benchmarks (not thread-safe). */
int passl_hip_last_igemm_kernel(void);
/* Human readable text for a passl_status. */
const char* passl_hip_strerror(int status);

/* ---------------------------------------------------------------- flat-buffer ops */

/* k[i] = k[i]*m + q[i]*(1-m) over a flat fp32 buffer; if k_lp != NULL also writes the bf16
 * copy of the new k (the key encoder's compute weights).
 * Replaces the 269 per-tensor paddle.assign launches of
 * MoCo._momentum_update_key_encoder, passl_v110/modeling/architectures/moco.py:82-90. */
int passl_hip_ema_update(float* k, const float* q, void* k_lp, int64_t n, float m,
                         passl_stream_t stream);

/* Inference-form BatchNorm affine of ALL layers of an encoder in one launch (the key encoder's fused
 * BN: scale folded into the conv epilogues): for i < n
 *   scale[i] = flat[gamma_idx[i]] * rsqrt(flat[var_idx[i]] + eps)
 *   shift[i] = flat[beta_idx[i]] - flat[mean_idx[i]] * scale[i]
 * The index lists address the encoder's flat parameter/statistics buffer.  Replaces the per-layer
 * running-statistics BatchNorm of the frozen key encoder (passl_v110/modules/freeze.py:18-23 +
 * paddle.nn.BatchNorm2D in eval form). */
int passl_hip_bn_fold(const float* flat, const int64_t* gamma_idx, const int64_t* beta_idx,
                      const int64_t* mean_idx, const int64_t* var_idx, int64_t n, float eps,
                      float* scale, float* shift, passl_stream_t stream);

/* Momentum-SGD with L2 decay folded into the gradient, over flat fp32 buffers:
 *   g' = g*grad_scale + wd*p;  v = mu*v + g';  p = p - lr*v
 * Replaces paddle.optimizer.Momentum.step() called from
 * passl_v110/hooks/optimizer_hook.py:43-47 (rule restated in-tree at
 * passl/optimizer/momentum.py:150-158). */
int passl_hip_momentum_sgd(float* p, const float* g, float* v, int64_t n, float lr, float mu,
                           float wd, float grad_scale, passl_stream_t stream);
/* The same update with the learning rate read from DEVICE memory (hyper[0]) when the kernel runs: the value of
 * a launch is not frozen at enqueue time, so a captured HIP graph of the training step can be replayed while the
 * schedule (reference passl_v110/hooks/lr_scheduler_hook.py:26-28, stepped every iteration) moves on — the host
 * writes the new value into pinned memory, a captured H2D copy node carries it to `hyper`. */
int passl_hip_momentum_sgd_dev(float* p, const float* g, float* v, int64_t n, const float* hyper, float mu,
                               float wd, float grad_scale, passl_stream_t stream);

/* LARS momentum over a flat fp32 buffer holding many parameter tensors ("segments").
 * The buffer is cut into blocks of at most 4096 elements, each inside ONE segment
 * (blk_off: element offset, which MUST be a multiple of 4: with p, g, v 16-byte aligned the kernels read and write
 * float4 at p + blk_off + 4 i; blk_len; blk_seg: segment index); per segment s:
 *   local_lr = lr*lars_coeff*|p_s| / (|g_s| + wd_s*|p_s| + epsilon)   if wd_s > 0, |p_s| > 0, |g_s| > 0
 *            = lr                                                     otherwise
 *   v = mu*v + local_lr*(g*grad_scale + wd_s*p);   p = p - v
 * norms: caller-owned fp32 workspace of 2*(n_seg + n_blocks) floats ([n_seg][2] squared norms followed by
 * the per-block partial sums; fully written).  blk_seg must be ascending (the blocks of one parameter are
 * consecutive).  Three launches (per-block partial sums, fixed-order per-parameter reduction — no atomics,
 * so data-parallel replicas compute bit-identical local learning rates — and the update).
 * Replaces paddle.fluid.optimizer.LarsMomentumOptimizer.minimize called from
 * passl_v110/hooks/optimizer_hook.py:44-45 (registered at passl_v110/solver/optimizer.py:25). */
int passl_hip_lars_momentum(float* p, const float* g, float* v, const int64_t* blk_off,
                            const int32_t* blk_len, const int32_t* blk_seg, int n_blocks,
                            const float* seg_wd, int n_seg, float* norms, float lr, float mu,
                            float lars_coeff, float epsilon, float grad_scale,
                            passl_stream_t stream);
/* ... with lr = hyper[0] read on the device (see passl_hip_momentum_sgd_dev). */
int passl_hip_lars_momentum_dev(float* p, const float* g, float* v, const int64_t* blk_off,
                                const int32_t* blk_len, const int32_t* blk_seg, int n_blocks,
                                const float* seg_wd, int n_seg, float* norms, const float* hyper, float mu,
                                float lars_coeff, float epsilon, float grad_scale, passl_stream_t stream);

/* MomentumLARC over the same segmented flat buffer and workspace (blk_*, seg_wd, norms as above), lr = hyper[0]:
 *   if |p_s| != 0 and |g_s| != 0:  a = trust_coefficient*|p_s| / (|g_s| + |p_s|*wd_s + epsilon)
 *                                  (clip != 0: a = min(a / lr, 1));   g' = a*(g*grad_scale + wd_s*p)
 *   else                        :  g' = g*grad_scale                 (no weight decay)
 *   v = mu*v + g';   p = p - lr*v
 * Replaces passl/optimizer/momentum_larc.py:56-111 (MomentumLARC.step: a Python loop of per-tensor norm / scale /
 * copy ops), the optimizer of tasks/ssl/simsiam/configs/simsiam_resnet50_lp_in1k_1n8c_dp_fp32.yaml. */
int passl_hip_larc_momentum_dev(float* p, const float* g, float* v, const int64_t* blk_off,
                                const int32_t* blk_len, const int32_t* blk_seg, int n_blocks,
                                const float* seg_wd, int n_seg, float* norms, const float* hyper, float mu,
                                float trust_coefficient, float epsilon, int clip, float grad_scale,
                                passl_stream_t stream);

/* dst_bf16[i] = bf16(src[i]) (round-to-nearest-even). */
int passl_hip_cast_f32_to_bf16(const float* src, void* dst, int64_t n, passl_stream_t stream);

/* Weight (re)packing for the implicit-GEMM kernels.  One launch executes `n_jobs` jobs read
 * from device memory; each job writes   dst[c][tr][ts][k] (or [k][tr][ts][c] when
 * !transpose) = src[k][r_base + tr*r_step][s_base + ts*s_step][c]   from the fp32 master
 * weights (physically [K][R][S][C]) into the compute-dtype buffer.  `jobs` is an array of
 * passl_pack_job, `block_job`/`block_start` map each 256-thread block to (job, first element). */
typedef struct passl_pack_job {
  int64_t src_off;   /* element offset into src (fp32) */
  int64_t dst_off;   /* element offset into dst (compute dtype) */
  int32_t K, R, S, C;          /* source dims */
  int32_t TR, TS;              /* taps kept */
  int32_t r_base, r_step, s_base, s_step;
  int32_t transpose;           /* 1: dst is [C][TR][TS][K]; 0: dst is [K][TR][TS][C];
                                * fast paths chosen by the host for whole-tensor jobs: 2 = R=S=1 transpose
                                * dst[c][k] = src[k][c] (block_start = index of a 32x32 tile, k fastest),
                                * 3 = contiguous cast dst[e] = src[e] (block_start = first element) */
  int32_t c_pad;               /* dst innermost-dim padding: dst C (or K) dim is c_pad wide (>= C), zero filled; 0 = no pad */
} passl_pack_job;
int passl_hip_pack_weights(const float* src, void* dst, int dtype, const passl_pack_job* jobs,
                           const int32_t* block_job, const int32_t* block_start, int n_blocks,
                           passl_stream_t stream);

/* x fp32 NCHW [N,C,H,W] -> y NHWC [N, H+2*pad, Wp, Cp] in `dtype`, zero border / zero extra
 * channels (Wp >= W+2*pad, Cp >= C).  The stem conv reads this padded image.
 * Replaces the NCHW input handling of paddle.nn.Conv2D at
 * passl_v110/modeling/backbones/resnetimagenet.py:190-195. */
int passl_hip_nchw_to_nhwc_pad(const float* x, void* y, int N, int C, int H, int W, int pad,
                               int Wp, int Cp, int dtype, passl_stream_t stream);

/* ---------------------------------------------------------------- implicit-GEMM convolution */

/* One descriptor drives forward convs, data-gradient convs (as convs over dy with repacked
 * weights, optionally writing a strided sub-lattice of dx) and Linear layers (1x1, OP=OQ=1).
 *
 *   y[n,op,oq,col] = epi( sum_{r,s,c} A[n, op*sh + r - ph, oq*sw + s - pw, c] * B[col][r][s][c] )
 *   epi(v) = relu?( v*scale[col] + shift[col] + residual[n,op,oq,col] )
 *
 * A is addressed with explicit element strides (a_sn,a_sh,a_sw; channel stride 1); taps
 * outside [0,IH)x[0,IW) contribute zero.  B is [NCOLS][R*S*C] row-major in `dtype`.
 * If C is not a multiple of the K-tile (64 bf16 / 32 fp32) the kernel decomposes k per
 * 16-byte chunk (stem).  Output rows are addressed with (y_sn,y_sh,y_sw), channel stride 1.
 * Replaces paddle.nn.Conv2D / nn.Linear forward+backward-data as used by
 * resnetimagenet.py:114-131,190-198,216-224 and necks/base_neck.py:80-97. */
typedef struct passl_conv_desc {
  const void* a;
  const void* b;
  void* y;
  const float* scale;      /* [NCOLS] or NULL (=1) */
  const float* shift;      /* [NCOLS] or NULL (=0) */
  const void* residual;    /* addressed like y, dtype = out dtype; or NULL */
  float* stats;            /* NULL, or the slab of fused BatchNorm statistics of the STORED output values
                              (bf16 output without residual only): stats_tiles = ceil(M/128) row tiles,
                                stats[t][col][0..1] = sum (v - s), sum (v - s)^2 over the rows of tile t,
                                s = shifts[t][col] = the tile's first-row value, stored behind the sums at
                                stats + stats_tiles*NCOLS*2 (shifted sums: no cancellation).
                              stats_tiles*NCOLS*3 floats, fully written by plain stores (no atomics, no
                              zeroing): feed it to passl_hip_bn_finalize with nblocks = stats_tiles,
                              rows_per_block = 128. */
  /* BatchNorm-backward statistics fused into a data-gradient launch (all NULL/0 when unused).  The
   * launch's output is the gradient w.r.t. the OUTPUT of a BatchNorm(+ReLU) layer whose input was
   * bnb_y (addressed like y).  The epilogue masks the gradient with that layer's ReLU mask
   * (bnb_relu: 0 none, 2 recomputed as bnb_y*bnb_scale + bnb_shift > 0, 3 bit mask bnb_mask as written
   * by passl_hip_bn_apply), STORES the masked gradient g, and writes per 128-row tile t
   *   bnb_partial[bnb_tile_off + t][col][0..1] = sum g, sum g * (bnb_y - bnb_mean[col]) * bnb_invstd[col]
   * (plain stores; passl_hip_bn_bwd_finalize consumes the slab, passl_hip_bn_bwd_reduce never runs).
   * bf16 only; relu must be 0. */
  const void* bnb_y;
  const uint8_t* bnb_mask;
  const float* bnb_mean;
  const float* bnb_invstd;
  const float* bnb_scale;
  const float* bnb_shift;
  float* bnb_partial;
  int32_t N, OP, OQ;       /* M = N*OP*OQ */
  int32_t NCOLS;
  int32_t R, S, C;
  int32_t IH, IW;
  int32_t sh, sw, ph, pw;
  int64_t a_sn, a_sh, a_sw;
  int64_t y_sn, y_sh, y_sw;
  int32_t relu;
  int32_t dtype;           /* passl_dtype of A, B */
  int32_t out_f32;         /* 1: y (and residual) are fp32 regardless of dtype */
  int32_t stats_tiles;     /* must equal ceil(N*OP*OQ / 128) when stats != NULL */
  int32_t bnb_relu;
  int32_t bnb_tile_off;    /* first slab row of this launch (residue-class launches share one slab) */
  /* A SECOND BatchNorm fed by the same gradient (all NULL = none; needs bnb_partial).  The output of a bottleneck block
   * with a downsample branch is relu(bn3(y3) + bn_ds(y_ds)): the masked gradient g this launch stores is the output
   * gradient of BOTH BatchNorm layers.  With bnb2_* set the epilogue also writes, per 128-row tile t,
   *   bnb2_partial[bnb_tile_off + t][col][0..1] = sum g, sum g * (bnb2_y - bnb2_mean[col]) * bnb2_invstd[col]
   * (bnb2_y addressed like y), so the second layer's backward needs no reduce pass over (g, bnb2_y) either.
   * Built for dense 1x1 / stride-1 launches with C % 64 == 0 and NCOLS >= 128 (the conv1 data gradients that follow a
   * downsample block: resnetimagenet.py:139-153); PASSL_EUNSUPPORTED otherwise — launch without and run
   * passl_hip_bn_bwd_reduce for the second layer. */
  const void* bnb2_y;
  const float* bnb2_mean;
  const float* bnb2_invstd;
  float* bnb2_partial;
} passl_conv_desc;
int passl_hip_conv_igemm(const passl_conv_desc* d, passl_stream_t stream);

/* The same launch with a transform of the A operand on its way into the kernel ("A-operand prologue"): the apply pass of
 * the BatchNorm whose output the convolution consumes, done by the convolution.  The kernel reads the BatchNorm's INPUT
 * as `d->a`, transforms every 8-channel chunk with the arithmetic of passl_hip_bn_apply / passl_hip_bn_bwd_apply (the
 * same device functions: bit-identical values), multiplies with the transformed chunk, and — workgroups of the first
 * column block only — stores it once to `a_out` (dense, same shape and dtype as `d->a`), where the weight gradient reads
 * it later.  a_out must not alias d->a or d->y.
 *   PASSL_APRO_BN_FWD  a_out = relu(a * a_scale[c] + a_shift[c])                    (a_scale, a_shift: fp32 [C])
 *   PASSL_APRO_BN_BWD  a_out = a_coef[c] * a + a_coef[C + c] * a2 + a_coef[2C + c]  (a = masked gradient g, a2 = the
 *                      BatchNorm's input, addressed like a; a_coef: the fp32 [3][C] of passl_hip_bn_bwd_finalize)
 * Everything else (epilogue, fused statistics, bnb_*) is passl_hip_conv_igemm's.  Served by the register-staged kernel
 * only: bf16, dense 1x1 / stride 1 / pad 0 launches with C % 64 == 0 and C < 512 and bf16 output, without bnb2_*;
 * BN_FWD with NCOLS > 64, BN_BWD with NCOLS <= 64 (one column block: every chunk is loaded once), not with option
 * igemm_persist.  Anything else: PASSL_EUNSUPPORTED and nothing is launched — run the streaming pass and
 * passl_hip_conv_igemm instead. */
enum passl_apro_mode { PASSL_APRO_BN_FWD = 1, PASSL_APRO_BN_BWD = 2 };
typedef struct passl_conv_apro {
  const void* a2;
  const float* a_scale;
  const float* a_shift;
  const float* a_coef;
  void* a_out;
  int32_t mode;            /* passl_apro_mode */
} passl_conv_apro;
int passl_hip_conv_igemm_apro(const passl_conv_desc* d, const passl_conv_apro* pro, passl_stream_t stream);

/* Weight gradient:  dw[col][r][s][c] += sum_{n,op,oq} dy[n,op,oq,col] * A[n, op*sh+r-ph, oq*sw+s-pw, c]
 * dw is fp32 [NCOLS][R*S*C] and is ACCUMULATED into (caller zeroes it).
 * dy is [M][NCOLS] dense (row stride dy_ld elements).  `splits` = number of M-slices (>=1): every
 * slice is one partial tile set.  With a workspace `ws` of at least splits*NCOLS*R*S*C floats
 * (`ws_floats`) each slice writes its tiles into its own slab and a second launch adds the slabs to dw
 * in slice order — bit-reproducible.  ws == NULL: slices > 1 accumulate with fp32 atomics (order-
 * dependent rounding).  The workspace may be shared by all layers (stream-ordered use).
 * Replaces Conv2D/Linear backward-filter (autograd of the call sites above). */
typedef struct passl_wgrad_desc {
  const void* a;
  const void* dy;
  float* dw;
  int32_t N, OP, OQ;
  int32_t NCOLS;
  int32_t R, S, C;
  int32_t IH, IW;
  int32_t sh, sw, ph, pw;
  int64_t a_sn, a_sh, a_sw;
  int64_t dy_ld;
  float* ws;               /* NULL or the split workspace (16-byte aligned) */
  int64_t ws_floats;
  int32_t dtype;
  int32_t splits;
} passl_wgrad_desc;

/* out[i] (+)= sum_{z < slabs} ws[z*n + i], slabs added in ascending order (fixed-order replacement of
 * atomic accumulation); n % 4 == 0, 16-byte aligned pointers. */
int passl_hip_slab_reduce(const float* ws, float* out, int64_t n, int slabs, int accumulate,
                          passl_stream_t stream);
int passl_hip_conv_wgrad(const passl_wgrad_desc* d, passl_stream_t stream);

/* ---------------------------------------------------------------- BatchNorm (+ReLU, +residual) */

/* Training-mode BN over NHWC rows x[M][C].  Three launches:
 *  stats:     slab b = rows [b*rpb, (b+1)*rpb), rpb = ceil(M/nblocks):
 *             partial[b][c][0..1] = sum (x - s), sum (x - s)^2 with s = shifts[b][c] = the slab's first row,
 *             shifts stored behind the sums at partial + nblocks*C*2  (nblocks*C*3 floats in total;
 *             shifted sums: the variance never comes from E[x^2] - mean^2 of large numbers).
 *             The conv epilogue writes the same layout with rpb = 128 (passl_conv_desc.stats).
 *  finalize:  fixed-order fp64 combine of the slabs (re-centred on slab 0's shift; ONE launch for any slab
 *             height since ABI 14) -> mean/invstd
 *             (biased var, eps), scale=gamma*invstd, shift=beta-mean*scale,
 *             running = momentum*running + (1-momentum)*batch   [Paddle: momentum 0.9, biased var]
 *  apply:     z = relu?( x*scale + shift + residual )
 * No atomics anywhere: results are bit-reproducible run to run.
 * Replaces paddle.nn.BatchNorm2D + ReLU (+ `out += identity`) at
 * resnetimagenet.py:133-153,196-197,236-238. */
/* Size (floats) of a `partial` buffer for nblocks slabs of C channels: the slab itself — [nblocks][C][2]
 * sums (+ [nblocks][C] shifts when shifted != 0: forward statistics) — followed by the fp64 scratch the
 * finalize kernels use to combine tall slabs segment by segment.  Every `partial` handed to
 * passl_hip_bn_finalize / passl_hip_bn_bwd_finalize (and the conv descriptor's `stats` / `bnb_partial`)
 * must be this large. */
int64_t passl_hip_bn_partial_floats(int nblocks, int C, int shifted);
int passl_hip_bn_stats(const void* x, float* partial, int64_t M, int C, int nblocks, int dtype,
                       passl_stream_t stream);
int passl_hip_bn_finalize(const float* partial, int nblocks, int64_t M, int C, int rows_per_block,
                          const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* mean, float* invstd, float* scale,
                          float* shift, passl_stream_t stream);
/* relu_mask (optional, needs relu): one bit per element of z (bit e of byte i <-> element 8*i+e,
 * set where z > 0), M*C/8 bytes — the ReLU mask the backward kernels can read instead of z. */
int passl_hip_bn_apply(const void* x, const float* scale, const float* shift, const void* residual,
                       void* z, uint8_t* relu_mask, int64_t M, int C, int relu, int dtype,
                       passl_stream_t stream);
/* Backward.  g = dz * relu-mask;   reduce: partial[b][c] = (sum g, sum g*xhat);
 * finalize: dgamma += .., dbeta += .. (accumulated) and the per-channel coefficients (A,B,Cc)
 *           of dx = A*g + B*x + Cc;
 * apply: writes dx and, if dres != NULL, dres = g (gradient of the residual branch).
 * `relu` selects where the ReLU mask comes from: 0 no ReLU; 1 `z` is the forward output
 * (mask z > 0); 2 recomputed as x*scale + shift > 0 from the forward's scale/shift (BN+ReLU
 * without residual: z is never read); 3 `z` is the bit mask written by passl_hip_bn_apply. */
int passl_hip_bn_bwd_reduce(const void* dz, const void* z, const void* x, const float* mean,
                            const float* invstd, const float* scale, const float* shift,
                            float* partial, int64_t M, int C, int nblocks, int relu, int dtype,
                            passl_stream_t stream);
int passl_hip_bn_bwd_finalize(const float* partial, int nblocks, int64_t M, int C,
                              const float* gamma, const float* mean, const float* invstd,
                              float* dgamma, float* dbeta, float* coef /* [3][C] */,
                              passl_stream_t stream);
/* Cross-rank (Sync) BatchNorm — reference passl/models/simsiam.py:160-162 (nn.SyncBatchNorm.convert_sync_batchnorm
 * under data parallelism): statistics over the batches of ALL ranks.  Forward: bn_moments folds this rank's slab to
 * fp64 {mean[C], M2[C], n[C]} (mom: 3*C doubles); the caller all-gathers them (rank order) and bn_finalize_moments
 * combines them with Chan's update and produces what bn_finalize produces (running statistics from the GLOBAL batch).
 * Backward: bn_bwd_sums folds the slab to fp64 {sum g, sum g*xhat} (2*C doubles), all-gathered; bn_bwd_finalize_sums
 * accumulates THIS rank's sums into dgamma / dbeta and writes the apply coefficients from the totals and the global
 * row count.  The collectives are the caller's (torch.distributed): the library never communicates. */
int passl_hip_bn_moments(const float* partial, int nblocks, int64_t M, int C, int rows_per_block, double* mom,
                         passl_stream_t stream);
int passl_hip_bn_finalize_moments(const double* mom_all, int world, int C, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, float momentum, float eps, float* mean,
                                  float* invstd, float* scale, float* shift, passl_stream_t stream);
int passl_hip_bn_bwd_sums(const float* partial, int nblocks, int64_t M, int C, double* sums, passl_stream_t stream);
int passl_hip_bn_bwd_finalize_sums(const double* sums_all, int world, int rank, int64_t M_total, int C,
                                   const float* gamma, const float* mean, const float* invstd, float* dgamma,
                                   float* dbeta, float* coef, passl_stream_t stream);
int passl_hip_bn_bwd_apply(const void* dz, const void* z, const void* x, const float* coef,
                           const float* scale, const float* shift, void* dx, void* dres, int64_t M,
                           int C, int relu, int dtype, passl_stream_t stream);
/* ---------------------------------------------------------------- pooling */

/* 3x3 stride-2 pad-1 max pool, NHWC; idx[n,p,q,c] (uint8) = winning tap r*3+s (first max in
 * row-major window order).  Replaces nn.MaxPool2D at resnetimagenet.py:198,239. */
int passl_hip_maxpool3x3s2_fwd(const void* x, void* y, uint8_t* idx, int N, int H, int W, int C,
                               int dtype, passl_stream_t stream);
int passl_hip_maxpool3x3s2_bwd(const void* dy, const uint8_t* idx, void* dx, int N, int H, int W,
                               int C, int dtype, passl_stream_t stream);
/* Training-mode BatchNorm + ReLU + the 3x3 / stride 2 / pad 1 max pool of the ResNet stem as ONE pass per direction
 * (csrc/stem_pool.hip): the BatchNorm output z and the pool's input gradient dz are never written.  x = the
 * BatchNorm input [N,H,W,C] (the stem convolution's output), scale / shift / mean / invstd / coef as produced by
 * passl_hip_bn_finalize / passl_hip_bn_bwd_finalize, idx as passl_hip_maxpool3x3s2_fwd writes it.
 *   fwd:        y[n,p,q,c] = max over the window of T(relu(x*scale + shift)), idx = the winning tap
 *   bwd_reduce: partial[b][c][0..1] = sum g, sum g*(x - mean)*invstd with g = T(max-pool gradient of dy) masked by
 *               x*scale + shift > 0; nblocks = passl_hip_bn_relu_maxpool_blocks(N,H,W,C) slab rows (buffer sized by
 *               passl_hip_bn_partial_floats(nblocks, C, 0)), consumed by passl_hip_bn_bwd_finalize with M = N*H*W.
 *               idx must come from the forward pass (a tap outside the image is never the arg-max).
 *   bwd_apply:  dx = A g + B x + C
 * Element for element the arithmetic of passl_hip_bn_apply -> maxpool3x3s2_fwd resp. maxpool3x3s2_bwd -> bn_bwd_reduce
 * (relu = 2) -> bn_bwd_apply: y, idx and (for equal coefficients) dx are bit-identical to that chain; the slab is
 * summed in another fixed order.  C/8 must divide 256; PASSL_EUNSUPPORTED otherwise (use the separate passes).
 * Replaces BatchNorm2D + ReLU + MaxPool2D at resnetimagenet.py:196-198 and their autograd. */
int passl_hip_bn_relu_maxpool_blocks(int N, int H, int W, int C);
int passl_hip_bn_relu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx, int N,
                                  int H, int W, int C, int dtype, passl_stream_t stream);
int passl_hip_bn_relu_maxpool_bwd_reduce(const void* dy, const uint8_t* idx, const void* x, const float* mean,
                                         const float* invstd, const float* scale, const float* shift, float* partial,
                                         int nblocks, int N, int H, int W, int C, int dtype, passl_stream_t stream);
int passl_hip_bn_relu_maxpool_bwd_apply(const void* dy, const uint8_t* idx, const void* x, const float* coef,
                                        const float* scale, const float* shift, void* dx, int N, int H, int W, int C,
                                        int dtype, passl_stream_t stream);
/* Global average pool [N,HW,C] -> [N,C] and its backward.  Replaces AdaptiveAvgPool2D((1,1)) at
 * necks/base_neck.py:79,94. */
int passl_hip_avgpool_fwd(const void* x, void* y, int N, int HW, int C, int dtype,
                          passl_stream_t stream);
int passl_hip_avgpool_bwd(const void* dy, void* dx, int N, int HW, int C, int dtype,
                          passl_stream_t stream);
/* dx = dy * (y > 0), n elements (multiple of 8) — backward of the projector's ReLU
 * (necks/base_neck.py:83). */
int passl_hip_relu_bwd(const void* dy, const void* y, void* dx, int64_t n, int dtype,
                       passl_stream_t stream);
/* out[c] = sum_m x[m][c] (fp32 out) — Linear bias gradient.  Rows are cut into at most 1024 slabs;
 * with a workspace `ws` (>= 1024*C floats, `ws_floats` = its size) the slab partials are added in
 * slab order (bit-reproducible); ws == NULL falls back to fp32 atomics when there is more than one slab. */
int passl_hip_colsum(const void* x, float* out, int64_t M, int C, int dtype, float* ws,
                     int64_t ws_floats, passl_stream_t stream);
/* out[c] += sum_m x[m][c] — accumulates straight into the (zero-initialised) gradient buffer. */
int passl_hip_colsum_acc(const void* x, float* out, int64_t M, int C, int dtype, float* ws,
                         int64_t ws_floats, passl_stream_t stream);

/* ---------------------------------------------------------------- contrastive head */

/* y = x / max(||x||_2, eps) per row (fp32), saves the clamped norm.
 * Replaces F.normalize(axis=1) at moco.py:159,170. */
int passl_hip_l2norm_fwd(const float* x, float* y, float* norm, int N, int D, float eps,
                         passl_stream_t stream);
/* dx = (dy - y*(y.dy)) / norm ; written as fp32 (dtype F32) or bf16. */
int passl_hip_l2norm_bwd(const float* dy, const float* y, const float* norm, void* dx, int N,
                         int D, int dtype, passl_stream_t stream);
/* SimSiam's criterion (reference passl/models/simsiam.py:69,93: nn.CosineSimilarity(axis=1) of the predictor output
 * against the stop-gradient projector output, negated and averaged): loss[0] = -(1/N) sum_i a_i.b_i / max(|a_i||b_i|,
 * eps); a, b fp32 [N,D]; stats [N,4] is saved for the backward.  The mean is one fixed-order sum. */
int passl_hip_cosine_loss_fwd(const float* a, const float* b, int N, int D, float eps, float* stats, float* loss,
                              passl_stream_t stream);
/* da [N,D] = gloss[0] * d loss / d a  (b is a constant); gloss: device scalar. */
int passl_hip_cosine_loss_bwd(const float* a, const float* b, const float* stats, const float* gloss, int N, int D,
                              float* da, passl_stream_t stream);

/* Fused InfoNCE forward (moco.py:178-180 + heads/contrastive_head.py:47-78):
 *   l_pos[i] = q[i].k[i];  l_neg[i][j] = q[i].queue[:,j];  logits = [l_pos | l_neg]/T
 *   loss = mean_i( logsumexp(logits[i]) - logits[i][0] ),  acc1/acc5 = % rows whose column 0
 *   has rank < 1 / < 5 among strictly greater logits.
 * q,k: [N][D] fp32, queue: [D][K] fp32 (dim-major, as the reference stores it).
 * Outputs: out[0..2] = loss, acc1, acc5 (fixed-order mean, fully written); row_lse[N]; optional
 * logits [N][K+1] (may be NULL).
 * workspace: >= passl_hip_infonce_workspace_bytes(N,K) bytes. D must be 128, K % 128 == 0. */
int64_t passl_hip_infonce_workspace_bytes(int N, int K);
int passl_hip_infonce_fwd(const float* q, const float* k, const float* queue, int N, int D, int K,
                          float T, float* out, float* row_lse, float* logits, void* workspace,
                          passl_stream_t stream);
/* dq[i] = gscale/(N*T) * ( (p_i0 - 1)*k[i] + sum_j p_ij * queue[:,j] ),  p = softmax(logits).
 * dq is fully written (no zeroing): every 128-column queue slice writes its own [N][D] slab of
 * `workspace` (>= passl_hip_infonce_bwd_workspace_bytes(N,K) bytes) and the slabs are added in slice
 * order — no atomics, bit-reproducible.  `gscale` device pointer to the upstream scalar gradient
 * (or NULL = 1). */
int64_t passl_hip_infonce_bwd_workspace_bytes(int N, int K);
int passl_hip_infonce_bwd(const float* q, const float* k, const float* queue,
                          const float* row_lse, const float* gscale, int N, int D, int K, float T,
                          float* dq, void* workspace, passl_stream_t stream);
/* queue[:, ptr:ptr+B] = keys^T  (keys [B][D]).  Replaces the slice-assign of
 * MoCo._dequeue_and_enqueue, moco.py:101-102 (the pointer arithmetic stays on the host). */
int passl_hip_enqueue(float* queue, const float* keys, int D, int K, int ptr, int B,
                      passl_stream_t stream);
/* The same with the pointer in DEVICE memory (MoCo's `queue_ptr` buffer itself, int64[1], moco.py:80): the launch
 * reads *ptr, writes the keys and then advances *ptr = (*ptr + B) % K — nothing about the step's position in
 * the queue is frozen at enqueue time (HIP-graph replay).  K % B == 0 (moco.py:99). */
int passl_hip_enqueue_dev(float* queue, const float* keys, int D, int K, int64_t* ptr, int B,
                          passl_stream_t stream);

/* Fused NT-Xent + CO2 head of SimCLR (passl_v110/modeling/heads/simclr_contrastive_head.py:42-102).
 * a, b: [B][D] fp32 rows of this rank (hidden1, hidden2); a_all, b_all: [BL][D] the column sets
 * (a_all = a, b_all = b, BL = B, row_offset = 0 reproduces the reference, which never gathers;
 * with all-gathered embeddings row i's positive column is row_offset + i).  D must be 128, BL >= 2.
 *   loss = mean_i( LSE([ab_i|aa_i]) - ab_i,pos + LSE([ba_i|bb_i]) - ba_i,pos )
 *          + co2_weight * sum_i( KL(Pb_i||Pa_i) + KL(Pa_i||Pb_i) ) / B          (self/positive masks
 *   as in the reference), acc1 = fraction of rows whose positive is the arg-max of ab_i.
 * out[0..1] = loss, acc1; rowstats [B][8] = (lse_ce_a, lse_ce_b, lse_Pa, lse_Pb, co2_i, pos, rank, 0)
 * is what the backward needs.  The B x BL logits are never written. */
int passl_hip_ntxent_fwd(const float* a, const float* b, const float* a_all, const float* b_all,
                         int B, int BL, int row_offset, int D, float T, float co2_weight,
                         float* out, float* rowstats, passl_stream_t stream);
/* Gradients (accumulated with atomics into zeroed buffers): da, db [B][D] = through the row role,
 * da_all, db_all [BL][D] = through the column role (the caller adds / reduce-scatters them).
 * The kl_div target carries no gradient (Paddle's kldiv_loss_grad). gscale: device scalar or NULL. */
int passl_hip_ntxent_bwd(const float* a, const float* b, const float* a_all, const float* b_all,
                         const float* rowstats, const float* gscale, int B, int BL, int row_offset,
                         int D, float T, float co2_weight, float* da, float* db, float* da_all,
                         float* db_all, passl_stream_t stream);

/* ---------------------------------------------------------------- ViT / MAE
 * Reference: class MAE, passl_v110/modeling/backbones/mae.py:318-564 (= passl/models/mae.py:37-290),
 * Mlp/Attention/Block :61-189.  Activations [rows][C] in `dtype`, C % 8 == 0. */

/* y = (x - mean)/sqrt(var + eps) * gamma + beta per row (biased var); saves mean, rstd [M]. */
int passl_hip_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y,
                            float* mean, float* rstd, int64_t M, int C, float eps, int dtype,
                            passl_stream_t stream);
/* dx (+ dres when non-NULL: the gradient arriving through the residual branch that forked off x, so
 * that `x + f(LN(x))` needs no separate add); dgamma/dbeta (fp32 [C]) are ACCUMULATED into: every block writes
 * its column sums to a slab of `ws` (>= passl_hip_layernorm_bwd_ws_floats(M, C) floats) and a second launch adds
 * the slabs in block order — no floating-point atomics, the result is bit-reproducible.  C <= 2048. */
int64_t passl_hip_layernorm_bwd_ws_floats(int64_t M, int C);
int passl_hip_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                            const float* rstd, const void* dres, void* dx, float* dgamma,
                            float* dbeta, int64_t M, int C, int dtype, float* ws, int64_t ws_floats,
                            passl_stream_t stream);
/* layernorm_bwd with dgamma == dbeta == NULL leaves its per-block partial sums in ws (which must then be the caller's
 * own buffer, not a shared scratch); this folds them — dgamma / dbeta += the fixed-order sums — on any stream. */
int passl_hip_layernorm_param_reduce(const float* ws, int64_t M, int C, float* dgamma, float* dbeta,
                                     passl_stream_t stream);
/* exact (erf) GELU and its backward dx = dy * gelu'(x); n % 8 == 0. */
int passl_hip_gelu_fwd(const void* x, void* y, int64_t n, int dtype, passl_stream_t stream);
int passl_hip_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype,
                       passl_stream_t stream);
/* y = tanh(x);  dx = dy * (1 - tanh(x)^2)   (n a multiple of 8, 16-byte aligned).  Reference: the
 * `representation_size` head of the v2 VisionTransformer, passl/models/vision_transformer.py:318-321,340-343. */
int passl_hip_tanh_fwd(const void* x, void* y, int64_t n, int dtype, passl_stream_t stream);
int passl_hip_tanh_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, passl_stream_t stream);
/* Fused softmax(q k^T * scale) v per (image, head) on the fused projection qkv [B,T,3,H,DH];
 * out [B,T,H,DH]; lse [B,H,T] (row log-sum-exp, saved for the backward).  DH in {32, 64},
 * T <= 208 (PASSL_EUNSUPPORTED otherwise).  Replaces Attention.forward, mae.py:141-155.
 * causal != 0: key j visible to query i iff j <= i (the CLIP text tower's additive triu(-inf, 1)
 * mask, passl_v110/modeling/backbones/clip.py:284-286 + vision_transformer.py:107-113). */
int passl_hip_attention_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, int DH,
                            float scale, int causal, int dtype, passl_stream_t stream);
/* dqkv [B,T,3,H,DH] (fully written) from dout [B,T,H,DH]. */
int passl_hip_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                            void* dqkv, int B, int T, int H, int DH, float scale, int causal,
                            int dtype, passl_stream_t stream);
/* random_masking (mae.py:461-488) without the sort: ids_restore[b,l] = rank of noise[b,l] in its row
 * (ties by index), ids_keep[b,rank] = l for rank < len_keep, mask[b,l] = rank >= len_keep. */
int passl_hip_mae_mask(const float* noise, int B, int L, int len_keep, int32_t* ids_keep,
                       int32_t* ids_restore, float* mask, passl_stream_t stream);
/* encoder input (mae.py:494-503): out[b,0] = cls + pos[0]; out[b,1+k] = x[b,ids_keep[b,k]] +
 * pos[1+ids_keep[b,k]];  x [B,L,D], pos [L+1,D], out [B,K+1,D].  D a multiple of 8; x, cls, pos and out 16-byte
 * aligned (PASSL_EINVAL otherwise, before any launch). */
int passl_hip_mae_gather(const void* x, const float* cls, const float* pos, const int32_t* ids_keep,
                         void* out, int B, int L, int K, int D, int dtype, passl_stream_t stream);
/* its backward: dx [B,L,D] fully written (zeros at masked patches), dcls += sum_b dout[b,0] (images added in
 * a fixed order).  dout and dx 16-byte aligned (PASSL_EINVAL otherwise, before any launch). */
int passl_hip_mae_gather_bwd(const void* dout, const int32_t* ids_restore, void* dx, float* dcls,
                             int B, int L, int K, int D, int dtype, passl_stream_t stream);
/* decoder input (mae.py:516-527): out[b,0] = x[b,0] + pos[0]; out[b,1+l] = (r = ids_restore[b,l]) < K
 * ? x[b,1+r] : mask_token, + pos[1+l];  x [B,K+1,D], out [B,L+1,D].  x, mask_token, pos and out 16-byte aligned
 * (PASSL_EINVAL otherwise, before any launch). */
int passl_hip_mae_unshuffle(const void* x, const float* mask_token, const float* pos,
                            const int32_t* ids_restore, void* out, int B, int L, int K, int D,
                            int dtype, passl_stream_t stream);
/* its backward: dx [B,K+1,D] fully written, dmask_token += sum over masked positions (token-block slabs in
 * `ws`, >= 1024 * D floats, added in order: no atomics).  dout, dx, dmask_token and ws 16-byte aligned (PASSL_EINVAL
 * otherwise, before any launch). */
int passl_hip_mae_unshuffle_bwd(const void* dout, const int32_t* ids_keep, const int32_t* ids_restore,
                                void* dx, float* dmask_token, int B, int L, int K, int D, int dtype,
                                float* ws, int64_t ws_floats, passl_stream_t stream);
/* imgs fp32 NCHW -> out [B*L, p*p*C] in `dtype`, column order (ph, pw, c): the patch-embed conv
 * (mae.py:87-121) as a GEMM, and MAE.patchify's order (mae.py:433-445). */
int passl_hip_patchify(const float* img, void* out, int B, int C, int H, int W, int p, int dtype,
                       passl_stream_t stream);
/* forward_loss (mae.py:541-557): pred fp32 [B, L+1, P] (row 0 of every image = cls, ignored);
 * loss[0] = sum_l mask * mean_P (pred - target)^2 / denom, target = patches of img, normalised per
 * patch ((x - mean)/sqrt(var_unbiased + 1e-6)) when norm_pix.  denom = sum(mask).  ws: B * (L + 1) floats (the
 * per-patch terms, summed in one fixed order). */
int passl_hip_mae_loss_fwd(const float* img, const float* pred, const float* mask, float* loss, int B,
                           int C, int H, int W, int p, int norm_pix, float denom, float* ws,
                           int64_t ws_floats, passl_stream_t stream);
int passl_hip_mae_loss_bwd(const float* img, const float* pred, const float* mask,
                           const float* gscale, float* dpred, int B, int C, int H, int W, int p,
                           int norm_pix, float denom, passl_stream_t stream);
/* AdamW over a flat fp32 buffer (paddle adamw op): p *= 1 - lr*wd; m = b1 m + (1-b1) g;
 * v = b2 v + (1-b2) g^2; p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps*sqrt(1-b2^t)), with
 * g scaled by grad_scale.  Replaces paddle.optimizer.AdamW.step (solver/optimizer.py:22). */
int passl_hip_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float epsilon, float weight_decay, float beta1_pow, float beta2_pow,
                    float grad_scale, passl_stream_t stream);
/* ... with the step-dependent scalars read on the device: hyper = {lr, beta1^t, beta2^t} (see
 * passl_hip_momentum_sgd_dev).  Both forms derive sqrt(1-b2^t) etc. inside the kernel: identical bits. */
int passl_hip_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, float beta1,
                        float beta2, float epsilon, float weight_decay, float grad_scale, passl_stream_t stream);
/* ... with parameter groups: a learning-rate multiplier and a weight decay per SEGMENT of the buffer, still one launch.
 * seg_end / seg_lr_scale / seg_wd: device arrays of n_seg entries; seg_end holds ascending exclusive end offsets in
 * elements, every one a multiple of 4 and the last one n (n % 4 == 0): element i belongs to the first segment with
 * i < seg_end[s], slot padding to the parameter in front of it.  Per segment lr_s = hyper[0] * seg_lr_scale[s] (one
 * fp32 multiply), then exactly the update of passl_hip_adamw with (lr_s, seg_wd[s]) — the two kernels share one
 * device function, so a segment gets the bits passl_hip_adamw gives that slice alone.  The table is read from global
 * memory (a binary search per workgroup tile): there is NO segment limit beyond n_seg fitting an int; the caller
 * validates the table's contents (the library cannot read device memory on the host), the kernel keeps every access
 * in bounds whatever it holds.  NULL pointers, n < 0, n % 4, n_seg <= 0, misalignment -> PASSL_EINVAL; n == 0 -> OK.
 * Replaces the per-group optimizer loop of tasks/ssl/mae/main_finetune.py:478-484 (param_groups_lrd -> AdamW) and the
 * lr_scale read of passl/optimizer/optimizer.py:117-123. */
int passl_hip_adamw_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                               const float* seg_lr_scale, const float* seg_wd, int n_seg, const float* hyper,
                               float beta1, float beta2, float epsilon, float grad_scale, passl_stream_t stream);

/* ---------------------------------------------------------------- global-norm gradient clipping (AdamW)
 * Reference: class ClipGradByGlobalNorm and clip_grad_norm_, passl/core/grad_clip.py:30-139, called once per parameter
 * group by passl/optimizer/adamw.py:53-55.  For one SET of parameters
 *     norm = sqrtf(sum (g*grad_scale)^2),   coef = 1                                    if !always_clip && norm <= clip_norm
 *                                                = min(clip_norm / (norm + 1e-6f), clip_norm_max)   otherwise
 * (a non-finite norm is "not <=": its coefficient propagates).  Three steps, none of which returns anything to the
 * host and none of which uses an atomic — the result is bit-identical wherever the inputs are:
 *   1. passl_hip_grad_sumsq, one launch per gradient buffer: partial[c] = sum over chunk c = g[chunk_off[c],
 *      chunk_off[c] + chunk_len[c]) of fp32(g*grad_scale)^2, one workgroup per chunk, one fixed order.  A chunk holds at
 *      most PASSL_GRAD_CLIP_CHUNK elements; offsets and lengths are multiples of 4.  The caller builds the table so that
 *      no chunk crosses the boundary of a set or covers a parameter left out of clipping, and hands every launch its own
 *      range of ONE partial buffer.  Workspace: n_chunks floats.
 *   2. passl_hip_grad_clip_finalize, one launch: out[s] = {norm, coef} (2 floats per set) from the partials
 *      set_chunks[set_ptr[s] .. set_ptr[s+1]) (a CSR index into the partial buffer: n_sets + 1 / n_idx int32), summed in
 *      index order by one workgroup per set; sqrtf and the division are correctly rounded.  clip_norm_max: +inf for "no
 *      upper limit".  clip_norm and clip_norm_max must be > 0.
 *   3. the clip variants of the update: gg = (g*grad_scale)*coef, then exactly passl_hip_adamw_dev /
 *      passl_hip_adamw_groups_dev (one shared device function).  The flat variant reads coef[0]; the grouped variant
 *      reads clip[2*seg_set[s] + 1] from the {norm, coef} table of step 2, seg_set[s] outside [0, n_sets) (-1) meaning
 *      coefficient 1.  n % 4 == 0 for both.
 * The gradient buffer is NOT rewritten (the reference scales it in place).  The library cannot read device tables on the
 * host: the caller validates their contents, the kernels keep every access inside [0, n) / the partial buffer whatever
 * they hold.  NULL pointers, n <= 0 (sumsq), n < 0 (updates), n % 4, counts <= 0, misalignment -> PASSL_EINVAL.
 * passl_hip_grad_clip_chunk(PASSL_HIP_ABI_VERSION) returns PASSL_GRAD_CLIP_CHUNK as the library was built (any other
 * argument: PASSL_EINVAL). */
#define PASSL_GRAD_CLIP_CHUNK 16384
int passl_hip_grad_clip_chunk(int abi_version);
int passl_hip_grad_sumsq(const float* g, int64_t n, const int64_t* chunk_off, const int32_t* chunk_len, int n_chunks,
                         float grad_scale, float* partial, passl_stream_t stream);
int passl_hip_grad_clip_finalize(const float* partial, int n_partial, const int32_t* set_ptr, const int32_t* set_chunks,
                                 int n_idx, int n_sets, float clip_norm, float clip_norm_max, int always_clip, float* out,
                                 passl_stream_t stream);
int passl_hip_adamw_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                             const float* coef, float beta1, float beta2, float epsilon, float weight_decay,
                             float grad_scale, passl_stream_t stream);
int passl_hip_adamw_groups_clip_dev(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_end,
                                    const float* seg_lr_scale, const float* seg_wd, const int32_t* seg_set, int n_seg,
                                    const float* hyper, const float* clip, int n_sets, float beta1, float beta2,
                                    float epsilon, float grad_scale, passl_stream_t stream);

/* ---------------------------------------------------------------- Adan (flat buffer)
 * Reference: class Adan, passl/optimizer/adan.py:117-148 with is_vanilla=False (arXiv 2208.06677); replaces its
 * per-parameter loop of framework element-wise ops by ONE launch over six flat fp32 vectors: p, m (exp_avg),
 * d (exp_avg_diff), s (exp_avg_sq), pre (pre_grad) are updated from g, one float4 of each per lane:
 *     gg   = g*grad_scale                       [clip variants: gg *= coef]
 *     diff = first ? 0 : gg - pre
 *     m    = b1*m + (1-b1)*gg;   d = b2*d + (1-b2)*diff;   u = gg + b2*diff;   s = b3*s + (1-b3)*u*u
 *     den  = sqrt(s)/sqrt(1-b3^t) + eps;   upd = (m/(1-b1^t) + b2*d/(1-b2^t)) / den
 *     p    = (p - lr*upd) / (1 + lr*wd)         [no_prox != 0: p = p*(1 - lr*wd) - lr*upd]
 *     pre  = gg                                 (the scaled, clipped gradient, as the reference stores it)
 * Every step-dependent scalar is read on the device: hyper = 8 floats {lr, b1^t, b2^t, b3^t, first (1.0 at t == 1,
 * else 0.0), 0, 0, 0} — a recorded plan or a HIP graph replays correctly whichever step it was recorded at.  With
 * first != 0 the contents of pre have no influence on any output (the reference creates pre_grad = grad.clone()).
 * no_prox is configuration and travels by value.
 *   passl_hip_adan_dev               one weight decay for the whole buffer.
 *   passl_hip_adan_clip_dev          ... with the gradient times coef[0], a device float (passl_hip_grad_clip_finalize).
 *   passl_hip_adan_groups_dev        a learning-rate multiplier and a weight decay per segment: the table of
 *                                    passl_hip_adamw_groups_dev, unchanged (lr_s = hyper[0] * seg_lr_scale[s], one fp32
 *                                    multiply, then exactly the flat update with (lr_s, seg_wd[s]): one shared device
 *                                    function, so a segment gets the bits passl_hip_adan_dev gives that slice alone).
 *   passl_hip_adan_groups_clip_dev   ... with the gradient of segment s times clip[2*seg_set[s] + 1]; seg_set[s] outside
 *                                    [0, n_sets) (-1) means coefficient 1.
 * The caller validates the tables' contents; the kernels keep every access inside [0, n) whatever they hold.  NULL
 * pointers, n < 0, n % 4, n_seg <= 0, n_sets <= 0 (groups_clip), buffers not 16-byte aligned -> PASSL_EINVAL before
 * any launch; n == 0 -> PASSL_OK without a launch. */
int passl_hip_adan_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                       const float* hyper, float beta1, float beta2, float beta3, float epsilon, float weight_decay,
                       int no_prox, float grad_scale, passl_stream_t stream);
int passl_hip_adan_clip_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                            const float* hyper, const float* coef, float beta1, float beta2, float beta3, float epsilon,
                            float weight_decay, int no_prox, float grad_scale, passl_stream_t stream);
int passl_hip_adan_groups_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                              const int64_t* seg_end, const float* seg_lr_scale, const float* seg_wd, int n_seg,
                              const float* hyper, float beta1, float beta2, float beta3, float epsilon, int no_prox,
                              float grad_scale, passl_stream_t stream);
int passl_hip_adan_groups_clip_dev(float* p, const float* g, float* m, float* d, float* s, float* pre, int64_t n,
                                   const int64_t* seg_end, const float* seg_lr_scale, const float* seg_wd,
                                   const int32_t* seg_set, int n_seg, const float* hyper, const float* clip, int n_sets,
                                   float beta1, float beta2, float beta3, float epsilon, int no_prox, float grad_scale,
                                   passl_stream_t stream);

/* ---------------------------------------------------------------- stochastic depth
 * Reference: class DropPath / drop_path(), passl_v110/modeling/backbones/mae.py:32-50; the ladder
 * linspace(0, drop_path_rate, depth) :234; the two uses per Block :186-187.  Token rows [B*T][C] in `dtype`, sample b
 * owns rows b*T .. (b+1)*T-1; C % 8 == 0. */

/* The keep table of one forward pass (paddle.rand + floor of drop_path(), mae.py:44-46, for every DropPath of the
 * model in one launch): keep[slot][b] = (keep_prob[slot] + u >= 1.0f) ? 1 : 0, the sum rounded to fp32, with
 * u = float(x0 >> 8) * 2^-24 and x0 the first output word of Philox4x32-10 on counter (b, slot, step_lo32, step_hi32),
 * key (seed_lo32, seed_hi32); seed and *step taken as unsigned 64-bit patterns.  keep_prob [slots] is device memory
 * (>= 1: always kept).  Every element uses the value *step (device, 8-byte aligned) had when the launch began; the
 * launch leaves *step + 1 behind.  No argument varies from step to step: a step plan replays the launch as recorded
 * and still draws a new table.  slots * B <= 2^24. */
int passl_hip_drop_path_draw(float* keep, const float* keep_prob, int slots, int B, int64_t seed, int64_t* step,
                             passl_stream_t stream);
/* out = residual + keep[b] * (branch / keep_prob): `x + self.drop_path(f(norm(x)))`, mae.py:186-187, with
 * drop_path() = x.divide(keep_prob) * random_tensor :47.  fp32 arithmetic, IEEE division, one rounding to `dtype`.
 * Rows of a dropped sample (keep[b] == 0) are copied from residual; branch is not read for them.  keep: one row [B] of
 * the table above; 0 < keep_prob <= 1. */
int passl_hip_drop_path_add(const void* branch, const void* residual, const float* keep, float keep_prob, void* out,
                            int B, int T, int C, int dtype, passl_stream_t stream);
/* Its backward: dbranch = keep[b] * (dy / keep_prob); zeros for a dropped sample, dy not read.  The residual's gradient
 * is dy itself. */
int passl_hip_drop_path_bwd(const void* dy, const float* keep, float keep_prob, void* dbranch, int B, int T, int C,
                            int dtype, passl_stream_t stream);

/* ---------------------------------------------------------------- ConvNeXt block: depthwise 7x7, layer scale
 * Reference: class Block, passl/models/convnext.py:68-103: `self.dwconv = nn.Conv2D(dim, dim, 7, padding=3, groups=dim)`
 * and the tail `x = input + self.drop_path(self.gamma * x)` :100-102.  x, y, dy, dx, add are NHWC [N][H][W][C] in
 * `dtype`; w is fp32 in the parameter's own layout [C][1][7][7] (49 * C floats, read as it lies), bias fp32 [C].
 * C % 8 == 0, every pointer 16-byte aligned, any H, W >= 1.  fp32 accumulation, one rounding to `dtype` at the store;
 * no floating-point atomics: every result is bit-reproducible from launch to launch.
 * NULL pointers (but `add` / `keep`, which may be NULL), sizes <= 0, C % 8, misalignment, a short workspace ->
 * PASSL_EINVAL; an unknown dtype or a grid beyond 2^31 workgroups -> PASSL_EUNSUPPORTED. */

/* y[n,p,q,c] = bias[c] + sum_{r,s} x[n,p+r-3,q+s-3,c] * w[c,0,r,s], zero padding. */
int passl_hip_dwconv7_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C,
                          int dtype, passl_stream_t stream);
/* dx[n,h,w,c] = add[n,h,w,c] + sum_{r,s} dy[n,h+3-r,w+3-s,c] * w[c,0,r,s].  add (may be NULL) is the gradient that
 * arrives over the block's residual fork: it is added in fp32 before the single rounding. */
int passl_hip_dwconv7_bwd_data(const void* dy, const float* w, const void* add, void* dx, int N, int H, int W, int C,
                               int dtype, passl_stream_t stream);
/* dw[c,0,r,s] = sum_{n,p,q} dy[n,p,q,c] * x[n,p+r-3,q+s-3,c] and dbias[c] = sum dy, WRITTEN (not accumulated) in fp32.
 * Every workgroup leaves its sums in a slab of ws and a second and third launch add the slabs in ascending order.
 * ws_floats >= PASSL_DWCONV7_WGRAD_WS_FLOATS(N, H, W, C). */
#define PASSL_DWCONV7_WGRAD_TILE_H 8
#define PASSL_DWCONV7_WGRAD_TILE_W 16
#define PASSL_DWCONV7_WGRAD_MAX_SLABS 512
#define PASSL_DWCONV7_WGRAD_TILES(N, H, W)                                                  \
  ((int64_t)(N) * (((H) + PASSL_DWCONV7_WGRAD_TILE_H - 1) / PASSL_DWCONV7_WGRAD_TILE_H) *   \
   (((W) + PASSL_DWCONV7_WGRAD_TILE_W - 1) / PASSL_DWCONV7_WGRAD_TILE_W))
#define PASSL_DWCONV7_WGRAD_SLABS(N, H, W)                                        \
  (PASSL_DWCONV7_WGRAD_TILES(N, H, W) < PASSL_DWCONV7_WGRAD_MAX_SLABS             \
       ? PASSL_DWCONV7_WGRAD_TILES(N, H, W) : (int64_t)PASSL_DWCONV7_WGRAD_MAX_SLABS)
#define PASSL_DWCONV7_WGRAD_WS_FLOATS(N, H, W, C) (PASSL_DWCONV7_WGRAD_SLABS(N, H, W) * 50 * (C))
int passl_hip_dwconv7_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, float* ws, int64_t ws_floats,
                                 int N, int H, int W, int C, int dtype, passl_stream_t stream);

/* Rows [B*T][C] in `dtype`, sample b owns rows b*T .. (b+1)*T-1; gamma fp32 [C]; keep one row [B] of the table
 * passl_hip_drop_path_draw writes, or NULL (rate 0, evaluation), and then keep_prob is not read.
 * out = residual + keep[b] * ((gamma[c] * branch) / keep_prob): four fp32 operations in the reference's order (`gamma * x`
 * :100, `x.divide(keep_prob) * random_tensor`, `input + ...`), each rounded, none contracted into an fma, then one
 * rounding to `dtype`.  keep == NULL: out = residual + gamma[c] * branch.  Rows of a dropped sample are copied from
 * residual, branch is not read for them.  0 < keep_prob <= 1 when keep is given. */
int passl_hip_layer_scale_add_fwd(const void* branch, const void* residual, const float* gamma, const float* keep,
                                  float keep_prob, void* out, int B, int T, int C, int dtype, passl_stream_t stream);
/* With g = keep[b] * (dy / keep_prob) (g = dy when keep == NULL): dbranch = gamma[c] * g (zeros for a dropped sample,
 * dy and branch not read) and dgamma[c] = sum_rows branch * g, WRITTEN in fp32: one slab of ws per workgroup, added in
 * ascending order by a second launch.  The residual's gradient is dy itself.  C <= PASSL_LAYER_SCALE_MAX_C;
 * ws_floats >= PASSL_LAYER_SCALE_BWD_WS_FLOATS(B * T, C). */
#define PASSL_LAYER_SCALE_MAX_C 8192
#define PASSL_LAYER_SCALE_MAX_SLABS 1024
#define PASSL_LAYER_SCALE_ROWS_PER_SLAB(M) \
  (((int64_t)(M) + PASSL_LAYER_SCALE_MAX_SLABS - 1) / PASSL_LAYER_SCALE_MAX_SLABS)
#define PASSL_LAYER_SCALE_BWD_WS_FLOATS(M, C) \
  ((((int64_t)(M) + PASSL_LAYER_SCALE_ROWS_PER_SLAB(M) - 1) / PASSL_LAYER_SCALE_ROWS_PER_SLAB(M)) * (C))
int passl_hip_layer_scale_add_bwd(const void* dy, const void* branch, const float* gamma, const float* keep,
                                  float keep_prob, void* dbranch, float* dgamma, float* ws, int64_t ws_floats, int B,
                                  int T, int C, int dtype, passl_stream_t stream);

/* ---------------------------------------------------------------- ConvMAE (csrc/convmae.hip)
 * Reference: class CBlock, passl/models/convmae/conv_vit.py:82-99: `self.attn = nn.Conv2D(dim, dim, 5, padding=2,
 * groups=dim)` applied to `mask * conv1(norm1(x))`.  x, y, dy, dx are NHWC [N][H][W][C] in `dtype`; w is fp32 in the
 * parameter's own layout [C][1][5][5] (25 * C floats, read as it lies), bias fp32 [C].  C % 8 == 0, every tensor 16-byte
 * aligned, any H, W >= 1.  fp32 accumulation, one rounding to `dtype` at the store; no floating-point atomics: every
 * result is bit-reproducible from launch to launch.
 * mask: the fp32 table [N][Hm * Wm] of passl_hip_mae_mask (1 = removed), or NULL for no mask (Hm, Wm are then not
 * read).  With g = H / Hm = W / Wm (an integer >= 1), keep(n, h, w) = 1 - mask[n][(h / g) * Wm + w / g]; no map-sized
 * mask tensor exists.  A factor of exactly 0 or 1 is applied exactly (a removed pixel is not even loaded); any other
 * factor is applied in fp32 and, for a bf16 input, rounded to bf16 once when the pixel is staged.
 * NULL pointers (but `mask`), sizes <= 0, C % 8, misalignment, a short workspace, H % Hm, W % Wm, H / Hm != W / Wm ->
 * PASSL_EINVAL; an unknown dtype or a grid beyond 2^31 workgroups -> PASSL_EUNSUPPORTED. */

/* y[n,h,w,c] = bias[c] + sum_{r,s} w[c,0,r,s] * keep(n,h+r-2,w+s-2) * x[n,h+r-2,w+s-2,c], zero padding. */
int passl_hip_dwconv5_masked_fwd(const void* x, const float* w, const float* bias, const float* mask, void* y, int N,
                                 int H, int W, int C, int Hm, int Wm, int dtype, passl_stream_t stream);
/* dx[n,h,w,c] = keep(n,h,w) * sum_{r,s} dy[n,h+2-r,w+2-s,c] * w[c,0,r,s]; a removed pixel gets +0. */
int passl_hip_dwconv5_masked_bwd_data(const void* dy, const float* w, const float* mask, void* dx, int N, int H, int W,
                                      int C, int Hm, int Wm, int dtype, passl_stream_t stream);
/* dw[c,0,r,s] = sum_{n,p,q} dy[n,p,q,c] * keep(n,p+r-2,q+s-2) * x[n,p+r-2,q+s-2,c] and dbias[c] = sum dy, WRITTEN (not
 * accumulated) in fp32.  Every workgroup leaves its sums in a slab of ws and a second and third launch add the slabs in
 * ascending order.  ws_floats >= PASSL_DWCONV5_WGRAD_WS_FLOATS(N, H, W, C). */
#define PASSL_DWCONV5_WGRAD_TILE_H 8
#define PASSL_DWCONV5_WGRAD_TILE_W 16
#define PASSL_DWCONV5_WGRAD_MAX_SLABS 512
#define PASSL_DWCONV5_WGRAD_TILES(N, H, W)                                                  \
  ((int64_t)(N) * (((H) + PASSL_DWCONV5_WGRAD_TILE_H - 1) / PASSL_DWCONV5_WGRAD_TILE_H) *   \
   (((W) + PASSL_DWCONV5_WGRAD_TILE_W - 1) / PASSL_DWCONV5_WGRAD_TILE_W))
#define PASSL_DWCONV5_WGRAD_SLABS(N, H, W)                                        \
  (PASSL_DWCONV5_WGRAD_TILES(N, H, W) < PASSL_DWCONV5_WGRAD_MAX_SLABS             \
       ? PASSL_DWCONV5_WGRAD_TILES(N, H, W) : (int64_t)PASSL_DWCONV5_WGRAD_MAX_SLABS)
#define PASSL_DWCONV5_WGRAD_WS_FLOATS(N, H, W, C) (PASSL_DWCONV5_WGRAD_SLABS(N, H, W) * 26 * (C))
int passl_hip_dwconv5_masked_bwd_weight(const void* x, const void* dy, const float* mask, float* dw, float* dbias,
                                        float* ws, int64_t ws_floats, int N, int H, int W, int C, int Hm, int Wm,
                                        int dtype, passl_stream_t stream);

/* The kept patches of an NHWC map as GEMM rows (conv_mae.py:249-266 runs the stage decoders and patch_embed3 over all
 * patches and then keeps K of them; they are per-patch functions, so they run on the kept ones only).
 * x [B][Hm*p][Wm*p][C], ids_keep int32 [B][K] (patch numbers of the Hm x Wm grid, as passl_hip_mae_mask writes them),
 * out [B*K][p*p*C] with column order (ph, pw, c): the K-order of a patch convolution's weight stored [Cout][p][p][C].
 * An index outside the grid gives a row of zeros.  C % 8 == 0, K <= Hm * Wm. */
int passl_hip_patch_gather_fwd(const void* x, const int32_t* ids_keep, void* out, int B, int K, int Hm, int Wm, int p,
                               int C, int dtype, passl_stream_t stream);
/* Its backward: dx [B][Hm*p][Wm*p][C] fully written from dout [B*K][p*p*C] and ids_restore int32 [B][Hm*Wm] (the rank
 * of every patch): zeros at the patches whose rank is >= K.  A pixel belongs to exactly one patch: no atomics. */
int passl_hip_patch_gather_bwd(const void* dout, const int32_t* ids_restore, void* dx, int B, int K, int Hm, int Wm,
                               int p, int C, int dtype, passl_stream_t stream);

/* MAE token kernels for a model WITHOUT a class row (conv_mae.py); x, out, dout, dx in `dtype`, pos and mask_token
 * fp32, D % 8 == 0, 1 <= K <= L.
 * encoder input: out[b,k] = x[b,k] + pos[ids_keep[b,k]];  x, out [B][K][D], pos [L][D].  Its data gradient is dout. */
int passl_hip_tokens_pos_gather_add(const void* x, const float* pos, const int32_t* ids_keep, void* out, int B, int L,
                                    int K, int D, int dtype, passl_stream_t stream);
/* dpos [L][D] fp32, ACCUMULATED as the other parameter gradients of the token kernels are: dpos[l] += the sum over the
 * images b = 0, 1, ... (added in that order, from 0) whose rank r = ids_restore[b,l] is < K of dout[b,r]. */
int passl_hip_tokens_pos_gather_add_bwd(const void* dout, const int32_t* ids_restore, float* dpos, int B, int L, int K,
                                        int D, int dtype, passl_stream_t stream);
/* decoder input: out[b,l] = ((r = ids_restore[b,l]) < K ? x[b,r] : mask_token) + pos[l];  x [B][K][D], out [B][L][D]. */
int passl_hip_tokens_unshuffle(const void* x, const float* mask_token, const float* pos, const int32_t* ids_restore,
                               void* out, int B, int L, int K, int D, int dtype, passl_stream_t stream);
/* its backward: dx [B][K][D] fully written (dx[b,k] = dout[b,ids_keep[b,k]]), dmask_token += sum of dout over the
 * removed positions (position-block slabs in `ws`, added in order: no atomics).
 * ws_floats >= PASSL_TOKENS_UNSHUFFLE_BWD_WS_FLOATS(D) covers every shape. */
#define PASSL_TOKENS_UNSHUFFLE_MAX_SLABS 1024
#define PASSL_TOKENS_UNSHUFFLE_BWD_WS_FLOATS(D) ((int64_t)PASSL_TOKENS_UNSHUFFLE_MAX_SLABS * (D))
int passl_hip_tokens_unshuffle_bwd(const void* dout, const int32_t* ids_keep, const int32_t* ids_restore, void* dx,
                                   float* dmask_token, int B, int L, int K, int D, int dtype, float* ws,
                                   int64_t ws_floats, passl_stream_t stream);

/* forward_loss (conv_mae.py:300-316) on pred fp32 [B][L][P] with no class row: passl_hip_mae_loss_fwd / _bwd
 * otherwise.  ws: B * L floats (the per-patch terms, summed in one fixed order). */
int passl_hip_tokens_mae_loss_fwd(const float* img, const float* pred, const float* mask, float* loss, int B, int C,
                                  int H, int W, int p, int norm_pix, float denom, float* ws, int64_t ws_floats,
                                  passl_stream_t stream);
int passl_hip_tokens_mae_loss_bwd(const float* img, const float* pred, const float* mask, const float* gscale,
                                  float* dpred, int B, int C, int H, int W, int p, int norm_pix, float denom,
                                  passl_stream_t stream);

/* ---------------------------------------------------------------- Swin Transformer (csrc/window_attention.hip)
 * Reference: WindowAttention.forward, passl/models/swin_transformer.py:112-200, with the roll, window_partition,
 * attn_mask, window_reverse and roll of SwinTransformerBlock.forward :291-340 as address arithmetic.
 * qkv [B, Hp*Wp, 3, nH, DH] in `dtype`: the qkv projection of the UNSHIFTED, UNPARTITIONED tokens; out, dout
 * [B, Hp*Wp, nH, DH] in the same token order; table fp32 [(2 ws - 1)^2, nH], the relative_position_bias_table as it
 * lies; lse fp32 [B * nW, nH, T], nW = (Hp / ws)(Wp / ws), T = ws^2.  Token i = (iy, ix) of window (wy, wx) is row
 * ((wy ws + iy + shift) mod Hp) Wp + ((wx ws + ix + shift) mod Wp) of its image, and
 * score[i, j] = (q_i . k_j) scale + table[(iy - jy + ws - 1)(2 ws - 1) + (ix - jx + ws - 1), h] + m[i, j] in fp32;
 * for shift > 0, m = -100 where label(i) != label(j), label = 3 r(wy ws + iy, Hp) + r(wx ws + ix, Wp),
 * r(y, n) = 0 if y < n - ws, 1 if y < n - shift, else 2.
 * Accepted: 1 <= ws <= 14, DH in {32, 64} (PASSL_EUNSUPPORTED otherwise); Hp, Wp multiples of ws, 0 <= shift < ws,
 * shift > 0 only with min(Hp, Wp) > ws, bf16 tensors 16-byte aligned (PASSL_EINVAL otherwise). */
int passl_hip_window_attention_fwd(const void* qkv, const float* table, void* out, float* lse, int B, int Hp, int Wp,
                                   int ws, int shift, int nH, int DH, float scale, int dtype, passl_stream_t stream);
/* dqkv [B, Hp*Wp, 3, nH, DH] (fully written) and dtable fp32 [(2 ws - 1)^2, nH] (WRITTEN) = the sum of
 * dS = P (dP - delta) over every image, window and pair of a bin, taken from the fp32 dS.  No atomics: `slabs` =
 * min(ceil(windows / 2), 2048 / nH) workgroups per head each walk a fixed set of windows and write one [T, T] partial to ws_buf, which two small launches
 * add in slab order and fold into the bins in a fixed order; two runs give the same bits.
 * ws_floats >= PASSL_WINDOW_ATTENTION_WS_FLOATS(B * nW, nH, ws). */
#define PASSL_WINDOW_ATTENTION_WORKGROUPS 2048 /* slabs * nH aims at this many: about eight per CU */
#define PASSL_WINDOW_ATTENTION_SLABS(windows, nH)                                                         \
  ((((windows) + 1) / 2) < (PASSL_WINDOW_ATTENTION_WORKGROUPS / (nH) > 0 ? PASSL_WINDOW_ATTENTION_WORKGROUPS / (nH) : 1) \
       ? (((windows) + 1) / 2)                                                                            \
       : (PASSL_WINDOW_ATTENTION_WORKGROUPS / (nH) > 0 ? PASSL_WINDOW_ATTENTION_WORKGROUPS / (nH) : 1))
#define PASSL_WINDOW_ATTENTION_WS_FLOATS(windows, nH, ws) \
  ((int64_t)PASSL_WINDOW_ATTENTION_SLABS(windows, nH) * (nH) * (ws) * (ws) * (ws) * (ws))
int passl_hip_window_attention_bwd(const void* qkv, const float* table, const void* out, const void* dout,
                                   const float* lse, void* dqkv, float* dtable, float* ws_buf, int64_t ws_floats, int B,
                                   int Hp, int Wp, int ws, int shift, int nH, int DH, float scale, int dtype,
                                   passl_stream_t stream);
/* PatchMerging's gather (swin_transformer.py:343-384): x [B, H, W, C] -> y [B, H/2, W/2, 4C],
 * y[b, oy, ox, k C + c] = x[b, 2 oy + (k & 1), 2 ox + (k >> 1), c] (x0, x1, x2, x3 of the reference), one streaming
 * launch of 16-byte accesses.  H, W even, C % 8 == 0, 16-byte aligned tensors (PASSL_EINVAL otherwise).  _bwd: the
 * inverse copy, dx [B, H, W, C] fully written from dy [B, H/2, W/2, 4C]. */
int passl_hip_patch_merge(const void* x, void* y, int B, int H, int W, int C, int dtype, passl_stream_t stream);
int passl_hip_patch_merge_bwd(const void* dy, void* dx, int B, int H, int W, int C, int dtype, passl_stream_t stream);

/* ---------------------------------------------------------------- CaiT (csrc/cait_attention.hip)
 * Talking-heads attention.  Reference: TalkingHeadAttn.forward, passl/models/cait.py:137-185.
 * qkv [B, T, 3, H, DH] in `dtype`; out, dout [B, T, H, DH]; lse fp32 [B, H, T], the log-sum-exp of A_g's rows.
 * wl [H, H], bl [H] (proj_l) and ww [H, H], bw [H] (proj_w) are fp32, [in, out] as the parameters lie.  Per image:
 *   S_h = (q_h k_h^T) scale;  A_g = sum_h S_h wl[h, g] + bl[g];  P_g = softmax_j A_g over the T keys;
 *   R_g = sum_h P_h ww[h, g] + bw[g];  O_g = R_g v_g.
 * All arithmetic is fp32 on the stored values in both dtypes; bf16 rounds only what it stores.
 * Accepted: DH = 48, 1 <= T <= 208, 1 <= H <= 8 (PASSL_EUNSUPPORTED otherwise); tensors in `dtype` 16-byte aligned
 * (PASSL_EINVAL otherwise).  Nothing is launched when a status other than PASSL_OK is returned for these reasons. */
int passl_hip_talking_heads_attention_fwd(const void* qkv, const float* wl, const float* bl, const float* ww,
                                          const float* bw, void* out, float* lse, int B, int T, int H, int DH,
                                          float scale, int dtype, passl_stream_t stream);
/* dqkv [B, T, 3, H, DH] (fully written); dwl, dww fp32 [H, H] and dbl, dbw fp32 [H] (WRITTEN, summed over the batch).
 * ws_buf holds delta [B, H, T] (delta_h[i] = sum_j P_h dP_h, written by the dQ sweep and read by the dK / dV sweep) and
 * one partial [144] of the small gradients per workgroup, added in a fixed order by a last launch: no atomics, two
 * runs give the same bits.  ws_floats >= PASSL_TALKING_HEADS_ATTENTION_WS_FLOATS(B, T, H). */
#define PASSL_TALKING_HEADS_ATTENTION_WS_FLOATS(B, T, H) \
  ((int64_t)(B) * (H) * (T) + (int64_t)(B) * (((T) + 15) / 16) * 144)
int passl_hip_talking_heads_attention_bwd(const void* qkv, const float* wl, const float* bl, const float* ww,
                                          const float* bw, const void* dout, const float* lse, void* dqkv, float* dwl,
                                          float* dbl, float* dww, float* dbw, float* ws_buf, int64_t ws_floats, int B,
                                          int T, int H, int DH, float scale, int dtype, passl_stream_t stream);
/* Class attention.  Reference: ClassAttn.forward, cait.py:46-88, after the three Linears.  q, out, dout, dq
 * [B, H * DH] (the class rows); k, v, dk, dv [B, T, H * DH]; lse fp32 [B, H].  out_h = softmax_j((q_h . k_jh) scale) v_h.
 * One wave per (image, head); k and v are read once per direction.  Same envelope as above. */
int passl_hip_class_attention_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int T,
                                  int H, int DH, float scale, int dtype, passl_stream_t stream);
int passl_hip_class_attention_bwd(const void* q, const void* k, const void* v, const void* dout, const float* lse,
                                  void* dq, void* dk, void* dv, int B, int T, int H, int DH, float scale, int dtype,
                                  passl_stream_t stream);
/* Token plumbing of the CaiT model over rows of C channels in `dtype` (C % 8 == 0, tensors 16-byte aligned; PASSL_EINVAL
 * otherwise), one streaming launch each:
 *   pos_add:    out[b, t] = x[b, t] + pos[t], pos fp32 [L, C]; cait.py:354 (the class row joins later and has no position)
 *   cls_concat: out [B, 1 + L, C] = concat(c, x) along the token axis, x [B, L, C]; c [B, C], or [C] when c_per_image == 0
 *               (cait.py:130 and the expand of :360)
 *   cls_split:  its backward: dc [B, C] = dout[:, 0], dx [B, L, C] = dout[:, 1:] (+ add [B, L, C] unless NULL). */
int passl_hip_cait_pos_add(const void* x, const float* pos, void* out, int B, int L, int C, int dtype,
                           passl_stream_t stream);
int passl_hip_cait_cls_concat(const void* c, int c_per_image, const void* x, void* out, int B, int L, int C, int dtype,
                              passl_stream_t stream);
int passl_hip_cait_cls_split(const void* dout, const void* add, void* dc, void* dx, int B, int L, int C, int dtype,
                             passl_stream_t stream);

/* ---------------------------------------------------------------- token merging, ToMe (csrc/tome.hip)
 * Reference: passl/models/utils/tome.py — bipartite_soft_matching :28-118, merge_wavg :121-133, ToMeAttention :172-195.
 *
 * Matching.  qkv [B, T, 3, H, DH] in `dtype`, the projection the attention kernel reads.  metric[t] = the mean over
 * heads of the K slice (k.mean(1)), formed and L2-normalised in fp32.  A = the even tokens (ceil(T/2), token 0 is the
 * class token), B = the odd tokens (floor(T/2)).  For A row i: node_max[i], node_idx[i] = max and arg-max over B of
 * metric[2i] . metric[2j+1]; row 0 is -inf / 0 (the class token is never merged, tome.py:63-64).  The r rows of largest
 * node_max are merged into their arg-max B token.
 *   Ties (ours; the reference's argsort is not stable): the arg-max is the LOWEST B index of equal scores; of equal
 *   node_max the LOWER A index ranks first.  A key that is all zero has metric 0 (the reference: NaN).
 * dest int32 [B, T] = the output row, 0 .. T-r-1, of every input token, in the reference's output order (tome.py:76-78,
 * 99): the unmerged A tokens in ascending order (the class token stays row 0), then every B token in order; a merged A
 * token has the row of its B token.  node_max fp32 [B, ceil(T/2)] and node_idx int32 [B, ceil(T/2)] are written unless
 * NULL.  One launch, one workgroup per image; the score matrix never reaches memory.
 * Accepted: 3 <= T <= 208, DH in {32, 64} (PASSL_EUNSUPPORTED otherwise); 1 <= r <= (T-1)/2, the clamp of tome.py:53
 * with the class token protected, qkv 16-byte aligned (PASSL_EINVAL otherwise: the caller clamps, and does not call with
 * r = 0). */
int passl_hip_tome_match(const void* qkv, int32_t* dest, float* node_max, int32_t* node_idx, int B, int T, int H, int DH,
                         int r, int dtype, passl_stream_t stream);
/* merge_wavg: y[b, row] = sum over {t : dest[b, t] = row} of size[b, t] x[b, t] / size_out[b, row], size_out[b, row] =
 * the sum of those size[b, t].  x [B, T, C], y [B, T-r, C] in `dtype`; size fp32 [B, T] or NULL (all ones); size_out fp32
 * [B, T-r]; logsize_out fp32 [B, T-r] = log(size_out) unless NULL (the key bias of the next proportional attention).
 * fp32 sums in ascending t, one rounding at the store; a gather per output row: no atomics, no scratch, two runs give the
 * same bits.  A dest outside [0, T-r) is ignored.  1 <= r < T <= 208, C % 8 == 0, x and y 16-byte aligned. */
int passl_hip_tome_merge_fwd(const void* x, const float* size, const int32_t* dest, void* y, float* size_out,
                             float* logsize_out, int B, int T, int r, int C, int dtype, passl_stream_t stream);
/* dx[b, t] = dy[b, dest[b, t]] * (size[b, t] / size_out[b, dest[b, t]]), fully written; the matching and the sizes carry no
 * gradient (the reference matches under no_grad). */
int passl_hip_tome_merge_bwd(const void* dy, const float* size, const float* size_out, const int32_t* dest, void* dx,
                             int B, int T, int r, int C, int dtype, passl_stream_t stream);
/* Proportional attention, forward only (tome.py:183-185): passl_hip_attention_fwd without the causal flag and with
 * score = (q . k) scale + key_bias[b, j], key_bias fp32 [B, T] = log(size).  Same envelope, same routing by dtype and
 * options; with key_bias = 0 the output has the bits of passl_hip_attention_fwd. */
int passl_hip_attention_fwd_keybias(const void* qkv, const float* key_bias, void* out, float* lse, int B, int T, int H,
                                    int DH, float scale, int dtype, passl_stream_t stream);
/* Key-tiled attention for longer sequences (csrc/attention_tiled.hip): the layouts and the result of
 * passl_hip_attention_fwd / _bwd without a causal flag — qkv [B,T,3,H,DH], out and dout [B,T,H,DH], lse fp32 [B,H,T],
 * dqkv [B,T,3,H,DH] fully written.  Replaces Attention.forward, passl/models/vision_transformer.py:142-156, at the 577 /
 * 578 tokens of DeiT at 384 pixels (passl/models/deit.py).
 * A workgroup owns a block of query rows of one (image, head) — the grid is over (image, head, block) — and streams the
 * head's K and V through LDS 64 rows at a time under an online softmax in fp32 (running max, running sum, an accumulator
 * rescaled when the max rises; out = accumulator / sum at the end): the T x T scores never reach memory and the LDS
 * footprint does not depend on T.  The backward is two sweeps, own query rows against streamed K and V blocks for dQ and
 * own key columns against streamed Q and dO blocks for dK and dV; P is recomputed from lse, delta_i = dO_i . O_i.  No
 * atomics, no scratch, no workspace: two launches give the same bits.
 * Operands as in passl_hip_attention_fwd: fp32 activations, and bf16 activations of which some pointer is not 16-byte
 * aligned, use exact-fp32 MFMA; aligned bf16 activations use bf16 MFMA and round P (unnormalised, exp(s - running max))
 * or dS as the operand of the second product, and every store.
 * Accepted: 1 <= T <= 1024, DH in {32, 64}, B and H positive (PASSL_EUNSUPPORTED otherwise, and for an unknown dtype);
 * a NULL pointer is PASSL_EINVAL.  Nothing is launched unless PASSL_OK is returned. */
int passl_hip_attention_tiled_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, int DH, float scale,
                                  int dtype, passl_stream_t stream);
int passl_hip_attention_tiled_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                  int B, int T, int H, int DH, float scale, int dtype, passl_stream_t stream);
/* Token assembly with NP = 1 or 2 learnable prefix rows (csrc/deit_tokens.hip; DistilledVisionTransformer.forward_features,
 * passl/models/deit.py:238-247: concat(cls_token, dist_token, patches) + pos_embed).  x [B, L, C] and out [B, NP + L, C] in
 * `dtype`; prefix0, prefix1 fp32 [C] (prefix1 is not read when NP = 1 and may be NULL), pos fp32 [NP + L, C]:
 *   out[b, t] = (t < NP ? prefix_t : x[b, t - NP]) + pos[t].
 * The backward writes dx[b, t - NP] = dout[b, NP + t] fully and ADDS sum_b dout[b, t] to dprefix_t (fp32 [C], images in
 * order); dpos is passl_hip_colsum_acc over dout as [B, (NP + L) C].  One streaming launch each; no atomics, two runs give
 * the same bits.  C % 8 == 0, every pointer 16-byte aligned, NP in {1, 2} (PASSL_EINVAL otherwise). */
int passl_hip_prefix_tokens_fwd(const void* x, const float* prefix0, const float* prefix1, const float* pos, void* out,
                                int B, int L, int NP, int C, int dtype, passl_stream_t stream);
int passl_hip_prefix_tokens_bwd(const void* dout, void* dx, float* dprefix0, float* dprefix1, int B, int L, int NP, int C,
                                int dtype, passl_stream_t stream);
/* out[i] = (a[i] + b[i]) / 2 over n fp32 elements: the distilled DeiT's (head(x) + head_dist(x_dist)) / 2 (deit.py:259).
 * b == NULL: out = a / 2, the gradient both heads receive.  n > 0 and a, out non-NULL (PASSL_EINVAL otherwise). */
int passl_hip_mean2(const float* a, const float* b, float* out, int64_t n, passl_stream_t stream);

/* ---------------------------------------------------------------- CAE pre-training (csrc/cross_attention.hip, cae.hip)
 * Reference: passl/models/cae.py, tasks/ssl/cae/engine_pretrain.py. */

/* Cross-attention with separate operands and lengths (CAECrossAttention.forward, cae.py:244-257):
 *   out = softmax(q k^T scale) v  per (image, head),
 * q, out, dout, dq [B,Tq,H,DH]; k, v, dk, dv [B,Tk,H,DH], all contiguous in `dtype`; lse fp32 [B,H,Tq].  dq, dk and dv are
 * three tensors and are fully written.  The kernels are those of passl_hip_attention_tiled_fwd / _bwd with the loop
 * bounds Tq on the query side and Tk on the key side: a workgroup owns a block of query rows (dK / dV sweep: key columns)
 * of one (image, head) and streams K and V (Q and dO) through LDS 64 rows at a time; fp32 online softmax; a padding key
 * is not a key; P is recomputed from lse in the backward, delta_i = dO_i . O_i.  No atomics, no scratch, no workspace: two
 * launches give the same bits, and with Tq = Tk and q, k, v the slices of one qkv the results have the bits of
 * passl_hip_attention_tiled_fwd / _bwd.
 * Operand routing is passl_hip_attention_tiled_fwd's: aligned bf16 takes bf16 MFMA; fp32, and bf16 with some pointer off
 * 16-byte alignment, take exact-fp32 MFMA.
 * Accepted: 1 <= Tq <= 1024, 1 <= Tk <= 1024, DH in {32, 64}, B and H positive (PASSL_EUNSUPPORTED otherwise, and for an
 * unknown dtype); a NULL pointer is PASSL_EINVAL.  Nothing is launched unless PASSL_OK is returned. */
int passl_hip_cross_attention_fwd(const void* q, const void* k, const void* v, void* out, float* lse, int B, int Tq,
                                  int Tk, int H, int DH, float scale, int dtype, passl_stream_t stream);
int passl_hip_cross_attention_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                  const float* lse, void* dq, void* dk, void* dv, int B, int Tq, int Tk, int H, int DH,
                                  float scale, int dtype, passl_stream_t stream);
/* The operands of the latent regressor (cae.py:440-444, 811-815, 1009-1015) from the visible latents xu [B,u0+Nu,C], read
 * from row u0 of every image (u0 = 1 skips the encoder's class row, cae.py:1017, without a copy), the masked rows
 * xm [B,Nm,C] (`dtype`), the fixed position table pos fp32 [1 + L, C] (row 0 is the class token's) and the
 * index tables ids_vis int32 [B,Nu], ids_msk int32 [B,Nm] of patch numbers in [0, L):
 *   q_in [B,Nm,C]      = xm + pos[1 + ids_msk]
 *   v_in [B,Nu+Nm,C]   = concat(xu, xm)
 *   k_in [B,Nu+Nm,C]   = v_in + concat(pos[1 + ids_vis], pos[1 + ids_msk])
 * Any output may be NULL (not all three); with k_in = v_in = NULL only the masked rows are visited and xu, ids_vis are
 * not read: the decoder's x_masked + pos_embed_masked (cae.py:823).  Sums in fp32, one rounding at the store; an index
 * outside [0, L) is clamped.  One streaming launch, no expanded position tensor and no concat copy.
 * The backward writes dxm = dq_in + dk_in[:, Nu:] + dv_in[:, Nu:] and dxu = dk_in[:, :Nu] + dv_in[:, :Nu] fully (fp32
 * sums in that order, no accumulation; a NULL gradient counts as zero; dxu may be NULL: only dxm is formed).  dxu is
 * [B,u0+Nu,C] and its first u0 rows of every image are written as zeros.  The table is fixed: there is no dpos.
 * C % 8 == 0, every pointer 16-byte aligned, u0 >= 0, Nu >= 0, Nm > 0, dxu NULL when Nu == 0 (PASSL_EINVAL otherwise). */
int passl_hip_cae_tokens_assemble(const void* xu, const void* xm, const float* pos, const int32_t* ids_vis,
                                  const int32_t* ids_msk, void* q_in, void* k_in, void* v_in, int B, int u0, int Nu,
                                  int Nm, int L, int C, int dtype, passl_stream_t stream);
int passl_hip_cae_tokens_assemble_bwd(const void* dq_in, const void* dk_in, const void* dv_in, void* dxu, void* dxm,
                                      int B, int u0, int Nu, int Nm, int C, int dtype, passl_stream_t stream);
/* The index tables of a 0/1 fp32 mask [B, L] (1 = masked) with L - Nu ones per image, in ascending patch order — the
 * order of the reference's boolean indexing x[~bool_masked_pos] / x[bool_masked_pos] (cae.py:662, 1011-1015):
 *   ids_vis int32 [B, Nu]    the visible patches,      ids_msk int32 [B, L - Nu]   the masked patches,
 *   rank int32 [B, L]        a visible patch's place among the visible ones, Nu + its place among the masked ones for a
 *                            masked patch (passl_hip_mae_gather_bwd's ids_restore for the gather on ids_vis).
 * One launch, one wave per image: passl_hip_mae_mask with the mask as its noise gives ids_vis and rank, this entry the
 * masked side as well.  A mask with another count of ones writes nothing outside the tables and fills what is left of
 * them with 0.  0 < Nu < L (PASSL_EINVAL otherwise). */
int passl_hip_cae_mask_ids(const float* mask, int32_t* ids_vis, int32_t* ids_msk, int32_t* rank, int B, int L, int Nu,
                           passl_stream_t stream);
/* F.mse_loss(pred.float(), target.float(), 'mean') (engine_pretrain.py:29-31): pred [B,Tm,C], target [B,Tm+t0,C] read
 * from row t0 of every image (t0 = 1 drops the teacher's class row, cae.py:984, without a copy), both in `dtype`.
 * loss[0] = sum (pred - target)^2 / (B Tm C): differences, squares and sums in fp32, one wave per row into ws (B Tm
 * floats), the rows added in a fixed order.  The backward is dpred = gloss 2 (pred - target) / (B Tm C) in `dtype`
 * (gloss: device scalar, NULL = 1); the target has no gradient.  C % 8 == 0, pointers 16-byte aligned. */
int passl_hip_mse_fwd(const void* pred, const void* target, float* loss, int B, int Tm, int t0, int C, int dtype,
                      float* ws, int64_t ws_floats, passl_stream_t stream);
int passl_hip_mse_bwd(const void* pred, const void* target, const float* gloss, void* dpred, int B, int Tm, int t0, int C,
                      int dtype, passl_stream_t stream);

/* ---------------------------------------------------------------- mixup / cutmix and soft-target cross-entropy
 * Reference: class Mixup, passl_v110/datasets/preprocess/mixup.py:108-276 (the reference mixes on the host, in numpy or
 * through the framework's CPU tensors); SoftTargetCrossEntropy, tasks/ssl/mae/util/loss.py:44-47. */

/* Mixup._mix_batch (mixup.py:248-264) on a resident batch: x, out fp32 NCHW [B,C,H,W], OUT OF PLACE (x is not written;
 * x == out is refused).  The partner of sample b is B-1-b (x.flip(0)); the middle sample of an odd B is its own partner.
 *   mode 0 (mixup, :261-263): out = fl(fl(x * lam) + fl(x' * one_minus_lam)), fp32, two separately rounded products
 *     and a rounded sum (no FMA).  The caller passes float(lam) and float(1.0 - lam), the subtraction done in double.
 *   mode 1 (CutMix, :259): out = x' in rows [yl, yh) x columns [xl, xh) of every channel, x elsewhere; lam and
 *     one_minus_lam are ignored.  An empty box copies x.
 * The box must satisfy 0 <= yl <= yh <= H, 0 <= xl <= xh <= W in both modes.  One lane handles the same elements of a
 * sample and of its partner, so a launch reads and writes each byte of the batch once.  16-byte accesses when
 * C*H*W % 4 == 0 and both pointers are 16-byte aligned, single floats otherwise. */
int passl_hip_batch_mix(const float* x, float* out, int B, int C, int H, int W, float lam, float one_minus_lam, int yl,
                        int yh, int xl, int xh, int mode, passl_stream_t stream);
/* mixup_target (mixup.py:29-37): labels int64 [N] -> target fp32 [N,C] (16-byte aligned),
 * target[i] = lam * smooth(onehot(labels[i])) + (1 - lam) * smooth(onehot(labels[N-1-i])),
 * smooth(v) = (1 - eps) * v + eps / C.  lam = 1: plain label smoothing; lam = 1, eps = 0: one-hot.  lam, eps in [0, 1].
 * A label outside [0,C) makes every row that uses it NaN. */
int passl_hip_mixup_target(const int64_t* labels, float* target, int N, int C, float lam, float eps,
                           passl_stream_t stream);
/* SoftTargetCrossEntropy (util/loss.py:44-47; passl/loss/celoss.py:48-49): scores, target fp32 [N,C] ->
 * lse [N], tsum [N] (T_i = sum_j t_ij; both saved for the backward), out = {mean_i (lse_i T_i - sum_j t_ij s_ij),
 * acc1 (%), acc5 (%)}.  Rows need not sum to one.  Accuracy is taken against argmax_j t_ij (lowest index on ties; the
 * wrappers that accept mixup_fn do the same, architectures/ViTWrapper.py:91-108) by rank counting as in
 * passl_hip_softmax_ce_fwd.  ws: 3 * N floats (per-row terms, summed in a fixed order). */
int passl_hip_soft_ce_fwd(const float* scores, const float* target, int N, int C, float* lse, float* tsum, float* out,
                          float* ws, int64_t ws_floats, passl_stream_t stream);
/* dscores[i][j] = gloss/N * (exp(scores_ij - lse_i) * tsum_i - target_ij); gloss: device scalar. */
int passl_hip_soft_ce_bwd(const float* scores, const float* target, const float* lse, const float* tsum,
                          const float* gloss, int N, int C, float* dscores, passl_stream_t stream);

/* ---------------------------------------------------------------- random erasing
 * Reference: class RandomErasing, passl_v110/datasets/preprocess/random_erasing.py:34-115 (it erases on the host, sample
 * by sample).  x, out fp32 NCHW [B,C,H,W]; boxes: a DEVICE table int32 [B][4] = (top, left, h, w), h == 0 or w == 0
 * meaning "this sample is not erased".  One row per sample is the whole interface: the reference erases at most one box
 * per sample whatever max_count is (`_erase` returns after its first successful box, :89-103; the drawn count only
 * divides the target area).
 *   out != x: out of place, one pass; out = x outside the box and the fill inside it, x is never written.
 *   out == x: in place; only box elements are stored, x is not loaded.  (Buffers that overlap otherwise: undefined
 *     values, no access outside them.)
 *   mode 0 ('const'): the fill is 0.0f.
 *   mode 1 ('pixel'): the fill is a standard normal defined by position.  e = (c*H + y)*W + x_col (the element's index
 *     inside its sample), g = e >> 2, (w0,w1,w2,w3) = Philox4x32-10(counter (g, b, step_lo32, step_hi32), key (seed_lo32,
 *     seed_hi32)); u0 = (float(w0 >> 8) + 1) * 2^-24 and u2 likewise from w2, in (0, 1]; u1 = float(w1 >> 8) * 2^-24 and
 *     u3 likewise from w3, in [0, 1); r01 = sqrtf(-2 logf(u0)), r23 = sqrtf(-2 logf(u2));
 *     z = (r01 cos 2 pi u1, r01 sin 2 pi u1, r23 cos 2 pi u3, r23 sin 2 pi u3); element e gets z[e & 3].  Precise
 *     single-precision logf / sqrtf / sincospif.  A sample's values depend on (seed, step, b, e) only: not on B, not on
 *     the grid, not on the box.
 *   The reference's 'rand' mode (one colour per box) is not built: its class raises on any box whose width is not 3.
 * 16-byte accesses when C*H*W % 4 == 0 and both pointers are 16-byte aligned, single floats otherwise.  The library
 * cannot read the table on the host: the caller validates it; the kernel clamps every box to the image, so no access
 * leaves the tensor whatever the table holds.  NULL pointers, B < 0, C, H, W <= 0, C*H*W >= 2^31, an unknown mode,
 * pointers not 4-byte aligned -> PASSL_EINVAL; B == 0 -> PASSL_OK, nothing launched. */
int passl_hip_random_erase(const float* x, float* out, const int32_t* boxes, int B, int C, int H, int W, int mode,
                           int64_t seed, int64_t step, passl_stream_t stream);

/* ---------------------------------------------------------------- random resized crop, flip, normalise
 * Reference: RandCropImage / MAERandCropImage, RandFlipImage / RandomHorizontalFlip, NormalizeImage, ToCHWImage of
 * passl/data/preprocess/basic_transforms.py (:373-419, :635-767), which run on the host through Pillow, sample by sample.
 * src uint8 [B][Hs][Ws][3] (HWC, never written); out fp32 [B][3][S][S]; table: a DEVICE table int32 [B][8] =
 * (top, left, h, w, flip, 0, 0, 0); mean_std_scale: 7 HOST floats (mean[3], std[3], scale), read during the call.
 *   out[b] = Pillow's 8-bit Image.resize((S, S), BICUBIC) of src[b, top:top+h, left:left+w], flipped left-right when
 *   flip != 0, then (float(v) * scale - mean[c]) / std[c], each operation rounded to fp32 on its own.
 *   Resampling, per axis (n_in crop pixels -> S outputs), in IEEE double without contraction: scale = n_in / S,
 *   fs = max(1, scale), support = 2 fs; output i: center = (i + 0.5) scale, lo = max((int)(center - support + 0.5), 0),
 *   hi = min((int)(center + support + 0.5), n_in), w_k = bicubic_{a = -0.5}(((k + lo) - center + 0.5) (1 / fs)) for
 *   k < hi - lo, divided by their sum (k order), K_k = (int)(w_k 2^22 +- 0.5) (truncation, the sign of w_k);
 *   a pass = clip((2^21 + sum_k K_k p[lo + k]) >> 22, 0, 255).  The horizontal pass first, rounded to uint8; the vertical
 *   pass on those values.  Taps are clamped to the crop, not to the source.  Bit-equal to the reference's PIL path.
 * Envelope (PASSL_EUNSUPPORTED beyond): one band of 16 output rows must fit 64 KiB of LDS — with r = max(1, Hs / S),
 * rw = max(1, Ws / S), KH = 2 ceil(2 rw) + 1, KV = 2 ceil(2 r) + 1, NR = ceil(15 r) + 2 ceil(2 r) + 3:
 * 4 S (KH + 2) + 64 (KV + 2) + 3072 + 3 S NR (each term rounded up to 16) <= 65536.
 * The library cannot read the table on the host: the kernel clamps every box to the source (top, left into it, then
 * 1 <= h <= Hs - top, 1 <= w <= Ws - left), so no access leaves a tensor whatever the table holds.  NULL pointers,
 * B < 0, Hs, Ws, S <= 0, a source or output sample of 2^31 bytes / elements or more, a zero std, out or table not
 * 4-byte aligned -> PASSL_EINVAL; B == 0 -> PASSL_OK, nothing launched. */
int passl_hip_crop_resize_norm(const uint8_t* src, float* out, const int32_t* table, int B, int Hs, int Ws, int S,
                               const float* mean_std_scale, passl_stream_t stream);

/* The same crop and resampling (the same device code path up to the vertical pass), ending in the resized image itself:
 * out uint8 [B][S][S][3] (HWC), flipped left-right when flip != 0; no normalisation.  The input of the colour stage below.
 * Same envelope and argument checks (out needs no alignment). */
int passl_hip_crop_resize_u8(const uint8_t* src, uint8_t* out, const int32_t* table, int B, int Hs, int Ws, int S,
                             passl_stream_t stream);

/* ---------------------------------------------------------------- colour jitter, grayscale, solarise, Gaussian blur
 * Reference: ColorJitter, RandomGrayscale, SimCLRGaussianBlur, BYOLSolarize of passl/data/preprocess/basic_transforms.py
 * (:770-787, :872-944), which run on the host through Pillow, sample by sample.  img uint8 [B][H][W][3] (HWC, never
 * written).  table: a DEVICE table int32 [B][24], one row per sample:
 *   [0] n, the number of operations (<= 8)   [1] flip   [2] blur r (< 0: the sample is not blurred)   [3] ww   [4] fw
 *   [5] split: operations [0, split) run before the blur, [split, n) after it (split = n without a blur)
 *   [6] the index of the sample's contrast entry (< 0: none; at most one, before split)   [7] 0
 *   [8..16) codes: 0 none, 1 brightness, 2 contrast, 3 saturation, 4 hue, 5 grayscale, 6 solarise
 *   [16..24) values: the bits of the fp32 factor (1, 2, 3), the hue shift in [0, 256) (4), unused otherwise
 * RESULT, Pillow's 8-bit arithmetic bit for bit:
 *   blend(deg, v, a) = float(deg) + a * float(v - deg), the product and the sum each rounded to fp32 (no fused
 *     multiply-add); for 0 <= a <= 1 truncated to uint8, otherwise 0 for t <= 0, 255 for t >= 255, truncated in between
 *   gray = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *   brightness: blend(0, v, a); saturation: blend(gray, v, a); contrast: blend(m, v, a), m = (2 sums[b] + H W) / (2 H W);
 *   hue: RGB -> HSV, H = (H + shift) mod 256, HSV -> RGB, as Pillow's Convert.c (csrc/view_aug_pixel.h);
 *   grayscale: R = G = B = gray; solarise: v < 128 ? v : 255 - v.
 * The library cannot read the table on the host: the caller validates it; the kernels clamp every count, index and radius
 * and treat an unknown code as "none", so no access leaves a tensor whatever the table holds.  Common argument errors:
 * NULL pointers, B < 0, H, W <= 0, a sample of 2^31 bytes or more, a table not 4-byte aligned -> PASSL_EINVAL; B == 0 ->
 * PASSL_OK, nothing launched.
 *
 * view_gray_sum: sums[b] (8-byte aligned, [B]) = the sum of gray over sample b after its operations [0, contrast index),
 *   0 for a sample without a contrast entry.  Integer sums, one workgroup per sample: exact and order-free, no atomics. */
int passl_hip_view_gray_sum(const uint8_t* img, const int32_t* table, uint64_t* sums, int B, int H, int W,
                            passl_stream_t stream);
/* view_pointwise: the operations of one part of every sample's list: part 0 = [0, n), 1 = [0, split), 2 = [split, n).
 *   Exactly one output: out_u8 uint8 [B][H][W][3] (the flip is NOT applied), or out_f32 fp32 [B][3][H][W], flipped
 *   left-right when flip != 0 and normalised, (float(v) * scale - mean[c]) / std[c] as passl_hip_crop_resize_norm does
 *   (mean_std_scale: 7 HOST floats; 16-byte stores when W % 4 == 0 and out_f32 is 16-byte aligned, single floats
 *   otherwise).  sums: what view_gray_sum wrote, or NULL when no sample has a contrast entry. */
int passl_hip_view_pointwise(const uint8_t* img, const int32_t* table, const uint64_t* sums, uint8_t* out_u8,
                             float* out_f32, int B, int H, int W, int part, const float* mean_std_scale,
                             passl_stream_t stream);
/* gaussian_blur_u8: Pillow's ImageFilter.GaussianBlur = three box passes along x, then three along y, each rounding to
 *   uint8, every tap clamped to the image at every pass:
 *     out[x] = (ww sum_{|k| <= r} p[x + k] + fw (p[x - r - 1] + p[x + r + 1]) + 2^23) >> 24     (32-bit unsigned)
 *   (r, ww, fw) per sample from the table, computed by the host (fp32: s2 = radius^2 / 3, L = sqrt(12 s2 + 1),
 *   l = floor((L - 1) / 2), fr = l + (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)), r = (int)fr,
 *   ww = (uint32)(2^24 / (2 fr + 1)), fw = (2^24 - (2r + 1) ww) / 2).  Out of place (img == out -> PASSL_EINVAL); samples
 *   with r < 0 are copied.  r_max: the largest r of the table, as the caller knows it; above the built maximum (1, which
 *   covers a radius up to about 2.3) -> PASSL_EUNSUPPORTED.  The kernel clamps r to the built maximum. */
int passl_hip_gaussian_blur_u8(const uint8_t* img, uint8_t* out, const int32_t* table, int B, int H, int W, int r_max,
                               passl_stream_t stream);

/* ---------------------------------------------------------------- measurement hooks */

/* When enabled, every passl_hip_conv_igemm / passl_hip_conv_wgrad launch is bracketed by HIP
 * events on its own stream; passl_hip_prof_collect synchronises those events and returns the
 * accumulated kernel time (ms) and launch count per kernel class (0 = ring igemm, 1 = wgrad, 2 = register-staged
 * igemm / stem, 3 = 8-phase igemm). */
int passl_hip_prof_enable(int on);
int passl_hip_prof_collect(int kernel_class, double* total_ms, int64_t* launches);
/* Algorithmic work of the launches timed since the last call for this class: FLOPs (2 x MACs of the real
 * taps) and HBM bytes (every operand element once).  Classes: 0 igemm_ring_kernel, 1 weight gradients,
 * 2 igemm_kernel (register-staged). */
int passl_hip_prof_collect_work(int kernel_class, double* flops, double* bytes);
/* Average reading (us) of n back-to-back event pairs with nothing in between on `stream`: what the event bracket of
 * prof_enable adds to a kernel's own duration (synchronises the stream). */
int passl_hip_prof_event_overhead(int n, passl_stream_t stream, double* avg_us);

/* ---------------------------------------------------------------- CLIP
 * Reference: class CLIP, passl_v110/modeling/backbones/clip.py:183-336; QuickGELU
 * base_transformer.py:25-28; CLIPHead, passl_v110/modeling/heads/clip_head.py:24-36. */

/* QuickGELU y = x * sigmoid(1.702 x) and dx = dy * d/dx; n % 8 == 0. */
int passl_hip_quick_gelu_fwd(const void* x, void* y, int64_t n, int dtype, passl_stream_t stream);
int passl_hip_quick_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype,
                             passl_stream_t stream);
/* encode_text input (clip.py:295-298): out[b,t] = table[text[b,t]] + pos[t]; text int64 [B,T],
 * table fp32 [vocab,C], pos fp32 [T,C], out [B*T,C] in `dtype`.  Ids outside [0,vocab) read as 0. */
int passl_hip_embed_fwd(const int64_t* text, const float* table, const float* pos, void* out, int B,
                        int T, int C, int vocab, int dtype, passl_stream_t stream);
/* its backward: dtable[text[b,t]] += dout[b,t] (scatter-add), dpos[t] += sum_b dout[b,t]; both fp32,
 * ACCUMULATED into.  C <= 2048.  Bit-reproducible: the scatter-add accumulates 64-bit FIXED-POINT values (one
 * power-of-two scale per launch, chosen from max|dout|) with integer atomics — exact and order-independent —
 * in `acc` (>= passl_hip_embed_bwd_acc_bytes(vocab, C) bytes, a PERSISTENT buffer of the caller that is zero
 * before the first call and is left zero by every call); the position sums go through slabs in `ws`
 * (>= passl_hip_embed_bwd_ws_floats(B, T, C) floats, per-call scratch). */
int64_t passl_hip_embed_bwd_acc_bytes(int vocab, int C);
int64_t passl_hip_embed_bwd_ws_floats(int B, int T, int C);
int passl_hip_embed_bwd(const int64_t* text, const void* dout, float* dtable, float* dpos, int B,
                        int T, int C, int vocab, int dtype, void* acc, int64_t acc_bytes, float* ws,
                        int64_t ws_floats, passl_stream_t stream);
/* out[r] = x[idx[r]] for r < n (class-token rows x[:, 0], EOT rows x[i][argmax text[i]]). */
int passl_hip_gather_rows(const void* x, const int32_t* idx, void* out, int n, int C, int dtype,
                          passl_stream_t stream);
/* backward of gather_rows for distinct idx: dx [rows_total, C] = 0 except dx[idx[r]] = dout[r]. */
int passl_hip_scatter_rows(const void* dout, const int32_t* idx, void* dx, int n, int64_t rows_total,
                           int C, int dtype, passl_stream_t stream);
/* idx[b] = b*T + argmax_t text[b,t] (first maximum) — clip.py:303-306. */
int passl_hip_eot_index(const int64_t* text, int B, int T, int32_t* idx, passl_stream_t stream);
/* CLIP.forward's logits (clip.py:317-336) from fp32 features img, txt [B,D] (D % 16 == 0):
 * logits [B,B] = exp(logit_scale) * (img/|img|) (txt/|txt|)^T = image_logits; text_logits is its
 * transpose.  logit_scale (device scalar, the parameter) is then clipped in place to
 * [clip_lo, clip_hi].  ws: caller-owned fp32 workspace of passl_hip_clip_logits_ws_floats(B, D) floats
 * that must survive until the backward call. */
int64_t passl_hip_clip_logits_ws_floats(int B, int D);
int passl_hip_clip_logits_fwd(const float* img, const float* txt, float* logit_scale, int B, int D,
                              float clip_lo, float clip_hi, float* ws, float* logits,
                              passl_stream_t stream);
/* dimg, dtxt [B,D] fully written; dlogit_scale[0] += sum(dlogits .* logits) (<= 256 block partials in
 * `scratch` (>= 256 floats), added in block order). */
int passl_hip_clip_logits_bwd(const float* dlogits, const float* logits, const float* ws, int B, int D,
                              float* dimg, float* dtxt, float* dlogit_scale, float* scratch,
                              passl_stream_t stream);
/* Building blocks of the CROSS-RANK form of the same logits (BASELINE configs[4]: the negatives of
 * every rank; pattern of passl/models/mocov3.py:187-198 — gather the other modality's features, labels
 * arange(B) + B*rank): image_logits = exp(s) * I^_local . T^_all^T  [B][W*B] and the text counterpart.
 *   clip_scale:  alpha = exp(*logit_scale), then *logit_scale = clip(*logit_scale) (clip.py:309-311)
 *   gemm_f32_nt: C[M][N] = *alpha * A[M][K] . B[N][K]^T        (exact-fp32 MFMA; K % 16 == 0)
 *   gemm_f32_gx: C[M][N] = *alpha * op(G) . X[K][N], op(G) = G [M][K] (trans 0) or G^T, G [K][M] (trans 1)
 *   dot_acc:     *out += sum_e a[e]*b[e]  (fixed order: <= 256 block partials in ws (>= 256 floats), then one sum)
 * Row normalisation without epsilon = passl_hip_l2norm_fwd/bwd with eps 0; the row cross-entropy with
 * offset labels = passl_hip_softmax_ce_fwd/bwd. */
int passl_hip_clip_scale(float* logit_scale, float* alpha, float clip_lo, float clip_hi,
                         passl_stream_t stream);
int passl_hip_gemm_f32_nt(const float* A, const float* B, float* C, int M, int N, int K, const float* alpha,
                          passl_stream_t stream);
int passl_hip_gemm_f32_gx(const float* G, const float* X, float* C, int M, int N, int K, int trans,
                          const float* alpha, passl_stream_t stream);
int passl_hip_dot_acc(const float* a, const float* b, int64_t n, float* out, float* ws,
                      passl_stream_t stream);
/* CLIPHead (clip_head.py:24-36) with labels arange(B): out = {CE over the rows of logits (img_loss),
 * CE over its columns (= rows of text_logits; text_loss), their sum (loss)}; lse [2B] = row and
 * column log-sum-exp, saved for the backward.  ws: 2 * B floats (per-row / per-column terms, summed in a fixed
 * order). */
int passl_hip_clip_ce_fwd(const float* logits, int B, float* lse, float* out, float* ws, int64_t ws_floats,
                          passl_stream_t stream);
/* dlogits[i][j] = gloss/B * (softmax_row_i[j] + softmax_col_j[i] - 2 [i == j]); gloss: device scalar. */
int passl_hip_clip_ce_bwd(const float* logits, const float* lse, const float* gloss, int B,
                          float* dlogits, passl_stream_t stream);

/* ---------------------------------------------------------------- linear probe
 * Reference: ClasHead.loss + accuracy, passl_v110/modeling/heads/clas_head.py:47-72. */

/* scores fp32 [N,C], labels int64 [N] -> lse [N] (row log-sum-exp, saved for the backward),
 * out = {mean cross-entropy, acc1 (%), acc5 (%)}.  Top-k membership by rank counting (ties resolve to
 * the lower index).  A label outside [0,C) makes the loss NaN.  ws: 3 * N floats (per-row terms, summed in a
 * fixed order). */
int passl_hip_softmax_ce_fwd(const float* scores, const int64_t* labels, int N, int C, float* lse,
                             float* out, float* ws, int64_t ws_floats, passl_stream_t stream);
/* dscores[i][j] = gloss/N * (softmax(scores_i)[j] - [j == labels[i]]); gloss: device scalar. */
int passl_hip_softmax_ce_bwd(const float* scores, const float* lse, const int64_t* labels,
                             const float* gloss, int N, int C, float* dscores, passl_stream_t stream);

/* ---------------------------------------------------------------- native step plans
 * Reference: the iteration of passl_v110/engine/trainer.py:287-337 (model forward, then OptimizerHook:
 * clear_grad -> backward -> step, hooks/optimizer_hook.py:25-50) is ~1 400 launches here, each of which the
 * reference-side host code (Python) would issue one by one.  A plan is that launch list recorded ONCE while a
 * step executes normally, and replayed from one call per segment:
 *   create -> record_begin -> [the step runs: every kernel this library launches, on any thread, is appended
 *   with its stream and a copy of its arguments; the host reports its cross-stream edges with event_record /
 *   stream_wait and closes a segment with cut wherever something that is not a library launch must happen in
 *   between, e.g. a collective] -> record_end -> replay(segment) ... -> destroy.
 * Contract of a replay: every pointer a recorded launch carried must still be valid and mean the same thing
 * (the host keeps the recorded step's allocations in a private pool and step-varying scalars in device memory);
 * streams are the recorded ones.  One plan records at a time per process; a plan records once.
 * event_record returns the id (>= 0) of a plan-owned event = "everything enqueued on `stream` up to here";
 * while recording nothing is enqueued for it (the executing step orders itself with the caller's own events).
 * plan_info(what): 0 segments, 1 kernel launches, 2 event records, 3 stream waits, 4 memsets, 5 argument bytes,
 * 6 replays so far, 7 distinct streams. */
typedef struct passl_plan passl_plan_t;
int passl_hip_plan_create(passl_plan_t** out);
int passl_hip_plan_destroy(passl_plan_t* plan);
int passl_hip_plan_record_begin(passl_plan_t* plan);
int passl_hip_plan_cut(passl_plan_t* plan);                 /* -> index of the segment that starts here */
int passl_hip_plan_record_end(passl_plan_t* plan);
int passl_hip_plan_event_record(passl_plan_t* plan, passl_stream_t stream);
int passl_hip_plan_stream_wait(passl_plan_t* plan, passl_stream_t stream, int event_id);
int passl_hip_plan_replay(passl_plan_t* plan, int segment);
int64_t passl_hip_plan_info(passl_plan_t* plan, int what);

/* The step's remaining framework launches as library kernels, so that a recorded step holds library launches
 * only (reference call sites: `clear_grad()` optimizer_hook.py:31; `self.queue.clone().detach()` moco.py:180;
 * the implicit dtype casts Paddle inserts around fp32 heads; the stem filter's padded gradient):
 *   fill_zero: p[0:bytes] = 0                      copy_bytes: dst[0:bytes] = src[0:bytes] (no overlap)
 *   cast_bf16_to_f32: dst[i] = float(src[i])       (both 16-byte aligned)
 *   unpad_add: dst[row][r][s][c] += src[row][r][s][c], s < dst_S, c < dst_C; src rows are [R][src_S][src_C] */
int passl_hip_fill_zero(void* p, int64_t bytes, passl_stream_t stream);
int passl_hip_copy_bytes(void* dst, const void* src, int64_t bytes, passl_stream_t stream);
int passl_hip_cast_bf16_to_f32(const void* src, float* dst, int64_t n, passl_stream_t stream);
int passl_hip_unpad_add(const float* src, float* dst, int64_t rows, int R, int dst_S, int dst_C, int src_S,
                        int src_C, passl_stream_t stream);

/* ---- element-wise dropout (csrc/dropout.hip) ------------------------------------------------------------
 * paddle.nn.Dropout(p), mode `upscale_in_train` [Paddle-semantics]: training out = kept ? x * factor : 0 with
 * factor = float32(1 / (1 - float32(p))); evaluation is the identity and launches nothing.  Reference call sites:
 * passl/models/vision_transformer.py Mlp :106-112, Attention :153-155, VisionTransformer pos_drop :358.
 * The mask is defined by position: chunk k (elements 8k .. 8k+7) of the tensor at dropout site `site` takes
 * Philox4x32-10 on counter (k, site, step_lo, step_hi), key (seed_lo, seed_hi) -> words x[0..3]; element e of the
 * chunk is kept iff ((x[e >> 1] >> (16 * (e & 1))) & 0xFFFF) >= thr, thr = floor(p * 65536 + 0.5) in [0, 65535].
 * `step` is a uint64 in device memory (8-byte aligned) that the launches READ; passl_hip_dropout_advance adds 1 to it
 * (one thread), so a replayed step plan draws fresh masks with unchanged argument bytes.  n elements, a multiple of 8
 * and at most 2^35 (PASSL_EUNSUPPORTED beyond); every tensor 16-byte aligned; fp32 arithmetic, one rounding to `dtype`.
 *   dropout           out = mask * (in * factor)                  (applied to dy: the backward of every site)
 *   dropout_add       out = residual + mask * (branch * factor)   (the product rounded to fp32 before the add)
 *   gelu_dropout_fwd  out = mask * (gelu(x) * factor)
 *   gelu_dropout_bwd  dx  = (mask * (dy * factor)) * gelu'(x) */
int passl_hip_dropout_advance(int64_t* step, passl_stream_t stream);
int passl_hip_dropout(const void* in, void* out, int64_t n, int thr, float factor, int64_t seed, const int64_t* step,
                      int site, int dtype, passl_stream_t stream);
int passl_hip_dropout_add(const void* branch, const void* residual, void* out, int64_t n, int thr, float factor,
                          int64_t seed, const int64_t* step, int site, int dtype, passl_stream_t stream);
int passl_hip_gelu_dropout_fwd(const void* x, void* out, int64_t n, int thr, float factor, int64_t seed,
                               const int64_t* step, int site, int dtype, passl_stream_t stream);
int passl_hip_gelu_dropout_bwd(const void* dy, const void* x, void* dx, int64_t n, int thr, float factor,
                               int64_t seed, const int64_t* step, int site, int dtype, passl_stream_t stream);

/* ViTCELoss(type='sigmoid'), passl/loss/celoss.py:58-95, over fp32 scores [N][C] and integer labels: the target is
 * t_on at the label and t_off elsewhere (onehot * (1 - eps) + eps, rounded once by the caller).
 *   fwd: out[0] = 1/N sum_i sum_c max(x, 0) - x t + log1p(exp(-|x|));  ws: N floats, row i's sum / N stays in ws[i]
 *   bwd: dscores = (sigmoid(x) - t) * gloss[0] / N */
int passl_hip_sigmoid_ce_fwd(const float* scores, const int64_t* labels, int N, int C, float t_on, float t_off,
                             float* out, float* ws, int64_t ws_floats, passl_stream_t stream);
int passl_hip_sigmoid_ce_bwd(const float* scores, const int64_t* labels, const float* gloss, int N, int C, float t_on,
                             float t_off, float* dscores, passl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PASSL_HIP_H_ */
