// ConvNeXt's two block-level operators that are not GEMMs (reference: passl/models/convnext.py, class Block :68-103):
// the depthwise 7x7 convolution (`self.dwconv`, padding 3, groups = dim) and the block's tail
// `input + drop_path(gamma * x)`.  Activations are NHWC [N, H, W, C] in `dtype`, parameters and their gradients fp32.
//
// Depthwise 7x7, forward and data gradient (ONE kernel: the data gradient is the forward with the filter read
// reversed and the residual fork's gradient `add` in the place of the bias):
//   a workgroup owns TH x 16 output pixels x 32 channels.  It stages the (TH + 6) x 22 input pixels of those channels
//   once in LDS, in the storage type, and the 49 x 32 filter taps as fp32 [tap][channel].  A lane owns one output row,
//   8 consecutive output columns and 4 channels: per filter row it reads the 14 input pixels under its 8 outputs once
//   (one 8- or 16-byte LDS read per pixel, bf16 pairs unpacked once per read) and slides the 7 taps over them, so every
//   value read feeds up to seven FMAs.  32 fp32 accumulators, one rounding at the store.  TH = 16 (256 threads) for
//   bf16 and 8 (128 threads) for fp32, which keeps the image below 64 KiB.
//   LDS pitch: a pixel is 32 channels, a row 23 pixels (22 + 1 pad).  A wave is 8 channel groups x 8 rows; with the
//   pad the row pitch is 32 (fp32) / 48 (bf16) dwords mod 64, which puts the rows of every service group of
//   ds_read_b128 (16 lanes) and ds_read_b64 (32 lanes) on disjoint banks.
// Weight and bias gradient: the same tile geometry (TH = 8) with the dy tile next to the x tile.  A lane owns 4 channels
//   and ONE filter row r (lanes r == 7 own the bias gradient): 28 accumulators, kept over every tile the workgroup
//   visits; along a row it reads each x pixel and each dy pixel once and does 28 FMAs per pair.  The four waves split
//   the tile's rows, are added in wave order through LDS, and the workgroup writes one slab of the caller's workspace;
//   slab_reduce_kernel (flat.hip) adds the slabs in ascending order.  No floating-point atomics anywhere.
//
// Layer scale + stochastic depth + residual, rows [B*T][C]:
//   fwd:  out = residual + keep[b] * ((gamma[c] * branch) / keep_prob), every operation rounded to fp32 (contraction
//         is switched off in these kernels), rows of a dropped sample copied from residual, branch not read.
//   bwd:  g = keep[b] * (dy / keep_prob), dbranch = gamma[c] * g, dgamma[c] = sum_rows branch * g through one slab per
//         workgroup and the same fixed-order reduce.
#include "common.h"

int passl_slab_reduce_launch(const float* ws, float* out, int64_t n, int slabs, int accumulate,
                             hipStream_t st);   // flat.hip

namespace {

constexpr int kTW = 16;                  // output columns of a tile
constexpr int kCC = 32;                  // channels of a tile
constexpr int kHaloW = kTW + 6;          // staged pixels per row
constexpr int kPitch = (kHaloW + 1) * kCC;   // elements per staged row (one pad pixel: see the header comment)
constexpr int kWgradTH = PASSL_DWCONV7_WGRAD_TILE_H;
constexpr int kWgradThreads = 256;

template <typename T> struct ConvGeo {
  static constexpr int TH = sizeof(T) == 2 ? 16 : 8;
  static constexpr int THREADS = 8 * 2 * TH;
  static constexpr int WAVES = sizeof(T) == 2 ? 4 : 2;   // per SIMD: the workgroups per CU the LDS image allows
};

// 4 consecutive channels from LDS as floats
__device__ __forceinline__ void lds4(const float* p, float (&v)[4]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void lds4(const bf16_t* p, float (&v)[4]) {
  const uint2 a = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xffff0000u);
  v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xffff0000u);
}
__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) { lds4(p, v); }
__device__ __forceinline__ void ld4(const bf16_t* p, float (&v)[4]) { lds4(p, v); }
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st4(bf16_t* p, const float (&v)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
}

// rows x kHaloW (or kTW) pixels x 32 channels of src around (h0, w0) -> LDS, zero where the image or C ends.
// PX pixels per row are staged at `pitch` elements per row.
template <typename T, int PX, int NT>
__device__ __forceinline__ void stage_tile(T* __restrict__ lds, const T* __restrict__ src, int64_t img, int h0, int w0,
                                           int c0, int rows, int pitch, int H, int W, int C) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int CPP = kCC / VEC;                       // 16-byte chunks per pixel
  constexpr int U = 4;                                 // loads a lane has in flight before its first LDS write
  const int total = rows * PX * CPP;
  for (int base = threadIdx.x; base < total; base += NT * U) {
    uint4 v[U];
    int dst[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * NT;
      const int sub = i % CPP, t = i / CPP;
      const int px = t % PX, row = t / PX;
      const int gh = h0 + row, gw = w0 + px, c = c0 + sub * VEC;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      dst[u] = i < total ? row * pitch + px * kCC + sub * VEC : -1;
      if (i < total && gh >= 0 && gh < H && gw >= 0 && gw < W && c < C)
        v[u] = *reinterpret_cast<const uint4*>(src + ((img * H + gh) * W + gw) * C + c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (dst[u] >= 0) *reinterpret_cast<uint4*>(lds + dst[u]) = v[u];
    }
  }
}

// Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own; neighbouring tiles share their halo
// pixels and the two channel chunks of a 128-byte line share that line.  This renumbering (a bijection on [0, n)) hands
// each XCD a contiguous run of tiles, so those shared bytes are fetched into one L2, once.  Speed only: any placement
// computes the same result.
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int q = n >> 3;
  return b < (q << 3) ? (b & 7) * q + (b >> 3) : b;
}

// where channel ch of tap k lies in the staged filter: a group of 4 channels stays contiguous and 16-byte aligned
__device__ __forceinline__ int wl_at(int k, int ch) { return k * kCC + ((ch + 4 * k) & (kCC - 1)); }

// block -> (image, tile row, tile column, channel chunk); the channel chunk runs fastest
template <typename T, bool BWD>
__global__ void __launch_bounds__(ConvGeo<T>::THREADS, ConvGeo<T>::WAVES) dwconv7_kernel(const T* __restrict__ x,
                                                                      const float* __restrict__ w,
                                                                      const float* __restrict__ bias,
                                                                      const T* __restrict__ add, T* __restrict__ y,
                                                                      int H, int W, int C, int tilesH, int tilesW,
                                                                      int cchunks) {
  constexpr int TH = ConvGeo<T>::TH, NT = ConvGeo<T>::THREADS;
  __shared__ __attribute__((aligned(16))) T tile[(TH + 6) * kPitch];
  __shared__ __attribute__((aligned(16))) float wl[49 * kCC];

  int b = xcd_contiguous(blockIdx.x, gridDim.x);
  const int cc = b % cchunks; b /= cchunks;
  const int tw = b % tilesW; b /= tilesW;
  const int th = b % tilesH;
  const int64_t img = b / tilesH;
  const int h0 = th * TH, w0 = tw * kTW, c0 = cc * kCC;

  // [C][49] as it lies -> [tap][channel], reversed for BWD.  Consecutive lanes hold consecutive taps of one channel:
  // tap k's row is rotated by 4 k channels (wl_at), which spreads their writes over 8 banks instead of one
  for (int i = threadIdx.x; i < 49 * kCC; i += NT) {
    const int ch = i / 49, k = i - ch * 49;
    wl[wl_at(BWD ? 48 - k : k, ch)] = (c0 + ch < C) ? w[(int64_t)(c0 + ch) * 49 + k] : 0.0f;
  }
  stage_tile<T, kHaloW, NT>(tile, x, img, h0 - 3, w0 - 3, c0, TH + 6, kPitch, H, W, C);
  __syncthreads();

  const int cg = threadIdx.x & 7;
  const int row = (threadIdx.x >> 3) % TH;
  const int strip = threadIdx.x / (8 * TH);
  // a wave is 8 rows of one strip: where the image ends inside the tile, the waves wholly outside it leave (56 = 7 x 8:
  // no wave of a 56 x 56 image computes a dead output; of a 7 x 7 image one wave of the four works)
  if (h0 + (row & ~7) >= H || w0 + strip * 8 >= W) return;
  float acc[8][4];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] = 0.0f;
  }
  const T* xrow = tile + row * kPitch + strip * 8 * kCC + cg * 4;
#pragma unroll 1
  for (int r = 0; r < 7; ++r) {
    float wv[7][4];
#pragma unroll
    for (int s = 0; s < 7; ++s) lds4(wl + wl_at(r * 7 + s, cg * 4), wv[s]);
#pragma unroll
    for (int j = 0; j < 14; ++j) {
      float xv[4];
      lds4(xrow + r * kPitch + j * kCC, xv);
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const int o = j - s;
        if (o >= 0 && o < 8) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[o][e] = fmaf(xv[e], wv[s][e], acc[o][e]);
        }
      }
    }
  }

  const int gh = h0 + row, c = c0 + cg * 4;
  if (gh >= H || c >= C) return;
  float extra[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!BWD) lds4(bias + c, extra);
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int gw = w0 + strip * 8 + o;
    if (gw >= W) break;
    const int64_t off = ((img * H + gh) * W + gw) * C + c;
    if (BWD && add) ld4(add + off, extra);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] += extra[e];
    st4(y + off, acc[o]);
  }
}

// workgroup (slab z, channel chunk cc): tiles z, z + slabs, ...
template <typename T>
__global__ void __launch_bounds__(kWgradThreads) dwconv7_wgrad_kernel(const T* __restrict__ x,
                                                                      const T* __restrict__ dy,
                                                                      float* __restrict__ ws_dw,
                                                                      float* __restrict__ ws_db, int H, int W, int C,
                                                                      int tilesH, int tilesW, int tiles, int slabs,
                                                                      int cchunks) {
  constexpr int TH = kWgradTH, NT = kWgradThreads;
  constexpr int XT_BYTES = (TH + 6) * kPitch * (int)sizeof(T);
  constexpr int RED_BYTES = 4 * 50 * kCC * 4;
  constexpr int BUF_BYTES = XT_BYTES > RED_BYTES ? XT_BYTES : RED_BYTES;
  __shared__ __attribute__((aligned(16))) char buf[BUF_BYTES];        // x tile, then the four waves' sums
  __shared__ __attribute__((aligned(16))) T dt[TH * kTW * kCC];
  T* xt = reinterpret_cast<T*>(buf);
  float* red = reinterpret_cast<float*>(buf);

  const int bid = xcd_contiguous(blockIdx.x, gridDim.x);
  const int cc = bid % cchunks, z = bid / cchunks;
  const int c0 = cc * kCC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cg = lane & 7, r = lane >> 3;                // r == 7: the bias gradient's lanes
  const int rr = r < 7 ? r : 6;

  float acc[7][4], db[4];
#pragma unroll
  for (int s = 0; s < 7; ++s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[s][e] = 0.0f;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) db[e] = 0.0f;

  for (int t = z; t < tiles; t += slabs) {
    const int tw = t % tilesW, u = t / tilesW;
    const int th = u % tilesH;
    const int64_t img = u / tilesH;
    const int h0 = th * TH, w0 = tw * kTW;
    __syncthreads();                                     // the previous tile's readers are done
    stage_tile<T, kHaloW, NT>(xt, x, img, h0 - 3, w0 - 3, c0, TH + 6, kPitch, H, W, C);
    stage_tile<T, kTW, NT>(dt, dy, img, h0, w0, c0, TH, kTW * kCC, H, W, C);
    __syncthreads();
#pragma unroll 1
    for (int pp = 0; pp < TH / 4; ++pp) {
      const int p = wave * (TH / 4) + pp;
      if (h0 + p >= H) break;                            // dy is zero below the image
#pragma unroll 1
      for (int half = 0; half < kTW / 8; ++half) {       // 8 columns at a time: 14 x pixels live, not 22
        if (w0 + half * 8 >= W) break;                   // dy is zero right of the image
        const T* xrow = xt + (p + rr) * kPitch + half * 8 * kCC + cg * 4;
        const T* drow = dt + (p * kTW + half * 8) * kCC + cg * 4;
        float xs[14][4];
#pragma unroll
        for (int j = 0; j < 6; ++j) lds4(xrow + j * kCC, xs[j]);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float dv[4];
          lds4(xrow + (q + 6) * kCC, xs[q + 6]);
          lds4(drow + q * kCC, dv);
#pragma unroll
          for (int s = 0; s < 7; ++s) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[s][e] = fmaf(dv[e], xs[q + s][e], acc[s][e]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) db[e] += dv[e];
        }
      }
    }
  }

  __syncthreads();                                       // buf changes hands: x tile -> sums
  float* mine = red + wave * 50 * kCC;
  if (r < 7) {
#pragma unroll
    for (int s = 0; s < 7; ++s) st4(mine + (r * 7 + s) * kCC + cg * 4, acc[s]);
  } else {
    st4(mine + 49 * kCC + cg * 4, db);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 50 * kCC; i += NT) {
    const int k = i / kCC, c = c0 + i % kCC;
    if (c >= C) continue;
    const float v = ((red[i] + red[50 * kCC + i]) + red[2 * 50 * kCC + i]) + red[3 * 50 * kCC + i];
    if (k < 49) ws_dw[((int64_t)z * C + c) * 49 + k] = v;
    else ws_db[(int64_t)z * C + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------- layer scale
constexpr int kThreads = 256;
constexpr int kU = 4;

// chunk = 8 elements; per = chunks of one sample (T * C/8); tiles = workgroups per sample; cols = C/8
template <typename T, bool TABLE>
__global__ void __launch_bounds__(kThreads) layer_scale_add_kernel(const T* __restrict__ branch,
                                                                   const T* __restrict__ res,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ keep, float keep_prob,
                                                                   T* __restrict__ out, int per, int tiles, int cols) {
#pragma clang fp contract(off)
  const int b = blockIdx.x / tiles;
  const int first = (blockIdx.x - b * tiles) * (kThreads * kU) + threadIdx.x;
  const int64_t off = (int64_t)b * per;
  const float kb = TABLE ? keep[b] : 1.0f;            // uniform over the workgroup
  float r[kU][8];
#pragma unroll
  for (int u = 0; u < kU; ++u) {                      // branch-free: a lane past the end re-reads the last chunk
    const int i = first + u * kThreads;
    ElemTraits<T>::load8(res + (off + (i < per ? i : per - 1)) * 8, r[u]);
  }
  if (kb != 0.0f) {
    float v[kU][8], g[kU][8];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int i = first + u * kThreads;
      const int ii = i < per ? i : per - 1;
      ElemTraits<T>::load8(branch + (off + ii) * 8, v[u]);
      ElemTraits<float>::load8(gamma + (ii % cols) * 8, g[u]);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = g[u][e] * v[u][e];
        if (TABLE) {
          t = t / keep_prob;                          // IEEE division (no fast-math in the build)
          t = t * kb;
        }
        r[u][e] = r[u][e] + t;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int i = first + u * kThreads;
    if (i >= per) break;
    ElemTraits<T>::store8(out + (off + i) * 8, r[u]);
  }
}

// workgroup z owns rows [z * rows_per, min(M, (z + 1) * rows_per)); a thread owns one 8-channel column (cols <= 256:
// kThreads / cols row lanes share the rows) or every 256th column
template <typename T, bool TABLE>
__global__ void __launch_bounds__(kThreads) layer_scale_add_bwd_kernel(const T* __restrict__ dy,
                                                                       const T* __restrict__ branch,
                                                                       const float* __restrict__ gamma,
                                                                       const float* __restrict__ keep,
                                                                       float keep_prob, T* __restrict__ dbranch,
                                                                       float* __restrict__ ws, int64_t M, int Trows,
                                                                       int cols, int rows_per) {
  extern __shared__ float sums[];                     // [row lanes][cols * 8]
  const int z = blockIdx.x;
  const int64_t r0 = (int64_t)z * rows_per;
  const int64_t r1 = r0 + rows_per < M ? r0 + rows_per : M;
  const int RL = cols >= kThreads ? 1 : kThreads / cols;
  const int rl = cols >= kThreads ? 0 : threadIdx.x / cols;
  const int cfirst = cols >= kThreads ? threadIdx.x : threadIdx.x % cols;
  const int cstep = cols >= kThreads ? kThreads : cols;
  const bool active = rl < RL;
  const int64_t C8 = (int64_t)cols * 8;
  if (active) {
    for (int col = cfirst; col < cols; col += cstep) {
      float gm[8], acc[8];
      ElemTraits<float>::load8(gamma + col * 8, gm);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
      for (int64_t row = r0 + rl; row < r1; row += RL) {
        const float kb = TABLE ? keep[row / Trows] : 1.0f;
        float g[8], d[8];
        if (kb != 0.0f) {
          float v[8];
          ElemTraits<T>::load8(dy + row * C8 + col * 8, g);
          ElemTraits<T>::load8(branch + row * C8 + col * 8, v);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if (TABLE) g[e] = kb * (g[e] / keep_prob);
            d[e] = gm[e] * g[e];
            acc[e] = fmaf(v[e], g[e], acc[e]);
          }
        } else {                                        // a dropped sample: zeros, dy and branch not read
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = 0.0f;
        }
        ElemTraits<T>::store8(dbranch + row * C8 + col * 8, d);
      }
      ElemTraits<float>::store8(sums + rl * C8 + col * 8, acc);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C8; i += kThreads) {
    float v = sums[i];
    for (int l = 1; l < RL; ++l) v += sums[l * C8 + i];
    ws[(int64_t)z * C8 + i] = v;
  }
}

// shape checks of the three 7x7 entry points: -> tile counts, or a status
static int conv_geometry(int N, int H, int W, int C, int dtype, int th, int* tilesH, int* tilesW, int64_t* tiles) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return PASSL_EINVAL;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  *tilesH = (H + th - 1) / th;
  *tilesW = (W + kTW - 1) / kTW;
  *tiles = (int64_t)N * *tilesH * *tilesW;
  const int64_t cchunks = (C + kCC - 1) / kCC;
  if (*tiles * cchunks > 0x7fffffffll || (int64_t)H * W > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

template <bool BWD>
static int launch_conv(const void* x, const float* w, const float* bias, const void* add, void* y, int N, int H, int W,
                       int C, int dtype, passl_stream_t stream) {
  int tilesH = 0, tilesW = 0;
  int64_t tiles = 0;
  const int th = dtype == PASSL_BF16 ? ConvGeo<bf16_t>::TH : ConvGeo<float>::TH;
  const int rc = conv_geometry(N, H, W, C, dtype, th, &tilesH, &tilesW, &tiles);
  if (rc != PASSL_OK) return rc;
  const int cchunks = (C + kCC - 1) / kCC;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((dwconv7_kernel<T, BWD>), dim3((unsigned)(tiles * cchunks)),
                                                 dim3(ConvGeo<T>::THREADS), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(x), w, bias, reinterpret_cast<const T*>(add),
                                                 reinterpret_cast<T*>(y), H, W, C, tilesH, tilesW, cchunks);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

// shape checks shared by layer_scale_add fwd / bwd
static int rows_geometry(int B, int T, int C, const float* keep, float keep_prob) {
  if (B <= 0 || T <= 0 || C <= 0 || (C & 7)) return PASSL_EINVAL;
  if (keep && !(keep_prob > 0.0f && keep_prob <= 1.0f)) return PASSL_EINVAL;
  return PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_dwconv7_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W,
                                     int C, int dtype, passl_stream_t stream) {
  if (!x || !w || !bias || !y || !aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y))
    return PASSL_EINVAL;
  return launch_conv<false>(x, w, bias, nullptr, y, N, H, W, C, dtype, stream);
}

extern "C" int passl_hip_dwconv7_bwd_data(const void* dy, const float* w, const void* add, void* dx, int N, int H,
                                          int W, int C, int dtype, passl_stream_t stream) {
  if (!dy || !w || !dx || !aligned16(dy) || !aligned16(w) || !aligned16(add) || !aligned16(dx)) return PASSL_EINVAL;
  return launch_conv<true>(dy, w, nullptr, add, dx, N, H, W, C, dtype, stream);
}

extern "C" int passl_hip_dwconv7_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, float* ws,
                                            int64_t ws_floats, int N, int H, int W, int C, int dtype,
                                            passl_stream_t stream) {
  if (!x || !dy || !dw || !dbias || !ws || !aligned16(x) || !aligned16(dy) || !aligned16(dw) || !aligned16(dbias) ||
      !aligned16(ws))
    return PASSL_EINVAL;
  int tilesH = 0, tilesW = 0;
  int64_t tiles = 0;
  const int rc = conv_geometry(N, H, W, C, dtype, kWgradTH, &tilesH, &tilesW, &tiles);
  if (rc != PASSL_OK) return rc;
  const int slabs = (int)(tiles < PASSL_DWCONV7_WGRAD_MAX_SLABS ? tiles : PASSL_DWCONV7_WGRAD_MAX_SLABS);
  if (ws_floats < (int64_t)slabs * 50 * C) return PASSL_EINVAL;
  const int cchunks = (C + kCC - 1) / kCC;
  float* ws_db = ws + (int64_t)slabs * 49 * C;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(dwconv7_wgrad_kernel<T>, dim3((unsigned)(slabs * cchunks)),
                                                 dim3(kWgradThreads), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(dy), ws,
                                                 ws_db, H, W, C, tilesH, tilesW, (int)tiles, slabs, cchunks);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  int rc2 = passl_slab_reduce_launch(ws, dw, (int64_t)49 * C, slabs, 0, as_stream(stream));
  if (rc2 == PASSL_OK) rc2 = passl_slab_reduce_launch(ws_db, dbias, C, slabs, 0, as_stream(stream));
  return rc2;
}

extern "C" int passl_hip_layer_scale_add_fwd(const void* branch, const void* residual, const float* gamma,
                                             const float* keep, float keep_prob, void* out, int B, int T, int C,
                                             int dtype, passl_stream_t stream) {
  if (!branch || !residual || !gamma || !out || !aligned16(branch) || !aligned16(residual) || !aligned16(gamma) ||
      !aligned16(out))
    return PASSL_EINVAL;
  const int rc = rows_geometry(B, T, C, keep, keep_prob);
  if (rc != PASSL_OK) return rc;
  const int64_t p = (int64_t)T * (C >> 3);
  const int64_t t = (p + kThreads * kU - 1) / (kThreads * kU);
  if (p > 0x7fffffffll - kThreads * kU || t * B > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const int per = (int)p, tiles = (int)t, cols = C >> 3;
  if (keep) {
    PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((layer_scale_add_kernel<T, true>), dim3((unsigned)(tiles * B)),
                                                   dim3(kThreads), 0, as_stream(stream),
                                                   reinterpret_cast<const T*>(branch),
                                                   reinterpret_cast<const T*>(residual), gamma, keep, keep_prob,
                                                   reinterpret_cast<T*>(out), per, tiles, cols);)
  } else {
    PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((layer_scale_add_kernel<T, false>), dim3((unsigned)(tiles * B)),
                                                   dim3(kThreads), 0, as_stream(stream),
                                                   reinterpret_cast<const T*>(branch),
                                                   reinterpret_cast<const T*>(residual), gamma, keep, 1.0f,
                                                   reinterpret_cast<T*>(out), per, tiles, cols);)
  }
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_layer_scale_add_bwd(const void* dy, const void* branch, const float* gamma, const float* keep,
                                             float keep_prob, void* dbranch, float* dgamma, float* ws,
                                             int64_t ws_floats, int B, int T, int C, int dtype,
                                             passl_stream_t stream) {
  if (!dy || !branch || !gamma || !dbranch || !dgamma || !ws || !aligned16(dy) || !aligned16(branch) ||
      !aligned16(gamma) || !aligned16(dbranch) || !aligned16(dgamma) || !aligned16(ws))
    return PASSL_EINVAL;
  const int rc = rows_geometry(B, T, C, keep, keep_prob);
  if (rc != PASSL_OK) return rc;
  if (C > PASSL_LAYER_SCALE_MAX_C) return PASSL_EUNSUPPORTED;        // the workgroup's column sums live in LDS
  const int trows = T;                                 // T names the element type inside the dispatch
  const int64_t M = (int64_t)B * trows;
  const int64_t rows_per = (M + PASSL_LAYER_SCALE_MAX_SLABS - 1) / PASSL_LAYER_SCALE_MAX_SLABS;
  if (rows_per > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const int slabs = (int)((M + rows_per - 1) / rows_per);
  if (ws_floats < (int64_t)slabs * C) return PASSL_EINVAL;
  const int cols = C >> 3;
  const int RL = cols >= kThreads ? 1 : kThreads / cols;
  const size_t lds = (size_t)RL * C * sizeof(float);
  if (keep) {
    PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((layer_scale_add_bwd_kernel<T, true>), dim3((unsigned)slabs),
                                                   dim3(kThreads), lds, as_stream(stream),
                                                   reinterpret_cast<const T*>(dy), reinterpret_cast<const T*>(branch),
                                                   gamma, keep, keep_prob, reinterpret_cast<T*>(dbranch), ws, M,
                                                   trows, cols, (int)rows_per);)
  } else {
    PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((layer_scale_add_bwd_kernel<T, false>), dim3((unsigned)slabs),
                                                   dim3(kThreads), lds, as_stream(stream),
                                                   reinterpret_cast<const T*>(dy), reinterpret_cast<const T*>(branch),
                                                   gamma, keep, 1.0f, reinterpret_cast<T*>(dbranch), ws, M, trows,
                                                   cols, (int)rows_per);)
  }
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return passl_slab_reduce_launch(ws, dgamma, C, slabs, 0, as_stream(stream));
}
