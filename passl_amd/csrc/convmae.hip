// ConvMAE's operators that no other unit covers (reference: passl/models/convmae/conv_vit.py, class CBlock :82-99, and
// conv_mae.py, forward_encoder :249-266): the depthwise 5x5 convolution of a CBlock, whose input is multiplied by the
// patch mask, the gather of the kept patches in front of the stage decoders, and the token kernels of a MAE without a
// class row.  Activations are NHWC [N, H, W, C] in `dtype`, parameters and their gradients fp32.
//
// The mask is the float table [N, Hm * Wm] that passl_hip_mae_mask writes (1 = removed).  With g = H / Hm = W / Wm the
// keep factor of pixel (h, w) is 1 - mask[n, (h / g) * Wm + w / g]: expanding the table to the map is address
// arithmetic.  A workgroup first writes the factors of the (TH + 4) x 20 pixels around its tile into LDS (one or two
// integer divisions per thread), so neither the staging loop nor the store loop divides.
//
// Masked depthwise 5x5, forward and data gradient (ONE kernel, as the 7x7 of dwconv.hip: the data gradient is the
// forward with the filter read reversed):
//   a workgroup owns TH x 16 output pixels x 32 channels.  It stages the (TH + 4) x 20 input pixels of those channels
//   once in LDS, in the storage type, and the 25 x 32 filter taps as fp32 [tap][channel].  The forward multiplies a
//   pixel by its keep factor while it goes into LDS: once per staged pixel, not once per tap; a removed pixel is not
//   loaded at all.  A factor of exactly 1 or 0 (all that passl_hip_mae_mask writes) leaves the value or a zero, so the
//   staged tile holds the exact products; any other factor is applied in fp32 and, for bf16, rounded once more when it
//   is staged.  The data gradient stages dy as it lies and applies the factor of the OUTPUT pixel to the fp32 sum
//   before the single rounding (a removed pixel stores +0).
//   A lane owns one output row, 8 consecutive output columns and 4 channels: per filter row it reads the 12 input
//   pixels under its 8 outputs once and slides the 5 taps over them, so every value read feeds up to five FMAs.
//   32 fp32 accumulators, one rounding at the store.  TH = 16 (256 threads) for bf16 and 8 (128 threads) for fp32.
//   LDS pitch.  A pixel is 32 channels = 32 dwords (fp32) or 16 dwords (bf16); a wave is 8 channel groups x 8 rows and
//   all its lanes read the same pixel column, so the bank of a lane is (row * pitch + 4 cg) mod 64 (fp32) or
//   (row * pitch + 2 cg) mod 64 (bf16).  ds_read_b128 (fp32) is served in groups of 16 lanes, each of which is four
//   half-rows of 16 dwords from four different rows; the four land on disjoint banks iff pitch = 32 (mod 64), that is
//   iff the row holds an ODD number of pixels.  ds_read_b64 (bf16) is served in groups of 32 lanes = four whole rows of
//   16 dwords; they are disjoint iff pitch = 16 or 48 (mod 64), again an odd number of pixels.  The 7x7 tile had
//   22 + 1 pixels per row (pitch 32 / 48 mod 64); the 4-pixel halo gives 20, an even number (pitch 0 / 0 mod 64: a
//   4-way conflict), so one pad pixel is still needed: 21 pixels, pitch 672 = 32 (mod 64) dwords for fp32 and
//   336 = 16 (mod 64) for bf16.
//   LDS per workgroup: bf16 20 x 21 x 64 B + 3.1 KiB taps + 1.6 KiB factors = 31 KiB (four workgroups of 256 threads
//   per CU: 4 waves per SIMD); fp32 12 x 21 x 128 B + 3.1 + 0.9 KiB = 35.5 KiB (four workgroups of 128 threads).
// Weight and bias gradient: the same tile geometry (TH = 8) with the dy tile next to the masked x tile.  A lane owns
//   4 channels and ONE filter row r (lanes r == 5 own the bias gradient, lanes r >= 6 have no sum: a wave's eight row
//   lanes are fixed by the tile, the 5x5 filter fills six of them): 20 accumulators, kept over every tile the
//   workgroup visits.  The four waves split the tile's rows, are added in wave order through LDS, and the workgroup
//   writes one slab of the caller's workspace; slab_reduce_kernel (flat.hip) adds the slabs in ascending order.
//   No floating-point atomics anywhere: two launches give the same bits.
//
// Kept-patch gather: the rows [B * K][p * p * C] of the kept patches in the column order (ph, pw, c) of PatchConv2D's
//   packed weight, and its backward, which writes every pixel of dx (a pixel belongs to exactly one patch).
// Tokens without a class row: out[b, k] = x[b, k] + pos[ids_keep[b, k]] and its pos gradient (images added in
//   ascending order), the decoder's unshuffle and its backward (mask-token gradient through slabs), the masked-patch
//   loss on pred [B, L, P] (the kernels of vit.hip, which skip a class row, restated without one).
#include "common.h"

int passl_slab_reduce_launch(const float* ws, float* out, int64_t n, int slabs, int accumulate,
                             hipStream_t st);   // flat.hip

namespace {

constexpr int kTW = 16;                  // output columns of a tile
constexpr int kCC = 32;                  // channels of a tile
constexpr int kR = 5;                    // filter rows and columns
constexpr int kTaps = kR * kR;
constexpr int kHalo = kR / 2;
constexpr int kHaloW = kTW + 2 * kHalo;  // staged pixels per row
constexpr int kPitch = (kHaloW + 1) * kCC;   // elements per staged row (one pad pixel: see the header comment)
constexpr int kWin = 8 + 2 * kHalo;      // input pixels under a lane's 8 outputs
constexpr int kWgradTH = PASSL_DWCONV5_WGRAD_TILE_H;
constexpr int kWgradThreads = 256;
constexpr int kSums = kTaps + 1;         // per channel: 25 taps and the bias

template <typename T> struct ConvGeo {
  static constexpr int TH = sizeof(T) == 2 ? 16 : 8;
  static constexpr int THREADS = 8 * 2 * TH;
  static constexpr int WAVES = sizeof(T) == 2 ? 4 : 2;   // per SIMD: four workgroups per CU
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
__device__ __forceinline__ void st4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void st4(bf16_t* p, const float (&v)[4]) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
}

// 16 bytes of T times a keep factor that is neither 0 nor 1 (fp32 product, rounded to T)
template <typename T> __device__ __forceinline__ uint4 scale16(uint4 v, float k);
template <> __device__ __forceinline__ uint4 scale16<float>(uint4 v, float k) {
  return make_uint4(__float_as_uint(__uint_as_float(v.x) * k), __float_as_uint(__uint_as_float(v.y) * k),
                    __float_as_uint(__uint_as_float(v.z) * k), __float_as_uint(__uint_as_float(v.w) * k));
}
__device__ __forceinline__ uint32_t scale2bf(uint32_t a, float k) {
  return pack2bf(__uint_as_float(a << 16) * k, __uint_as_float(a & 0xffff0000u) * k);
}
template <> __device__ __forceinline__ uint4 scale16<bf16_t>(uint4 v, float k) {
  return make_uint4(scale2bf(v.x, k), scale2bf(v.y, k), scale2bf(v.z, k), scale2bf(v.w, k));
}

// the mask table and how the map lies over it
struct MaskGeo {
  const float* mask;   // [N][Lm], 1 = removed; NULL: no mask
  int g, Wm, Lm;
};

// keep factors of rows x kHaloW pixels around (h0, w0) -> LDS; 0 outside the image
template <int NT>
__device__ __forceinline__ void fill_keep(float* __restrict__ kp, const MaskGeo m, int64_t img, int h0, int w0, int rows,
                                          int H, int W) {
  for (int i = threadIdx.x; i < rows * kHaloW; i += NT) {
    const int row = i / kHaloW, px = i - row * kHaloW;
    const int gh = h0 + row, gw = w0 + px;
    float k = 0.0f;
    if (gh >= 0 && gh < H && gw >= 0 && gw < W) k = 1.0f - m.mask[img * m.Lm + (gh / m.g) * m.Wm + gw / m.g];
    kp[i] = k;
  }
}

// rows x PX pixels x 32 channels of src around (h0, w0) -> LDS at `pitch` elements per row, zero where the image or C
// ends.  kp (LDS, [rows][PX], or NULL): the pixels' keep factors; a pixel whose factor is 0 is not loaded.
template <typename T, int PX, int NT>
__device__ __forceinline__ void stage_tile(T* __restrict__ lds, const T* __restrict__ src, const float* __restrict__ kp,
                                           int64_t img, int h0, int w0, int c0, int rows, int pitch, int H, int W,
                                           int C) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int CPP = kCC / VEC;                       // 16-byte chunks per pixel
  constexpr int U = 4;                                 // loads a lane has in flight before its first LDS write
  const int total = rows * PX * CPP;
  for (int base = threadIdx.x; base < total; base += NT * U) {
    uint4 v[U];
    float kf[U];
    int dst[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * NT;
      const int sub = i % CPP, t = i / CPP;
      const int px = t % PX, row = t / PX;
      const int gh = h0 + row, gw = w0 + px, c = c0 + sub * VEC;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      kf[u] = 1.0f;
      dst[u] = i < total ? row * pitch + px * kCC + sub * VEC : -1;
      if (i < total && gh >= 0 && gh < H && gw >= 0 && gw < W && c < C) {
        const float k = kp ? kp[row * PX + px] : 1.0f;
        if (k != 0.0f) {
          v[u] = *reinterpret_cast<const uint4*>(src + ((img * H + gh) * W + gw) * C + c);
          kf[u] = k;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (dst[u] >= 0) *reinterpret_cast<uint4*>(lds + dst[u]) = kf[u] == 1.0f ? v[u] : scale16<T>(v[u], kf[u]);
    }
  }
}

// Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own; this renumbering (a bijection on
// [0, n)) hands each XCD a contiguous run of tiles, so the halo pixels neighbours share are fetched into one L2.
// Speed only: any placement computes the same result.
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int q = n >> 3;
  return b < (q << 3) ? (b & 7) * q + (b >> 3) : b;
}

// where channel ch of tap k lies in the staged filter: a group of 4 channels stays contiguous and 16-byte aligned
__device__ __forceinline__ int wl_at(int k, int ch) { return k * kCC + ((ch + 4 * k) & (kCC - 1)); }

// block -> (image, tile row, tile column, channel chunk); the channel chunk runs fastest
template <typename T, bool BWD>
__global__ void __launch_bounds__(ConvGeo<T>::THREADS, ConvGeo<T>::WAVES) dwconv5_masked_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, const MaskGeo m,
    T* __restrict__ y, int H, int W, int C, int tilesH, int tilesW, int cchunks) {
  constexpr int TH = ConvGeo<T>::TH, NT = ConvGeo<T>::THREADS;
  __shared__ __attribute__((aligned(16))) T tile[(TH + 2 * kHalo) * kPitch];
  __shared__ __attribute__((aligned(16))) float wl[kTaps * kCC];
  __shared__ float kp[(TH + 2 * kHalo) * kHaloW];

  int b = xcd_contiguous(blockIdx.x, gridDim.x);
  const int cc = b % cchunks; b /= cchunks;
  const int tw = b % tilesW; b /= tilesW;
  const int th = b % tilesH;
  const int64_t img = b / tilesH;
  const int h0 = th * TH, w0 = tw * kTW, c0 = cc * kCC;
  const bool masked = m.mask != nullptr;               // uniform over the grid

  // [C][25] as it lies -> [tap][channel], reversed for BWD (the rotation of wl_at spreads the writes over 8 banks)
  for (int i = threadIdx.x; i < kTaps * kCC; i += NT) {
    const int ch = i / kTaps, k = i - ch * kTaps;
    wl[wl_at(BWD ? kTaps - 1 - k : k, ch)] = (c0 + ch < C) ? w[(int64_t)(c0 + ch) * kTaps + k] : 0.0f;
  }
  if (masked) {
    fill_keep<NT>(kp, m, img, h0 - kHalo, w0 - kHalo, TH + 2 * kHalo, H, W);
    if (!BWD) __syncthreads();                         // the staging below reads the factors
  }
  stage_tile<T, kHaloW, NT>(tile, x, (masked && !BWD) ? kp : nullptr, img, h0 - kHalo, w0 - kHalo, c0, TH + 2 * kHalo,
                            kPitch, H, W, C);
  __syncthreads();

  const int cg = threadIdx.x & 7;
  const int row = (threadIdx.x >> 3) % TH;
  const int strip = threadIdx.x / (8 * TH);
  // a wave is 8 rows of one strip: where the image ends inside the tile, the waves wholly outside it leave
  if (h0 + (row & ~7) >= H || w0 + strip * 8 >= W) return;
  float acc[8][4];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] = 0.0f;
  }
  const T* xrow = tile + row * kPitch + strip * 8 * kCC + cg * 4;
#pragma unroll 1
  for (int r = 0; r < kR; ++r) {
    float wv[kR][4];
#pragma unroll
    for (int s = 0; s < kR; ++s) lds4(wl + wl_at(r * kR + s, cg * 4), wv[s]);
#pragma unroll
    for (int j = 0; j < kWin; ++j) {
      float xv[4];
      lds4(xrow + r * kPitch + j * kCC, xv);
#pragma unroll
      for (int s = 0; s < kR; ++s) {
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
    if (BWD) {
      if (masked) {
        const float k = kp[(row + kHalo) * kHaloW + strip * 8 + o + kHalo];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[o][e] = k == 0.0f ? 0.0f : (k == 1.0f ? acc[o][e] : acc[o][e] * k);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[o][e] += extra[e];
    }
    st4(y + off, acc[o]);
  }
}

// workgroup (slab z, channel chunk cc): tiles z, z + slabs, ...
template <typename T>
__global__ void __launch_bounds__(kWgradThreads) dwconv5_masked_wgrad_kernel(
    const T* __restrict__ x, const T* __restrict__ dy, const MaskGeo m, float* __restrict__ ws_dw,
    float* __restrict__ ws_db, int H, int W, int C, int tilesH, int tilesW, int tiles, int slabs, int cchunks) {
  constexpr int TH = kWgradTH, NT = kWgradThreads;
  constexpr int XT_BYTES = (TH + 2 * kHalo) * kPitch * (int)sizeof(T);
  constexpr int RED_BYTES = 4 * kSums * kCC * 4;
  constexpr int BUF_BYTES = XT_BYTES > RED_BYTES ? XT_BYTES : RED_BYTES;
  __shared__ __attribute__((aligned(16))) char buf[BUF_BYTES];        // x tile, then the four waves' sums
  __shared__ __attribute__((aligned(16))) T dt[TH * kTW * kCC];
  __shared__ float kp[(TH + 2 * kHalo) * kHaloW];
  T* xt = reinterpret_cast<T*>(buf);
  float* red = reinterpret_cast<float*>(buf);

  const int bid = xcd_contiguous(blockIdx.x, gridDim.x);
  const int cc = bid % cchunks, z = bid / cchunks;
  const int c0 = cc * kCC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cg = lane & 7, r = lane >> 3;                // r == 5: the bias gradient's lanes; r >= 6: no sum
  const int rr = r < kR ? r : kR - 1;
  const bool masked = m.mask != nullptr;

  float acc[kR][4], db[4];
#pragma unroll
  for (int s = 0; s < kR; ++s) {
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
    if (masked) {
      fill_keep<NT>(kp, m, img, h0 - kHalo, w0 - kHalo, TH + 2 * kHalo, H, W);
      __syncthreads();
    }
    stage_tile<T, kHaloW, NT>(xt, x, masked ? kp : nullptr, img, h0 - kHalo, w0 - kHalo, c0, TH + 2 * kHalo, kPitch, H,
                              W, C);
    stage_tile<T, kTW, NT>(dt, dy, nullptr, img, h0, w0, c0, TH, kTW * kCC, H, W, C);
    __syncthreads();
#pragma unroll 1
    for (int pp = 0; pp < TH / 4; ++pp) {
      const int p = wave * (TH / 4) + pp;
      if (h0 + p >= H) break;                            // dy is zero below the image
#pragma unroll 1
      for (int half = 0; half < kTW / 8; ++half) {       // 8 columns at a time: 12 x pixels live, not 20
        if (w0 + half * 8 >= W) break;                   // dy is zero right of the image
        const T* xrow = xt + (p + rr) * kPitch + half * 8 * kCC + cg * 4;
        const T* drow = dt + (p * kTW + half * 8) * kCC + cg * 4;
        float xs[kWin][4];
#pragma unroll
        for (int j = 0; j < 2 * kHalo; ++j) lds4(xrow + j * kCC, xs[j]);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float dv[4];
          lds4(xrow + (q + 2 * kHalo) * kCC, xs[q + 2 * kHalo]);
          lds4(drow + q * kCC, dv);
#pragma unroll
          for (int s = 0; s < kR; ++s) {
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
  float* mine = red + wave * kSums * kCC;
  if (r < kR) {
#pragma unroll
    for (int s = 0; s < kR; ++s) st4(mine + (r * kR + s) * kCC + cg * 4, acc[s]);
  } else if (r == kR) {
    st4(mine + kTaps * kCC + cg * 4, db);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSums * kCC; i += NT) {
    const int k = i / kCC, c = c0 + i % kCC;
    if (c >= C) continue;
    const float v = ((red[i] + red[kSums * kCC + i]) + red[2 * kSums * kCC + i]) + red[3 * kSums * kCC + i];
    if (k < kTaps) ws_dw[((int64_t)z * C + c) * kTaps + k] = v;
    else ws_db[(int64_t)z * C + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------- kept-patch gather
constexpr int kThreads = 256;

static unsigned grid_for(int64_t items) {
  const int64_t blocks = (items + kThreads - 1) / kThreads;
  return (unsigned)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

// out[b * K + k][(i * p + j) * C + c] = x[b][ph * p + i][pw * p + j][c], (ph, pw) = patch ids_keep[b, k] of the
// Hm x Wm grid.  A work item is one 16-byte chunk; the run (j, c) is contiguous on both sides.  An index outside the
// grid gives a row of zeros.
template <typename T>
__global__ void __launch_bounds__(kThreads) patch_gather_kernel(const T* __restrict__ x,
                                                                const int32_t* __restrict__ ids_keep,
                                                                T* __restrict__ out, int B, int K, int Hm, int Wm, int p,
                                                                int C) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int run = p * C / VEC;                           // chunks of one patch row
  const int64_t total = (int64_t)B * K * p * run;
  const int64_t W = (int64_t)Wm * p;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int q = (int)(i % run);
    const int64_t t = i / run;
    const int pi = (int)(t % p);
    const int64_t rowk = t / p;                          // b * K + k
    const int64_t b = rowk / K;
    const int l = ids_keep[rowk];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (l >= 0 && l < Hm * Wm) {
      const int ph = l / Wm, pw = l - ph * Wm;
      v = *reinterpret_cast<const uint4*>(x + ((b * Hm * p + (int64_t)ph * p + pi) * W + (int64_t)pw * p) * C +
                                          (int64_t)q * VEC);
    }
    *reinterpret_cast<uint4*>(out + i * VEC) = v;
  }
}

// dx[b][h][w][c] = dout[b * K + r][...] with r = ids_restore[b, patch of (h, w)] when r < K, else 0: every chunk of dx
// is written by exactly one work item.
template <typename T>
__global__ void __launch_bounds__(kThreads) patch_gather_bwd_kernel(const T* __restrict__ dout,
                                                                    const int32_t* __restrict__ ids_restore,
                                                                    T* __restrict__ dx, int B, int K, int Hm, int Wm,
                                                                    int p, int C) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int run = p * C / VEC;
  const int64_t total = (int64_t)B * Hm * p * Wm * run;  // dx in its own order: [b][ph][pi][pw][run]
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int q = (int)(i % run);
    int64_t t = i / run;
    const int pw = (int)(t % Wm); t /= Wm;
    const int pi = (int)(t % p); t /= p;
    const int ph = (int)(t % Hm);
    const int64_t b = t / Hm;
    const int r = ids_restore[b * Hm * Wm + ph * Wm + pw];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (r >= 0 && r < K) v = *reinterpret_cast<const uint4*>(dout + (((b * K + r) * p + pi) * run + q) * VEC);
    *reinterpret_cast<uint4*>(dx + i * VEC) = v;
  }
}

// ---------------------------------------------------------------------------------------------- tokens, no class row
// out[b, k] = x[b, k] + pos[ids_keep[b, k]]  (fp32 add, one rounding)
template <typename T>
__global__ void __launch_bounds__(kThreads) pos_gather_add_kernel(const T* __restrict__ x, const float* __restrict__ pos,
                                                                  const int32_t* __restrict__ ids_keep,
                                                                  T* __restrict__ out, int B, int L, int K, int D) {
  const int cpr = D >> 3;
  const int64_t total = (int64_t)B * K * cpr;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % cpr) * 8;
    const int64_t tok = i / cpr;
    float v[8], p[8];
    int l = ids_keep[tok];
    l = l < 0 ? 0 : (l < L ? l : L - 1);
    ElemTraits<T>::load8(x + tok * D + c, v);
    ElemTraits<float>::load8(pos + (int64_t)l * D + c, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    ElemTraits<T>::store8(out + tok * D + c, v);
  }
}

// dpos[l] += sum over the images b = 0, 1, ... (in that order) that kept patch l of dout[b, ids_restore[b, l]]
template <typename T>
__global__ void __launch_bounds__(kThreads) pos_gather_add_bwd_kernel(const T* __restrict__ dout,
                                                                      const int32_t* __restrict__ ids_restore,
                                                                      float* __restrict__ dpos, int B, int L, int K,
                                                                      int D) {
  const int cpr = D >> 3;
  const int64_t total = (int64_t)L * cpr;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % cpr) * 8;
    const int l = (int)(i / cpr);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
      const int r = ids_restore[(int64_t)b * L + l];
      if (r < 0 || r >= K) continue;
      float v[8];
      ElemTraits<T>::load8(dout + ((int64_t)b * K + r) * D + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
    float cur[8];
    ElemTraits<float>::load8(dpos + (int64_t)l * D + c, cur);
#pragma unroll
    for (int e = 0; e < 8; ++e) cur[e] += acc[e];
    ElemTraits<float>::store8(dpos + (int64_t)l * D + c, cur);
  }
}

// decoder input: out[b, l] = ((r = ids_restore[b, l]) < K ? x[b, r] : mask_token) + pos[l]
template <typename T>
__global__ void __launch_bounds__(kThreads) unshuffle_nocls_kernel(const T* __restrict__ x,
                                                                   const float* __restrict__ mask_token,
                                                                   const float* __restrict__ pos,
                                                                   const int32_t* __restrict__ ids_restore,
                                                                   T* __restrict__ out, int B, int L, int K, int D) {
  const int cpr = D >> 3;
  const int64_t total = (int64_t)B * L * cpr;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % cpr) * 8;
    const int64_t tok = i / cpr;
    const int l = (int)(tok % L);
    const int64_t b = tok / L;
    float v[8], p[8];
    const int r = ids_restore[tok];
    if (r >= 0 && r < K) ElemTraits<T>::load8(x + (b * K + r) * D + c, v);
    else ElemTraits<float>::load8(mask_token + c, v);
    ElemTraits<float>::load8(pos + (int64_t)l * D + c, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    ElemTraits<T>::store8(out + tok * D + c, v);
  }
}

// backward: dx[b, k] = dout[b, ids_keep[b, k]]; the mask token's gradient = sum of dout over the removed positions.
// Block = 32 column chunks x 8 position lanes, grid.y = position slabs (as mae_unshuffle_bwd_kernel, vit.hip): a
// thread keeps one column chunk, the eight lanes are added in lane order through LDS, slab blockIdx.y of the
// workspace gets the sum.
template <typename T>
__global__ void __launch_bounds__(kThreads) unshuffle_nocls_bwd_kernel(const T* __restrict__ dout,
                                                                       const int32_t* __restrict__ ids_keep,
                                                                       const int32_t* __restrict__ ids_restore,
                                                                       T* __restrict__ dx, float* __restrict__ ws, int B,
                                                                       int L, int K, int D, int toks_per_block) {
  __shared__ float red[8][32 * 8 + 8];
  const int cc = threadIdx.x & 31, tl = threadIdx.x >> 5;
  const int c = (blockIdx.x * 32 + cc) * 8;
  const int64_t ntok = (int64_t)B * L;
  const int64_t t0 = (int64_t)blockIdx.y * toks_per_block;
  int64_t t1 = t0 + toks_per_block;
  if (t1 > ntok) t1 = ntok;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < D) {
    for (int64_t tok = t0 + tl; tok < t1; tok += 8) {
      const int t = (int)(tok % L);
      const int64_t b = tok / L;
      float v[8];
      if (t < K) {                                       // destination row t of dx
        int src = ids_keep[b * K + t];
        src = src < 0 ? 0 : (src < L ? src : L - 1);
        ElemTraits<T>::load8(dout + (b * L + src) * D + c, v);
        ElemTraits<T>::store8(dx + (b * K + t) * D + c, v);
      }
      const int r = ids_restore[tok];
      if (r < 0 || r >= K) {
        ElemTraits<T>::load8(dout + tok * D + c, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tl][cc * 8 + e] = acc[e];
  __syncthreads();
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col < D) {
    float s = 0.f;
#pragma unroll
    for (int l = 0; l < 8; ++l) s += red[l][threadIdx.x];
    ws[(int64_t)blockIdx.y * D + col] = s;
  }
}

// ---------------------------------------------------------------------------------------------- masked-patch loss
// one wave per patch, as mae_loss_kernel (vit.hip) with no class row to skip.  pred fp32 [B, L, P], target from the
// image: optional per-patch (mean, unbiased var) normalisation, loss = sum_l mask * mean_P (pred - target)^2 / denom.
// BWD writes dpred (zeros on kept patches).
template <bool BWD>
__global__ void __launch_bounds__(kThreads) tokens_mae_loss_kernel(
    const float* __restrict__ img, const float* __restrict__ pred, const float* __restrict__ mask,
    const float* __restrict__ gscale, float* __restrict__ out, float* __restrict__ dpred, int B, int C, int H, int W,
    int p, int norm_pix, float inv_denom) {
  const int gh = H / p, gw = W / p, L = gh * gw, P = p * p * C;
  const int lane = threadIdx.x & 63;
  const int64_t patch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (patch >= (int64_t)B * L) return;
  const int l = (int)(patch % L), b = (int)(patch / L);
  float* dr = BWD ? dpred + patch * P : nullptr;
  if (mask[patch] == 0.f) {
    if (BWD) for (int i = lane; i < P; i += 64) dr[i] = 0.f;
    else if (lane == 0) out[patch] = 0.f;
    return;
  }
  const int w_ = l % gw, h_ = l / gw;
  float s = 0.f, ss = 0.f;
  for (int i = lane; i < P; i += 64) {
    const int c = i % C, pw = (i / C) % p, ph = i / (C * p);
    const float v = img[(((int64_t)b * C + c) * H + h_ * p + ph) * W + w_ * p + pw];
    s += v; ss += v * v;
  }
  s = wave_sum(s); ss = wave_sum(ss);
  float mu = 0.f, rs = 1.f;
  if (norm_pix) {
    mu = s / (float)P;
    float var = (ss - (float)P * mu * mu) / (float)(P - 1);      // unbiased (paddle var default)
    var = var < 0.f ? 0.f : var;
    rs = rsqrtf(var + 1e-6f);
  }
  const float* pr = pred + patch * P;
  const float g = BWD ? (gscale ? *gscale : 1.f) * 2.f * inv_denom / (float)P : 0.f;
  float acc = 0.f;
  for (int i = lane; i < P; i += 64) {
    const int c = i % C, pw = (i / C) % p, ph = i / (C * p);
    const float v = img[(((int64_t)b * C + c) * H + h_ * p + ph) * W + w_ * p + pw];
    const float d = pr[i] - (v - mu) * rs;
    if (BWD) dr[i] = g * d;
    else acc += d * d;
  }
  if (!BWD) {
    acc = wave_sum(acc);
    if (lane == 0) out[patch] = acc / (float)P * inv_denom;        // (the per-patch workspace)
  }
}

// out[0] = sum_i v[i] in ONE fixed order: thread t adds elements t, t+256, ...; wave shuffles; 4 wave sums in order
__global__ void __launch_bounds__(kThreads) tokens_ordered_sum_kernel(const float* __restrict__ v, int64_t n,
                                                                      float* __restrict__ out) {
  __shared__ float part[4];
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) a += v[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = part[0] + part[1] + part[2] + part[3];
}

static int loss_geometry(int B, int C, int H, int W, int p, float denom, int64_t* rows) {
  if (B <= 0 || C <= 0 || p <= 0 || H <= 0 || W <= 0 || (H % p) || (W % p) || !(denom > 0.f)) return PASSL_EINVAL;
  *rows = (int64_t)B * (H / p) * (W / p);
  if ((*rows + 3) / 4 > 0x7fffffffll || (int64_t)p * p * C > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

// shape checks of the three 5x5 entry points: -> tile counts and the mask geometry, or a status
static int conv_geometry(const float* mask, int N, int H, int W, int C, int Hm, int Wm, int dtype, int th, int* tilesH,
                         int* tilesW, int64_t* tiles, MaskGeo* m) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7)) return PASSL_EINVAL;
  m->mask = mask;
  m->g = 1; m->Wm = W; m->Lm = 0;
  if (mask) {
    if ((reinterpret_cast<uintptr_t>(mask) & 3u) || Hm <= 0 || Wm <= 0 || H % Hm || W % Wm || H / Hm != W / Wm)
      return PASSL_EINVAL;
    m->g = H / Hm; m->Wm = Wm; m->Lm = Hm * Wm;
  }
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  *tilesH = (H + th - 1) / th;
  *tilesW = (W + kTW - 1) / kTW;
  *tiles = (int64_t)N * *tilesH * *tilesW;
  const int64_t cchunks = (C + kCC - 1) / kCC;
  if (*tiles * cchunks > 0x7fffffffll || (int64_t)H * W > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

template <bool BWD>
static int launch_conv(const void* x, const float* w, const float* bias, const float* mask, void* y, int N, int H, int W,
                       int C, int Hm, int Wm, int dtype, passl_stream_t stream) {
  int tilesH = 0, tilesW = 0;
  int64_t tiles = 0;
  MaskGeo m;
  const int th = dtype == PASSL_BF16 ? ConvGeo<bf16_t>::TH : ConvGeo<float>::TH;
  const int rc = conv_geometry(mask, N, H, W, C, Hm, Wm, dtype, th, &tilesH, &tilesW, &tiles, &m);
  if (rc != PASSL_OK) return rc;
  const int cchunks = (C + kCC - 1) / kCC;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((dwconv5_masked_kernel<T, BWD>), dim3((unsigned)(tiles * cchunks)),
                                                 dim3(ConvGeo<T>::THREADS), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(x), w, bias, m, reinterpret_cast<T*>(y), H,
                                                 W, C, tilesH, tilesW, cchunks);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

// shape checks of the two gather entry points
static int gather_geometry(int B, int K, int Hm, int Wm, int p, int C) {
  if (B <= 0 || K <= 0 || Hm <= 0 || Wm <= 0 || p <= 0 || C <= 0 || (C & 7)) return PASSL_EINVAL;
  if ((int64_t)Hm * Wm > 0x7fffffffll || K > Hm * Wm) return PASSL_EINVAL;
  if ((int64_t)p * C > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  return PASSL_OK;
}

static int tokens_geometry(int B, int L, int K, int D) {
  return (B <= 0 || L <= 0 || K <= 0 || K > L || D <= 0 || (D & 7)) ? PASSL_EINVAL : PASSL_OK;
}

}  // namespace

extern "C" int passl_hip_dwconv5_masked_fwd(const void* x, const float* w, const float* bias, const float* mask, void* y,
                                            int N, int H, int W, int C, int Hm, int Wm, int dtype,
                                            passl_stream_t stream) {
  if (!x || !w || !bias || !y || !aligned16(x) || !aligned16(w) || !aligned16(bias) || !aligned16(y))
    return PASSL_EINVAL;
  return launch_conv<false>(x, w, bias, mask, y, N, H, W, C, Hm, Wm, dtype, stream);
}

extern "C" int passl_hip_dwconv5_masked_bwd_data(const void* dy, const float* w, const float* mask, void* dx, int N,
                                                 int H, int W, int C, int Hm, int Wm, int dtype,
                                                 passl_stream_t stream) {
  if (!dy || !w || !dx || !aligned16(dy) || !aligned16(w) || !aligned16(dx)) return PASSL_EINVAL;
  return launch_conv<true>(dy, w, nullptr, mask, dx, N, H, W, C, Hm, Wm, dtype, stream);
}

extern "C" int passl_hip_dwconv5_masked_bwd_weight(const void* x, const void* dy, const float* mask, float* dw,
                                                   float* dbias, float* ws, int64_t ws_floats, int N, int H, int W,
                                                   int C, int Hm, int Wm, int dtype, passl_stream_t stream) {
  if (!x || !dy || !dw || !dbias || !ws || !aligned16(x) || !aligned16(dy) || !aligned16(dw) || !aligned16(dbias) ||
      !aligned16(ws))
    return PASSL_EINVAL;
  int tilesH = 0, tilesW = 0;
  int64_t tiles = 0;
  MaskGeo m;
  const int rc = conv_geometry(mask, N, H, W, C, Hm, Wm, dtype, kWgradTH, &tilesH, &tilesW, &tiles, &m);
  if (rc != PASSL_OK) return rc;
  const int slabs = (int)(tiles < PASSL_DWCONV5_WGRAD_MAX_SLABS ? tiles : PASSL_DWCONV5_WGRAD_MAX_SLABS);
  if (ws_floats < (int64_t)slabs * kSums * C) return PASSL_EINVAL;
  const int cchunks = (C + kCC - 1) / kCC;
  float* ws_db = ws + (int64_t)slabs * kTaps * C;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(dwconv5_masked_wgrad_kernel<T>, dim3((unsigned)(slabs * cchunks)),
                                                 dim3(kWgradThreads), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(x), reinterpret_cast<const T*>(dy), m, ws,
                                                 ws_db, H, W, C, tilesH, tilesW, (int)tiles, slabs, cchunks);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  int rc2 = passl_slab_reduce_launch(ws, dw, (int64_t)kTaps * C, slabs, 0, as_stream(stream));
  if (rc2 == PASSL_OK) rc2 = passl_slab_reduce_launch(ws_db, dbias, C, slabs, 0, as_stream(stream));
  return rc2;
}

extern "C" int passl_hip_patch_gather_fwd(const void* x, const int32_t* ids_keep, void* out, int B, int K, int Hm,
                                          int Wm, int p, int C, int dtype, passl_stream_t stream) {
  if (!x || !ids_keep || !out || !aligned16(x) || !aligned16(out)) return PASSL_EINVAL;
  const int rc = gather_geometry(B, K, Hm, Wm, p, C);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(patch_gather_kernel<T>,
                                                 dim3(grid_for((int64_t)B * K * p * p * C / (16 / (int)sizeof(T)))),
                                                 dim3(kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(x),
                                                 ids_keep, reinterpret_cast<T*>(out), B, K, Hm, Wm, p, C);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_patch_gather_bwd(const void* dout, const int32_t* ids_restore, void* dx, int B, int K, int Hm,
                                          int Wm, int p, int C, int dtype, passl_stream_t stream) {
  if (!dout || !ids_restore || !dx || !aligned16(dout) || !aligned16(dx)) return PASSL_EINVAL;
  const int rc = gather_geometry(B, K, Hm, Wm, p, C);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(patch_gather_bwd_kernel<T>,
                                                 dim3(grid_for((int64_t)B * Hm * Wm * p * p * C / (16 / (int)sizeof(T)))),
                                                 dim3(kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(dout),
                                                 ids_restore, reinterpret_cast<T*>(dx), B, K, Hm, Wm, p, C);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_tokens_pos_gather_add(const void* x, const float* pos, const int32_t* ids_keep, void* out,
                                               int B, int L, int K, int D, int dtype, passl_stream_t stream) {
  if (!x || !pos || !ids_keep || !out || !aligned16(x) || !aligned16(pos) || !aligned16(out)) return PASSL_EINVAL;
  const int rc = tokens_geometry(B, L, K, D);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(pos_gather_add_kernel<T>, dim3(grid_for((int64_t)B * K * (D >> 3))),
                                                 dim3(kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(x),
                                                 pos, ids_keep, reinterpret_cast<T*>(out), B, L, K, D);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_tokens_pos_gather_add_bwd(const void* dout, const int32_t* ids_restore, float* dpos, int B,
                                                   int L, int K, int D, int dtype, passl_stream_t stream) {
  if (!dout || !ids_restore || !dpos || !aligned16(dout) || !aligned16(dpos)) return PASSL_EINVAL;
  const int rc = tokens_geometry(B, L, K, D);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(pos_gather_add_bwd_kernel<T>, dim3(grid_for((int64_t)L * (D >> 3))),
                                                 dim3(kThreads), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(dout), ids_restore, dpos, B, L, K, D);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_tokens_unshuffle(const void* x, const float* mask_token, const float* pos,
                                          const int32_t* ids_restore, void* out, int B, int L, int K, int D, int dtype,
                                          passl_stream_t stream) {
  if (!x || !mask_token || !pos || !ids_restore || !out || !aligned16(x) || !aligned16(mask_token) || !aligned16(pos) ||
      !aligned16(out))
    return PASSL_EINVAL;
  const int rc = tokens_geometry(B, L, K, D);
  if (rc != PASSL_OK) return rc;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(unshuffle_nocls_kernel<T>, dim3(grid_for((int64_t)B * L * (D >> 3))),
                                                 dim3(kThreads), 0, as_stream(stream), reinterpret_cast<const T*>(x),
                                                 mask_token, pos, ids_restore, reinterpret_cast<T*>(out), B, L, K, D);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_tokens_unshuffle_bwd(const void* dout, const int32_t* ids_keep, const int32_t* ids_restore,
                                              void* dx, float* dmask_token, int B, int L, int K, int D, int dtype,
                                              float* ws, int64_t ws_floats, passl_stream_t stream) {
  if (!dout || !ids_keep || !ids_restore || !dx || !dmask_token || !ws || !aligned16(dout) || !aligned16(dx) ||
      !aligned16(ws) || !aligned16(dmask_token))
    return PASSL_EINVAL;
  const int rc = tokens_geometry(B, L, K, D);
  if (rc != PASSL_OK) return rc;
  if (dtype != PASSL_F32 && dtype != PASSL_BF16) return PASSL_EUNSUPPORTED;
  const int64_t ntok = (int64_t)B * L;
  int slabs = (int)((ntok + 127) / 128 < PASSL_TOKENS_UNSHUFFLE_MAX_SLABS ? (ntok + 127) / 128
                                                                           : PASSL_TOKENS_UNSHUFFLE_MAX_SLABS);
  const int64_t tpb64 = (ntok + slabs - 1) / slabs;
  if (tpb64 > 0x7fffffffll) return PASSL_EUNSUPPORTED;
  const int tpb = (int)tpb64;
  slabs = (int)((ntok + tpb - 1) / tpb);
  if (ws_floats < (int64_t)slabs * D) return PASSL_EINVAL;
  PASSL_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(unshuffle_nocls_bwd_kernel<T>, dim3((D + 255) / 256, slabs),
                                                 dim3(kThreads), 0, as_stream(stream),
                                                 reinterpret_cast<const T*>(dout), ids_keep, ids_restore,
                                                 reinterpret_cast<T*>(dx), ws, B, L, K, D, tpb);)
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return passl_slab_reduce_launch(ws, dmask_token, D, slabs, 1, as_stream(stream));
}

// workspace: one float per (image, patch) row = B * L
extern "C" int passl_hip_tokens_mae_loss_fwd(const float* img, const float* pred, const float* mask, float* loss, int B,
                                             int C, int H, int W, int p, int norm_pix, float denom, float* ws,
                                             int64_t ws_floats, passl_stream_t stream) {
  if (!img || !pred || !mask || !loss || !ws) return PASSL_EINVAL;
  int64_t rows = 0;
  const int rc = loss_geometry(B, C, H, W, p, denom, &rows);
  if (rc != PASSL_OK) return rc;
  if (ws_floats < rows) return PASSL_EINVAL;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tokens_mae_loss_kernel<false>, dim3((unsigned)((rows + 3) / 4)), dim3(kThreads), 0, st, img, pred,
                     mask, nullptr, ws, nullptr, B, C, H, W, p, norm_pix, 1.0f / denom);
  hipLaunchKernelGGL(tokens_ordered_sum_kernel, dim3(1), dim3(kThreads), 0, st, ws, rows, loss);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}

extern "C" int passl_hip_tokens_mae_loss_bwd(const float* img, const float* pred, const float* mask, const float* gscale,
                                             float* dpred, int B, int C, int H, int W, int p, int norm_pix, float denom,
                                             passl_stream_t stream) {
  if (!img || !pred || !mask || !dpred) return PASSL_EINVAL;
  int64_t rows = 0;
  const int rc = loss_geometry(B, C, H, W, p, denom, &rows);
  if (rc != PASSL_OK) return rc;
  hipLaunchKernelGGL(tokens_mae_loss_kernel<true>, dim3((unsigned)((rows + 3) / 4)), dim3(kThreads), 0,
                     as_stream(stream), img, pred, mask, gscale, nullptr, dpred, B, C, H, W, p, norm_pix, 1.0f / denom);
  PASSL_RETURN_IF_LAUNCH_FAILED();
  return PASSL_OK;
}
