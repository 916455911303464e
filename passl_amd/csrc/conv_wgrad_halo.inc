// Spatially tiled 3x3 / stride-1 weight gradient (default since round 5; option wgrad_halo = 0 turns it off); included by conv_wgrad.hip
// inside its anonymous namespace (WParams, wg_store, lds_read_tr64).  Design and layout: wgrad_halo_geom.h.
//
// Workgroup = 4 waves (2 x 2), a 64 (oc) x 64 (c) block of dW for all nine taps: 36 accumulator fragments per wave.
// k-tile = one 8 x 8 patch (64 reduction rows); NST LDS stages of 28 KB (dY 8 KB | X halo 20 KB), filled by LDS-DMA
// (7 pieces per wave and k-tile); per k-tile: counted vmcnt -> barrier -> issue the k-tile NST-1 ahead -> the dY
// fragments of both k-steps (8 transposing reads) -> nine taps, each 8 transposing reads of the X halo at
// compile-time offsets (overlapped with the previous tap's 8 MFMAs).
// OVERHANG = false: images whose sides are multiples of 8 (the form measured on hardware); true: any image, the pixels of
// a patch outside it fetched as zeros (checked by the emulator only so far).
template <int NST, bool OVERHANG>
__global__ void __launch_bounds__(kThreads, NST == 2 ? 2 : 1) wgrad_halo_kernel(const WParams p, const wgh::Geom g) {
  constexpr int FM = 2, FN = 2, KS = 2;
  constexpr int IPT = 7;                       // LDS-DMA pieces per wave and k-tile: 2 of dY, 5 of the halo
  static_assert(NST == 2 || NST == 3, "ring depth");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int vb;
  {
    const int bid = blockIdx.x, nb = gridDim.x;
    const int xcd = bid & 7, local = bid >> 3;
    const int q = nb >> 3, r = nb & 7;
    vb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  }
  const int bx = vb % p.grid_j, by = (vb / p.grid_j) % p.grid_oc, bz = vb / (p.grid_j * p.grid_oc);
  const int oc0 = by * 64, c0 = bx * 64;
  const int kt_begin = bz * p.tiles_per_split;
  int kt_end = kt_begin + p.tiles_per_split;
  if (kt_end > p.nk_total) kt_end = p.nk_total;
  if (kt_begin >= kt_end) return;
  const int nk = kt_end - kt_begin;

  __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(p.a), 0, (uint32_t)((int64_t)g.N * g.a_sn2), 0x00020000);
  __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<char*>(p.dy), 0,
      OVERHANG ? (uint32_t)((int64_t)g.N * g.IH * g.IW * g.dy_pitch) : (uint32_t)((int64_t)g.npatches * 64 * g.dy_pitch), 0x00020000);

  // ---- lane-static DMA geometry
  uint32_t dy_st[2], h_st[5];
  int dy_yx[2], h_yx[5];                     // OVERHANG: the lane's pixel / halo position; else h_yx = border flags
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if constexpr (OVERHANG) dy_st[i] = wgh::dy_static(g, oc0, i * 4 + wave, lane, dy_yx[i]);
    else { dy_st[i] = wgh::dy_static_tiled(g, oc0, i * 4 + wave, lane); dy_yx[i] = 0; }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    if constexpr (OVERHANG) h_st[i] = wgh::halo_static(g, c0, i * 4 + wave, lane, h_yx[i]);
    else h_st[i] = wgh::halo_static_tiled(g, c0, i * 4 + wave, lane, h_yx[i]);
  }

  // patch of the NEXT k-tile to issue (wave-uniform)
  int i_n, i_y0, i_x0;
  wgh::patch_origin(g, kt_begin, i_n, i_y0, i_x0);
  int issued = 0;
  auto issue_tile = [&]() {
    char* sb = smem + (issued % NST) * wgh::kStage;
    const uint32_t dy_base = (uint32_t)wgh::patch_m(g, i_n, i_y0, i_x0) * (uint32_t)g.dy_pitch;
    const uint32_t x_base = wgh::patch_x(g, i_n, i_y0, i_x0);
    const int emask = OVERHANG ? 0 : wgh::edge_mask(g, i_y0, i_x0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint32_t off;
      if constexpr (OVERHANG) off = (dy_st[i] == wgh::kNoSrc || !wgh::dy_inside(g, i_y0, i_x0, dy_yx[i])) ? wgh::kNoSrc : dy_st[i] + dy_base;
      else off = dy_st[i] == wgh::kNoSrc ? wgh::kNoSrc : dy_st[i] + dy_base;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_dy, (__attribute__((address_space(3))) void*)(sb + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      uint32_t off;
      if constexpr (OVERHANG) off = wgh::halo_inside(g, i_y0, i_x0, h_yx[i]) ? h_st[i] + x_base : wgh::kNoSrc;
      else off = (h_yx[i] & emask) ? wgh::kNoSrc : h_st[i] + x_base;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_a, (__attribute__((address_space(3))) void*)(sb + wgh::kDyBytes + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
    }
    ++issued;
    i_x0 += 8;
    if constexpr (OVERHANG) {
      if (i_x0 >= g.IW) { i_x0 = 0; i_y0 += 8; if (i_y0 >= g.IH) { i_y0 = 0; ++i_n; } }
    } else {
      if (i_x0 == g.IW) { i_x0 = 0; i_y0 += 8; if (i_y0 == g.IH) { i_y0 = 0; ++i_n; } }
    }
  };

  // ---- fragment read addresses (bytes inside a stage)
  uint32_t a_rd[2][FM];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < FM; ++i) a_rd[h][i] = wgh::dy_frag(wm * 32 + i * 16, 0, h, lane);
  const uint32_t x_rd = wgh::x_frag_lane(lane) + (uint32_t)(wn * 32 * 2);

  f32x4 acc[9][FM][FN];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 af[KS][FM], bfr[2][KS][FN];
  auto read_b = [&](auto TAP, auto SET, uint32_t xb) {
    constexpr int T_ = decltype(TAP)::value, S_ = decltype(SET)::value;
    constexpr int R_ = T_ / 3, Q_ = T_ % 3;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // (ks, j) are compile-time after unrolling only through constexpr arguments: spell the four fragments out
      if (ks == 0) {
        const uint2 l0 = lds_read_tr64<wgh::x_frag_const(0, 0, 0, R_, Q_)>(xb), h0 = lds_read_tr64<wgh::x_frag_const(0, 0, 1, R_, Q_)>(xb);
        const uint2 l1 = lds_read_tr64<wgh::x_frag_const(16, 0, 0, R_, Q_)>(xb), h1 = lds_read_tr64<wgh::x_frag_const(16, 0, 1, R_, Q_)>(xb);
        bfr[S_][0][0] = make_uint4(l0.x, l0.y, h0.x, h0.y);
        bfr[S_][0][1] = make_uint4(l1.x, l1.y, h1.x, h1.y);
      } else {
        const uint2 l0 = lds_read_tr64<wgh::x_frag_const(0, 1, 0, R_, Q_)>(xb), h0 = lds_read_tr64<wgh::x_frag_const(0, 1, 1, R_, Q_)>(xb);
        const uint2 l1 = lds_read_tr64<wgh::x_frag_const(16, 1, 0, R_, Q_)>(xb), h1 = lds_read_tr64<wgh::x_frag_const(16, 1, 1, R_, Q_)>(xb);
        bfr[S_][1][0] = make_uint4(l0.x, l0.y, h0.x, h0.y);
        bfr[S_][1][1] = make_uint4(l1.x, l1.y, h1.x, h1.y);
      }
    }
  };
  auto mfma_tap = [&](auto TAP, auto SET) {
    constexpr int T_ = decltype(TAP)::value, S_ = decltype(SET)::value;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[T_][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[ks][i]),
                                                                   __builtin_bit_cast(bf16x8_t, bfr[S_][ks][j]),
                                                                   acc[T_][i][j], 0, 0, 0);
  };

  for (int t = 0; t < NST && t < nk; ++t) issue_tile();
  for (int t = 0; t < nk; ++t) {
    // k-tile t landed; the k-tiles issued after it may stay in flight
    if (t == 0) {
      if (NST == 3 && nk >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPT) : "memory");
      else if (nk >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      if (NST == 3 && t + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();      // everybody's k-tile t landed; everybody finished reading stage (t - 1) % NST
    if (t >= 1 && t - 1 + NST < nk) issue_tile();          // k-tile t - 1 + NST into stage (t - 1) % NST
    const uint32_t sb = lds0 + (uint32_t)((t % NST) * wgh::kStage);
    const uint32_t xb = sb + x_rd;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const uint2 l0 = lds_read_tr64<0>(sb + a_rd[0][i]), h0 = lds_read_tr64<0>(sb + a_rd[1][i]);
      const uint2 l1 = lds_read_tr64<32 * 128>(sb + a_rd[0][i]), h1 = lds_read_tr64<32 * 128>(sb + a_rd[1][i]);
      af[0][i] = make_uint4(l0.x, l0.y, h0.x, h0.y);
      af[1][i] = make_uint4(l1.x, l1.y, h1.x, h1.y);
    }
    read_b(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, xb);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#define PASSL_WGH_TAP(T)                                                                             \
    if constexpr (T < 8) read_b(std::integral_constant<int, (T < 8 ? T + 1 : 8)>{}, std::integral_constant<int, (T + 1) & 1>{}, xb); \
    mfma_tap(std::integral_constant<int, T>{}, std::integral_constant<int, T & 1>{});                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                               \
    __builtin_amdgcn_sched_barrier(0);
    PASSL_WGH_TAP(0) PASSL_WGH_TAP(1) PASSL_WGH_TAP(2) PASSL_WGH_TAP(3) PASSL_WGH_TAP(4)
    PASSL_WGH_TAP(5) PASSL_WGH_TAP(6) PASSL_WGH_TAP(7) PASSL_WGH_TAP(8)
#undef PASSL_WGH_TAP
  }

  // ---- epilogue: partial block -> dW[oc][tap * C + c] / workspace slab (wg_store)
  const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int oc = oc0 + wm * 32 + i * 16 + l4 * 4 + r;
          const int c = c0 + wn * 32 + j * 16 + l15;
          if (oc < p.NCOLS && c < p.C && !(p.dbg & 1)) wg_store(p, bz, oc, t * p.C + c, acc[t][i][j][r]);
        }
}

// EUNSUPPORTED: switched off (the default) or outside the envelope
template <int NST, bool OVERHANG>
int launch_halo(const WParams& p, const wgh::Geom& g, int splits, hipStream_t st) {
  constexpr int LDS = NST * wgh::kStage;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_halo_kernel<NST, OVERHANG>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    attr_set = true;
  }
  t_eff_splits = splits;
  hipLaunchKernelGGL((wgrad_halo_kernel<NST, OVERHANG>), dim3(p.grid_j * p.grid_oc * splits), dim3(kThreads), LDS, st, p, g);
  return hipGetLastError() == hipSuccess ? PASSL_OK : PASSL_ELAUNCH;
}

int wgrad_halo_try(const WParams& p0, int splits, int64_t a_bytes, int64_t dy_bytes, hipStream_t st) {
  const int halo = passl_opt(Opt::wgrad_halo);    // 1: images whose sides are multiples of 8, 2: every such layer
  if (!halo) return PASSL_EUNSUPPORTED;
  if (p0.R != 3 || p0.S != 3 || p0.sh != 1 || p0.sw != 1 || p0.ph != 1 || p0.pw != 1) return PASSL_EUNSUPPORTED;
  if (p0.IH != p0.OP || p0.IW != p0.OQ) return PASSL_EUNSUPPORTED;
  if (halo == 1 && ((p0.IH & 7) || (p0.IW & 7))) return PASSL_EUNSUPPORTED;      // 2: also images that the patches overhang
  const int64_t lim = 0x7ffffff0ll;
  if (a_bytes >= lim || dy_bytes >= lim) return PASSL_EUNSUPPORTED;
  if ((int64_t)(p0.IH - 1) * p0.a_sh + (int64_t)(p0.IW - 1) * p0.a_sw + p0.C > p0.a_sn) return PASSL_EUNSUPPORTED;
  WParams p = p0;
  wgh::Geom g;
  const int N = p.M / (p.OP * p.OQ);
  g.N = N; g.IH = p.IH; g.IW = p.IW; g.C = p.C; g.NCOLS = p.NCOLS;
  g.PXN = (p.IW + 7) / 8; g.PN = ((p.IH + 7) / 8) * g.PXN; g.npatches = N * g.PN;
  g.a_sn2 = (int)(p.a_sn * 2); g.a_sh2 = (int)(p.a_sh * 2); g.a_sw2 = (int)(p.a_sw * 2);
  g.dy_pitch = (int)(p.dy_ld * 2);
  g.d_pn = halo::make_fdiv((uint32_t)g.PN); g.d_pxn = halo::make_fdiv((uint32_t)g.PXN);
  // a k-tile is a patch: 64 reduction rows — as many as the caller counted (M / 64) when the patches tile the
  // image, more otherwise; the slices are re-cut over the patches, never more of them than the caller provided slabs for
  p.nk_total = g.npatches;
  if (splits > p.nk_total) splits = p.nk_total;
  p.tiles_per_split = (p.nk_total + splits - 1) / splits;
  splits = (p.nk_total + p.tiles_per_split - 1) / p.tiles_per_split;
  p.grid_j = (p.C + 63) / 64;
  p.grid_oc = (p.NCOLS + 63) / 64;
  p.nsplits = splits;
  const int nst = passl_opt(Opt::wgrad_halo_stages);
  if ((p.IH & 7) || (p.IW & 7))
    return nst == 3 ? launch_halo<3, true>(p, g, splits, st) : launch_halo<2, true>(p, g, splits, st);
  return nst == 3 ? launch_halo<3, false>(p, g, splits, st) : launch_halo<2, false>(p, g, splits, st);
}
