// The library's tuning and diagnostic switches, each declared once: name, default, accepted values.  runtime.hip turns
// the list into the table behind passl_hip_set_option / passl_hip_get_option; the launch paths read a value by its
// index (passl_opt).  On the first access to any option every option takes its default, then the value of the
// environment variable PASSL_<NAME in upper case> when that is set (and accepted).  include/passl_hip.h documents them.
// Accepted values: ANY int, RANGE(lo, hi) or ONE_OF(v, ...) (at most four values).
#pragma once

#define PASSL_OPTION_LIST(X)                                                                                         \
  /* conv_igemm_ring.hip: the LDS-DMA ring kernel */                                                                 \
  X(igemm_ring,             1,    ANY)                /* != 0: use it where it applies */                            \
  X(igemm_ring_min_nk,      8,    ANY)                /* ... for reductions of at least n 64-element K-tiles */      \
  X(igemm_ring_min_tiles,   1,    ANY)                /* ... and launches of at least n output tiles */              \
  X(igemm_ring_bm,          128,  ONE_OF(128, 256))   /* row tile */                                                 \
  X(igemm_ring_bk,          64,   ONE_OF(32, 64))     /* K-tile */                                                   \
  X(igemm_ring_stages32,    4,    ONE_OF(3, 4))       /* ring depth of the BK = 32 variant */                        \
  /* conv_igemm_8p.hip: the 256 x 256-tile 8-phase kernel and its cost model (0.01 us, margin in %) */               \
  X(igemm_8p,               1,    RANGE(0, 2))        /* never / when the cost model prefers it / always */          \
  X(igemm_8p_min_nk,        8,    RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_direct,        1,    ANY)                /* != 0: persistent form */                                    \
  X(igemm_8p_dense,         1,    RANGE(0, 2))        /* matrix-operand form: off / persistent / also staged */      \
  X(igemm_8p_tk,            145,  RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_te,            1000, RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_te_direct,     900,  RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_ring_tk,       112,  RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_ring_te,       420,  RANGE(1, INT_MAX))                                                                 \
  X(igemm_8p_margin,        100,  RANGE(1, INT_MAX))                                                                 \
  /* conv3x3_wave.hip: the wave-per-patch 3x3 kernel */                                                              \
  X(conv3x3_wave,           1,    ANY)                /* != 0: on */                                                 \
  X(conv3x3_wave_rows,      4,    ONE_OF(4, 8))       /* patch rows per wave */                                      \
  X(conv3x3_wave_modes,     7,    RANGE(0, 7))        /* launches that take it: bit mask */                          \
  X(conv3x3_wave_dbg,       0,    ANY)                /* ablation bits */                                            \
  /* conv_igemm.hip: the register-staged kernel */                                                                   \
  X(igemm_persist,          0,    ANY)                /* != 0: persistent form */                                    \
  X(igemm_persist_grid,     0,    RANGE(0, INT_MAX))  /* its grid (& ~7; 0: the device's resident workgroups) */     \
  X(igemm_nk1,              24,   ANY)                /* K-tiles up to which the single-stage variant runs */        \
  X(igemm_lean,             1,    RANGE(0, 1))        /* 4-workgroup form of the K = 64 dense launches */            \
  X(igemm_dbg,              0,    RANGE(0, 63))       /* ablation bits */                                            \
  /* conv_stem.hip */                                                                                                \
  X(stem_kernel,            1,    ANY)                /* != 0: on */                                                 \
  /* conv_wgrad.hip, conv_wgrad_halo.inc: weight gradients */                                                        \
  X(wgrad_dma,              1,    RANGE(0, 1))        /* LDS-DMA kernels for bf16 */                                 \
  X(wgrad_tile,             0,    ANY)                /* 0 by shape, 1-4 one fixed tile */                           \
  X(wgrad_pipe,             2,    ANY)                /* register double-buffered kernel: 0 off, 1, 2 */             \
  X(wgrad_halo,             2,    RANGE(0, 2))        /* spatially tiled 3x3 kernel: off / sides % 8 == 0 / all */   \
  X(wgrad_halo_stages,      2,    ONE_OF(2, 3))                                                                      \
  X(wgrad_dbg,              0,    RANGE(0, 1))        /* 1: skip the epilogue stores */                              \
  /* bn.hip */                                                                                                       \
  X(bn_stream_unroll,       4,    ONE_OF(0, 2, 4, 8)) /* streaming kernels: grid-stride (0) / tile form of U */      \
  /* stem_pool.hip */                                                                                                \
  X(stem_pool_form,         1,    RANGE(0, 1))                                                                       \
  X(stem_pool_wgs,          1024, RANGE(1, 65536))                                                                   \
  /* attention.hip, attention_bf16.hip */                                                                            \
  X(attn_f32mfma,           0,    RANGE(0, 1))        /* 1: bf16 activations through the fp32-MFMA kernels */        \
  X(attn_waves,             0,    ONE_OF(0, 4, 8))    /* waves per workgroup (0: by sequence length) */

enum class Opt {
#define PASSL_OPT_ENUM(name, def, values) name,
  PASSL_OPTION_LIST(PASSL_OPT_ENUM)
#undef PASSL_OPT_ENUM
  kCount
};

// the current value of an option (host code; no string compare, no environment read)
int passl_opt(Opt o);
