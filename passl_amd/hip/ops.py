"""Tensor-level wrappers over the C ABI (no autograd here; see functional.py).

torch is used for device memory and the current stream only.  Every function launches HIP
kernels from libpassl_hip.so; host tensors are refused (lib.ptr raises).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import config
from . import lib as L
from . import plan as P


def _lib():
    return L.load()


# ------------------------------------------------------------------ shared fp32 workspace
class _Workspace:
    """ONE grow-only fp32 scratch buffer per device for the fixed-order (atomic-free) reductions:
    split-M weight-gradient slabs, InfoNCE dq slabs, column-sum partials.  Every user launches its
    producer and its reduce kernel back to back on the current stream, so stream order makes sharing
    safe; the buffer is never read across ops.  Keyed by stream as well: the weight gradients run on the
    side stream (hip/streams.py) with their own scratch."""

    def __init__(self):
        self._bufs = {}

    def get(self, n_floats, device):
        # one buffer per (device, stream): users on different streams must not share scratch
        key = (device.type, device.index, L.stream() if device.type == 'cuda' else 0)     # raw handle: ~0.3 us
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < n_floats:
            # grow-only with a 4 MB floor (most users need a few KB; the largest weight-gradient slabs ask for more)
            buf = torch.empty(max(int(n_floats), 1 << 20), dtype=torch.float32, device=device)
            self._bufs[key] = buf
        return buf

    def pin(self):
        """References to every scratch buffer that exists right now, for somebody whose recorded launches carry raw
        pointers into them (hip/replay.py): ``get`` REPLACES a buffer when a later call asks for more, and the old one
        must then outlive its last recorded user.  Dropping the returned list is the unpin.  (The library's own
        finalize-counter slices, csrc/bn.hip, live as long as the library: recorded launches hold those too, and a
        plan and an eager step must not run concurrently on one device for that reason.)"""
        return list(self._bufs.values())


workspace = _Workspace()


# ------------------------------------------------------------------ fills / copies / casts
# Library kernels for what would otherwise be the step's last ATen launches: a step plan (hip/replay.py) replays
# the launches of THIS library, so a training step must not depend on a kernel torch launches.
def fill_zero(t):
    """t[...] = 0 for a contiguous device tensor."""
    assert t.is_contiguous()
    if t.numel():
        L.check(_lib().passl_hip_fill_zero(L.ptr(t), t.numel() * t.element_size(), L.stream()), 'fill_zero')
    return t


def zeros(*shape, dtype=None, device=None):
    return fill_zero(torch.empty(*shape, dtype=dtype, device=device))


def zeros_like(x):
    return fill_zero(torch.empty(x.shape, dtype=x.dtype, device=x.device))


def copy_into(dst, src):
    """dst[...] = src[...]: same dtype and element count, both contiguous, no overlap."""
    assert dst.is_contiguous() and src.is_contiguous() and dst.dtype == src.dtype and dst.numel() == src.numel()
    if dst.numel():
        L.check(_lib().passl_hip_copy_bytes(L.ptr(dst), L.ptr(src), dst.numel() * dst.element_size(), L.stream()),
                'copy_bytes')
    return dst


def clone(x):
    return copy_into(torch.empty(x.shape, dtype=x.dtype, device=x.device), x.contiguous())


def cast_f32(x):
    """bf16 -> fp32 copy (fp32 input is returned as is)."""
    if x.dtype == torch.float32:
        return x
    assert x.dtype == torch.bfloat16
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(_lib().passl_hip_cast_bf16_to_f32(L.ptr(x), L.ptr(y), x.numel(), L.stream()), 'cast_bf16_to_f32')
    return y


def cast_to(x, dtype):
    """fp32 <-> bf16 copy through the library's cast kernels (identity when the dtype already matches)."""
    if x.dtype == dtype:
        return x
    if dtype == torch.float32:
        return cast_f32(x)
    assert dtype == torch.bfloat16 and x.dtype == torch.float32
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    cast_bf16(x.view(-1), y.view(-1))
    return y


def unpad_add(src, dst, rows, R, dst_S, dst_C, src_S, src_C):
    """dst[row][r][s][c] += src[row][r][s][c] over the dense extents of a padded block (the stem filter's gradient)."""
    L.check(_lib().passl_hip_unpad_add(L.ptr(src), L.ptr(dst), rows, R, dst_S, dst_C, src_S, src_C, L.stream()),
            'unpad_add')


def add_into(dst, src):
    """dst += src for contiguous fp32 tensors of the same size (the fixed-order slab adder with one slab)."""
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.numel() == src.numel()
    assert dst.is_contiguous() and src.is_contiguous()
    L.check(_lib().passl_hip_slab_reduce(L.ptr(src), L.ptr(dst), dst.numel(), 1, 1, L.stream()), 'slab_reduce')
    return dst


_ones = {}


def ones_like_cached(t):
    """A resident all-ones tensor shaped like t (the root gradient of ``loss.backward()``: autograd would otherwise
    launch a fill kernel per step)."""
    key = (t.device, t.dtype, tuple(t.shape))
    o = _ones.get(key)
    if o is None:
        o = _ones[key] = torch.ones(t.shape, dtype=t.dtype, device=t.device)
    return o


# ------------------------------------------------------------------ convolution
_desc_cache = {}


def _conv_struct(d: P.Desc):
    key = id(d)
    hit = _desc_cache.get(key)
    if hit is not None and hit[0] is d:
        return hit[1]
    s = L.ConvDesc()
    for f in ('N', 'OP', 'OQ', 'NCOLS', 'R', 'S', 'C', 'IH', 'IW', 'sh', 'sw', 'ph', 'pw',
              'a_sn', 'a_sh', 'a_sw', 'y_sn', 'y_sh', 'y_sw'):
        setattr(s, f, getattr(d, f))
    s.stats = None
    s.stats_tiles = 0
    _desc_cache[key] = (d, s)
    return s


def conv_tiles(d: P.Desc):
    """Number of 128-row output tiles of a launch = slab rows of its fused statistics."""
    return (d.N * d.OP * d.OQ + 127) // 128


def conv_igemm(d: P.Desc, a, b, y, scale=None, shift=None, residual=None, relu=False,
               out_f32=False, stats=None, bnb=None, apro=None):
    """Launch one implicit-GEMM conv described by `d` (plan.Desc).  `a` activation tensor,
    `b` packed weights [NCOLS, R*S*C] (same dtype as a), `y` output tensor (written in place at
    d.y_off with d's strides).  `stats`: fp32 slab from conv_stats_buffer (fused forward BatchNorm
    statistics of the stored output, bf16 only).  `bnb`: dict(y, mask, mean, invstd, scale, shift,
    relu, partial, tile_off) — BatchNorm-backward statistics fused into this data-gradient launch
    (include/passl_hip.h: passl_conv_desc.bnb_*).
    `apro`: dict(mode, out, scale, shift | a2, coef) — the apply pass of the BatchNorm whose output this launch consumes,
    done on the A operand inside the launch (passl_hip_conv_igemm_apro): `a` is then that BatchNorm's INPUT (mode 1) or
    its masked output gradient (mode 2, `a2` its input), and the transformed operand is also written to `out`.
    Returns None, with nothing launched, when the library does not serve the launch in that form: the caller runs
    the streaming pass and calls again without `apro`."""
    s = _conv_struct(d)
    esz = 4 if out_f32 else y.element_size()
    s.a = L.ptr(a)
    s.b = L.ptr(b)
    s.y = L.ptr(y) + d.y_off * esz
    s.scale = L.ptr(scale)
    s.shift = L.ptr(shift)
    s.residual = (L.ptr(residual) + d.y_off * esz) if residual is not None else None
    s.relu = 1 if relu else 0
    s.dtype = L.dt(a)
    s.out_f32 = 1 if out_f32 else 0
    s.stats = L.ptr(stats)
    s.stats_tiles = conv_tiles(d) if stats is not None else 0
    if bnb is not None:
        s.bnb_y = L.ptr(bnb['y']) + d.y_off * esz
        # the bit mask is indexed like the dense tensor: shift it with the sub-lattice origin (y_off % 8 == 0)
        mask = bnb.get('mask')
        s.bnb_mask = (L.ptr(mask) + (d.y_off >> 3)) if mask is not None else None
        s.bnb_mean, s.bnb_invstd = L.ptr(bnb['mean']), L.ptr(bnb['invstd'])
        s.bnb_scale, s.bnb_shift = L.ptr(bnb.get('scale')), L.ptr(bnb.get('shift'))
        s.bnb_partial = L.ptr(bnb['partial'])
        s.bnb_relu, s.bnb_tile_off = int(bnb['relu']), int(bnb['tile_off'])
        if bnb.get('partial2') is not None:          # a second BatchNorm behind the same gradient (bnb2_*)
            s.bnb2_y = L.ptr(bnb['y2']) + d.y_off * esz
            s.bnb2_mean, s.bnb2_invstd = L.ptr(bnb['mean2']), L.ptr(bnb['invstd2'])
            s.bnb2_partial = L.ptr(bnb['partial2'])
        else:
            s.bnb2_y = s.bnb2_mean = s.bnb2_invstd = s.bnb2_partial = None
    else:
        s.bnb_y = s.bnb_mask = s.bnb_mean = s.bnb_invstd = s.bnb_scale = s.bnb_shift = None
        s.bnb_partial = None
        s.bnb_relu = s.bnb_tile_off = 0
        s.bnb2_y = s.bnb2_mean = s.bnb2_invstd = s.bnb2_partial = None
    if apro is not None:
        if d.y_off or bnb is not None and bnb.get('partial2') is not None:
            return None
        pro = L.ConvApro()
        pro.mode = int(apro['mode'])
        pro.a2, pro.a_coef = L.ptr(apro.get('a2')), L.ptr(apro.get('coef'))
        pro.a_scale, pro.a_shift = L.ptr(apro.get('scale')), L.ptr(apro.get('shift'))
        pro.a_out = L.ptr(apro['out'])
        rc = _lib().passl_hip_conv_igemm_apro(C.byref(s), C.byref(pro), L.stream())
        if rc == L.EUNSUPPORTED:
            return None
        L.check(rc, 'conv_igemm_apro')
        return y
    rc = _lib().passl_hip_conv_igemm(C.byref(s), L.stream())
    if rc == L.EUNSUPPORTED and bnb is not None and bnb.get('partial2') is not None:
        # include/passl_hip.h (bnb2_*): the two-BatchNorm instantiations cover fewer launches than the Python-side test
        # can know (K-tile thresholds, kernel selection options, operand strides): run this launch without the second
        # layer — its own backward then does its reduce pass — and tell the caller through bnb['partial2_done']
        s.bnb2_y = s.bnb2_mean = s.bnb2_invstd = s.bnb2_partial = None
        bnb['partial2_done'] = False
        rc = _lib().passl_hip_conv_igemm(C.byref(s), L.stream())
    elif bnb is not None and bnb.get('partial2') is not None:
        bnb['partial2_done'] = True
    L.check(rc, 'conv_igemm')
    return y


_wdesc_cache = {}


def wgrad_slices(d: P.Desc, dtype):
    """Number of reduction slices of a weight-gradient launch (host logic, no GPU): the product kernels' heuristic,
    or — only with the EXPERIMENTAL spatially tiled kernel switched on (config.wgrad_halo) and for the launches it
    takes — the count that fits ITS grid."""
    halo = config.wgrad_halo()
    if (halo and dtype == torch.bfloat16 and d.R == 3 and d.S == 3 and d.sh == 1 and d.sw == 1 and d.ph == 1 and
            d.pw == 1 and d.IH == d.OP and d.IW == d.OQ and (halo == 2 or (d.IH % 8 == 0 and d.IW % 8 == 0))):
        return P.wgrad_halo_splits(d.N, d.IH, d.IW, d.NCOLS, d.C)
    M = d.N * d.OP * d.OQ
    bkm = 64 if dtype == torch.bfloat16 else 32
    esz = 2 if dtype == torch.bfloat16 else 4
    return P.wgrad_splits(M, d.NCOLS, d.R * d.S * d.C, bkm, target_blocks=P.wgrad_target_blocks(d.IH * d.IW > 1),
                          row_bytes=max(d.NCOLS, d.C * d.sh * d.sw) * esz)


def conv_wgrad(d: P.Desc, a, dy, dw, splits=None):
    """dw[NCOLS, R*S*C] (fp32) += dy^T . gather(a)."""
    key = id(d)
    hit = _wdesc_cache.get(key)
    if hit is not None and hit[0] is d:
        s = hit[1]
    else:
        s = L.WgradDesc()
        for f in ('N', 'OP', 'OQ', 'NCOLS', 'R', 'S', 'C', 'IH', 'IW', 'sh', 'sw', 'ph', 'pw',
                  'a_sn', 'a_sh', 'a_sw'):
            setattr(s, f, getattr(d, f))
        _wdesc_cache[key] = (d, s)
    s.a = L.ptr(a)
    s.dy = L.ptr(dy)
    s.dw = L.ptr(dw)
    s.dy_ld = d.NCOLS
    s.dtype = L.dt(a)
    s.splits = splits or wgrad_slices(d, a.dtype)
    # split-M partial tiles go to slabs of the shared workspace and are added in slice order
    need = s.splits * d.NCOLS * d.R * d.S * d.C
    ws = workspace.get(need, dw.device) if s.splits > 1 else None
    s.ws = L.ptr(ws)
    s.ws_floats = ws.numel() if ws is not None else 0
    L.check(_lib().passl_hip_conv_wgrad(C.byref(s), L.stream()), 'conv_wgrad')
    return dw


# ------------------------------------------------------------------ batch norm
def _bn_blocks(M, Cch, cap=1024):
    lanes = max(1, 256 // max(Cch // 8, 1))
    return int(max(1, min(cap, -(-M // (16 * lanes)))))


def conv_stats_buffer(d: P.Desc, device):
    """Slab for the conv epilogue's fused BN statistics of launch `d`: [tiles][C][2] shifted sums
    followed by [tiles][C] shifts (include/passl_hip.h: passl_conv_desc.stats).  Fully written by the
    kernel: no zeroing, no atomics.  Returns (tensor, tiles)."""
    t = conv_tiles(d)
    return torch.empty(bn_partial_floats(t, d.NCOLS, True), dtype=torch.float32, device=device), t


def bn_partial_floats(nblocks, Cch, shifted):
    """Floats of a BatchNorm partial buffer: slab + the finalize kernels' segment scratch."""
    return nblocks * Cch * (3 if shifted else 2) + 16 * Cch * 4


def _gather_doubles(t):
    """all_gather of a small fp64 device tensor in rank order -> [world, *t.shape]."""
    import torch.distributed as dist
    world = dist.get_world_size()
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t)            # (concatenation along dim 0: the form every backend accepts)
    return out.view((world,) + tuple(t.shape))


def bn_train_fwd(x, gamma, beta, rmean, rvar, residual=None, relu=True, momentum=0.9, eps=1e-5,
                 partial=None, want_mask=False, sync=False, apply=True):
    """x: [..., C] NHWC rows.  Returns z, stats[4,C] (mean, invstd, scale, shift), relu bit mask
    (or None); updates rmean/rvar in place.  `partial` = (slab, tiles) of fused statistics a conv
    epilogue already wrote (conv_stats_buffer); without it a stats pass over x is launched.
    `apply=False`: statistics only -> (None, stats, None) (the caller applies them: bn_relu_maxpool_fwd).
    `sync`: statistics over the batches of every rank (SyncBatchNorm): this rank's slab is folded to fp64
    moments, the moments are all-gathered and combined in rank order (csrc/bn.hip)."""
    Cch = x.shape[-1]
    M = x.numel() // Cch
    dev = x.device
    stats = torch.empty(4, Cch, dtype=torch.float32, device=dev)   # mean, invstd, scale, shift
    lib, st, dtc = _lib(), L.stream(), L.dt(x)
    if partial is None:
        nb = _bn_blocks(M, Cch)
        rpb = -(-M // nb)
        nb = -(-M // rpb)                   # every slab holds rows
        partial = torch.empty(bn_partial_floats(nb, Cch, True), dtype=torch.float32, device=dev)
        L.check(lib.passl_hip_bn_stats(L.ptr(x), L.ptr(partial), M, Cch, nb, dtc, st), 'bn_stats')
    else:
        partial, nb = partial
        rpb = 128
    if sync:
        mom = torch.empty(3, Cch, dtype=torch.float64, device=dev)
        L.check(lib.passl_hip_bn_moments(L.ptr(partial), nb, M, Cch, rpb, L.ptr(mom), st), 'bn_moments')
        mom_all = _gather_doubles(mom)
        L.check(lib.passl_hip_bn_finalize_moments(L.ptr(mom_all), mom_all.shape[0], Cch, L.ptr(gamma), L.ptr(beta),
                                                  L.ptr(rmean), L.ptr(rvar), momentum, eps, L.ptr(stats[0]),
                                                  L.ptr(stats[1]), L.ptr(stats[2]), L.ptr(stats[3]), L.stream()),
                'bn_finalize_moments')
    else:
        L.check(lib.passl_hip_bn_finalize(L.ptr(partial), nb, M, Cch, rpb, L.ptr(gamma), L.ptr(beta),
                                          L.ptr(rmean), L.ptr(rvar), momentum, eps,
                                          L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(stats[2]),
                                          L.ptr(stats[3]), st), 'bn_finalize')
    if not apply:
        return None, stats, None
    z = torch.empty_like(x)
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=dev) if (want_mask and relu) \
        else None
    L.check(lib.passl_hip_bn_apply(L.ptr(x), L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(residual),
                                   L.ptr(z), L.ptr(mask), M, Cch, 1 if relu else 0, dtc, L.stream()),
            'bn_apply')
    return z, stats, mask


def bn_apply(x, scale, shift, residual=None, relu=False, out=None):
    """z = relu?(x*scale + shift + residual) with given per-channel affine (inference BN; `out`: write z there)."""
    Cch = x.shape[-1]
    M = x.numel() // Cch
    z = torch.empty_like(x) if out is None else out
    L.check(_lib().passl_hip_bn_apply(L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(residual),
                                      L.ptr(z), None, M, Cch, 1 if relu else 0, L.dt(x),
                                      L.stream()), 'bn_apply')
    return z


def bn_bwd(dz, z, x, gamma, mean, invstd, dgamma, dbeta, relu=True, want_dres=False,
           scale=None, shift=None, fused=None, sync=False, defer=False):
    """Returns dx (and dres).  dgamma/dbeta (fp32 [C]) are accumulated into.
    `relu`: False/0 none, True/1 mask = z > 0, 2 mask recomputed from x*scale+shift (z unused),
    3 `z` is the bit mask written by the forward's bn_apply.
    `fused` = (slab, tiles): the data-gradient launch that produced `dz` already masked it and wrote
    the (sum g, sum g*xhat) slab (conv_igemm(bnb=...)): no reduce pass, no mask in the apply pass,
    and the residual-branch gradient IS dz (returned as dres without a copy).
    `defer` (with `fused`): no apply pass either -> (dx, dres, coef) with dx allocated and EMPTY: the data-gradient
    launch that consumes dx computes it from (dz, x, coef) on its way in and fills it (conv_igemm(apro=...)), or
    the caller runs bn_bwd_apply_fused."""
    Cch = x.shape[-1]
    M = x.numel() // Cch
    dev = x.device
    coef = torch.empty(3 * Cch, dtype=torch.float32, device=dev)
    lib, st, dtc = _lib(), L.stream(), L.dt(x)
    r = int(relu)
    zp = L.ptr(z) if r in (1, 3) else None
    if fused is not None:
        partial, nb = fused
        r, zp = 0, None
    else:
        # 768 = 3 resident workgroups per CU x 256 CUs: the backward-reduce kernel needs 136 VGPRs (3 waves per SIMD), and
        # a 1024-block launch ran a second, one-third-occupied round (the stem's reduce: 822 MB in 292 us = 2.8 TB/s)
        nb = _bn_blocks(M, Cch, cap=768)
        partial = torch.empty(bn_partial_floats(nb, Cch, False), dtype=torch.float32, device=dev)
        L.check(lib.passl_hip_bn_bwd_reduce(L.ptr(dz), zp, L.ptr(x), L.ptr(mean), L.ptr(invstd),
                                            L.ptr(scale), L.ptr(shift), L.ptr(partial), M, Cch, nb, r,
                                            dtc, st), 'bn_bwd_reduce')
    if sync:         # SyncBatchNorm: {sum g, sum g*xhat} of every rank, row count of the global batch
        import torch.distributed as dist
        sums = torch.empty(2, Cch, dtype=torch.float64, device=dev)
        L.check(lib.passl_hip_bn_bwd_sums(L.ptr(partial), nb, M, Cch, L.ptr(sums), st), 'bn_bwd_sums')
        sums_all = _gather_doubles(sums)
        L.check(lib.passl_hip_bn_bwd_finalize_sums(L.ptr(sums_all), sums_all.shape[0], dist.get_rank(),
                                                   M * sums_all.shape[0], Cch, L.ptr(gamma), L.ptr(mean),
                                                   L.ptr(invstd), L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef),
                                                   L.stream()), 'bn_bwd_finalize_sums')
    else:
        L.check(lib.passl_hip_bn_bwd_finalize(L.ptr(partial), nb, M, Cch, L.ptr(gamma), L.ptr(mean),
                                              L.ptr(invstd), L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef),
                                              st), 'bn_bwd_finalize')
    dx = torch.empty_like(x)
    if fused is not None:
        dres_out, dres = None, (dz if want_dres else None)
    else:
        dres_out = dres = torch.empty_like(x) if want_dres else None
    if defer and fused is not None:
        return dx, dres, coef
    L.check(lib.passl_hip_bn_bwd_apply(L.ptr(dz), zp, L.ptr(x), L.ptr(coef), L.ptr(scale),
                                       L.ptr(shift), L.ptr(dx), L.ptr(dres_out), M, Cch, r, dtc, L.stream()),
            'bn_bwd_apply')
    return dx, dres


def bn_bwd_apply_fused(g, x, coef, dx):
    """The apply pass bn_bwd(defer=True) left out: dx = coef[0] * g + coef[1] * x + coef[2] (g already masked)."""
    Cch = x.shape[-1]
    L.check(_lib().passl_hip_bn_bwd_apply(L.ptr(g), None, L.ptr(x), L.ptr(coef), None, None, L.ptr(dx), None,
                                          x.numel() // Cch, Cch, 0, L.dt(x), L.stream()), 'bn_bwd_apply')
    return dx


# ------------------------------------------------------------------ pooling / layout
def nchw_to_nhwc_pad(x, pad, Wp, Cp, dtype):
    N, Cc, H, W = x.shape
    y = torch.empty(N, H + 2 * pad, Wp, Cp, dtype=dtype, device=x.device)
    L.check(_lib().passl_hip_nchw_to_nhwc_pad(L.ptr(x), L.ptr(y), N, Cc, H, W, pad, Wp, Cp,
                                              L.dt(dtype), L.stream()), 'nchw_to_nhwc_pad')
    return y


def maxpool_fwd(x):
    N, H, W, Cc = x.shape
    P_, Q_ = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty(N, P_, Q_, Cc, dtype=x.dtype, device=x.device)
    idx = torch.empty(N, P_, Q_, Cc, dtype=torch.uint8, device=x.device)
    L.check(_lib().passl_hip_maxpool3x3s2_fwd(L.ptr(x), L.ptr(y), L.ptr(idx), N, H, W, Cc,
                                              L.dt(x), L.stream()), 'maxpool_fwd')
    return y, idx


def maxpool_bwd(dy, idx, H, W):
    N, _, _, Cc = dy.shape
    dx = torch.empty(N, H, W, Cc, dtype=dy.dtype, device=dy.device)
    L.check(_lib().passl_hip_maxpool3x3s2_bwd(L.ptr(dy), L.ptr(idx), L.ptr(dx), N, H, W, Cc,
                                              L.dt(dy), L.stream()), 'maxpool_bwd')
    return dx


def bn_relu_maxpool_supported(x):
    """The fused stem pass (csrc/stem_pool.hip) takes this BatchNorm input: [N,H,W,C] with C/8 dividing 256."""
    return x.dim() == 4 and _lib().passl_hip_bn_relu_maxpool_blocks(*x.shape) > 0


def bn_relu_maxpool_fwd(x, stats):
    """max-pool(relu(x * scale + shift)) in one pass; stats[4,C] from bn_train_fwd(..., apply=False) -> y, idx."""
    N, H, W, Cc = x.shape
    P_, Q_ = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty(N, P_, Q_, Cc, dtype=x.dtype, device=x.device)
    idx = torch.empty(N, P_, Q_, Cc, dtype=torch.uint8, device=x.device)
    L.check(_lib().passl_hip_bn_relu_maxpool_fwd(L.ptr(x), L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(y), L.ptr(idx),
                                                 N, H, W, Cc, L.dt(x), L.stream()), 'bn_relu_maxpool_fwd')
    return y, idx


def bn_relu_maxpool_bwd(dy, idx, x, gamma, stats, dgamma, dbeta, parts=1, on_part=None):
    """Backward of bn_relu_maxpool_fwd w.r.t. x; dgamma / dbeta (fp32 [C]) are accumulated into.
    parts > 1: the apply pass runs over that many pieces of the batch; on_part(dx, n0, n1, i, parts) is called after the launch
    that wrote dx[n0:n1], piece i of `parts` (the caller hands the piece to whoever consumes it: the stem's weight gradient)."""
    N, H, W, Cc = x.shape
    lib, st, dtc, dev = _lib(), L.stream(), L.dt(x), x.device
    nb = lib.passl_hip_bn_relu_maxpool_blocks(N, H, W, Cc)
    partial = torch.empty(bn_partial_floats(nb, Cc, False), dtype=torch.float32, device=dev)
    coef = torch.empty(3 * Cc, dtype=torch.float32, device=dev)
    L.check(lib.passl_hip_bn_relu_maxpool_bwd_reduce(L.ptr(dy), L.ptr(idx), L.ptr(x), L.ptr(stats[0]), L.ptr(stats[1]),
                                                     L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(partial), nb, N, H, W, Cc,
                                                     dtc, st), 'bn_relu_maxpool_bwd_reduce')
    L.check(lib.passl_hip_bn_bwd_finalize(L.ptr(partial), nb, N * H * W, Cc, L.ptr(gamma), L.ptr(stats[0]),
                                          L.ptr(stats[1]), L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), st),
            'bn_bwd_finalize')
    dx = torch.empty_like(x)
    parts = max(1, min(int(parts), N))
    for i in range(parts):
        n0, n1 = N * i // parts, N * (i + 1) // parts
        L.check(lib.passl_hip_bn_relu_maxpool_bwd_apply(L.ptr(dy[n0:n1]), L.ptr(idx[n0:n1]), L.ptr(x[n0:n1]), L.ptr(coef),
                                                        L.ptr(stats[2]), L.ptr(stats[3]), L.ptr(dx[n0:n1]), n1 - n0, H, W,
                                                        Cc, dtc, st), 'bn_relu_maxpool_bwd_apply')
        if on_part is not None:
            on_part(dx, n0, n1, i, parts)
    return dx


def avgpool_fwd(x):
    N, H, W, Cc = x.shape
    y = torch.empty(N, Cc, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_avgpool_fwd(L.ptr(x), L.ptr(y), N, H * W, Cc, L.dt(x), L.stream()),
            'avgpool_fwd')
    return y


def avgpool_bwd(dy, H, W):
    N, Cc = dy.shape
    dx = torch.empty(N, H, W, Cc, dtype=dy.dtype, device=dy.device)
    L.check(_lib().passl_hip_avgpool_bwd(L.ptr(dy), L.ptr(dx), N, H * W, Cc, L.dt(dy), L.stream()),
            'avgpool_bwd')
    return dx


def relu_bwd(dy, y):
    dx = torch.empty_like(dy)
    L.check(_lib().passl_hip_relu_bwd(L.ptr(dy), L.ptr(y), L.ptr(dx), dy.numel(), L.dt(dy),
                                      L.stream()), 'relu_bwd')
    return dx


def colsum_into(x, out, accumulate=False):
    """out[C] (fp32) = (accumulate: +=) column sums of x [M, C]."""
    M, Cc = x.shape
    fn = _lib().passl_hip_colsum_acc if accumulate else _lib().passl_hip_colsum
    ws = workspace.get(1024 * Cc, x.device)
    L.check(fn(L.ptr(x), L.ptr(out), M, Cc, L.dt(x), L.ptr(ws), ws.numel(), L.stream()), 'colsum')
    return out


# ------------------------------------------------------------------ contrastive head
def l2norm_fwd(x, eps=1e-12):
    N, Dd = x.shape
    y = torch.empty_like(x)
    norm = torch.empty(N, dtype=torch.float32, device=x.device)
    L.check(_lib().passl_hip_l2norm_fwd(L.ptr(x), L.ptr(y), L.ptr(norm), N, Dd, eps, L.stream()),
            'l2norm_fwd')
    return y, norm


def l2norm_bwd(dy, y, norm, out_dtype):
    N, Dd = y.shape
    dx = torch.empty(N, Dd, dtype=out_dtype, device=y.device)
    L.check(_lib().passl_hip_l2norm_bwd(L.ptr(dy), L.ptr(y), L.ptr(norm), L.ptr(dx), N, Dd,
                                        L.dt(out_dtype), L.stream()), 'l2norm_bwd')
    return dx


def cosine_loss_fwd(a, b, eps=1e-8):
    """-> loss [1] = -mean_i cos(a_i, b_i), stats [N,4] (for the backward)."""
    N, Dd = a.shape
    stats = torch.empty(N, 4, dtype=torch.float32, device=a.device)
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    L.check(_lib().passl_hip_cosine_loss_fwd(L.ptr(a), L.ptr(b), N, Dd, eps, L.ptr(stats), L.ptr(loss), L.stream()),
            'cosine_loss_fwd')
    return loss, stats


def cosine_loss_bwd(a, b, stats, gloss):
    N, Dd = a.shape
    da = torch.empty_like(a)
    L.check(_lib().passl_hip_cosine_loss_bwd(L.ptr(a), L.ptr(b), L.ptr(stats), L.ptr(gloss), N, Dd, L.ptr(da),
                                             L.stream()), 'cosine_loss_bwd')
    return da


def infonce_fwd(q, k, queue, T, want_logits=False):
    """Returns out[3] (loss, acc1, acc5), row_lse[N], logits[N,K+1] or None."""
    N, Dd = q.shape
    K = queue.shape[1]
    lib = _lib()
    ws = torch.empty(max(lib.passl_hip_infonce_workspace_bytes(N, K) // 4, 4),
                     dtype=torch.float32, device=q.device)
    out = torch.empty(3, dtype=torch.float32, device=q.device)
    lse = torch.empty(N, dtype=torch.float32, device=q.device)
    logits = torch.empty(N, K + 1, dtype=torch.float32, device=q.device) if want_logits else None
    L.check(lib.passl_hip_infonce_fwd(L.ptr(q), L.ptr(k), L.ptr(queue), N, Dd, K, T, L.ptr(out),
                                      L.ptr(lse), L.ptr(logits), L.ptr(ws), L.stream()),
            'infonce_fwd')
    return out, lse, logits


def infonce_bwd(q, k, queue, lse, gscale, T):
    N, Dd = q.shape
    K = queue.shape[1]
    dq = torch.empty_like(q)
    lib = _lib()
    ws = workspace.get(lib.passl_hip_infonce_bwd_workspace_bytes(N, K) // 4, q.device)
    L.check(lib.passl_hip_infonce_bwd(L.ptr(q), L.ptr(k), L.ptr(queue), L.ptr(lse),
                                      L.ptr(gscale), N, Dd, K, T, L.ptr(dq), L.ptr(ws), L.stream()),
            'infonce_bwd')
    return dq


def enqueue(queue, keys, ptr):
    Dd, K = queue.shape
    B = keys.shape[0]
    L.check(_lib().passl_hip_enqueue(L.ptr(queue), L.ptr(keys), Dd, K, int(ptr), B, L.stream()),
            'enqueue')


# ------------------------------------------------------------------ flat buffers
def ema_update(k_flat, q_flat, m, k_lp=None):
    L.check(_lib().passl_hip_ema_update(L.ptr(k_flat), L.ptr(q_flat), L.ptr(k_lp),
                                        k_flat.numel(), m, L.stream()), 'ema_update')


def bn_fold(flat, idx, eps, scale, shift):
    """scale / shift of every inference-form BatchNorm of an encoder (idx = (gamma, beta, mean, var) int64
    index lists into `flat`), one launch."""
    gi, bi, mi, vi = idx
    L.check(_lib().passl_hip_bn_fold(L.ptr(flat), L.ptr(gi), L.ptr(bi), L.ptr(mi), L.ptr(vi), gi.numel(),
                                     float(eps), L.ptr(scale), L.ptr(shift), L.stream()), 'bn_fold')


def momentum_sgd(p, g, v, lr, mu, wd, grad_scale=1.0):
    L.check(_lib().passl_hip_momentum_sgd(L.ptr(p), L.ptr(g), L.ptr(v), p.numel(), lr, mu, wd,
                                          grad_scale, L.stream()), 'momentum_sgd')


def momentum_sgd_dev(p, g, v, hyper, mu, wd, grad_scale=1.0):
    """hyper: device float32 tensor, [0] = learning rate (read when the kernel runs: HIP-graph replays)."""
    L.check(_lib().passl_hip_momentum_sgd_dev(L.ptr(p), L.ptr(g), L.ptr(v), p.numel(), L.ptr(hyper), mu, wd,
                                              grad_scale, L.stream()), 'momentum_sgd_dev')


def enqueue_dev(queue, keys, ptr_dev):
    """ptr_dev: int64[1] device tensor (MoCo's queue_ptr buffer); read and advanced on the device."""
    Dd, K = queue.shape
    L.check(_lib().passl_hip_enqueue_dev(L.ptr(queue), L.ptr(keys), Dd, K, L.ptr(ptr_dev), keys.shape[0],
                                         L.stream()), 'enqueue_dev')


def cast_bf16(src, dst):
    L.check(_lib().passl_hip_cast_f32_to_bf16(L.ptr(src), L.ptr(dst), src.numel(), L.stream()),
            'cast_f32_to_bf16')


def pack_weights(src, dst, jobs_dev, block_job, block_start, n_blocks):
    L.check(_lib().passl_hip_pack_weights(L.ptr(src), L.ptr(dst), L.dt(dst), L.ptr(jobs_dev),
                                          L.ptr(block_job), L.ptr(block_start), n_blocks,
                                          L.stream()), 'pack_weights')


# ------------------------------------------------------------------ SimCLR head / LARS
def ntxent_fwd(a, b, a_all, b_all, row_offset, T, co2_weight=3.0):
    """Returns out[2] (loss, acc1) and rowstats [B, 8] (saved for the backward)."""
    B, Dd = a.shape
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    rowstats = torch.empty(B, 8, dtype=torch.float32, device=a.device)
    L.check(_lib().passl_hip_ntxent_fwd(L.ptr(a), L.ptr(b), L.ptr(a_all), L.ptr(b_all), B,
                                        a_all.shape[0], int(row_offset), Dd, T, co2_weight,
                                        L.ptr(out), L.ptr(rowstats), L.stream()), 'ntxent_fwd')
    return out, rowstats


def ntxent_bwd(a, b, a_all, b_all, rowstats, gscale, row_offset, T, co2_weight=3.0):
    """Returns (da, db, da_all, db_all): row-role and column-role gradients."""
    B, Dd = a.shape
    da, db = zeros_like(a), zeros_like(b)
    da_all, db_all = zeros_like(a_all), zeros_like(b_all)
    L.check(_lib().passl_hip_ntxent_bwd(L.ptr(a), L.ptr(b), L.ptr(a_all), L.ptr(b_all),
                                        L.ptr(rowstats), L.ptr(gscale), B, a_all.shape[0],
                                        int(row_offset), Dd, T, co2_weight, L.ptr(da), L.ptr(db),
                                        L.ptr(da_all), L.ptr(db_all), L.stream()), 'ntxent_bwd')
    return da, db, da_all, db_all


def lars_momentum(p, g, v, table, lr, mu, coeff, eps, grad_scale=1.0):
    """`table` = dict(blk_off int64[nb], blk_len int32[nb], blk_seg int32[nb], seg_wd float[ns],
    norms float[ns + nb, 2] = workspace: squared norms + per-block partial sums) on the device (built
    once by the optimizer)."""
    assert table['norms'].numel() >= 2 * (table['seg_wd'].numel() + table['blk_off'].numel())
    L.check(_lib().passl_hip_lars_momentum(L.ptr(p), L.ptr(g), L.ptr(v), L.ptr(table['blk_off']),
                                           L.ptr(table['blk_len']), L.ptr(table['blk_seg']),
                                           table['blk_off'].numel(), L.ptr(table['seg_wd']),
                                           table['seg_wd'].numel(), L.ptr(table['norms']), lr, mu,
                                           coeff, eps, grad_scale, L.stream()), 'lars_momentum')


def lars_momentum_dev(p, g, v, table, hyper, mu, coeff, eps, grad_scale=1.0):
    """lars_momentum with lr = hyper[0] read on the device."""
    assert table['norms'].numel() >= 2 * (table['seg_wd'].numel() + table['blk_off'].numel())
    L.check(_lib().passl_hip_lars_momentum_dev(L.ptr(p), L.ptr(g), L.ptr(v), L.ptr(table['blk_off']),
                                               L.ptr(table['blk_len']), L.ptr(table['blk_seg']),
                                               table['blk_off'].numel(), L.ptr(table['seg_wd']),
                                               table['seg_wd'].numel(), L.ptr(table['norms']), L.ptr(hyper), mu,
                                               coeff, eps, grad_scale, L.stream()), 'lars_momentum_dev')


def larc_momentum_dev(p, g, v, table, hyper, mu, trust, eps, clip, grad_scale=1.0):
    """MomentumLARC over the flat arena (include/passl_hip.h), lr = hyper[0] on the device; same table as LARS."""
    assert table['norms'].numel() >= 2 * (table['seg_wd'].numel() + table['blk_off'].numel())
    L.check(_lib().passl_hip_larc_momentum_dev(L.ptr(p), L.ptr(g), L.ptr(v), L.ptr(table['blk_off']),
                                               L.ptr(table['blk_len']), L.ptr(table['blk_seg']),
                                               table['blk_off'].numel(), L.ptr(table['seg_wd']),
                                               table['seg_wd'].numel(), L.ptr(table['norms']), L.ptr(hyper), mu,
                                               trust, eps, int(bool(clip)), grad_scale, L.stream()),
            'larc_momentum_dev')


# ------------------------------------------------------------------ ViT / MAE
def layernorm_fwd(x, gamma, beta, eps):
    Cc = x.shape[-1]
    M = x.numel() // Cc
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    L.check(_lib().passl_hip_layernorm_fwd(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), L.ptr(mean),
                                           L.ptr(rstd), M, Cc, eps, L.dt(x), L.stream()), 'layernorm_fwd')
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=None, defer_params=False):
    """dres: gradient of the residual branch that forked off x (added to dx inside the kernel).
    defer_params: only dx now; -> (dx, partials, fold) where ``fold()`` adds the fixed-order parameter sums into
    dgamma / dbeta on whatever stream is current when it is called (hip/nn.py runs it on the side stream: a
    latency-bound launch the input-gradient chain does not wait for)."""
    Cc = x.shape[-1]
    M = x.numel() // Cc
    dx = torch.empty_like(x)
    need = -(-M // 16) * 2 * Cc                              # >= passl_hip_layernorm_bwd_ws_floats(M, C)
    lib = _lib()
    if defer_params:
        ws = torch.empty(need, dtype=torch.float32, device=x.device)      # its own buffer: read later, elsewhere
        L.check(lib.passl_hip_layernorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(gamma), L.ptr(mean), L.ptr(rstd),
                                            L.ptr(dres) if dres is not None else None, L.ptr(dx), None, None, M, Cc,
                                            L.dt(x), L.ptr(ws), ws.numel(), L.stream()), 'layernorm_bwd')

        def fold():
            L.check(lib.passl_hip_layernorm_param_reduce(L.ptr(ws), M, Cc, L.ptr(dgamma), L.ptr(dbeta), L.stream()),
                    'layernorm_param_reduce')
        return dx, ws, fold
    ws = workspace.get(need, x.device)
    L.check(lib.passl_hip_layernorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(gamma), L.ptr(mean), L.ptr(rstd),
                                        L.ptr(dres) if dres is not None else None, L.ptr(dx),
                                        L.ptr(dgamma), L.ptr(dbeta), M, Cc, L.dt(x), L.ptr(ws), ws.numel(),
                                        L.stream()), 'layernorm_bwd')
    return dx


def _unary(name, x, dy=None):
    """The streaming activations (csrc/eltwise.h): passl_hip_<name>(x, y, ...) or, with dy, (dy, x, dx, ...)."""
    out = torch.empty_like(x)
    args = (L.ptr(x), L.ptr(out)) if dy is None else (L.ptr(dy), L.ptr(x), L.ptr(out))
    L.check(getattr(_lib(), 'passl_hip_' + name)(*args, x.numel(), L.dt(x), L.stream()), name)
    return out


def gelu_fwd(x):
    return _unary('gelu_fwd', x)


def gelu_bwd(dy, x):
    return _unary('gelu_bwd', x, dy)


def tanh_fwd(x):
    return _unary('tanh_fwd', x)


def tanh_bwd(dy, x):
    return _unary('tanh_bwd', x, dy)


# the envelope of csrc/attention.hip / attention_bf16.hip (shape_ok): model constructors check it up front
ATTENTION_HEAD_DIMS = frozenset((32, 64))
ATTENTION_MAX_TOKENS = 208


def attention_fwd(qkv, B, T, H, DH, scale, causal=False):
    """qkv [B*T, 3*H*DH] -> out [B*T, H*DH], lse [B, H, T]."""
    out = torch.empty(B * T, H * DH, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
    L.check(_lib().passl_hip_attention_fwd(L.ptr(qkv), L.ptr(out), L.ptr(lse), B, T, H, DH, scale,
                                           int(causal), L.dt(qkv), L.stream()), 'attention_fwd')
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, T, H, DH, scale, causal=False):
    dqkv = torch.empty_like(qkv)
    L.check(_lib().passl_hip_attention_bwd(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(dqkv),
                                           B, T, H, DH, scale, int(causal), L.dt(qkv), L.stream()),
            'attention_bwd')
    return dqkv


# the envelope of csrc/attention_tiled.hip (check_shape): the key-tiled kernels, same head dimensions, no causal flag
ATTENTION_TILED_MAX_TOKENS = 1024


def attention_tiled_fwd(qkv, B, T, H, DH, scale):
    """qkv [B*T, 3*H*DH] -> out [B*T, H*DH], lse [B, H, T]; T <= ATTENTION_TILED_MAX_TOKENS."""
    out = torch.empty(B * T, H * DH, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
    L.check(_lib().passl_hip_attention_tiled_fwd(L.ptr(qkv), L.ptr(out), L.ptr(lse), B, T, H, DH, scale, L.dt(qkv),
                                                 L.stream()), 'attention_tiled_fwd')
    return out, lse


def attention_tiled_bwd(qkv, out, dout, lse, B, T, H, DH, scale):
    dqkv = torch.empty_like(qkv)
    L.check(_lib().passl_hip_attention_tiled_bwd(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(dqkv), B, T, H,
                                                 DH, scale, L.dt(qkv), L.stream()), 'attention_tiled_bwd')
    return dqkv


# ------------------------------------------------------------------ CAE (csrc/cross_attention.hip, csrc/cae.hip)
# the envelope of csrc/cross_attention.hip (check_shape): either length, same head dimensions
CROSS_ATTENTION_MAX_TOKENS = 1024


def cross_attention_fwd(q, k, v, B, Tq, Tk, H, DH, scale):
    """q [B*Tq, H*DH], k and v [B*Tk, H*DH] -> out [B*Tq, H*DH], lse [B, H, Tq]."""
    out = torch.empty(B * Tq, H * DH, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, Tq, dtype=torch.float32, device=q.device)
    L.check(_lib().passl_hip_cross_attention_fwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(lse), B, Tq, Tk, H, DH,
                                                 scale, L.dt(q), L.stream()), 'cross_attention_fwd')
    return out, lse


def cross_attention_bwd(q, k, v, out, dout, lse, B, Tq, Tk, H, DH, scale):
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    L.check(_lib().passl_hip_cross_attention_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(dout), L.ptr(lse),
                                                 L.ptr(dq), L.ptr(dk), L.ptr(dv), B, Tq, Tk, H, DH, scale, L.dt(q),
                                                 L.stream()), 'cross_attention_bwd')
    return dq, dk, dv


def cae_tokens_assemble(xu, xm, pos, ids_vis, ids_msk, B, want_q=True, want_kv=True, u0=0):
    """xu [B*(u0 + Nu), C] (read from row u0 of every image) or None, xm [B*Nm, C], pos fp32 [1 + L, C], ids int32
    [B, Nu] / [B, Nm] -> (q_in [B*Nm, C], k_in [B*(Nu + Nm), C], v_in likewise); what is not wanted is None."""
    Nm, D = ids_msk.shape[1], xm.shape[-1]
    Nu = ids_vis.shape[1] if (want_kv and ids_vis is not None) else 0
    q_in = torch.empty(B * Nm, D, dtype=xm.dtype, device=xm.device) if want_q else None
    k_in = torch.empty(B * (Nu + Nm), D, dtype=xm.dtype, device=xm.device) if want_kv else None
    v_in = torch.empty_like(k_in) if want_kv else None
    L.check(_lib().passl_hip_cae_tokens_assemble(L.ptr(xu if Nu else None), L.ptr(xm), L.ptr(pos),
                                                 L.ptr(ids_vis if Nu else None), L.ptr(ids_msk), L.ptr(q_in),
                                                 L.ptr(k_in), L.ptr(v_in), B, u0, Nu, Nm, pos.shape[0] - 1, D, L.dt(xm),
                                                 L.stream()), 'cae_tokens_assemble')
    return q_in, k_in, v_in


def cae_tokens_assemble_bwd(dq_in, dk_in, dv_in, B, Nu, Nm, u0=0):
    """-> (dxu [B*(u0 + Nu), C] with zero leading rows, or None when Nu = 0, dxm [B*Nm, C]); a gradient that is None
    counts as zero."""
    ref = next(t for t in (dq_in, dk_in, dv_in) if t is not None)
    D = ref.shape[-1]
    dxu = torch.empty(B * (u0 + Nu), D, dtype=ref.dtype, device=ref.device) if Nu else None
    dxm = torch.empty(B * Nm, D, dtype=ref.dtype, device=ref.device)
    L.check(_lib().passl_hip_cae_tokens_assemble_bwd(L.ptr(dq_in), L.ptr(dk_in), L.ptr(dv_in), L.ptr(dxu), L.ptr(dxm),
                                                     B, u0, Nu, Nm, D, L.dt(ref), L.stream()), 'cae_tokens_assemble_bwd')
    return dxu, dxm


def cae_mask_ids(mask, Nu):
    """mask fp32 [B, L] (1 = masked, L - Nu ones per image) -> (ids_vis [B, Nu], ids_msk [B, L - Nu], rank [B, L]) int32."""
    B, Ln = mask.shape
    ids_vis = torch.empty(B, Nu, dtype=torch.int32, device=mask.device)
    ids_msk = torch.empty(B, Ln - Nu, dtype=torch.int32, device=mask.device)
    rank = torch.empty(B, Ln, dtype=torch.int32, device=mask.device)
    L.check(_lib().passl_hip_cae_mask_ids(L.ptr(mask), L.ptr(ids_vis), L.ptr(ids_msk), L.ptr(rank), B, Ln, Nu,
                                          L.stream()), 'cae_mask_ids')
    return ids_vis, ids_msk, rank


def mse_fwd(pred, target, B, Tm, t0):
    """pred [B*Tm, C], target [B*(Tm + t0), C] read from row t0 of every image -> loss fp32 [1]."""
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = workspace.get(B * Tm, pred.device)
    L.check(_lib().passl_hip_mse_fwd(L.ptr(pred), L.ptr(target), L.ptr(loss), B, Tm, t0, pred.shape[-1], L.dt(pred),
                                     L.ptr(ws), ws.numel(), L.stream()), 'mse_fwd')
    return loss


def mse_bwd(pred, target, gloss, B, Tm, t0):
    dpred = torch.empty_like(pred)
    L.check(_lib().passl_hip_mse_bwd(L.ptr(pred), L.ptr(target), L.ptr(gloss), L.ptr(dpred), B, Tm, t0, pred.shape[-1],
                                     L.dt(pred), L.stream()), 'mse_bwd')
    return dpred


# ------------------------------------------------------------------ DeiT token assembly (csrc/deit_tokens.hip)
def prefix_tokens_fwd(x, prefixes, pos, B, Ln):
    """x [B*L, C], prefixes: one or two fp32 [C] rows, pos fp32 [NP + L, C] -> [B*(NP + L), C] = [prefixes | x] + pos."""
    NP, D = len(prefixes), x.shape[-1]
    out = torch.empty(B * (NP + Ln), D, dtype=x.dtype, device=x.device)
    p1 = prefixes[1] if NP > 1 else None
    L.check(_lib().passl_hip_prefix_tokens_fwd(L.ptr(x), L.ptr(prefixes[0]), L.ptr(p1), L.ptr(pos), L.ptr(out), B, Ln, NP,
                                               D, L.dt(x), L.stream()), 'prefix_tokens_fwd')
    return out


def prefix_tokens_bwd(dout, dprefixes, B, Ln):
    """dout [B*(NP + L), C] -> dx [B*L, C]; dprefixes[t] (fp32 [C]) += sum_b dout[b, t]."""
    NP, D = len(dprefixes), dout.shape[-1]
    dx = torch.empty(B * Ln, D, dtype=dout.dtype, device=dout.device)
    d1 = dprefixes[1] if NP > 1 else None
    L.check(_lib().passl_hip_prefix_tokens_bwd(L.ptr(dout), L.ptr(dx), L.ptr(dprefixes[0]), L.ptr(d1), B, Ln, NP, D,
                                               L.dt(dout), L.stream()), 'prefix_tokens_bwd')
    return dx


def mean2(a, b=None):
    """(a + b) / 2 over fp32 tensors of one shape; ``b`` None: a / 2."""
    out = torch.empty_like(a)
    L.check(_lib().passl_hip_mean2(L.ptr(a), L.ptr(b), L.ptr(out), a.numel(), L.stream()), 'mean2')
    return out


# ------------------------------------------------------------------ token merging, ToMe (csrc/tome.hip)
# the envelope of tome_match (match_shape_ok): the attention kernels', and one A token besides the class token
TOME_HEAD_DIMS = ATTENTION_HEAD_DIMS
TOME_MAX_TOKENS = ATTENTION_MAX_TOKENS
TOME_MIN_TOKENS = 3


def tome_max_r(T):
    """The clamp of tome.py:53 with the class token protected: at most half of the other tokens go."""
    return (T - 1) // 2


def tome_match(qkv, B, T, H, DH, r, want_nodes=False):
    """qkv [B*T, 3*H*DH] -> dest int32 [B, T], the output row (0 .. T-r-1) of every token (include/passl_hip.h has the
    order and the tie rule); with ``want_nodes`` also node_max fp32 [B, ceil(T/2)] and node_idx int32."""
    dest = torch.empty(B, T, dtype=torch.int32, device=qkv.device)
    nmax = nidx = None
    if want_nodes:
        nmax = torch.empty(B, (T + 1) // 2, dtype=torch.float32, device=qkv.device)
        nidx = torch.empty(B, (T + 1) // 2, dtype=torch.int32, device=qkv.device)
    L.check(_lib().passl_hip_tome_match(L.ptr(qkv), L.ptr(dest), L.ptr(nmax), L.ptr(nidx), B, T, H, DH, r, L.dt(qkv),
                                        L.stream()), 'tome_match')
    return (dest, nmax, nidx) if want_nodes else dest


def tome_merge_fwd(x, size, dest, B, T, r, want_log=False):
    """x [B*T, C], size fp32 [B, T] or None (ones), dest int32 [B, T] -> y [B*(T-r), C], size_out fp32 [B, T-r] and,
    with ``want_log``, log(size_out)."""
    Cc = x.shape[-1]
    y = torch.empty(B * (T - r), Cc, dtype=x.dtype, device=x.device)
    size_out = torch.empty(B, T - r, dtype=torch.float32, device=x.device)
    log_out = torch.empty(B, T - r, dtype=torch.float32, device=x.device) if want_log else None
    L.check(_lib().passl_hip_tome_merge_fwd(L.ptr(x), L.ptr(size), L.ptr(dest), L.ptr(y), L.ptr(size_out),
                                            L.ptr(log_out), B, T, r, Cc, L.dt(x), L.stream()), 'tome_merge_fwd')
    return (y, size_out, log_out) if want_log else (y, size_out)


def tome_merge_bwd(dy, size, size_out, dest, B, T, r):
    """dy [B*(T-r), C] -> dx [B*T, C], fully written."""
    Cc = dy.shape[-1]
    dx = torch.empty(B * T, Cc, dtype=dy.dtype, device=dy.device)
    L.check(_lib().passl_hip_tome_merge_bwd(L.ptr(dy), L.ptr(size), L.ptr(size_out), L.ptr(dest), L.ptr(dx), B, T, r,
                                            Cc, L.dt(dy), L.stream()), 'tome_merge_bwd')
    return dx


def attention_fwd_keybias(qkv, key_bias, B, T, H, DH, scale):
    """attention_fwd with score + key_bias[b, j] before the softmax; key_bias fp32 [B, T].  Forward only."""
    out = torch.empty(B * T, H * DH, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
    L.check(_lib().passl_hip_attention_fwd_keybias(L.ptr(qkv), L.ptr(key_bias), L.ptr(out), L.ptr(lse), B, T, H, DH,
                                                   scale, L.dt(qkv), L.stream()), 'attention_fwd_keybias')
    return out, lse


# ------------------------------------------------------------------ Swin Transformer (csrc/window_attention.hip)
WINDOW_ATTENTION_MAX_WINDOW = 14
WINDOW_ATTENTION_WORKGROUPS = 2048   # include/passl_hip.h: PASSL_WINDOW_ATTENTION_WORKGROUPS


def window_attention_ws_floats(windows, nH, ws):
    """include/passl_hip.h: PASSL_WINDOW_ATTENTION_WS_FLOATS."""
    return min((windows + 1) // 2, max(WINDOW_ATTENTION_WORKGROUPS // nH, 1)) * nH * ws ** 4


def window_attention_fwd(qkv, table, B, Hp, Wp, ws, shift, nH, DH, scale):
    """qkv [B*Hp*Wp, 3*nH*DH] of the unshifted, unpartitioned tokens, table fp32 [(2 ws - 1)^2, nH] ->
    out [B*Hp*Wp, nH*DH] in the same token order, lse fp32 [B*nW, nH, ws^2]."""
    out = torch.empty(B * Hp * Wp, nH * DH, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B * (Hp // max(ws, 1)) * (Wp // max(ws, 1)), nH, ws * ws, dtype=torch.float32, device=qkv.device)
    L.check(_lib().passl_hip_window_attention_fwd(L.ptr(qkv), L.ptr(table), L.ptr(out), L.ptr(lse), B, Hp, Wp, ws,
                                                  shift, nH, DH, scale, L.dt(qkv), L.stream()), 'window_attention_fwd')
    return out, lse


def window_attention_bwd_into(qkv, table, out, dout, lse, dtable, B, Hp, Wp, ws, shift, nH, DH, scale):
    """-> dqkv; dtable fp32 [(2 ws - 1)^2, nH] is WRITTEN."""
    dqkv = torch.empty_like(qkv)
    buf = workspace.get(window_attention_ws_floats(B * (Hp // ws) * (Wp // ws), nH, ws), qkv.device)
    L.check(_lib().passl_hip_window_attention_bwd(L.ptr(qkv), L.ptr(table), L.ptr(out), L.ptr(dout), L.ptr(lse),
                                                  L.ptr(dqkv), L.ptr(dtable), L.ptr(buf), buf.numel(), B, Hp, Wp, ws,
                                                  shift, nH, DH, scale, L.dt(qkv), L.stream()), 'window_attention_bwd')
    return dqkv


def patch_merge(x, B, H, W):
    """Rows [B*H*W, C] -> [B*(H/2)*(W/2), 4C]: the x0, x1, x2, x3 gather of PatchMerging (swin_transformer.py:343-384)."""
    Cc = x.shape[-1]
    y = torch.empty(B * (H // 2) * (W // 2), 4 * Cc, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_patch_merge(L.ptr(x), L.ptr(y), B, H, W, Cc, L.dt(x), L.stream()), 'patch_merge')
    return y


def patch_merge_bwd(dy, B, H, W):
    """The inverse copy: dy [B*(H/2)*(W/2), 4C] -> dx [B*H*W, C], fully written."""
    Cc = dy.shape[-1] // 4
    dx = torch.empty(B * H * W, Cc, dtype=dy.dtype, device=dy.device)
    L.check(_lib().passl_hip_patch_merge_bwd(L.ptr(dy), L.ptr(dx), B, H, W, Cc, L.dt(dy), L.stream()),
            'patch_merge_bwd')
    return dx


# ------------------------------------------------------------------ CaiT (csrc/cait_attention.hip)
# the envelope of the two kernels (check_shape): model constructors check it up front
CAIT_ATTENTION_HEAD_DIM = 48
CAIT_ATTENTION_MAX_HEADS = 8
CAIT_ATTENTION_MAX_TOKENS = 208


def talking_heads_attention_ws_floats(B, T, H):
    """include/passl_hip.h: PASSL_TALKING_HEADS_ATTENTION_WS_FLOATS."""
    return B * H * T + B * ((T + 15) // 16) * 144


def talking_heads_attention_fwd(qkv, wl, bl, ww, bw, B, T, H, DH, scale):
    """qkv [B*T, 3*H*DH]; wl, ww fp32 [H, H] ([in, out]) and bl, bw fp32 [H] -> out [B*T, H*DH], lse fp32 [B, H, T]."""
    out = torch.empty(B * T, H * DH, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
    L.check(_lib().passl_hip_talking_heads_attention_fwd(L.ptr(qkv), L.ptr(wl), L.ptr(bl), L.ptr(ww), L.ptr(bw),
                                                         L.ptr(out), L.ptr(lse), B, T, H, DH, scale, L.dt(qkv),
                                                         L.stream()), 'talking_heads_attention_fwd')
    return out, lse


def talking_heads_attention_bwd_into(qkv, wl, bl, ww, bw, dout, lse, dwl, dbl, dww, dbw, B, T, H, DH, scale):
    """-> dqkv; the four fp32 gradients dwl, dbl, dww, dbw are WRITTEN."""
    dqkv = torch.empty_like(qkv)
    buf = workspace.get(talking_heads_attention_ws_floats(B, T, H), qkv.device)
    L.check(_lib().passl_hip_talking_heads_attention_bwd(L.ptr(qkv), L.ptr(wl), L.ptr(bl), L.ptr(ww), L.ptr(bw),
                                                         L.ptr(dout), L.ptr(lse), L.ptr(dqkv), L.ptr(dwl), L.ptr(dbl),
                                                         L.ptr(dww), L.ptr(dbw), L.ptr(buf), buf.numel(), B, T, H, DH,
                                                         scale, L.dt(qkv), L.stream()), 'talking_heads_attention_bwd')
    return dqkv


def class_attention_fwd(q, k, v, B, T, H, DH, scale):
    """q [B, H*DH] (the class rows), k, v [B*T, H*DH] -> out [B, H*DH], lse fp32 [B, H]."""
    out = torch.empty(B, H * DH, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, dtype=torch.float32, device=q.device)
    L.check(_lib().passl_hip_class_attention_fwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), L.ptr(lse), B, T, H, DH,
                                                 scale, L.dt(q), L.stream()), 'class_attention_fwd')
    return out, lse


def class_attention_bwd(q, k, v, dout, lse, B, T, H, DH, scale):
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    L.check(_lib().passl_hip_class_attention_bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(dout), L.ptr(lse), L.ptr(dq),
                                                 L.ptr(dk), L.ptr(dv), B, T, H, DH, scale, L.dt(q), L.stream()),
            'class_attention_bwd')
    return dq, dk, dv


def cait_pos_add(x, pos, B, Ln):
    """x rows [B*Ln, C] + pos fp32 [Ln, C] (broadcast over the batch) -> rows [B*Ln, C]."""
    out = torch.empty_like(x)
    L.check(_lib().passl_hip_cait_pos_add(L.ptr(x), L.ptr(pos), L.ptr(out), B, Ln, x.shape[-1], L.dt(x), L.stream()),
             'cait_pos_add')
    return out


def cait_cls_concat(c, x, B, Ln):
    """c rows [B, C] (or [1, C]: the same class row for every image) and x rows [B*Ln, C] -> rows [B*(Ln+1), C]."""
    Cc = x.shape[-1]
    out = torch.empty(B * (Ln + 1), Cc, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_cait_cls_concat(L.ptr(c), int(c.shape[0] != 1 or B == 1), L.ptr(x), L.ptr(out), B, Ln,
                                              Cc, L.dt(x), L.stream()), 'cait_cls_concat')
    return out


def cait_cls_split(dout, add, B, Ln):
    """dout rows [B*(Ln+1), C] -> (dc [B, C], dx [B*Ln, C] = the patch rows, plus `add` when given)."""
    Cc = dout.shape[-1]
    dc = torch.empty(B, Cc, dtype=dout.dtype, device=dout.device)
    dx = torch.empty(B * Ln, Cc, dtype=dout.dtype, device=dout.device)
    L.check(_lib().passl_hip_cait_cls_split(L.ptr(dout), L.ptr(add), L.ptr(dc), L.ptr(dx), B, Ln, Cc, L.dt(dout),
                                             L.stream()), 'cait_cls_split')
    return dc, dx


def mae_mask(noise, len_keep):
    B, Ln = noise.shape
    dev = noise.device
    ids_keep = torch.empty(B, len_keep, dtype=torch.int32, device=dev)
    ids_restore = torch.empty(B, Ln, dtype=torch.int32, device=dev)
    mask = torch.empty(B, Ln, dtype=torch.float32, device=dev)
    L.check(_lib().passl_hip_mae_mask(L.ptr(noise), B, Ln, len_keep, L.ptr(ids_keep), L.ptr(ids_restore),
                                      L.ptr(mask), L.stream()), 'mae_mask')
    return ids_keep, ids_restore, mask


def mae_gather(x, cls, pos, ids_keep, B, Ln):
    K, D = ids_keep.shape[1], x.shape[-1]
    out = torch.empty(B * (K + 1), D, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_mae_gather(L.ptr(x), L.ptr(cls), L.ptr(pos), L.ptr(ids_keep), L.ptr(out), B,
                                        Ln, K, D, L.dt(x), L.stream()), 'mae_gather')
    return out


def mae_gather_bwd(dout, ids_restore, dcls, B, Ln, K):
    D = dout.shape[-1]
    dx = torch.empty(B * Ln, D, dtype=dout.dtype, device=dout.device)
    L.check(_lib().passl_hip_mae_gather_bwd(L.ptr(dout), L.ptr(ids_restore), L.ptr(dx), L.ptr(dcls), B, Ln,
                                            K, D, L.dt(dout), L.stream()), 'mae_gather_bwd')
    return dx


def mae_unshuffle(x, mask_token, pos, ids_restore, B, K):
    Ln, D = ids_restore.shape[1], x.shape[-1]
    out = torch.empty(B * (Ln + 1), D, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_mae_unshuffle(L.ptr(x), L.ptr(mask_token), L.ptr(pos), L.ptr(ids_restore),
                                           L.ptr(out), B, Ln, K, D, L.dt(x), L.stream()), 'mae_unshuffle')
    return out


def mae_unshuffle_bwd(dout, ids_keep, ids_restore, dmask_token, B):
    K, Ln, D = ids_keep.shape[1], ids_restore.shape[1], dout.shape[-1]
    dx = torch.empty(B * (K + 1), D, dtype=dout.dtype, device=dout.device)
    ws = workspace.get(1024 * D, dout.device)
    L.check(_lib().passl_hip_mae_unshuffle_bwd(L.ptr(dout), L.ptr(ids_keep), L.ptr(ids_restore), L.ptr(dx),
                                               L.ptr(dmask_token), B, Ln, K, D, L.dt(dout), L.ptr(ws),
                                               ws.numel(), L.stream()), 'mae_unshuffle_bwd')
    return dx


def patchify(img, p, dtype):
    B, Cc, H, W = img.shape
    out = torch.empty(B * (H // p) * (W // p), p * p * Cc, dtype=dtype, device=img.device)
    L.check(_lib().passl_hip_patchify(L.ptr(img), L.ptr(out), B, Cc, H, W, p, L.dt(dtype), L.stream()),
            'patchify')
    return out


# ------------------------------------------------------------------ stochastic depth (csrc/drop_path.hip)
def drop_path_draw(keep, keep_prob, seed, step):
    """One launch: keep [slots, B] fp32 <- 0 / 1 from Philox4x32-10 on (b, slot, *step) keyed by ``seed`` (a Python int,
    its low 64 bits are used); ``step`` is a device int64 [1] that the launch reads and advances by one."""
    slots, B = keep.shape
    seed &= (1 << 64) - 1
    if seed >= 1 << 63:
        seed -= 1 << 64                                   # the same 64-bit pattern as a signed argument
    L.check(_lib().passl_hip_drop_path_draw(L.ptr(keep), L.ptr(keep_prob), slots, B, seed, L.ptr(step), L.stream()),
            'drop_path_draw')
    return keep


def drop_path_add(branch, residual, keep_row, keep_prob, B, T):
    """residual + keep_row[b] * (branch / keep_prob) over rows [B*T, C]; keep_row: fp32 [B] on the device."""
    Cc = branch.shape[-1]
    out = torch.empty_like(branch)
    L.check(_lib().passl_hip_drop_path_add(L.ptr(branch), L.ptr(residual), L.ptr(keep_row), keep_prob, L.ptr(out),
                                           B, T, Cc, L.dt(branch), L.stream()), 'drop_path_add')
    return out


def drop_path_bwd(dy, keep_row, keep_prob, B, T):
    Cc = dy.shape[-1]
    dbranch = torch.empty_like(dy)
    L.check(_lib().passl_hip_drop_path_bwd(L.ptr(dy), L.ptr(keep_row), keep_prob, L.ptr(dbranch), B, T, Cc,
                                           L.dt(dy), L.stream()), 'drop_path_bwd')
    return dbranch


# ------------------------------------------------------------------ ConvNeXt block (csrc/dwconv.hip)
def dwconv7_wgrad_ws_floats(N, H, W, Cc):
    """include/passl_hip.h: PASSL_DWCONV7_WGRAD_WS_FLOATS."""
    return min(N * -(-H // 8) * -(-W // 16), 512) * 50 * Cc


def layer_scale_bwd_ws_floats(M, Cc):
    """include/passl_hip.h: PASSL_LAYER_SCALE_BWD_WS_FLOATS."""
    rows_per = -(-M // 1024)
    return -(-M // rows_per) * Cc


def dwconv7_fwd(x, w, bias):
    """Depthwise 7x7, padding 3: x NHWC [N, H, W, C]; w fp32 [C, 1, 7, 7] (the parameter as it lies), bias fp32 [C]."""
    N, H, W, Cc = x.shape
    y = torch.empty_like(x)
    L.check(_lib().passl_hip_dwconv7_fwd(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), N, H, W, Cc, L.dt(x), L.stream()),
            'dwconv7_fwd')
    return y


def dwconv7_bwd_data(dy, w, add=None):
    """dx of dwconv7_fwd (+ add, the gradient of the residual fork, inside the same rounding)."""
    N, H, W, Cc = dy.shape
    dx = torch.empty_like(dy)
    L.check(_lib().passl_hip_dwconv7_bwd_data(L.ptr(dy), L.ptr(w), L.ptr(add), L.ptr(dx), N, H, W, Cc, L.dt(dy),
                                              L.stream()), 'dwconv7_bwd_data')
    return dx


def dwconv7_bwd_weight_into(x, dy, dw, dbias):
    """dw [C, 1, 7, 7] and dbias [C] (fp32, WRITTEN) of dwconv7_fwd."""
    N, H, W, Cc = x.shape
    ws = workspace.get(dwconv7_wgrad_ws_floats(N, H, W, Cc), x.device)
    L.check(_lib().passl_hip_dwconv7_bwd_weight(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(dbias), L.ptr(ws), ws.numel(),
                                                N, H, W, Cc, L.dt(x), L.stream()), 'dwconv7_bwd_weight')
    return dw, dbias


# ------------------------------------------------------------------ ConvMAE (csrc/convmae.hip)
def dwconv5_wgrad_ws_floats(N, H, W, Cc):
    """include/passl_hip.h: PASSL_DWCONV5_WGRAD_WS_FLOATS."""
    return min(N * -(-H // 8) * -(-W // 16), 512) * 26 * Cc


def tokens_unshuffle_bwd_ws_floats(D):
    """include/passl_hip.h: PASSL_TOKENS_UNSHUFFLE_BWD_WS_FLOATS."""
    return 1024 * D


def _mask_grid(mask, grid):
    """(Hm, Wm) for the entry points: the grid of a given mask table, zeros (not read) without one."""
    if mask is None:
        return 0, 0
    Hm, Wm = grid
    if mask.dtype != torch.float32 or mask.shape[-1] != Hm * Wm:
        raise ValueError('mask %s %s does not hold an fp32 %d x %d grid' % (tuple(mask.shape), mask.dtype, Hm, Wm))
    return Hm, Wm


def dwconv5_masked_fwd(x, w, bias, mask=None, grid=None):
    """Depthwise 5x5, padding 2, of keep * x: x NHWC [N, H, W, C]; w fp32 [C, 1, 5, 5] (the parameter as it lies), bias
    fp32 [C]; mask fp32 [N, Hm * Wm] (1 = removed, grid = (Hm, Wm)) or None."""
    N, H, W, Cc = x.shape
    Hm, Wm = _mask_grid(mask, grid)
    y = torch.empty_like(x)
    L.check(_lib().passl_hip_dwconv5_masked_fwd(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(mask), L.ptr(y), N, H, W, Cc,
                                                Hm, Wm, L.dt(x), L.stream()), 'dwconv5_masked_fwd')
    return y


def dwconv5_masked_bwd_data(dy, w, mask=None, grid=None):
    """dx of dwconv5_masked_fwd: zero at the removed pixels."""
    N, H, W, Cc = dy.shape
    Hm, Wm = _mask_grid(mask, grid)
    dx = torch.empty_like(dy)
    L.check(_lib().passl_hip_dwconv5_masked_bwd_data(L.ptr(dy), L.ptr(w), L.ptr(mask), L.ptr(dx), N, H, W, Cc, Hm, Wm,
                                                     L.dt(dy), L.stream()), 'dwconv5_masked_bwd_data')
    return dx


def dwconv5_masked_bwd_weight_into(x, dy, dw, dbias, mask=None, grid=None):
    """dw [C, 1, 5, 5] and dbias [C] (fp32, WRITTEN) of dwconv5_masked_fwd."""
    N, H, W, Cc = x.shape
    Hm, Wm = _mask_grid(mask, grid)
    ws = workspace.get(dwconv5_wgrad_ws_floats(N, H, W, Cc), x.device)
    L.check(_lib().passl_hip_dwconv5_masked_bwd_weight(L.ptr(x), L.ptr(dy), L.ptr(mask), L.ptr(dw), L.ptr(dbias),
                                                       L.ptr(ws), ws.numel(), N, H, W, Cc, Hm, Wm, L.dt(x), L.stream()),
            'dwconv5_masked_bwd_weight')
    return dw, dbias


def patch_gather_fwd(x, ids_keep, grid, p):
    """x NHWC [B, Hm*p, Wm*p, C], ids_keep int32 [B, K] -> the kept patches' GEMM rows [B*K, p*p*C], columns (ph, pw, c)."""
    B, H, W, Cc = x.shape
    Hm, Wm = grid
    if H != Hm * p or W != Wm * p:
        raise ValueError('patch_gather: a %d x %d map is not a %d x %d grid of %d x %d patches' % (H, W, Hm, Wm, p, p))
    K = ids_keep.shape[1]
    out = torch.empty(B * K, p * p * Cc, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_patch_gather_fwd(L.ptr(x), L.ptr(ids_keep), L.ptr(out), B, K, Hm, Wm, p, Cc, L.dt(x),
                                              L.stream()), 'patch_gather_fwd')
    return out


def patch_gather_bwd(dout, ids_restore, B, K, grid, p, Cc):
    """dx NHWC [B, Hm*p, Wm*p, C] of patch_gather_fwd, fully written (zeros at the removed patches)."""
    Hm, Wm = grid
    dx = torch.empty(B, Hm * p, Wm * p, Cc, dtype=dout.dtype, device=dout.device)
    L.check(_lib().passl_hip_patch_gather_bwd(L.ptr(dout), L.ptr(ids_restore), L.ptr(dx), B, K, Hm, Wm, p, Cc,
                                              L.dt(dout), L.stream()), 'patch_gather_bwd')
    return dx


def tokens_pos_gather_add(x, pos, ids_keep, B, Ln, K):
    """out[b, k] = x[b, k] + pos[ids_keep[b, k]]: x [B*K, D] (or [B, K, D]), pos fp32 [Ln, D]."""
    D = x.shape[-1]
    out = torch.empty_like(x)
    L.check(_lib().passl_hip_tokens_pos_gather_add(L.ptr(x), L.ptr(pos), L.ptr(ids_keep), L.ptr(out), B, Ln, K, D,
                                                   L.dt(x), L.stream()), 'tokens_pos_gather_add')
    return out


def tokens_pos_gather_add_bwd_into(dout, ids_restore, dpos, B, Ln, K):
    """dpos fp32 [Ln, D] += the kept rows of dout, added over the images in ascending order."""
    D = dout.shape[-1]
    L.check(_lib().passl_hip_tokens_pos_gather_add_bwd(L.ptr(dout), L.ptr(ids_restore), L.ptr(dpos), B, Ln, K, D,
                                                       L.dt(dout), L.stream()), 'tokens_pos_gather_add_bwd')
    return dpos


def tokens_unshuffle(x, mask_token, pos, ids_restore, B, K):
    """Decoder input without a class row: x [B*K, D] -> [B*Ln, D]."""
    D = x.shape[-1]
    Ln = ids_restore.shape[1]
    out = torch.empty(B * Ln, D, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_tokens_unshuffle(L.ptr(x), L.ptr(mask_token), L.ptr(pos), L.ptr(ids_restore), L.ptr(out),
                                              B, Ln, K, D, L.dt(x), L.stream()), 'tokens_unshuffle')
    return out


def tokens_unshuffle_bwd(dout, ids_keep, ids_restore, dmask_token, B):
    """dx [B*K, D]; dmask_token (fp32 [D]) += the removed positions' rows of dout."""
    D = dout.shape[-1]
    Ln, K = ids_restore.shape[1], ids_keep.shape[1]
    dx = torch.empty(B * K, D, dtype=dout.dtype, device=dout.device)
    ws = workspace.get(tokens_unshuffle_bwd_ws_floats(D), dout.device)
    L.check(_lib().passl_hip_tokens_unshuffle_bwd(L.ptr(dout), L.ptr(ids_keep), L.ptr(ids_restore), L.ptr(dx),
                                                  L.ptr(dmask_token), B, Ln, K, D, L.dt(dout), L.ptr(ws), ws.numel(),
                                                  L.stream()), 'tokens_unshuffle_bwd')
    return dx


def tokens_mae_loss_fwd(img, pred, mask, p, norm_pix, denom):
    """The masked-patch loss on pred fp32 [B*L, p*p*C] (no class rows)."""
    B, Cc, H, W = img.shape
    loss = torch.empty(1, dtype=torch.float32, device=img.device)
    ws = workspace.get(B * (H // p) * (W // p), img.device)
    L.check(_lib().passl_hip_tokens_mae_loss_fwd(L.ptr(img), L.ptr(pred), L.ptr(mask), L.ptr(loss), B, Cc, H, W, p,
                                                 1 if norm_pix else 0, denom, L.ptr(ws), ws.numel(), L.stream()),
            'tokens_mae_loss_fwd')
    return loss


def tokens_mae_loss_bwd(img, pred, mask, gscale, p, norm_pix, denom):
    B, Cc, H, W = img.shape
    dpred = torch.empty_like(pred)
    L.check(_lib().passl_hip_tokens_mae_loss_bwd(L.ptr(img), L.ptr(pred), L.ptr(mask), L.ptr(gscale), L.ptr(dpred), B,
                                                 Cc, H, W, p, 1 if norm_pix else 0, denom, L.stream()),
            'tokens_mae_loss_bwd')
    return dpred


def layer_scale_add_fwd(branch, residual, gamma, keep_row, keep_prob, B, T):
    """residual + keep_row[b] * ((gamma * branch) / keep_prob) over rows [B*T, C]; keep_row None: rate 0 / evaluation."""
    Cc = branch.shape[-1]
    out = torch.empty_like(branch)
    L.check(_lib().passl_hip_layer_scale_add_fwd(L.ptr(branch), L.ptr(residual), L.ptr(gamma), L.ptr(keep_row),
                                                 keep_prob, L.ptr(out), B, T, Cc, L.dt(branch), L.stream()),
            'layer_scale_add_fwd')
    return out


def layer_scale_add_bwd_into(dy, branch, gamma, keep_row, keep_prob, B, T, dgamma):
    """-> dbranch; dgamma [C] (fp32) is WRITTEN."""
    Cc = dy.shape[-1]
    dbranch = torch.empty_like(dy)
    ws = workspace.get(layer_scale_bwd_ws_floats(B * T, Cc), dy.device)
    L.check(_lib().passl_hip_layer_scale_add_bwd(L.ptr(dy), L.ptr(branch), L.ptr(gamma), L.ptr(keep_row), keep_prob,
                                                 L.ptr(dbranch), L.ptr(dgamma), L.ptr(ws), ws.numel(), B, T, Cc,
                                                 L.dt(dy), L.stream()), 'layer_scale_add_bwd')
    return dbranch


# ------------------------------------------------------------------ element-wise dropout (csrc/dropout.hip)
def dropout_params(p):
    """-> (thr, factor) of rate ``p``: thr = floor(p * 65536 + 0.5) in double, factor = float32(1 / (1 - float32(p)))
    [Paddle-semantics: upscale_in_train].  p outside [0, 1), or one that rounds to thr = 65536, is refused."""
    p = float(p)
    thr = int(math.floor(p * 65536.0 + 0.5)) if 0.0 <= p < 1.0 else -1
    if not 0 <= thr <= 65535:
        raise ValueError('dropout rate must be in [0, 1) (threshold floor(p * 65536 + 0.5) in [0, 65535]), got %r' % p)
    return thr, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _signed64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v          # the same 64-bit pattern as a signed argument


def dropout_advance(step):
    """step: device int64 [1]; one launch adds 1."""
    L.check(_lib().passl_hip_dropout_advance(L.ptr(step), L.stream()), 'dropout_advance')
    return step


def _dropout(name, tensors, thr, factor, seed, step, site, out=None):
    """The four launches of csrc/dropout.hip: passl_hip_<name>(*tensors, out, n, thr, factor, seed, step, site, ...)."""
    x = tensors[0]
    out = torch.empty_like(x) if out is None else out
    L.check(getattr(_lib(), 'passl_hip_' + name)(*[L.ptr(t) for t in tensors], L.ptr(out), x.numel(), int(thr),
                                                  float(factor), _signed64(int(seed)), L.ptr(step), int(site),
                                                  L.dt(x), L.stream()), name)
    return out


def dropout(x, thr, factor, seed, step, site, out=None):
    """mask * (x * factor); applied to dy it is the backward of every dropout site."""
    return _dropout('dropout', (x,), thr, factor, seed, step, site, out)


def dropout_add(branch, residual, thr, factor, seed, step, site, out=None):
    """residual + mask * (branch * factor)."""
    return _dropout('dropout_add', (branch, residual), thr, factor, seed, step, site, out)


def gelu_dropout_fwd(x, thr, factor, seed, step, site, out=None):
    """mask * (gelu(x) * factor)."""
    return _dropout('gelu_dropout_fwd', (x,), thr, factor, seed, step, site, out)


def gelu_dropout_bwd(dy, x, thr, factor, seed, step, site, out=None):
    """(mask * (dy * factor)) * gelu'(x)."""
    return _dropout('gelu_dropout_bwd', (dy, x), thr, factor, seed, step, site, out)


# ------------------------------------------------------------------ mixup / cutmix, soft targets (csrc/mixup.hip)
def batch_mix(x, lam, box=None):
    """Mixup._mix_batch on a resident fp32 NCHW batch, out of place (``x`` is not written); the partner of sample b is
    B-1-b.  ``box`` None: mixup, fl(fl(x * f32(lam)) + fl(x.flip(0) * f32(1 - lam))).  ``box`` = (yl, yh, xl, xh): CutMix,
    x.flip(0) inside the box.  lam and the box are host numbers (plain kernel arguments)."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    lam = float(lam)
    yl, yh, xl, xh = (0, 0, 0, 0) if box is None else (int(v) for v in box)
    L.check(_lib().passl_hip_batch_mix(L.ptr(x), L.ptr(out), B, Cc, H, W, lam, 1.0 - lam, yl, yh, xl, xh,
                                       0 if box is None else 1, L.stream()), 'batch_mix')
    return out


def mixup_target(labels, num_classes, lam=1.0, eps=0.0):
    """labels int64 [N] -> fp32 [N, num_classes]: lam * smooth(onehot(y)) + (1 - lam) * smooth(onehot(y.flip(0))),
    smooth(v) = (1 - eps) v + eps / C.  lam = 1: plain label smoothing."""
    assert labels.dtype == torch.int64 and labels.dim() == 1 and labels.is_contiguous()
    N = labels.shape[0]
    target = torch.empty(N, num_classes, dtype=torch.float32, device=labels.device)
    L.check(_lib().passl_hip_mixup_target(L.ptr(labels), L.ptr(target), N, num_classes, float(lam), float(eps),
                                          L.stream()), 'mixup_target')
    return target


# ------------------------------------------------------------------ random erasing (csrc/random_erasing.hip)
def random_erase(x, boxes, mode, seed, step, out=None):
    """x fp32 NCHW [B,C,H,W]; boxes int32 [B,4] = (top, left, h, w) on the device, h == 0 or w == 0: not erased (the
    caller has validated the table).  mode 0: zeros inside the box; mode 1: N(0,1) from Philox4x32-10 on
    (seed, step, sample, position) — include/passl_hip.h.  ``out`` None: a new tensor (``x`` is not written);
    ``out is x``: in place, only box elements are stored."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.is_contiguous() and tuple(boxes.shape) == (x.shape[0], 4)
    B, Cc, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    seed, step = int(seed) & ((1 << 64) - 1), int(step) & ((1 << 64) - 1)
    seed -= (seed >> 63) << 64                            # the same 64-bit patterns as signed arguments
    step -= (step >> 63) << 64
    L.check(_lib().passl_hip_random_erase(L.ptr(x), L.ptr(out), L.ptr(boxes), B, Cc, H, W, int(mode), seed, step,
                                          L.stream()), 'random_erase')
    return out


# ------------------------------------------------------------------ crop + resize + flip + normalise (csrc/crop_resize.hip)
def crop_resize_norm(src, table, size, mean, std, scale):
    """src uint8 [B,Hs,Ws,3] (HWC, not written); table int32 [B,8] = (top, left, h, w, flip, 0, 0, 0) on the device (the
    caller has validated it) -> a new fp32 [B,3,size,size]: Pillow's 8-bit bicubic resize of every crop, flipped
    left-right where flip is set, then (float(v) * scale - mean[c]) / std[c] — include/passl_hip.h.  mean, std: three
    Python floats each, scale: one; they are rounded to fp32 here."""
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()
    assert table.dtype == torch.int32 and table.is_contiguous() and tuple(table.shape) == (src.shape[0], 8)
    B, Hs, Ws, _ = src.shape
    size = int(size)
    out = torch.empty(B, 3, size, size, dtype=torch.float32, device=src.device)
    if B == 0 and src.is_cuda:
        return out                                        # (an empty tensor has no address to hand over)
    consts = (C.c_float * 7)(*[float(v) for v in mean], *[float(v) for v in std], float(scale))
    L.check(_lib().passl_hip_crop_resize_norm(L.ptr(src), L.ptr(out), L.ptr(table), B, Hs, Ws, size,
                                              C.cast(consts, C.c_void_p), L.stream()), 'crop_resize_norm')
    return out


def crop_resize_u8(src, table, size):
    """The same crop and bicubic resample, ending in the resized image: a new uint8 [B,size,size,3] (HWC), flipped
    where the table's flip is set — the input of the colour stage below."""
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and src.is_contiguous()
    assert table.dtype == torch.int32 and table.is_contiguous() and tuple(table.shape) == (src.shape[0], 8)
    B, Hs, Ws, _ = src.shape
    size = int(size)
    out = torch.empty(B, size, size, 3, dtype=torch.uint8, device=src.device)
    if B == 0 and src.is_cuda:
        return out
    L.check(_lib().passl_hip_crop_resize_u8(L.ptr(src), L.ptr(out), L.ptr(table), B, Hs, Ws, size, L.stream()),
            'crop_resize_u8')
    return out


# ------------------------------------------------------------------ colour jitter, grayscale, solarise, blur (csrc/view_aug.hip)
VIEW_ROW = 24                                             # int32 per row of the operation table (include/passl_hip.h)
BLUR_R_MAX = 1                                            # the box radius the blur kernel is built for


def _view_args(img, table):
    assert img.dtype == torch.uint8 and img.dim() == 4 and img.shape[3] == 3 and img.is_contiguous()
    assert table.dtype == torch.int32 and table.is_contiguous() and tuple(table.shape) == (img.shape[0], VIEW_ROW)
    return img.shape[0], img.shape[1], img.shape[2]


def view_gray_sum(img, table):
    """img uint8 [B,H,W,3]; table int32 [B,24] on the device -> int64 [B]: per sample the sum of gray over the image after
    the operations that precede its contrast entry (0 without one).  Exact integer sums."""
    B, H, W = _view_args(img, table)
    sums = torch.empty(B, dtype=torch.int64, device=img.device)
    if B:
        L.check(_lib().passl_hip_view_gray_sum(L.ptr(img), L.ptr(table), L.ptr(sums), B, H, W, L.stream()),
                'view_gray_sum')
    return sums


def view_pointwise(img, table, sums=None, part=0, normalize=None):
    """The operations of one part of every sample's list (0: all, 1: before the blur, 2: after it).  ``normalize`` None:
    a new uint8 [B,H,W,3]; (mean, std, scale): a new fp32 [B,3,H,W], flipped where the table says so and normalised."""
    B, H, W = _view_args(img, table)
    assert sums is None or (sums.dtype == torch.int64 and sums.is_contiguous() and sums.numel() == B)
    if normalize is None:
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=img.device)
        consts = None
    else:
        mean, std, scale = normalize
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=img.device)
        consts = C.cast((C.c_float * 7)(*[float(v) for v in mean], *[float(v) for v in std], float(scale)), C.c_void_p)
    view_pointwise_into(img, table, sums, part, out, consts)
    return out


def view_pointwise_into(img, table, sums, part, out, consts):
    """``out``: a uint8 [B,H,W,3] or fp32 [B,3,H,W] tensor (any 4-byte aligned address: a view is fine); consts: the
    7 host floats as a c_void_p, for the fp32 output."""
    B, H, W = _view_args(img, table)
    if B == 0:
        return out
    u8 = out.dtype == torch.uint8
    L.check(_lib().passl_hip_view_pointwise(L.ptr(img), L.ptr(table), L.ptr(sums), L.ptr(out) if u8 else None,
                                            None if u8 else L.ptr(out), B, H, W, int(part), consts, L.stream()),
            'view_pointwise')
    return out


def gaussian_blur_u8(img, table, r_max):
    """img uint8 [B,H,W,3] -> a new uint8 [B,H,W,3]: samples whose row carries r >= 0 blurred (three box passes per axis
    with the row's (r, ww, fw)), the others copied.  ``r_max``: the largest r of the table, known to the caller."""
    B, H, W = _view_args(img, table)
    if int(r_max) > BLUR_R_MAX:
        raise L.PasslHipError('gaussian_blur_u8: a box radius of %d is outside the built envelope (<= %d)'
                              % (int(r_max), BLUR_R_MAX))
    out = torch.empty_like(img)
    if B:
        L.check(_lib().passl_hip_gaussian_blur_u8(L.ptr(img), L.ptr(out), L.ptr(table), B, H, W, int(r_max), L.stream()),
                'gaussian_blur_u8')
    return out


def soft_ce_fwd(scores, target):
    """scores, target fp32 [N,C] -> out[3] = (loss, acc1 %, acc5 % against argmax target), lse [N], tsum [N]."""
    assert scores.shape == target.shape and target.dtype == torch.float32
    N, Cc = scores.shape
    lse = torch.empty(N, dtype=torch.float32, device=scores.device)
    tsum = torch.empty(N, dtype=torch.float32, device=scores.device)
    out = torch.empty(3, dtype=torch.float32, device=scores.device)
    ws = workspace.get(3 * N, scores.device)
    L.check(_lib().passl_hip_soft_ce_fwd(L.ptr(scores), L.ptr(target), N, Cc, L.ptr(lse), L.ptr(tsum), L.ptr(out),
                                         L.ptr(ws), ws.numel(), L.stream()), 'soft_ce_fwd')
    return out, lse, tsum


def soft_ce_bwd(scores, target, lse, tsum, gloss):
    N, Cc = scores.shape
    ds = torch.empty_like(scores)
    L.check(_lib().passl_hip_soft_ce_bwd(L.ptr(scores), L.ptr(target), L.ptr(lse), L.ptr(tsum), L.ptr(gloss), N, Cc,
                                         L.ptr(ds), L.stream()), 'soft_ce_bwd')
    return ds


def sigmoid_ce_targets(epsilon):
    """(t_on, t_off) of ViTCELoss: onehot * (1 - eps) + eps at the label / elsewhere, in double, rounded once."""
    if epsilon is None:
        return 1.0, 0.0
    eps = float(epsilon)
    return float(np.float32(1.0 * (1.0 - eps) + eps)), float(np.float32(eps))


def sigmoid_ce_fwd(scores, labels, t_on, t_off, rows=None):
    """scores fp32 [N,C], labels int64 [N] -> out[1] = the mean over rows of the summed binary cross entropy with
    logits.  ``rows``: an fp32 [N] buffer of the caller's that takes the place of the workspace (row i's sum / N)."""
    assert scores.dtype == torch.float32 and labels.dtype == torch.int64
    N, Cc = scores.shape
    out = torch.empty(1, dtype=torch.float32, device=scores.device)
    ws = workspace.get(N, scores.device) if rows is None else rows
    L.check(_lib().passl_hip_sigmoid_ce_fwd(L.ptr(scores), L.ptr(labels), N, Cc, t_on, t_off, L.ptr(out), L.ptr(ws),
                                            ws.numel(), L.stream()), 'sigmoid_ce_fwd')
    return out


def sigmoid_ce_bwd(scores, labels, gloss, t_on, t_off, out=None):
    N, Cc = scores.shape
    ds = torch.empty_like(scores) if out is None else out
    L.check(_lib().passl_hip_sigmoid_ce_bwd(L.ptr(scores), L.ptr(labels), L.ptr(gloss), N, Cc, t_on, t_off, L.ptr(ds),
                                            L.stream()), 'sigmoid_ce_bwd')
    return ds


def mae_loss_fwd(img, pred, mask, p, norm_pix, denom):
    B, Cc, H, W = img.shape
    loss = torch.empty(1, dtype=torch.float32, device=img.device)
    ws = workspace.get(B * ((H // p) * (W // p) + 1), img.device)
    L.check(_lib().passl_hip_mae_loss_fwd(L.ptr(img), L.ptr(pred), L.ptr(mask), L.ptr(loss), B, Cc, H, W, p,
                                          1 if norm_pix else 0, denom, L.ptr(ws), ws.numel(), L.stream()),
            'mae_loss_fwd')
    return loss


def mae_loss_bwd(img, pred, mask, gscale, p, norm_pix, denom):
    B, Cc, H, W = img.shape
    dpred = torch.empty_like(pred)
    L.check(_lib().passl_hip_mae_loss_bwd(L.ptr(img), L.ptr(pred), L.ptr(mask), L.ptr(gscale), L.ptr(dpred),
                                          B, Cc, H, W, p, 1 if norm_pix else 0, denom, L.stream()),
            'mae_loss_bwd')
    return dpred


def adamw(p, g, m, v, lr, b1, b2, eps, wd, b1pow, b2pow, grad_scale=1.0):
    L.check(_lib().passl_hip_adamw(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, b1, b2, eps, wd,
                                   b1pow, b2pow, grad_scale, L.stream()), 'adamw')


def adamw_dev(p, g, m, v, hyper, b1, b2, eps, wd, grad_scale=1.0):
    """hyper: device float32 [lr, beta1^t, beta2^t], read when the kernel runs."""
    L.check(_lib().passl_hip_adamw_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(hyper), b1, b2, eps,
                                       wd, grad_scale, L.stream()), 'adamw_dev')


def adamw_groups_table(seg_end, seg_lr_scale, seg_wd, n, device):
    """The segment table of passl_hip_adamw_groups_dev, validated HERE, once, on the host (the kernel trusts it):
    seg_end ascending exclusive end offsets in elements, every one a positive multiple of 4, the last one ``n``;
    finite multipliers; weight decays >= 0.  -> dict of device arrays (int64 / float32 / float32) + n, n_seg."""
    seg_end = [int(e) for e in seg_end]
    scales = [float(x) for x in seg_lr_scale]
    wds = [float(x) for x in seg_wd]
    if not seg_end or not len(seg_end) == len(scales) == len(wds):
        raise ValueError('adamw_groups_table: %d ends, %d multipliers, %d weight decays (equal and >= 1 wanted)'
                         % (len(seg_end), len(scales), len(wds)))
    n = int(n)
    if n % 4:
        raise ValueError('adamw_groups_table: n = %d is not a multiple of 4' % n)
    prev = 0
    for i, e in enumerate(seg_end):
        if e % 4:
            raise ValueError('adamw_groups_table: seg_end[%d] = %d is not a multiple of 4' % (i, e))
        if e <= prev:
            raise ValueError('adamw_groups_table: seg_end[%d] = %d does not ascend (previous end %d)' % (i, e, prev))
        prev = e
    if prev != n:
        raise ValueError('adamw_groups_table: the last segment ends at %d, the buffer holds %d elements' % (prev, n))
    for i, (sc, wd) in enumerate(zip(scales, wds)):
        if not math.isfinite(sc) or not math.isfinite(wd) or wd < 0:
            raise ValueError('adamw_groups_table: segment %d has multiplier %r, weight decay %r' % (i, sc, wd))
    return dict(seg_end=torch.tensor(seg_end, dtype=torch.int64, device=device),
                seg_lr_scale=torch.tensor(scales, dtype=torch.float32, device=device),
                seg_wd=torch.tensor(wds, dtype=torch.float32, device=device), n=n, n_seg=len(seg_end))


def adamw_groups_dev(p, g, m, v, table, hyper, b1, b2, eps, grad_scale=1.0):
    """AdamW with a learning-rate multiplier and a weight decay per segment (``table``: adamw_groups_table)."""
    if table['n'] != p.numel():
        raise ValueError('adamw_groups_dev: the table covers %d elements, the buffer holds %d' % (table['n'], p.numel()))
    L.check(_lib().passl_hip_adamw_groups_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(table['seg_end']),
                                              L.ptr(table['seg_lr_scale']), L.ptr(table['seg_wd']), table['n_seg'],
                                              L.ptr(hyper), b1, b2, eps, grad_scale, L.stream()), 'adamw_groups_dev')


# ---- global-norm gradient clipping (include/passl_hip.h "global-norm gradient clipping")
GRAD_CLIP_CHUNK = L.GRAD_CLIP_CHUNK


def grad_clip_plan(runs, sizes, n_sets, device):
    """The chunk tables and the CSR index of passl_hip_grad_sumsq / passl_hip_grad_clip_finalize, built and validated
    HERE, once, on the host (the kernels only keep their accesses in bounds).  ``runs``: per gradient buffer a list of
    (start, end, set) — ascending, disjoint element ranges [start, end) with offsets that are multiples of 4, each inside
    the buffer of ``sizes[b]`` elements and belonging to ONE set in [0, n_sets); what no run covers is in no norm.  Every
    run is tiled by chunks of at most GRAD_CLIP_CHUNK elements, so no chunk crosses a run.  Chunks are numbered buffer
    after buffer (``base[b]`` = the first chunk of buffer b in the one partial buffer); a set's chunks are listed in
    ascending number.  -> dict: per-buffer device tables chunk_off (int64) / chunk_len (int32), base, n_chunks; set_ptr /
    set_chunks (int32), partial (total floats), out ([n_sets, 2] = {norm, coef}); ``host``: the same tables as lists."""
    n_sets = int(n_sets)
    if n_sets <= 0 or len(runs) != len(sizes):
        raise ValueError('grad_clip_plan: %d sets, %d run lists for %d buffers' % (n_sets, len(runs), len(sizes)))
    offs, lens, sets_of = [], [], []
    for b, (rs, n) in enumerate(zip(runs, sizes)):
        n = int(n)
        if n % 4:
            raise ValueError('grad_clip_plan: buffer %d holds %d elements, not a multiple of 4' % (b, n))
        o, l, k = [], [], []
        prev = 0
        for start, end, st in rs:
            start, end, st = int(start), int(end), int(st)
            if start % 4 or end % 4 or not prev <= start < end <= n:
                raise ValueError('grad_clip_plan: buffer %d: run [%d, %d) after %d in a buffer of %d elements (ascending, '
                                 'disjoint, multiples of 4 wanted)' % (b, start, end, prev, n))
            if not 0 <= st < n_sets:
                raise ValueError('grad_clip_plan: buffer %d: run [%d, %d) names set %d of %d' % (b, start, end, st, n_sets))
            for c in range(start, end, GRAD_CLIP_CHUNK):
                o.append(c)
                l.append(min(GRAD_CLIP_CHUNK, end - c))
                k.append(st)
            prev = end
        offs.append(o)
        lens.append(l)
        sets_of.append(k)
    base, total = [], 0
    for o in offs:
        base.append(total)
        total += len(o)
    if total == 0:
        raise ValueError('grad_clip_plan: no run at all — nothing to clip')
    if total >= 2 ** 31:
        raise ValueError('grad_clip_plan: %d chunks do not fit an int32 index' % total)
    members = [[] for _ in range(n_sets)]
    for b, k in enumerate(sets_of):
        for i, st in enumerate(k):
            members[st].append(base[b] + i)
    set_ptr, set_chunks = [0], []
    for mm in members:
        set_chunks += mm
        set_ptr.append(len(set_chunks))
    assert sorted(set_chunks) == list(range(total))
    host = dict(chunk_off=offs, chunk_len=lens, chunk_set=sets_of, base=base, set_ptr=set_ptr, set_chunks=set_chunks)
    return dict(chunk_off=[torch.tensor(o, dtype=torch.int64, device=device) for o in offs],
                chunk_len=[torch.tensor(l, dtype=torch.int32, device=device) for l in lens],
                base=base, n_chunks=[len(o) for o in offs], sizes=[int(n) for n in sizes], total=total,
                set_ptr=torch.tensor(set_ptr, dtype=torch.int32, device=device),
                set_chunks=torch.tensor(set_chunks, dtype=torch.int32, device=device), n_sets=n_sets,
                partial=torch.zeros(total, dtype=torch.float32, device=device),
                out=torch.zeros(n_sets, 2, dtype=torch.float32, device=device), host=host)


def grad_sumsq(g, plan, b, grad_scale=1.0):
    """partial[base[b] + c] = sum of fp32(g*grad_scale)^2 over chunk c of gradient buffer b (nothing to do for a buffer
    without chunks)."""
    if plan['sizes'][b] != g.numel():
        raise ValueError('grad_sumsq: the plan covers %d elements of buffer %d, it holds %d' % (plan['sizes'][b], b, g.numel()))
    nc = plan['n_chunks'][b]
    if nc == 0:
        return
    L.check(_lib().passl_hip_grad_sumsq(L.ptr(g), g.numel(), L.ptr(plan['chunk_off'][b]), L.ptr(plan['chunk_len'][b]), nc,
                                        grad_scale, L.ptr(plan['partial'][plan['base'][b]:]), L.stream()), 'grad_sumsq')


def grad_clip_finalize(plan, clip_norm, clip_norm_max=None, always_clip=False):
    """plan['out'][s] = {norm, coef} of every set from the partials, by the rule of ClipGradByGlobalNorm."""
    L.check(_lib().passl_hip_grad_clip_finalize(L.ptr(plan['partial']), plan['total'], L.ptr(plan['set_ptr']),
                                                L.ptr(plan['set_chunks']), plan['total'], plan['n_sets'], clip_norm,
                                                float('inf') if clip_norm_max is None else clip_norm_max,
                                                1 if always_clip else 0, L.ptr(plan['out']), L.stream()),
            'grad_clip_finalize')
    return plan['out']


def adamw_clip_dev(p, g, m, v, hyper, coef, b1, b2, eps, wd, grad_scale=1.0):
    """adamw_dev with the gradient times coef[0] (a device float, e.g. plan['out'][s, 1:]): gg = (g*grad_scale)*coef."""
    L.check(_lib().passl_hip_adamw_clip_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(hyper), L.ptr(coef),
                                            b1, b2, eps, wd, grad_scale, L.stream()), 'adamw_clip_dev')


def adamw_groups_clip_table(seg_end, seg_lr_scale, seg_wd, seg_set, n, n_sets, device):
    """adamw_groups_table + the set of every segment (-1: not clipped), validated on the host."""
    sets = [int(x) for x in seg_set]
    if len(sets) != len(seg_end):
        raise ValueError('adamw_groups_clip_table: %d ends, %d sets' % (len(seg_end), len(sets)))
    for i, st in enumerate(sets):
        if not -1 <= st < int(n_sets):
            raise ValueError('adamw_groups_clip_table: segment %d names set %d of %d (-1: not clipped)' % (i, st, n_sets))
    table = adamw_groups_table(seg_end, seg_lr_scale, seg_wd, n, device)
    table['seg_set'] = torch.tensor(sets, dtype=torch.int32, device=device)
    table['n_sets'] = int(n_sets)
    return table


def adamw_groups_clip_dev(p, g, m, v, table, hyper, clip, b1, b2, eps, grad_scale=1.0):
    """adamw_groups_dev with the gradient of segment s times clip[seg_set[s], 1] (``clip``: the [n_sets, 2] table of
    grad_clip_finalize; ``table``: adamw_groups_clip_table)."""
    if table['n'] != p.numel():
        raise ValueError('adamw_groups_clip_dev: the table covers %d elements, the buffer holds %d' % (table['n'], p.numel()))
    if clip.numel() != 2 * table['n_sets']:
        raise ValueError('adamw_groups_clip_dev: the table names %d sets, the coefficient table holds %d'
                         % (table['n_sets'], clip.numel() // 2))
    L.check(_lib().passl_hip_adamw_groups_clip_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(),
                                                   L.ptr(table['seg_end']), L.ptr(table['seg_lr_scale']),
                                                   L.ptr(table['seg_wd']), L.ptr(table['seg_set']), table['n_seg'],
                                                   L.ptr(hyper), L.ptr(clip), table['n_sets'], b1, b2, eps, grad_scale,
                                                   L.stream()), 'adamw_groups_clip_dev')


# ---- Adan (include/passl_hip.h "Adan (flat buffer)"): p, m, d, s, pre from g; the tables are AdamW's
ADAN_HYPER = 8      # floats of the device block {lr, b1^t, b2^t, b3^t, first, 0, 0, 0}


def _adan_args(what, bufs, hyper, table=None):
    """The six buffers hold the same number of elements and the hyper block its eight floats (the kernel reads
    hyper[4]); a table covers exactly the buffer.  -> the device pointers of the buffers."""
    n = bufs[0].numel()
    if any(b.numel() != n for b in bufs):
        raise ValueError('%s: buffers of %r elements (equal sizes wanted)' % (what, [b.numel() for b in bufs]))
    if hyper.numel() < ADAN_HYPER:
        raise ValueError('%s: the hyper block holds %d floats, %d wanted' % (what, hyper.numel(), ADAN_HYPER))
    if table is not None and table['n'] != n:
        raise ValueError('%s: the table covers %d elements, the buffer holds %d' % (what, table['n'], n))
    return [L.ptr(b) for b in bufs]


def adan_dev(p, g, m, d, s, pre, hyper, b1, b2, b3, eps, wd, no_prox=False, grad_scale=1.0):
    """hyper: device float32 [lr, b1^t, b2^t, b3^t, first, 0, 0, 0], read when the kernel runs."""
    ptrs = _adan_args('adan_dev', (p, g, m, d, s, pre), hyper)
    L.check(_lib().passl_hip_adan_dev(*ptrs, p.numel(), L.ptr(hyper), b1, b2, b3, eps, wd, 1 if no_prox else 0,
                                      grad_scale, L.stream()), 'adan_dev')


def adan_clip_dev(p, g, m, d, s, pre, hyper, coef, b1, b2, b3, eps, wd, no_prox=False, grad_scale=1.0):
    """adan_dev with the gradient times coef[0] (a device float, e.g. plan['out'][s, 1:]): gg = (g*grad_scale)*coef."""
    ptrs = _adan_args('adan_clip_dev', (p, g, m, d, s, pre), hyper)
    L.check(_lib().passl_hip_adan_clip_dev(*ptrs, p.numel(), L.ptr(hyper), L.ptr(coef), b1, b2, b3, eps, wd,
                                           1 if no_prox else 0, grad_scale, L.stream()), 'adan_clip_dev')


def adan_groups_dev(p, g, m, d, s, pre, table, hyper, b1, b2, b3, eps, no_prox=False, grad_scale=1.0):
    """Adan with a learning-rate multiplier and a weight decay per segment (``table``: adamw_groups_table)."""
    ptrs = _adan_args('adan_groups_dev', (p, g, m, d, s, pre), hyper, table)
    L.check(_lib().passl_hip_adan_groups_dev(*ptrs, p.numel(), L.ptr(table['seg_end']), L.ptr(table['seg_lr_scale']),
                                             L.ptr(table['seg_wd']), table['n_seg'], L.ptr(hyper), b1, b2, b3, eps,
                                             1 if no_prox else 0, grad_scale, L.stream()), 'adan_groups_dev')


def adan_groups_clip_dev(p, g, m, d, s, pre, table, hyper, clip, b1, b2, b3, eps, no_prox=False, grad_scale=1.0):
    """adan_groups_dev with the gradient of segment s times clip[seg_set[s], 1] (``clip``: the [n_sets, 2] table of
    grad_clip_finalize; ``table``: adamw_groups_clip_table)."""
    if clip.numel() != 2 * table['n_sets']:
        raise ValueError('adan_groups_clip_dev: the table names %d sets, the coefficient table holds %d'
                         % (table['n_sets'], clip.numel() // 2))
    ptrs = _adan_args('adan_groups_clip_dev', (p, g, m, d, s, pre), hyper, table)
    L.check(_lib().passl_hip_adan_groups_clip_dev(*ptrs, p.numel(), L.ptr(table['seg_end']),
                                                  L.ptr(table['seg_lr_scale']), L.ptr(table['seg_wd']),
                                                  L.ptr(table['seg_set']), table['n_seg'], L.ptr(hyper), L.ptr(clip),
                                                  table['n_sets'], b1, b2, b3, eps, 1 if no_prox else 0, grad_scale,
                                                  L.stream()), 'adan_groups_clip_dev')


# ------------------------------------------------------------------ CLIP
def quick_gelu_fwd(x):
    return _unary('quick_gelu_fwd', x)


def quick_gelu_bwd(dy, x):
    return _unary('quick_gelu_bwd', x, dy)


def embed_fwd(text, table, pos, dtype):
    """text int64 [B,T]; table fp32 [V,C]; pos fp32 [T,C] -> [B*T, C] in `dtype`."""
    B, T = text.shape
    V, Cc = table.shape
    out = torch.empty(B * T, Cc, dtype=dtype, device=table.device)
    L.check(_lib().passl_hip_embed_fwd(L.ptr(text), L.ptr(table), L.ptr(pos), L.ptr(out), B, T, Cc, V,
                                       L.dt(out), L.stream()), 'embed_fwd')
    return out


_embed_acc = {}


def embed_bwd(text, dout, dtable, dpos):
    """dtable[text] += dout (exact fixed-point scatter-add), dpos += sum_b dout: see include/passl_hip.h."""
    B, T = text.shape
    V, Cc = dtable.shape
    lib = _lib()
    # the persistent accumulator of the fixed-point scatter: zero once, every call leaves it zero
    key = (dout.device.type, dout.device.index, V, Cc)
    acc = _embed_acc.get(key)
    if acc is None:
        acc = torch.zeros(int(lib.passl_hip_embed_bwd_acc_bytes(V, Cc)) // 8, dtype=torch.int64, device=dout.device)
        _embed_acc[key] = acc
    ws = workspace.get(int(lib.passl_hip_embed_bwd_ws_floats(B, T, Cc)), dout.device)
    L.check(lib.passl_hip_embed_bwd(L.ptr(text), L.ptr(dout), L.ptr(dtable), L.ptr(dpos), B, T, Cc, V,
                                    L.dt(dout), L.ptr(acc), acc.numel() * 8, L.ptr(ws), ws.numel(), L.stream()),
            'embed_bwd')


def gather_rows(x, idx):
    n, Cc = idx.numel(), x.shape[-1]
    out = torch.empty(n, Cc, dtype=x.dtype, device=x.device)
    L.check(_lib().passl_hip_gather_rows(L.ptr(x), L.ptr(idx), L.ptr(out), n, Cc, L.dt(x), L.stream()),
            'gather_rows')
    return out


def scatter_rows(dout, idx, rows_total):
    n, Cc = dout.shape
    dx = torch.empty(rows_total, Cc, dtype=dout.dtype, device=dout.device)
    L.check(_lib().passl_hip_scatter_rows(L.ptr(dout), L.ptr(idx), L.ptr(dx), n, rows_total, Cc, L.dt(dout),
                                          L.stream()), 'scatter_rows')
    return dx


def eot_index(text):
    B, T = text.shape
    idx = torch.empty(B, dtype=torch.int32, device=text.device)
    L.check(_lib().passl_hip_eot_index(L.ptr(text), B, T, L.ptr(idx), L.stream()), 'eot_index')
    return idx


def clip_logits_fwd(img, txt, logit_scale, clip_lo=-4.6, clip_hi=4.6):
    """-> logits [B,B] (= image_logits; text_logits is its transpose), ws (workspace for the backward).
    logit_scale (the fp32 parameter) is clipped in place after use."""
    B, Dd = img.shape
    ws = torch.empty(int(_lib().passl_hip_clip_logits_ws_floats(B, Dd)), dtype=torch.float32, device=img.device)
    logits = torch.empty(B, B, dtype=torch.float32, device=img.device)
    L.check(_lib().passl_hip_clip_logits_fwd(L.ptr(img), L.ptr(txt), L.ptr(logit_scale), B, Dd, clip_lo,
                                             clip_hi, L.ptr(ws), L.ptr(logits), L.stream()), 'clip_logits_fwd')
    return logits, ws


def clip_logits_bwd(dlogits, logits, ws, Dd, dlogit_scale):
    B = logits.shape[0]
    dimg = torch.empty(B, Dd, dtype=torch.float32, device=ws.device)
    dtxt = torch.empty(B, Dd, dtype=torch.float32, device=ws.device)
    scratch = workspace.get(256, ws.device)
    L.check(_lib().passl_hip_clip_logits_bwd(L.ptr(dlogits), L.ptr(logits), L.ptr(ws), B, Dd, L.ptr(dimg),
                                             L.ptr(dtxt), L.ptr(dlogit_scale), L.ptr(scratch), L.stream()),
            'clip_logits_bwd')
    return dimg, dtxt


def clip_scale(logit_scale, clip_lo=-4.6, clip_hi=4.6):
    """-> alpha (device scalar) = exp(logit_scale) as used by this step; logit_scale is clipped in place."""
    alpha = torch.empty(1, dtype=torch.float32, device=logit_scale.device)
    L.check(_lib().passl_hip_clip_scale(L.ptr(logit_scale), L.ptr(alpha), clip_lo, clip_hi, L.stream()), 'clip_scale')
    return alpha


def gemm_f32_nt(a, b, alpha):
    """alpha * a [M,K] @ b[N,K]^T -> [M,N] fp32 (exact-fp32 MFMA)."""
    M, K = a.shape
    N = b.shape[0]
    c = torch.empty(M, N, dtype=torch.float32, device=a.device)
    L.check(_lib().passl_hip_gemm_f32_nt(L.ptr(a), L.ptr(b), L.ptr(c), M, N, K, L.ptr(alpha), L.stream()), 'gemm_f32_nt')
    return c


def gemm_f32_gx(g, x, alpha, trans=False):
    """alpha * op(g) @ x[K,N]: op(g) = g [M,K] or (trans) g^T with g [K,M]."""
    K, N = x.shape
    M = g.shape[1] if trans else g.shape[0]
    c = torch.empty(M, N, dtype=torch.float32, device=x.device)
    L.check(_lib().passl_hip_gemm_f32_gx(L.ptr(g), L.ptr(x), L.ptr(c), M, N, K, 1 if trans else 0, L.ptr(alpha),
                                         L.stream()), 'gemm_f32_gx')
    return c


def dot_acc(a, b, out):
    """out[0] += sum(a * b), fixed summation order."""
    ws = workspace.get(256, a.device)
    L.check(_lib().passl_hip_dot_acc(L.ptr(a), L.ptr(b), a.numel(), L.ptr(out), L.ptr(ws), L.stream()), 'dot_acc')


def clip_ce_fwd(logits):
    """-> out[3] = (img_loss, text_loss, loss), lse [2B]."""
    B = logits.shape[0]
    lse = torch.empty(2 * B, dtype=torch.float32, device=logits.device)
    out = torch.empty(3, dtype=torch.float32, device=logits.device)
    ws = workspace.get(2 * B, logits.device)
    L.check(_lib().passl_hip_clip_ce_fwd(L.ptr(logits), B, L.ptr(lse), L.ptr(out), L.ptr(ws), ws.numel(),
                                         L.stream()), 'clip_ce_fwd')
    return out, lse


def clip_ce_bwd(logits, lse, gloss):
    dlogits = torch.empty_like(logits)
    L.check(_lib().passl_hip_clip_ce_bwd(L.ptr(logits), L.ptr(lse), L.ptr(gloss), logits.shape[0],
                                         L.ptr(dlogits), L.stream()), 'clip_ce_bwd')
    return dlogits


# ------------------------------------------------------------------ linear probe
def softmax_ce_fwd(scores, labels):
    """scores fp32 [N,C], labels int64 [N] -> out[3] = (loss, acc1 %, acc5 %), lse [N]."""
    N, Cc = scores.shape
    lse = torch.empty(N, dtype=torch.float32, device=scores.device)
    out = torch.empty(3, dtype=torch.float32, device=scores.device)
    ws = workspace.get(3 * N, scores.device)
    L.check(_lib().passl_hip_softmax_ce_fwd(L.ptr(scores), L.ptr(labels), N, Cc, L.ptr(lse), L.ptr(out),
                                            L.ptr(ws), ws.numel(), L.stream()), 'softmax_ce_fwd')
    return out, lse


def softmax_ce_bwd(scores, lse, labels, gloss):
    N, Cc = scores.shape
    ds = torch.empty_like(scores)
    L.check(_lib().passl_hip_softmax_ce_bwd(L.ptr(scores), L.ptr(lse), L.ptr(labels), L.ptr(gloss), N, Cc,
                                            L.ptr(ds), L.stream()), 'softmax_ce_bwd')
    return ds
