"""CPU helpers of the Swin tests (pure torch / numpy, no GPU, no kernel code).

Window attention is restated here the way the reference runs it (passl/models/swin_transformer.py:112-200, :291-340):
a literal ``roll`` of the map, ``window_partition``, the ``img_mask`` construction of the -100 mask, the
``relative_position_index`` gather of the bias, softmax, and ``window_reverse`` + ``roll`` back, in float64 with the
closed-form backward.  The kernels' closed forms (row addressing, region labels, bias index; include/passl_hip.h)
are stated separately in ``closed_*`` so that the host test can compare the two.

Layouts are the kernels': qkv [B, Hp*Wp, 3, nH, DH], out / dout / dq / dk / dv [B, Hp*Wp, nH, DH] in the order of the
unshifted, unpartitioned tokens, table [(2 ws - 1)^2, nH], lse [B * nW, nH, T].

reference        float64 (or float32 "eager") forward, backward and the component-wise bounds, P including bias and mask:
                 b_out = P |v|, b_dv = P^T |dO|, b_dq = a scale |k|, b_dk = a^T scale |q|,
                 a = P (|dP| + sum_d |dO_d| b_out_d), b_dtable = the per-bin sum of a
rounding_model   the same with bf16 roundings where the bf16-MFMA kernels round, optionally with a planted defect
"""
import functools

import numpy as np
import torch

import attention_util as A

CASES = ((2, 7, 7, 7, 0, 1, 32),        # one window, T = 49 ends inside a tile
         (1, 14, 14, 7, 3, 3, 32),      # all four window kinds of a shifted map, nH not a power of two
         (2, 8, 12, 4, 2, 2, 32),       # non-square map, T = 16 exactly one tile
         (1, 6, 6, 3, 1, 2, 64),        # T = 9 below one tile, DH = 64
         (1, 24, 24, 12, 6, 1, 32),     # T = 144, shifted
         (1, 14, 28, 14, 0, 1, 32),     # T = 196, the largest
         (8, 28, 28, 7, 3, 3, 32))      # more windows than table-gradient slabs
KINDS = ('plain', 'peaked', 'vmean')
TABLE_STD = (1.0, 8.0)
DEFECTS = ('mask_no_shift', 'bias_transposed', 'roll_wrong_way', 'dtable_rounded')
LIMIT_BF16 = dict(A.LIMIT_BF16, dtable=1.25 * A.U)
TENSORS = ('out', 'dq', 'dk', 'dv', 'dtable')


def case_id(case):
    return 'B%d-%dx%d-ws%d-s%d-h%d-d%d' % case


# ------------------------------------------------------------------ the reference's constructions, literally
def window_partition(x, ws):
    B, H, W, C = x.shape
    x = x.reshape(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, C)


def window_reverse(windows, ws, H, W):
    C = windows.shape[-1]
    x = windows.reshape(-1, H // ws, W // ws, ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).reshape(-1, H, W, C)


def relative_position_index(ws):
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing='ij'))
    flat = coords.flatten(1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)                                           # [T, T]


def attn_mask(Hp, Wp, ws, shift, unroll=False):
    """[nW, T, T] of 0 / -100 (zeros for shift 0, where the reference keeps no mask).  unroll: a planted defect, the
    region labels stay with the positions of the unshifted map."""
    T = ws * ws
    if shift == 0:
        return torch.zeros((Hp // ws) * (Wp // ws), T, T, dtype=torch.float64)
    img = torch.zeros(1, Hp, Wp, 1, dtype=torch.float64)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, hs, wsl, :] = cnt
            cnt += 1
    if unroll:
        img = torch.roll(img, shifts=(shift, shift), dims=(1, 2))
    mw = window_partition(img, ws).reshape(-1, T)
    m = mw[:, None, :] - mw[:, :, None]
    return torch.where(m != 0, torch.full_like(m, -100.0), torch.zeros_like(m))


# ------------------------------------------------------------------ the kernels' closed forms
def closed_rows(Hp, Wp, ws, shift):
    """[nW, T]: row of token i of window w in its image."""
    nWx = Wp // ws
    out = np.zeros(((Hp // ws) * nWx, ws * ws), dtype=np.int64)
    for w in range(out.shape[0]):
        wy, wx = divmod(w, nWx)
        for t in range(ws * ws):
            iy, ix = divmod(t, ws)
            out[w, t] = ((wy * ws + iy + shift) % Hp) * Wp + (wx * ws + ix + shift) % Wp
    return out


def closed_labels(Hp, Wp, ws, shift):
    def r(y, n):
        return 0 if y < n - ws else (1 if y < n - shift else 2)
    nWx = Wp // ws
    out = np.zeros(((Hp // ws) * nWx, ws * ws), dtype=np.int64)
    for w in range(out.shape[0]):
        wy, wx = divmod(w, nWx)
        for t in range(ws * ws):
            iy, ix = divmod(t, ws)
            out[w, t] = 3 * r(wy * ws + iy, Hp) + r(wx * ws + ix, Wp)
    return out


def closed_mask(Hp, Wp, ws, shift):
    T = ws * ws
    if shift == 0:
        return np.zeros(((Hp // ws) * (Wp // ws), T, T))
    lab = closed_labels(Hp, Wp, ws, shift)
    return np.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)


def closed_index(ws):
    t = np.arange(ws * ws)
    iy, ix = t // ws, t % ws
    return (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)


# ------------------------------------------------------------------ inputs
def make_inputs(case, kind, table_std, seed):
    """qkv [B, L, 3, nH, DH], dout [B, L, nH, DH] (fp32 holding bf16 values, attention_util.make_inputs with the
    image's tokens as the sequence) and table fp32 [(2 ws - 1)^2, nH] ~ N(0, table_std^2)."""
    B, Hp, Wp, ws, shift, nH, DH = case
    qkv, dout = A.make_inputs(kind, B, Hp * Wp, nH, DH, seed, peak_gain=A.PEAK_GAIN_CAUSAL)
    gen = torch.Generator().manual_seed(seed + 7)
    table = (torch.randn((2 * ws - 1) ** 2, nH, generator=gen) * table_std).float()
    return qkv, dout, table


ONE_PAIR_CASE = (1, 2, 2, 2, 0, 1, 32)          # one 2 x 2 window, one head: a corner bin of the table holds ONE pair


def one_pair_inputs():
    """An input on which both roundings that can reach dtable come close to their worst case, u each, with one sign.

    The 1.25 u limit of dtable allows u a for the rounded O in delta plus 0.25 u; a dS rounded to bf16 adds up to
    u |dS| <= u a per pair.  Random errors of many pairs do not add up to that (on the kernel cases, every input kind,
    both table deviations, the defective gradient uses 0.09 - 0.57 of the allowance), so the defect is shown where
    nothing averages: bin (dy, dx) = (1, 1) of a single 2 x 2 window holds the one pair (i, j) = (3, 0).
      q = k = 0, table = 0          P = 1/4 exactly, nothing rounds in the forward but O
      v_0 = 0, v_1..3 = 174/128     O_d = 0.75 * 174/128 = 1 + 10/512: a tie between 1 + 8/512 and 1 + 12/512, rounded to
                                    even, DOWN by 2/512 = 0.98 u;  dP_30 = dO_3 . v_0 = 0, so dS_30 = -P delta and
                                    |dS_30| = a_30 = P sum_d |dO_d| b_out_d: the pair's whole bound is the delta term
      dO = 255/128 everywhere       8 * 255/128 * 1.015625 = 16.187...: bf16 spacing 1/8 there, rounded DOWN to 16.125,
                                    another 0.97 u below (of 128 gradient values 1 + k/128 this one loses most)
    The fp32-dS gradient is then 0.98 u a from the reference (0.78 of the allowance), the rounded-dS one 1.95 u a."""
    qkv = torch.zeros(1, 4, 3, 1, 32)
    qkv[:, 1:, 2] = 174.0 / 128
    return qkv, torch.full((1, 4, 1, 32), 255.0 / 128), torch.zeros(9, 1), 32 ** -0.5


# ------------------------------------------------------------------ reference
def _to_windows(x, B, Hp, Wp, ws, shift, roll_sign=-1):
    """[B, L, ...] -> [B * nW, T, ...] by the reference's roll and window_partition."""
    tail = x.shape[2:]
    x = x.reshape(B, Hp, Wp, -1)
    if shift > 0:
        x = torch.roll(x, shifts=(roll_sign * shift, roll_sign * shift), dims=(1, 2))
    return window_partition(x, ws).reshape((-1, ws * ws) + tuple(tail))


def _from_windows(x, B, Hp, Wp, ws, shift, roll_sign=1):
    """[B * nW, T, ...] -> [B, L, ...] by window_reverse and the roll back."""
    tail = x.shape[2:]
    x = window_reverse(x.reshape(x.shape[0], ws, ws, -1), ws, Hp, Wp)
    if shift > 0:
        x = torch.roll(x, shifts=(roll_sign * shift, roll_sign * shift), dims=(1, 2))
    return x.reshape((B, Hp * Wp) + tuple(tail))


def _bins(x, index, nbins):
    """[BW, nH, T, T] -> [nbins, nH]: sum over windows, then over the pairs of a bin."""
    nH, T = x.shape[1], x.shape[2]
    flat = x.sum(0).reshape(nH, T * T).t().contiguous()
    return torch.zeros(nbins, nH, dtype=x.dtype).index_add_(0, index.reshape(-1), flat)


def reference(case, qkv, dout, table, scale, dtype=torch.float64, model=False, defect=None):
    """dict of out, dq, dk, dv [B, L, nH, DH], dtable [(2 ws - 1)^2, nH], lse [B * nW, nH, T] and (model False) the
    bounds b_*.  model=True rounds to bf16 where the bf16-MFMA kernels do: P as the operand of P V and P^T dO, the
    stored O, dS scale as the operand of dS K and dS^T Q, the stored dq / dk / dv; the table's gradient is the sum of
    the unrounded dS.  `defect` plants one bug into the model."""
    assert defect is None or defect in DEFECTS
    B, Hp, Wp, ws, shift, nH, DH = case
    T, nW = ws * ws, (Hp // ws) * (Wp // ws)
    rnd = A.bf16_round if model else (lambda x: x)
    win = _to_windows(qkv.to(dtype), B, Hp, Wp, ws, shift)                       # [BW, T, 3, nH, DH]
    q, k, v = [win[:, :, i].permute(0, 2, 1, 3) for i in range(3)]              # [BW, nH, T, DH]
    do = _to_windows(dout.to(dtype), B, Hp, Wp, ws, shift).permute(0, 2, 1, 3)
    index = relative_position_index(ws)
    if defect == 'bias_transposed':
        index = index.t().contiguous()
    bias = table.to(dtype)[index.reshape(-1)].reshape(T, T, nH).permute(2, 0, 1)
    mask = attn_mask(Hp, Wp, ws, shift, unroll=defect == 'mask_no_shift').to(dtype)
    s = (q @ k.transpose(-1, -2)) * scale + bias.unsqueeze(0)
    s = (s.reshape(B, nW, nH, T, T) + mask[None, :, None]).reshape(B * nW, nH, T, T)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = rnd(rnd(p) @ v)
    dp = do @ v.transpose(-1, -2)
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (dp - delta)                                                        # unscaled: the table's gradient
    dss = rnd(ds * scale)
    back = functools.partial(_from_windows, B=B, Hp=Hp, Wp=Wp, ws=ws, shift=shift,
                             roll_sign=-1 if defect == 'roll_wrong_way' else 1)
    tok = lambda x: back(x.permute(0, 2, 1, 3))                                  # noqa: E731
    nb = (2 * ws - 1) ** 2
    r = {'out': tok(out), 'dq': tok(rnd(dss @ k)), 'dk': tok(rnd(dss.transpose(-1, -2) @ q)),
         'dv': tok(rnd(rnd(p).transpose(-1, -2) @ do)),
         'dtable': _bins(A.bf16_round(ds) if defect == 'dtable_rounded' else ds, relative_position_index(ws), nb),
         'lse': lse}
    if not model:
        b_out = p @ v.abs()
        a = p * (dp.abs() + (do.abs() * b_out).sum(-1, keepdim=True))
        r.update({'b_out': tok(b_out), 'b_dq': tok((a * scale) @ k.abs()),
                  'b_dk': tok((a * scale).transpose(-1, -2) @ q.abs()), 'b_dv': tok(p.transpose(-1, -2) @ do.abs()),
                  'b_dtable': _bins(a, relative_position_index(ws), nb)})
    return r


@functools.lru_cache(maxsize=None)
def case_data(case, kind, table_std):
    """Inputs, float64 reference and float32 eager result of a case; computed once and shared (read-only)."""
    seed = 100000 + 1000 * CASES.index(case) + 10 * KINDS.index(kind) + TABLE_STD.index(table_std)
    qkv, dout, table = make_inputs(case, kind, table_std, seed)
    scale = case[6] ** -0.5
    return {'qkv': qkv, 'dout': dout, 'table': table, 'scale': scale,
            'ref': reference(case, qkv, dout, table, scale),
            'eager': reference(case, qkv, dout, table, scale, dtype=torch.float32)}


def limit_usage(got, ref, bound, limit):
    """attention_util.limit_usage for a tensor of any rank: (worst share of the allowance used, its flat index)."""
    return A.limit_usage(got, ref, bound, limit)


def describe(name, got, ref, bound, idx):
    g, r, b = got.double().flatten()[idx], ref.double().flatten()[idx], bound.double().flatten()[idx]
    where = tuple(int(x) for x in torch.unravel_index(torch.as_tensor(idx), ref.shape))
    return '%s at %s: got %.9g, reference %.9g, bound %.6g, |diff| / bound = %.4g' % (
        name, where, g, r, b, abs(g - r) / (b + A.TINY))
