"""Float64 restatement, component-wise bounds, rounding model and inputs for the CaiT attention kernels
(csrc/cait_attention.hip), shared by tests/test_cait_host.py and tests/test_cait_attention_gpu.py.  Pure torch-CPU.

Talking heads, per image (cait.py:163-185; w[h, g] is a Paddle Linear weight, [in, out]):
    S_h = scale q_h k_h^T     A_g = sum_h S_h wl[h, g] + bl[g]     P_g = softmax_j A_g
    R_g = sum_h P_h ww[h, g] + bw[g]     O_g = R_g v_g
backward, with dR_g = dO_g v_g^T:
    dv_g = R_g^T dO_g     dww[h, g] = sum P_h dR_g     dbw[g] = sum dR_g     dP_h = sum_g dR_g ww[h, g]
    delta_h[i] = sum_j P_h dP_h     dA_h = P_h (dP_h - delta_h)     dwl[h, g] = sum S_h dA_g     dbl[g] = sum dA_g
    dS_h = sum_g dA_g wl[h, g]     dq_h = scale dS_h k_h     dk_h = scale dS_h^T q_h
dbl is analytically zero (every row of dA sums to 0); it is held to its bound like any other tensor.

Bounds: every product replaced by the product of absolute values, e.g. b_out = (P |ww| + |bw|) |v| and
b_dA = P (|dP| + sum_j P |dP|) with |dP| = sum_g (|dO| |v|^T)_g |ww[h, g]|.

Rounding model: the kernels compute in fp32 from the stored values in both dtypes; the bf16 path rounds only what it
stores.  So the model is the restatement with out, dq, dk, dv rounded to bf16 once, and the a-priori limit of each of
the four is ONE rounding, 1 u of the bound, plus 0.25 u slack for the fp32 accumulation order and the fast exp
(attention_util.LIMIT_BF16 counts the same way).  lse and the four small gradients are fp32 and never rounded to bf16:
0.25 u.  Class attention: the same, out / dq / dk / dv one rounding each.

Planted defects (in the rounding model; the kernels are not involved):
    mix_transposed   wl[g, h] used for wl[h, g]
    bias_w_dropped   bw left out
    pad_key          at T no multiple of 16, one padded key with S = 0 (so A = bl[g]) takes part in the softmax
    delta_plain      delta = dO . O, the plain attention's identity, which the second mix breaks
"""
import torch

import attention_util as A

U = A.U
DH = 48
KINDS = ('plain', 'peaked', 'vmean')
DEVS = (0.25, 1.0)
PEAK_GAIN = 3.5
# (B, T, H) at DH = 48: one token, fewer tokens than a tile, one more than a tile, H = 8 with three tiles, the recipe's
# trunk shapes (13 row blocks, 4 key chunks), the largest T
CASES = [(2, 1, 2), (2, 5, 4), (2, 17, 3), (1, 33, 8), (2, 196, 4), (1, 196, 8), (1, 208, 8)]
CLS_CASES = [(2, T, H) for T in (1, 5, 17, 197, 208) for H in (2, 3, 8)]
TENSORS = ('out', 'dq', 'dk', 'dv', 'dwl', 'dbl', 'dww', 'dbw')
BIG = ('out', 'dq', 'dk', 'dv')
LIMIT_BF16 = {'out': 1.25 * U, 'dq': 1.25 * U, 'dk': 1.25 * U, 'dv': 1.25 * U,
              'dwl': 0.25 * U, 'dbl': 0.25 * U, 'dww': 0.25 * U, 'dbw': 0.25 * U}
CLS_TENSORS = ('out', 'dq', 'dk', 'dv')
CLS_LIMIT_BF16 = {n: 1.25 * U for n in CLS_TENSORS}
CLS_UNDERFLOW_CAP = 0.02     # share of a class-attention tensor whose bound may lie below 2^-100 (test_cait_host.py)
DEFECTS = ('mix_transposed', 'bias_w_dropped', 'pad_key', 'delta_plain')
FP32_FLOOR = 16 * 2.0 ** -24


def case_id(case):
    return 'B%dT%dH%d' % tuple(case)


def make_mix(H, dev, seed):
    """wl, bl, ww, bw fp32: identity plus dev * randn / sqrt(H); bl = dev * randn; bw = 0.1 * dev * randn."""
    gen = torch.Generator().manual_seed(seed)
    wl = torch.eye(H) + dev * torch.randn(H, H, generator=gen) / H ** 0.5
    ww = torch.eye(H) + dev * torch.randn(H, H, generator=gen) / H ** 0.5
    return wl, dev * torch.randn(H, generator=gen), ww, 0.1 * dev * torch.randn(H, generator=gen)


def make_case(case, kind, dev):
    """-> dict(qkv [B, T, 3, H, DH], dout [B, T, H, DH] (fp32 holding bf16 values), wl, bl, ww, bw, scale)."""
    B, T, H = case
    seed = 1000 * T + 10 * H + KINDS.index(kind)
    qkv, dout = A.make_inputs(kind, B, T, H, DH, seed, peak_gain=PEAK_GAIN)
    wl, bl, ww, bw = make_mix(H, dev, seed + 7)
    return dict(qkv=qkv, dout=dout, wl=wl, bl=bl, ww=ww, bw=bw, scale=DH ** -0.5)


def _mix(x, w):
    return torch.einsum('bhij,hg->bgij', x, w)


def _mix_t(x, w):
    return torch.einsum('bgij,hg->bhij', x, w)


def reference(d, dtype=torch.float64, round_out=False, defect=None):
    """The restatement in `dtype` with its bounds (keys b_<tensor>).  round_out: the rounding model (out, dq, dk, dv
    rounded to bf16).  defect: see the module docstring."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = A._heads(d['qkv'], d['dout'], dtype)                           # [B, H, T, DH]
    wl, bl, ww, bw = [d[n].to(dtype) for n in ('wl', 'bl', 'ww', 'bw')]
    scale, T = d['scale'], q.shape[2]
    col = lambda b: b.view(1, -1, 1, 1)                                          # noqa: E731
    S = (q @ k.transpose(-1, -2)) * scale
    Am = _mix(S, wl.t() if defect == 'mix_transposed' else wl) + col(bl)
    m = Am.max(-1, keepdim=True).values
    if defect == 'pad_key' and T % 16:
        m = torch.maximum(m, col(bl).expand_as(m))
    e = torch.exp(Am - m)
    z = e.sum(-1, keepdim=True)
    if defect == 'pad_key' and T % 16:
        z = z + torch.exp(col(bl) - m)
    lse = (m + torch.log(z)).squeeze(-1)
    P = e / z
    bw_f = torch.zeros_like(bw) if defect == 'bias_w_dropped' else bw
    R = _mix(P, ww) + col(bw_f)
    out = R @ v
    dR = do @ v.transpose(-1, -2)
    dP = _mix_t(dR, ww)
    if defect == 'delta_plain':
        delta = (do * out).sum(-1, keepdim=True)
    else:
        delta = (P * dP).sum(-1, keepdim=True)
    dA = P * (dP - delta)
    dS = _mix_t(dA, wl)
    r = {'out': out, 'dq': scale * (dS @ k), 'dk': scale * (dS.transpose(-1, -2) @ q), 'dv': R.transpose(-1, -2) @ do}
    # bounds
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    b_R = _mix(P, ww.abs()) + col(bw.abs())
    b_dR = ado @ av.transpose(-1, -2)
    b_dP = _mix_t(b_dR, ww.abs())
    b_dA = P * (b_dP + (P * b_dP).sum(-1, keepdim=True))
    b_S = (aq @ ak.transpose(-1, -2)) * scale
    b_dS = _mix_t(b_dA, wl.abs())
    r.update({'b_out': b_R @ av, 'b_dq': scale * (b_dS @ ak), 'b_dk': scale * (b_dS.transpose(-1, -2) @ aq),
              'b_dv': b_R.transpose(-1, -2) @ ado})
    r = {n: A._tokens(x) for n, x in r.items()}                                   # [B, T, H, DH]
    if round_out:
        for n in BIG:
            r[n] = A.bf16_round(r[n])
    r.update({'lse': lse,
              'dwl': torch.einsum('bhij,bgij->hg', S, dA), 'dbl': dA.sum((0, 2, 3)),
              'dww': torch.einsum('bhij,bgij->hg', P, dR), 'dbw': dR.sum((0, 2, 3)),
              'b_dwl': torch.einsum('bhij,bgij->hg', b_S, b_dA), 'b_dbl': b_dA.sum((0, 2, 3)),
              'b_dww': torch.einsum('bhij,bgij->hg', P, b_dR), 'b_dbw': b_dR.sum((0, 2, 3))})
    return r


def pad_key_inputs():
    """The input on which `pad_key` shows beyond doubt: T = 5, every score far below bl, so that the padded key of
    A = bl[g] would take nearly all of the softmax mass.  (On the general cases it shows as well; this one does not
    depend on the draw.)"""
    d = make_case((2, 5, 2), 'plain', 0.25)
    d['bl'] = torch.tensor([6.0, 5.0])
    return d


# ------------------------------------------------------------------ class attention
def make_cls_case(case, kind):
    """-> dict(q [B, H, DH], k, v [B, T, H, DH], dout [B, H, DH], scale): q is row 0 of the draw's queries."""
    B, T, H = case
    qkv, dout = A.make_inputs(kind, B, T, H, DH, 5000 + 1000 * T + 10 * H + KINDS.index(kind), peak_gain=PEAK_GAIN)
    return dict(q=qkv[:, 0, 0].contiguous(), k=qkv[:, :, 1].contiguous(), v=qkv[:, :, 2].contiguous(),
                dout=dout[:, 0].contiguous(), scale=DH ** -0.5)


def cls_reference(d, dtype=torch.float64, round_out=False):
    q, k, v, do = [d[n].to(dtype) for n in ('q', 'k', 'v', 'dout')]
    scale = d['scale']
    s = torch.einsum('bhd,bthd->bht', q, k) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = torch.einsum('bhd,bthd->bht', do, v)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    b_dp = torch.einsum('bhd,bthd->bht', do.abs(), v.abs())
    b_ds = p * (b_dp + (p * b_dp).sum(-1, keepdim=True))
    pt, dst, b_dst = [x.permute(0, 2, 1).unsqueeze(-1) for x in (p, ds, b_ds)]     # [B, T, H, 1]
    r = {'out': torch.einsum('bht,bthd->bhd', p, v), 'dq': scale * torch.einsum('bht,bthd->bhd', ds, k),
         'dk': scale * dst * q.unsqueeze(1), 'dv': pt * do.unsqueeze(1),
         'b_out': torch.einsum('bht,bthd->bhd', p, v.abs()), 'b_dq': scale * torch.einsum('bht,bthd->bhd', b_ds, k.abs()),
         'b_dk': scale * b_dst * q.abs().unsqueeze(1), 'b_dv': pt * do.abs().unsqueeze(1), 'lse': lse}
    if round_out:
        for n in CLS_TENSORS:
            r[n] = A.bf16_round(r[n])
    return r


# ------------------------------------------------------------------ criteria
def smallest_bound(ref, tensors):
    return min(float(ref['b_' + n].min()) for n in tensors)


def violations(got, ref, limits, tensors):
    """[(tensor, share of the allowance used, description)] for every tensor outside limit x bound."""
    bad = []
    for n in tensors:
        used, idx = A.limit_usage(got[n], ref[n], ref['b_' + n], limits[n])
        if not used <= 1:
            g, r, b = [x.double().flatten()[idx] for x in (got[n], ref[n], ref['b_' + n])]
            bad.append((n, used, '%s flat %d: got %.9g, reference %.9g, bound %.6g' % (n, idx, g, r, b)))
    return bad
