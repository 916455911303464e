"""CPU helpers of the token-merging tests: the float64 restatement of the matching, the merge, its gradient and key-bias
attention, written from the formulas (numpy / torch on the host, no kernel code), the decision margin of the matching
and the case matrix the host and the GPU tests share.

Layouts are the kernels': qkv [B, T, 3, H, DH], x [B, T, C], size [B, T], dest int [B, T].

The matching's decision margin
------------------------------
The kernel forms every score in fp32 (u = 2^-24).  For unit vectors a, b of DH channels:
  * head mean: H - 1 additions, the rounded factor 1 / H and the product, each relative to sum_h |k_h| / H: the metric
    of token t is off by at most (H + 1) u kappa_t of its own length, kappa_t = ||mean_h |k_h|| / ||mean_h k_h||
    (how much the heads cancel);
  * normalisation: the division by the largest magnitude (u), the sum of DH squares ((DH + 1) u on the sum, half of
    that on its root), the root (u) and the second division (u): at most (DH / 2 + 4) u per vector, which scales a
    score of magnitude <= 1;
  * the dot product: DH fmas, at most DH u sum_d |a_d b_d| <= DH u (Cauchy-Schwarz).
One score is therefore within  MARGIN = u (DH + 2 (DH / 2 + 4) + (H + 1)(kappa_i + kappa_j))
                                     <= u (2 DH + 8 + 2 (H + 1) kappa_max)
of its float64 value, kappa_max over the tokens of the case.  Two scores compare as in float64 when they differ by more
than 2 MARGIN: that is `decided`.  The seeded cases are searched (deterministically, from seed 0 up) until every relevant
float64 gap — the cut between rank r - 1 and rank r of every image, and top-1 minus top-2 of every merged row — is at
least 16 x 2 MARGIN; the host test asserts it.  Nothing here looks at a kernel's output.
"""
import functools
import math

import numpy as np
import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8            # bf16, as attention_util.U
GAP_FACTOR = 16


def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def max_r(T):
    return (T - 1) // 2


# ------------------------------------------------------------------ matching
def metric(qkv):
    """float64 [B, T, DH]: the mean over heads of K, L2-normalised; and kappa [B, T]."""
    k = qkv[:, :, 1].double().numpy()                        # [B, T, H, DH]
    m = k.mean(axis=2)
    kappa = np.linalg.norm(np.abs(k).mean(axis=2), axis=-1) / np.linalg.norm(m, axis=-1)
    return m / np.linalg.norm(m, axis=-1, keepdims=True), kappa


def margin(DH, H, kappa_max):
    return U32 * (2 * DH + 8 + 2 * (H + 1) * kappa_max)


def match(qkv, r):
    """The matching in float64 with the documented tie rule.  Returns a dict:
    scores [B, NA, NB] (row 0 = -inf), node_max [B, NA], node_idx [B, NA], merged bool [B, NA], dest int64 [B, T],
    cut_gap [B] (node_max of rank r - 1 minus rank r), arg_gap [B, NA] (top-1 minus top-2 of a row; inf with one B
    token), kappa_max."""
    m, kappa = metric(qkv)
    B, T, _ = m.shape
    NA, NB = (T + 1) // 2, T // 2
    assert 1 <= r <= max_r(T)
    a, b = m[:, 0::2], m[:, 1::2]
    scores = np.einsum('bid,bjd->bij', a, b)
    scores[:, 0, :] = -np.inf
    node_max = scores.max(axis=-1)
    node_idx = scores.argmax(axis=-1)                        # numpy: the first of equal maxima
    node_idx[:, 0] = 0
    order = np.argsort(-node_max, axis=-1, kind='stable')    # equal maxima: the lower A index first
    merged = np.zeros((B, NA), dtype=bool)
    np.put_along_axis(merged, order[:, :r], True, axis=-1)
    srt = np.take_along_axis(node_max, order, axis=-1)
    cut_gap = srt[:, r - 1] - srt[:, r]                      # rank r exists: the class row is never merged
    if NB > 1:
        top2 = np.sort(scores, axis=-1)[:, :, -2:]
        with np.errstate(invalid='ignore'):
            arg_gap = top2[:, :, 1] - top2[:, :, 0]
        arg_gap[:, 0] = np.inf
    else:
        arg_gap = np.full((B, NA), np.inf)
    dest = np.zeros((B, T), dtype=np.int64)
    nunm = NA - r
    for bi in range(B):
        row = 0
        for i in range(NA):
            if merged[bi, i]:
                dest[bi, 2 * i] = nunm + node_idx[bi, i]
            else:
                dest[bi, 2 * i] = row
                row += 1
        assert row == nunm
        dest[bi, 1::2] = nunm + np.arange(NB)
    return {'scores': scores, 'node_max': node_max, 'node_idx': node_idx, 'merged': merged, 'dest': dest,
            'cut_gap': cut_gap, 'arg_gap': arg_gap, 'kappa_max': float(kappa.max())}


def smallest_gap(res):
    """The smallest gap a decision of the case depends on: the cut of every image, the arg-max of every merged row."""
    g = float(res['cut_gap'].min())
    mg = res['arg_gap'][res['merged']]
    return min(g, float(mg.min())) if mg.size else g


def make_qkv(kind, B, T, H, DH, seed):
    """fp32 qkv [B, T, 3, H, DH] holding bf16 values.
    random   randn
    paired   every even token's K is an odd token's K plus noise whose size differs from row to row: scores near 1
             against one partner, spread out over the rows (what a trained ViT's redundant patches look like)"""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, DH, generator=gen)
    if kind == 'paired':
        NA, NB = (T + 1) // 2, T // 2
        for b in range(B):
            partner = torch.randint(0, NB, (NA,), generator=gen)
            amp = 0.2 + 0.8 * torch.rand(NA, generator=gen)
            qkv[b, 0::2, 1] = qkv[b, 1::2, 1][partner] + amp.view(NA, 1, 1) * torch.randn(NA, H, DH, generator=gen)
    else:
        assert kind == 'random'
    return bf16_round(qkv)


MATCH_T = (3, 17, 18, 37, 197, 208)
MATCH_B = (1, 3)
MATCH_HD = ((1, 32), (2, 64), (12, 64))


def r_values(T):
    return sorted({1, max(1, max_r(T) // 2), max_r(T)})


MATCH_CASES = [(T, r, B, H, DH) for T in MATCH_T for r in r_values(T) for B in MATCH_B for H, DH in MATCH_HD]


def match_case_id(c):
    return 'T%d-r%d-B%d-H%d-d%d' % c


@functools.lru_cache(maxsize=None)
def match_case(case):
    """(qkv, float64 result, margin, seed): the first seed from 0 whose float64 gaps are all >= GAP_FACTOR x 2 MARGIN.
    Short sequences are plain random; from 100 tokens on the keys are `paired`, where up to 103 arg-max decisions per
    image leave room between the best and the second partner."""
    T, r, B, H, DH = case
    kind = 'paired' if T >= 100 else 'random'
    for seed in range(400):
        qkv = make_qkv(kind, B, T, H, DH, 7919 * seed + T)
        res = match(qkv, r)
        mg = margin(DH, H, res['kappa_max'])
        if smallest_gap(res) >= GAP_FACTOR * 2 * mg:
            return qkv, res, mg, seed
    raise AssertionError('no seed below 400 decides %s' % match_case_id(case))


def tie_case(B=2, T=18, H=2, DH=32, seed=5):
    """Duplicated tokens: odd tokens 3 and 7 hold the same key, as do 5 and 9; even tokens 4 and 10 hold the key of odd
    token 3, so both have exactly the same best score against two B tokens (arg-max: the lower, B index 1), and equal
    node_max (rank: token 4, A index 2, before token 10, A index 5).  Every other key is far from these."""
    gen = torch.Generator().manual_seed(seed)
    qkv = bf16_round(torch.randn(B, T, 3, H, DH, generator=gen))
    k = qkv[:, :, 1]
    k[:, 7] = k[:, 3]
    k[:, 9] = k[:, 5]
    k[:, 4] = k[:, 3]
    k[:, 10] = k[:, 3]
    return qkv


NORM_CASE = (17, 4, 2, 2, 64)          # T, r, B, H, DH


@functools.lru_cache(maxsize=None)
def norm_case():
    """One key of norm ~6e20 and one of ~7e-24 per image (their squares leave fp32 range), both even tokens; seeded like
    match_case.  -> (qkv, float64 result, margin, seed)"""
    T, r, B, H, DH = NORM_CASE
    for seed in range(400):
        gen = torch.Generator().manual_seed(seed)
        qkv = torch.randn(B, T, 3, H, DH, generator=gen)
        qkv[:, 4, 1] *= 2.0 ** 66
        qkv[:, 8, 1] *= 2.0 ** -80
        qkv = bf16_round(qkv)
        res = match(qkv, r)
        mg = margin(DH, H, res['kappa_max'])
        if smallest_gap(res) >= GAP_FACTOR * 2 * mg:
            return qkv, res, mg, seed
    raise AssertionError('no seed below 400 decides the normalisation case')


# ------------------------------------------------------------------ merge
def merge(x, size, dest, To):
    """float64: y [B, To, C], size_out [B, To], bound = sum size |x| / sum size, n = sources per row [B, To]."""
    B, T, C = x.shape
    x = x.double()
    size = torch.ones(B, T, dtype=torch.float64) if size is None else size.double()
    d = torch.as_tensor(dest, dtype=torch.int64)
    num = torch.zeros(B, To, C, dtype=torch.float64)
    mag = torch.zeros(B, To, C, dtype=torch.float64)
    den = torch.zeros(B, To, dtype=torch.float64)
    n = torch.zeros(B, To, dtype=torch.float64)
    idx = d.unsqueeze(-1).expand(B, T, C)
    num.scatter_add_(1, idx, x * size.unsqueeze(-1))
    mag.scatter_add_(1, idx, x.abs() * size.unsqueeze(-1))
    den.scatter_add_(1, d, size)
    n.scatter_add_(1, d, torch.ones(B, T, dtype=torch.float64))
    return {'y': num / den.unsqueeze(-1), 'size_out': den, 'bound': mag / den.unsqueeze(-1), 'n': n}


def merge_bwd(dy, size, size_out, dest):
    """float64 dx [B, T, C] = dy[dest] size / size_out[dest]; bound = its magnitude."""
    B, To, C = dy.shape
    d = torch.as_tensor(dest, dtype=torch.int64)
    T = d.shape[1]
    size = torch.ones(B, T, dtype=torch.float64) if size is None else size.double()
    f = size / size_out.double().gather(1, d)
    dx = dy.double().gather(1, d.unsqueeze(-1).expand(B, T, C)) * f.unsqueeze(-1)
    return {'dx': dx, 'bound': dx.abs()}


# fp32 allowances in units of the bound, from the operation count: n fmas and the division (the sizes and their sum are
# small integers, exact); the factor size / size_out and one product
def merge_fwd_limit(n):
    return (n + 2.0) * U32


MERGE_BWD_LIMIT = 2.5 * U32


def random_dest(B, T, r, seed):
    """A valid matching result without a matching: r random even tokens (never token 0) go to random odd tokens."""
    gen = np.random.RandomState(seed)
    NA, NB = (T + 1) // 2, T // 2
    dest = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        merged = np.zeros(NA, dtype=bool)
        merged[1 + gen.permutation(NA - 1)[:r]] = True
        row = 0
        for i in range(NA):
            if merged[i]:
                dest[b, 2 * i] = NA - r + gen.randint(NB)
            else:
                dest[b, 2 * i] = row
                row += 1
        dest[b, 1::2] = NA - r + np.arange(NB)
    return dest


def previous_sizes(B, T, seed):
    """fp32 [B, T]: the sizes a merge of T + rp tokens of size one into T leaves (small integers)."""
    rp = min(5, T - 1)
    d = torch.as_tensor(random_dest(B, T + rp, rp, seed))
    s = torch.zeros(B, T, dtype=torch.float64)
    s.scatter_add_(1, d, torch.ones(B, T + rp, dtype=torch.float64))
    return s.float()


MERGE_C = (32, 768)
MERGE_CASES = [(T, r, 3, C, sizes) for T in MATCH_T for r in r_values(T) for C in MERGE_C for sizes in ('ones', 'prev')] \
    + [(37, 9, 1, 32, 'prev'), (208, 103, 1, 768, 'ones')]


def merge_case_id(c):
    return 'T%d-r%d-B%d-C%d-%s' % c


@functools.lru_cache(maxsize=None)
def merge_case(case):
    """x, dy (fp32 holding bf16 values), size (fp32 or None), dest int64 and the float64 results; shared, read-only."""
    T, r, B, C, sizes = case
    seed = 31 * T + 7 * r + B + C
    gen = torch.Generator().manual_seed(seed)
    x = bf16_round(torch.randn(B, T, C, generator=gen) + 0.5)
    dy = bf16_round(torch.randn(B, T - r, C, generator=gen))
    size = previous_sizes(B, T, seed) if sizes == 'prev' else None
    dest = random_dest(B, T, r, seed + 1)
    fwd = merge(x, size, dest, T - r)
    return {'x': x, 'dy': dy, 'size': size, 'dest': dest, 'fwd': fwd, 'bwd': merge_bwd(dy, size, fwd['size_out'], dest)}


# ------------------------------------------------------------------ key-bias attention
def keybias_reference(qkv, bias, scale, dtype=torch.float64, round_p=False):
    """softmax(q k^T scale + bias[b, j]) v in `dtype`: out [B, T, H, DH], lse [B, H, T], b_out = P |v|.  `round_p`: the
    bf16-MFMA kernel's roundings (P as an operand, O on store)."""
    q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3).to(dtype) for i in range(3)]
    s = (q @ k.transpose(-1, -2)) * scale + bias.to(dtype)[:, None, None, :]
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if round_p:
        m = s.max(dim=-1, keepdim=True).values
        e = torch.exp(s - m)
        out = bf16_round(bf16_round(e / e.sum(-1, keepdim=True)) @ v)
    else:
        out = p @ v
    return {'out': out.permute(0, 2, 1, 3).contiguous(), 'lse': lse,
            'b_out': (p @ v.abs()).permute(0, 2, 1, 3).contiguous()}


def log_sizes(B, T, seed):
    """fp32 [B, T]: log of integer sizes 1 .. 8."""
    gen = torch.Generator().manual_seed(seed)
    return torch.log(torch.randint(1, 9, (B, T), generator=gen).double()).float()


KEYBIAS_T = (17, 113, 208)


# ------------------------------------------------------------------ the host arithmetic of a patched pass
def schedule(T, rs):
    """(r_i after the clamp, T_i entering block i, T after the last block), restated."""
    r_out, t_in = [], []
    for r in rs:
        t_in.append(T)
        r = max(0, min(r, (T - 1) // 2))
        r_out.append(r)
        T -= r
    return r_out, t_in, T
