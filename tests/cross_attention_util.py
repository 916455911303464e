"""CPU helpers of the cross-attention tests (csrc/cross_attention.hip): pure torch, no GPU, no kernel code.

attention_util.py supplies the input families, the constants and the criteria.  This module restates what separate
operands and lengths change: q, out, dout, dq are [B, Tq, H, DH], k, v, dk, dv are [B, Tk, H, DH], lse is [B, H, Tq].

reference        float64 attention with its closed-form backward and attention_util.reference's component-wise bounds
tiled_forward /  attention_tiled_util's online softmax over key blocks of 64 and its rounding model, for separate
rounding_model   q / k / v (optionally with a planted defect)
DEFECTS          'stale_max' and 'skip_last_block' of the tiled forward, and 'kv_sweep_tq': the dK / dV sweep owns key
                 columns up to Tq where Tk belongs (visible where Tq < Tk: the keys beyond get no gradient)
CASES            the shape / kind matrix of the host and the GPU test
"""
import functools

import torch

import attention_tiled_util as TU
import attention_util as A

BLOCK = TU.BLOCK
DEFECTS = ('stale_max', 'skip_last_block', 'kv_sweep_tq')


def _heads(x, dtype):
    return x.permute(0, 2, 1, 3).to(dtype)                                      # [B, H, T, DH]


def reference(q, k, v, dout, scale, dtype=torch.float64):
    """attention_util.reference without a mask for q [B, Tq, H, DH] and k, v [B, Tk, H, DH]: out, lse, dq, dk, dv, the
    bounds b_* and the delta terms c_dq / c_dk, formula for formula."""
    q, k, v, do = [_heads(x, dtype) for x in (q, k, v, dout)]
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = p @ v
    dp = do @ v.transpose(-1, -2)
    delta = (do * out).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    b_out = p @ v.abs()
    a = p * (dp.abs() + (do.abs() * b_out).sum(-1, keepdim=True)) * scale
    c = p * (do.abs() * out.abs()).sum(-1, keepdim=True) * scale
    r = {'out': out, 'dq': ds @ k, 'dk': ds.transpose(-1, -2) @ q, 'dv': p.transpose(-1, -2) @ do,
         'b_out': b_out, 'b_dq': a @ k.abs(), 'b_dk': a.transpose(-1, -2) @ q.abs(),
         'b_dv': p.transpose(-1, -2) @ do.abs(), 'c_dq': c @ k.abs(), 'c_dk': c.transpose(-1, -2) @ q.abs()}
    r = {n: A._tokens(x) for n, x in r.items()}
    r['lse'] = lse
    return r


def tiled_forward(q, k, v, scale, block=BLOCK, defect=None):
    """attention_tiled_util.tiled_forward with the block loop over the KEYS' length: heads-first q [B, H, Tq, DH] and
    k, v [B, H, Tk, DH] in their dtype.  Returns (out as stored, lse).  exp(s - running max) is rounded to bf16 as the
    operand of P V, the accumulator is rescaled in the working precision, out = accumulator / sum is rounded once.

    `defect`: 'stale_max' the accumulator is not rescaled when the max rises (the sum is); 'skip_last_block' the last
    key block is never visited."""
    Bn, Hn, Tq, DH = q.shape
    Tk = k.shape[2]
    m = torch.full((Bn, Hn, Tq, 1), float('-inf'), dtype=q.dtype)
    z = torch.zeros(Bn, Hn, Tq, 1, dtype=q.dtype)
    o = torch.zeros(Bn, Hn, Tq, DH, dtype=q.dtype)
    starts = list(range(0, Tk, block))
    if defect == 'skip_last_block':
        starts = starts[:-1]
    for k0 in starts:
        n = min(block, Tk - k0)
        s = (q @ k[:, :, k0:k0 + n].transpose(-1, -2)) * scale
        mn = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        alpha = torch.exp(m - mn)                  # 0 at the first block
        e = torch.exp(s - mn)
        z = z * alpha + e.sum(-1, keepdim=True)
        if defect != 'stale_max':
            o = o * alpha
        o = o + A.bf16_round(e) @ v[:, :, k0:k0 + n]
        m = mn
    return A.bf16_round(o / z), (m + torch.log(z)).squeeze(-1)


def rounding_model(q, k, v, dout, scale, dtype=torch.float64, block=BLOCK, defect=None):
    """The bf16-MFMA kernels' roundings: tiled_forward over the Tk keys, then the backward of tiled_rounding_model on the
    stored O and lse.  'kv_sweep_tq': the key columns from Tq on are not owned by any wave of the dK / dV sweep, their
    dk and dv stay zero."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = [_heads(x, dtype) for x in (q, k, v, dout)]
    Tq, Tk = q.shape[2], k.shape[2]
    out, lse = tiled_forward(q, k, v, scale, block, defect)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse.unsqueeze(-1))
    delta = (do * out).sum(-1, keepdim=True)
    ds = A.bf16_round(p * (do @ v.transpose(-1, -2) - delta) * scale)
    pr = A.bf16_round(p)
    if defect == 'kv_sweep_tq':
        keep_k = (torch.arange(Tk) < Tq).view(1, 1, 1, Tk).to(dtype)            # key columns that are owned
        dsk, prk = ds * keep_k, pr * keep_k
    else:
        dsk, prk = ds, pr
    r = {'out': out, 'dq': A.bf16_round(ds @ k), 'dk': A.bf16_round(dsk.transpose(-1, -2) @ q),
         'dv': A.bf16_round(prk.transpose(-1, -2) @ do)}
    r = {n: A._tokens(x) for n, x in r.items()}
    r['lse'] = lse
    return r


# ------------------------------------------------------------------ the matrix
B, H = A.B, A.H
HEAD_DIMS = A.HEAD_DIMS
PAIRS_EDGE = ((1, 1), (1, 65), (16, 63), (17, 64), (64, 129), (129, 64), (5, 1024), (1024, 5))
PAIRS_ALL = ((75, 196), (76, 122), (196, 75), (130, 257), (208, 1024))


def _cases():
    out = []
    for DH in HEAD_DIMS:
        for Tq, Tk in PAIRS_EDGE:
            out += [(DH, Tq, Tk, kind) for kind in ('plain', 'negative')]
        for Tq, Tk in PAIRS_ALL:
            out += [(DH, Tq, Tk, kind) for kind in A.KINDS]
    return out


CASES = _cases()


def case_id(case):
    DH, Tq, Tk, kind = case
    return 'd%d-q%d-k%d-%s' % (DH, Tq, Tk, kind)


def case_inputs(case):
    """q [B, Tq, H, DH], k, v [B, Tk, H, DH], dout [B, Tq, H, DH]: the first rows of attention_util.make_inputs at
    max(Tq, Tk) tokens."""
    DH, Tq, Tk, kind = case
    seed = 1000 * Tk + 7 * Tq + 10 * DH + A.KINDS.index(kind)
    qkv, dout = A.make_inputs(kind, B, max(Tq, Tk), H, DH, seed)
    return (qkv[:, :Tq, 0].contiguous(), qkv[:, :Tk, 1].contiguous(), qkv[:, :Tk, 2].contiguous(),
            dout[:, :Tq].contiguous())


@functools.lru_cache(maxsize=None)
def case_data(case):
    """Inputs, float64 reference, float64 rounding model and float32 eager result of a case; computed once and shared
    (treat as read-only)."""
    q, k, v, dout = case_inputs(case)
    scale = case[0] ** -0.5
    return {'q': q, 'k': k, 'v': v, 'dout': dout, 'scale': scale,
            'ref': reference(q, k, v, dout, scale),
            'model': rounding_model(q, k, v, dout, scale),
            'eager': reference(q, k, v, dout, scale, dtype=torch.float32)}
