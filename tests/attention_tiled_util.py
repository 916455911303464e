"""CPU helpers of the key-tiled attention tests (csrc/attention_tiled.hip): pure torch, no GPU, no kernel code.

attention_util.py supplies the inputs, the float64 reference, the bounds and the criteria; they are shape-generic.
This module adds what tiling changes:

tiled_rounding_model   the forward as an online softmax over key blocks of BLOCK rows with the kernel's bf16 roundings:
                       exp(s - running max) rounded to bf16 as the operand of P V, the rescale of the accumulator in
                       the working precision, out = accumulator / sum rounded once at the store.  The backward is
                       attention_util.rounding_model's, formula for formula, on the tiled forward's stored O and lse: it
                       recomputes P from lse and does not see the tiling.
DEFECTS                three planted bugs of the tiled forward, to show that the criteria can see them
CASES                  the shape / kind matrix of the host and the GPU test
"""
import functools

import torch

import attention_util as A

BLOCK = 64                 # key rows per LDS block of the kernels (atile::kBlock)
DEFECTS = ('stale_max', 'skip_last_block', 'pad_zero')


def tiled_forward(q, k, v, scale, block=BLOCK, defect=None):
    """Online softmax over key blocks, heads-first tensors [B, H, T, DH] in their dtype.  Returns (out as stored, lse).

    `defect`: 'stale_max' the accumulator is not rescaled when the max rises (the sum is); 'skip_last_block' the last
    key block is never visited; 'pad_zero' the padding keys of a partial last block count with score 0 and value 0."""
    assert defect is None or defect in DEFECTS
    Bn, Hn, T, DH = q.shape
    m = torch.full((Bn, Hn, T, 1), float('-inf'), dtype=q.dtype)
    z = torch.zeros(Bn, Hn, T, 1, dtype=q.dtype)
    o = torch.zeros(Bn, Hn, T, DH, dtype=q.dtype)
    starts = list(range(0, T, block))
    if defect == 'skip_last_block':
        starts = starts[:-1]
    for k0 in starts:
        n = min(block, T - k0)
        s = (q @ k[:, :, k0:k0 + n].transpose(-1, -2)) * scale
        vb = v[:, :, k0:k0 + n]
        if defect == 'pad_zero' and n < block:
            s = torch.cat([s, torch.zeros(Bn, Hn, T, block - n, dtype=q.dtype)], dim=-1)
            vb = torch.cat([vb, torch.zeros(Bn, Hn, block - n, DH, dtype=q.dtype)], dim=2)
        mn = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        alpha = torch.exp(m - mn)                  # 0 at the first block
        e = torch.exp(s - mn)
        z = z * alpha + e.sum(-1, keepdim=True)
        if defect != 'stale_max':
            o = o * alpha
        o = o + A.bf16_round(e) @ vb
        m = mn
    return A.bf16_round(o / z), (m + torch.log(z)).squeeze(-1)


def tiled_rounding_model(qkv, dout, scale, dtype=torch.float64, block=BLOCK, defect=None):
    """Dict of out, dq, dk, dv [B, T, H, DH] and lse [B, H, T], as attention_util.rounding_model returns them."""
    q, k, v, do = A._heads(qkv, dout, dtype)
    out, lse = tiled_forward(q, k, v, scale, block, defect)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - lse.unsqueeze(-1))
    delta = (do * out).sum(-1, keepdim=True)
    ds = A.bf16_round(p * (do @ v.transpose(-1, -2) - delta) * scale)
    r = {'out': out, 'dq': A.bf16_round(ds @ k), 'dk': A.bf16_round(ds.transpose(-1, -2) @ q),
         'dv': A.bf16_round(A.bf16_round(p).transpose(-1, -2) @ do)}
    r = {n: A._tokens(x) for n, x in r.items()}
    r['lse'] = lse
    return r


# ------------------------------------------------------------------ the matrix
B, H = A.B, A.H
HEAD_DIMS = A.HEAD_DIMS
T_SHORT = (1, 17, 128, 129, 208)
T_LONG = (209, 255, 256, 257, 383, 385, 577, 578, 785, 1023, 1024)
T_HARD = (209, 257, 578, 1024)         # the lengths of the peaked / vmean / ramp kinds


def _cases():
    out = []
    for DH in HEAD_DIMS:
        for T in T_SHORT + T_LONG:
            out += [(DH, T, False, kind) for kind in ('plain', 'negative')]
        for T in T_HARD:
            out += [(DH, T, False, kind) for kind in ('peaked', 'vmean', 'ramp')]
    return out


CASES = _cases()                        # (DH, T, causal = False, kind): attention_util.case_id names them


@functools.lru_cache(maxsize=None)
def case_data(case):
    """attention_util.case_data with the tiled rounding model; computed once and shared (treat as read-only)."""
    DH, T, causal, kind = case
    assert not causal
    seed = 1000 * T + 10 * DH + A.KINDS.index(kind)
    qkv, dout = A.make_inputs(kind, B, T, H, DH, seed)
    scale = DH ** -0.5
    return {'qkv': qkv, 'dout': dout, 'scale': scale,
            'ref': A.reference(qkv, dout, scale, False),
            'model': tiled_rounding_model(qkv, dout, scale),
            'eager': A.reference(qkv, dout, scale, False, dtype=torch.float32)}
