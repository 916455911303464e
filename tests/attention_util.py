"""CPU helpers of the attention numerics tests (pure torch, no GPU, no kernel code).

Layouts are the kernels': qkv [B, T, 3, H, DH], out / dout / dq / dk / dv [B, T, H, DH], lse [B, H, T].

make_inputs      adversarial input families, already rounded to bf16 values
reference        float64 attention, closed-form backward and the component-wise magnitude bounds
rounding_model   the same mathematics with bf16 rounding where attention_bf16.hip rounds (optionally
                 with a planted defect, to show that the criteria below can see it)
scaled_error / limit_usage / bound_violations / closeness_violations
                 the element-wise criteria shared by the host and the GPU test
CASES            the shape / kind matrix both tests run
"""
import functools
import math

import torch

U = 2.0 ** -8              # bf16 unit round-off (8 significant bits, round to nearest even)
TINY = 2.0 ** -100         # bounds below this come from underflowed probabilities
KINDS = ('plain', 'peaked', 'vmean', 'negative', 'ramp')
DEFECTS = ('zero_key', 'mask_shift', 'drop_last', 'no_delta')

# a-priori limits of the bf16-MFMA kernels, in units of the bound: one operand rounding (P or dS) and the store
# rounding give 2 u for out / dv; dq / dk add the delta formed from the rounded O: 3 u.  0.25 u is slack for the
# fp32 accumulation order and the fast exp.
LIMIT_BF16 = {'out': 2.25 * U, 'dv': 2.25 * U, 'dq': 3.25 * U, 'dk': 3.25 * U}
RMS_CAP = 0.75             # rms((got - model) / bound) <= RMS_CAP * rms((model - ref) / bound) + RMS_FLOOR
SHARE_CAP = 0.01           # share of elements further than 0.5 u * bound from the model
# Where the rounding model is exact (T = 1: P = 1, out = v, dv = dO, dq = dk = 0) the right-hand side above is 0
# while an fp32 kernel still differs from float64 by its accumulation order (dP - delta does not cancel exactly).
# The floor admits that much and nothing a bf16-level defect could hide under: 16 fp32 round-offs, 2^-12 u.
RMS_FLOOR = 16 * 2.0 ** -24


def bf16_round(x):
    """x rounded to the nearest bf16 value (through fp32, as the kernels round), in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def ramp_slope(T):
    """Score increase per key of the `ramp` kind.  A slope of 1 (let alone more) over 208 keys pushes every
    probability of the first ~140 keys, and with them whole rows of dk / dv, below 2^-100, where nothing is
    compared; min(1, 60 / T) keeps the full score range at 60 (e^-60 ~ 2^-87)."""
    return min(1.0, 60.0 / T)


# `peaked` under the causal mask: the last key is seen by one query only, the one before by two, ...; with a
# gain of 6 (score spread 36 sigma) the own-key probability of those few rows is below 2^-100 about every other
# time, and 1.4 - 2.1 % of the rows of dk / dv have nothing to be compared with at T = 33 and 129.  The spread
# between a row's maximum (~3.1 sigma at T = 129) and a 1 %-low own score (-2.6 sigma) has to stay below
# ln 2^100 = 69: gain^2 <= 12, so causal cases use 3.5 (scores about +-50, the top key still takes > 90 %).
PEAK_GAIN_CAUSAL = 3.5


def make_inputs(kind, B, T, H, DH, seed, peak_gain=6.0):
    """qkv [B, T, 3, H, DH] and dout [B, T, H, DH], fp32 tensors holding bf16 values.  With u[h] a fixed random
    unit vector per head and scores meaning q.k * DH^-0.5:

    plain     randn                                                    (today's inputs)
    peaked    q, k *= peak_gain (6)                                    scores about +-150
    vmean     q, k *= 3, v += 3                                        dP - delta cancels, out ~ 3
    negative  q += a u, k -= a u, a = sqrt(30 sqrt(DH))                every score in about [-46, -18]
    ramp      q = 0.25 randn + c DH^(1/4) u,                           scores grow by c per key,
              k_j = 0.25 randn + (j - T/2) DH^(1/4) u                  c = ramp_slope(T) = min(1, 60 / T)
    """
    assert kind in KINDS
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(H, DH, generator=gen)
    u = u / u.norm(dim=-1, keepdim=True)
    qkv = torch.randn(B, T, 3, H, DH, generator=gen)
    dout = torch.randn(B, T, H, DH, generator=gen)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]                 # views [B, T, H, DH]
    if kind == 'peaked':
        q *= peak_gain
        k *= peak_gain
    elif kind == 'vmean':
        q *= 3
        k *= 3
        v += 3
    elif kind == 'negative':
        a = math.sqrt(30 * math.sqrt(DH))
        q += a * u
        k -= a * u
    elif kind == 'ramp':
        r = DH ** 0.25
        j = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1) - T / 2
        q.mul_(0.25).add_(ramp_slope(T) * r * u)
        k.mul_(0.25).add_(j * r * u)
    return bf16_round(qkv), bf16_round(dout)


def _heads(qkv, dout, dtype):
    q, k, v = [qkv[:, :, i].permute(0, 2, 1, 3).to(dtype) for i in range(3)]      # [B, H, T, DH]
    return q, k, v, dout.permute(0, 2, 1, 3).to(dtype)


def _tokens(x):
    return x.permute(0, 2, 1, 3).contiguous()                                    # [B, T, H, DH]


def _visible(T, causal, shift=0, drop_last=False):
    i = torch.arange(T).view(T, 1)
    j = torch.arange(T).view(1, T)
    vis = (j <= i + shift) if causal else torch.ones(T, T, dtype=torch.bool)
    if drop_last:
        vis = vis & (j < T - 1)
    return vis


def reference(qkv, dout, scale, causal, dtype=torch.float64):
    """Plain softmax attention with its closed-form backward, in `dtype` (float64: the reference; float32: the
    "eager" figure the fp32 kernels are measured against).  Returns a dict of out, lse, dq, dk, dv and the bounds
    b_out = P |v|, b_dv = P^T |dO|, b_dq = a |k|, b_dk = a^T |q| with a = P (|dO v^T| + sum_d |dO_d| b_out_d) scale
    (the sum is the room the delta formed from a rounded O needs).  c_dq / c_dk are that delta term alone with |O|
    in place of b_out: what one bf16 rounding of a stored O may move dq / dk by, in units of u."""
    q, k, v, do = _heads(qkv, dout, dtype)
    T = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~_visible(T, causal), float('-inf'))
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
    r = {n: _tokens(x) for n, x in r.items()}
    r['lse'] = lse
    return r


def rounding_model(qkv, dout, scale, causal, dtype=torch.float64, defect=None):
    """The algorithm of attention_bf16.hip's header comment with its bf16 roundings; everything else in `dtype`.
    Forward: scores, row max, exp, sum and lse in `dtype`; P rounded to bf16 as the operand of P V; O rounded on
    store.  Backward: P = exp(s - lse) recomputed, delta = dO . (stored O), dS = P (dP - delta) scale; dS rounded
    before dS K and dS^T Q, the recomputed P rounded before P^T dO; dq, dk, dv rounded on store.

    `defect` plants one bug (the kernels are not involved): 'zero_key' one extra key of score 0 and value 0 in
    the softmax sum, 'mask_shift' causal mask off by one (key i + 1 visible to query i), 'drop_last' the last
    key invisible, 'no_delta' delta left out of dS."""
    assert defect is None or defect in DEFECTS
    q, k, v, do = _heads(qkv, dout, dtype)
    T = q.shape[2]
    vis = _visible(T, causal, shift=1 if defect == 'mask_shift' else 0, drop_last=defect == 'drop_last')
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float('-inf'))
    m = s.max(dim=-1, keepdim=True).values
    if defect == 'zero_key':
        m = m.clamp_min(0)
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    if defect == 'zero_key':
        z = z + torch.exp(-m)
    lse = m + torch.log(z)
    out = bf16_round(bf16_round(e / z) @ v)
    p = torch.exp(s - lse)
    delta = (do * out).sum(-1, keepdim=True)
    if defect == 'no_delta':
        delta = torch.zeros_like(delta)
    ds = bf16_round(p * (do @ v.transpose(-1, -2) - delta) * scale)
    r = {'out': out, 'dq': bf16_round(ds @ k), 'dk': bf16_round(ds.transpose(-1, -2) @ q),
         'dv': bf16_round(bf16_round(p).transpose(-1, -2) @ do)}
    r = {n: _tokens(x) for n, x in r.items()}
    r['lse'] = lse.squeeze(-1)
    return r


# ------------------------------------------------------------------ criteria
def _where(idx, shape):
    b, t, h, d = [int(x) for x in torch.unravel_index(torch.as_tensor(idx), shape)]
    return '(b=%d, h=%d, t=%d, d=%d)' % (b, h, t, d)


def scaled_error(got, ref, bound):
    """Worst |got - ref| / (bound + 2^-100) over the elements whose bound is at least 2^-100, the flat index of
    that element, and the worst |got - ref| over the others (to be held to 2^-100 absolutely).  A non-finite
    `got` yields inf."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    live = bound >= TINY
    ratio = torch.where(live, err / (bound + TINY), torch.zeros_like(err)).flatten()
    idx = int(ratio.argmax())
    dead = err[~live]
    return float(ratio[idx]), idx, float(dead.max()) if dead.numel() else 0.0


def underflow_share(bound):
    return float((bound < TINY).double().mean())


def describe(name, got, ref, bound, idx, what='reference'):
    g, r, b = got.double().flatten()[idx], ref.double().flatten()[idx], bound.double().flatten()[idx]
    return '%s at %s: got %.9g, %s %.9g, bound %.6g, |diff| / bound = %.4g' % (
        name, _where(idx, ref.shape), g, what, r, b, abs(g - r) / (b + TINY))


def limit_usage(got, ref, bound, limit, extra=None):
    """max |got - ref| / allowance and its flat index; the allowance is limit * bound (+ extra, an element-wise
    term) wherever the bound is at least 2^-100, and 2^-100 elsewhere.  <= 1 means inside the limit."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    allow = limit * (bound + TINY) + (extra.double() if extra is not None else 0.0)
    allow = torch.where(bound >= TINY, allow, torch.full_like(allow, TINY))
    used = (err / allow).flatten()
    idx = int(used.argmax())
    return float(used[idx]), idx


def bound_violations(name, got, ref, bound, limit, extra=None):
    """[] or one message naming the worst element outside its allowance (see limit_usage)."""
    used, idx = limit_usage(got, ref, bound, limit, extra)
    if not used <= 1:
        return ['bound (limit %.4g, %.3f of the allowance used): %s' % (limit, used, describe(name, got, ref, bound, idx))]
    return []


def closeness(got, model, ref, bound):
    """(rms ratio numerator, denominator, share): rms((got - model) / bound), rms((model - ref) / bound) and the
    share of elements with |got - model| > 0.5 u bound."""
    got, model, ref, bound = got.double(), model.double(), ref.double(), bound.double() + TINY
    d = (got - model).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float('inf')))
    num = float((d / bound).pow(2).mean().sqrt())
    den = float(((model - ref) / bound).pow(2).mean().sqrt())
    return num, den, float((d > 0.5 * U * bound).double().mean())


def closeness_violations(name, got, model, ref, bound):
    num, den, share = closeness(got, model, ref, bound)
    msgs = []
    if not num <= RMS_CAP * den + RMS_FLOOR:
        idx = int(((got.double() - model.double()).abs() / (bound.double() + TINY)).flatten().nan_to_num(
            nan=float('inf')).argmax())
        msgs.append('rms: %s differs from the rounding model by %.4g rms, the model from the reference by %.4g '
                    '(ratio %.3f > %.2f); worst %s' % (name, num, den, num / max(den, 1e-300), RMS_CAP,
                                                        describe(name, got, model, bound, idx, 'model')))
    if not share <= SHARE_CAP:
        msgs.append('share: %.2f %% of %s is further than 0.5 u bound from the rounding model' % (100 * share, name))
    return msgs


TENSORS = ('out', 'dq', 'dk', 'dv')


def bf16_violations(got, model, ref):
    """Every §3 criterion of the bf16-MFMA paths; returns {'bound': [...], 'rms': [...], 'share': [...]}."""
    res = {'bound': [], 'rms': [], 'share': []}
    for n in TENSORS:
        res['bound'] += bound_violations(n, got[n], ref[n], ref['b_' + n], LIMIT_BF16[n])
        for msg in closeness_violations(n, got[n], model[n], ref[n], ref['b_' + n]):
            res[msg.split(':')[0]].append(msg)
    return res


# ------------------------------------------------------------------ the matrix
B, H = 2, 3                # head and image strides both in play, H no power of two
HEAD_DIMS = (32, 64)
T_FULL = (1, 15, 16, 17, 31, 32, 33, 112, 113, 127, 128, 129, 207, 208)
T_CAUSAL = (1, 16, 17, 33, 77, 113, 129, 208)


def _cases():
    out = []
    for DH in HEAD_DIMS:
        for T in T_FULL:
            out += [(DH, T, False, kind) for kind in ('plain', 'negative')]
        for T in (17, 113, 208):
            out += [(DH, T, False, kind) for kind in ('peaked', 'vmean', 'ramp')]
        for T in T_CAUSAL:
            out += [(DH, T, True, kind) for kind in ('negative', 'ramp')]
        for T in (33, 129):
            out += [(DH, T, True, kind) for kind in ('peaked', 'vmean')]
    return out


CASES = _cases()


def case_id(case):
    DH, T, causal, kind = case
    return 'd%d-T%d-%s-%s' % (DH, T, 'causal' if causal else 'full', kind)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """Inputs, float64 reference, float64 rounding model and float32 eager result of a case; computed once and
    shared (treat as read-only)."""
    DH, T, causal, kind = case
    seed = 1000 * T + 10 * DH + KINDS.index(kind) + (5 if causal else 0)
    qkv, dout = make_inputs(kind, B, T, H, DH, seed, peak_gain=PEAK_GAIN_CAUSAL if causal else 6.0)
    scale = DH ** -0.5
    return {'qkv': qkv, 'dout': dout, 'scale': scale,
            'ref': reference(qkv, dout, scale, causal),
            'model': rounding_model(qkv, dout, scale, causal),
            'eager': reference(qkv, dout, scale, causal, dtype=torch.float32)}
