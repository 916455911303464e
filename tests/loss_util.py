"""CPU helpers of the loss-kernel numerics tests (pure torch: no GPU, the native library is never loaded).

Case tables, seeded input families, float64 references, element-wise bounds, a float32 evaluation of every formula and
planted defects for the criterion kernels of csrc/clas.hip (softmax CE, sigmoid CE), mixup.hip (soft-target CE),
clip.hip (row normalise, logits GEMM, symmetric CE), head.hip (l2norm, InfoNCE, negative cosine) and ntxent.hip
(NT-Xent + CO2).  test_loss_numerics_host.py shows that the float32 evaluation uses at most half of every bound and
that each planted defect breaks one; test_loss_numerics_gpu.py judges the kernels by the same bounds.

Every family has  X_data(case) -> the fp32 inputs,  X_ref(case) -> {tensor name: (float64 reference, bound)}  and
X_eval32(case, defect=None) -> {tensor name: fp32 value}.  The references are computed end to end in float64 from the
fp32 inputs; a backward kernel is handed the forward's own fp32 results (lse, stats, ...), so its bound carries the
forward's bound.  A comparison is per element: usage = |got - ref64| / bound of that element, as bn_pool_util.usage.

Constants.  e = 2^-24 (fp32 rounding), u = 2^-8 (bf16 store).  TINY = 2^-126: __expf flushes results below the
smallest normal fp32 to zero, so every bound on a probability carries TINY next to its relative part (float64 keeps
exp(-150), fp32 cannot).  F_EXP = F_LOG = 4 are the accuracy, in units of e relative to the result, assumed for the
hardware exp2 / log2 behind __expf / __logf (and, generously, for the libm expf / log1pf / sqrtf / division of the
sigmoid, norm and cosine kernels).  They are the ONLY unmeasured constants here: the ISA guide at hand does not state
the accuracy of v_exp_f32 / v_log_f32, so they are twice the 1 ulp usually quoted, and they are not tuned to any output.

Pieces, each order-free (no kernel's reduction tree is copied):

  sum        n fp32 terms in any order: (n + 1) e sum |term|  (n - 1 additions, each at most e of the running
             magnitude <= sum |term|, plus the rounding that formed a term and one for second order).
  dot        D products through the fp32 MFMA or FMAs: (D + 1) e sum_d |a_d b_d|.  A logit x = dot / T also rounds
             1 / T and the product with it: dx = (D + 3) e sum_d |a_d b_d| / T  (|x| <= sum |a b| / T).
  lse        L = m + ln z, z = sum_j exp(x_j - m) over n terms, p_j = exp(x_j - L):
               e (|m| + |L|)                      the final add (and the rounding of m where it is not an input)
             + (n + 1) e                          the sum z, relative to z, hence absolute in ln z
             + sum_j p_j (r |x_j - m| + F_EXP (1 + R) + R) e      the exponentials: r = 2 roundings proportional to
                                                  the argument (the subtraction, the log2 e scaling inside __expf;
                                                  r = 3 where the kernel also multiplies by 1 / T inside), F_EXP
                                                  for exp2.  R counts online rescales z <- z exp(m_old - m_new):
                                                  the arguments of the chain telescope to x_j - m exactly (m only
                                                  grows), so only F_EXP + 1 (the exp and the multiply) recur.
                                                  R = 0 for the one-pass kernels, 1 for the InfoNCE finalize and
                                                  ceil(tiles / 4) + 5 for NT-Xent (tiles of a wave, two lane merges,
                                                  three wave merges).
             + F_LOG e (1 + |ln z|)               the logarithm
             + sum_j p_j dx_j                     where the x_j are themselves computed (d lse / d x_j = p_j).
  loss term  l - s_label, l T - sum t s, lse - lp:  the lse bound (and the bounds of T, the dot and the positive
             logit) + e times the magnitudes that cancel + 3 e |term| for the subtraction, 1 / N and the product.
  prob       fp32 exp(x - L) against p: p (r |x - L| e + B_lse + F_EXP e + dx) + TINY.
             (a flush to zero costs the whole p <= TINY (1 + rel), which p rel + TINY covers since p >= TINY there.)
  gradient   k (p - t), k (p T - t): |k| (prob bound (x T, + p B_T + e p T for the product) + 6 e |p T - t|),
             + u |value| for a bf16 store.  Relative to the element's own probability, never to the tensor maximum.
             6 e: three roundings (the subtraction, k = g / N, the product) hit every element, a float32
             evaluation reaches 1.8 e of the 3 e they allow, and it is to stay within half of the bound.
  fused      sum_j coef_j vec_jd (InfoNCE dq, NT-Xent d a / b / A / B, clip_logits_bwd):
             sum_j ((n + 1) e |coef_j| + B_coef_j) |vec_jd|, B_coef from the gradient line; + 4 e of the magnitude
             for the roundings of the common factor g / (T N).
  scalar     mean / sum over rows: the sum of the rows' bounds + the sum bound over the row terms.
  accuracy   a row is AMBIGUOUS for top-k when the label's score lies within the two logits' dx of enough other
             scores that its top-k status could flip.  The kernel's figure must lie between 100 / N x (sure hits)
             and 100 / N x (sure hits + ambiguous rows), to within ACC_TOL = 1e-3.  For the dense-row kernels dx = 0:
             ties are exact, the lower index wins, no row is ambiguous.  Ambiguous rows are allowed in the kinds
             `duplicate` and `collapsed` only, and no more than were planted (planted_rows); the host test checks it.

Kernel by kernel.

  softmax_ce    lse: the lse bound (r = 2, R = 0, dx = 0).  terms[0] = (l - s_label) / N: (B_lse + e (|L| + |s|)) / N
                + 3 e |term|.  out[0]: scalar.  out[1 / 2]: accuracy (exact ranks).  ds: gradient.  A label outside
                [0, C) makes terms[0][row] and out[0] NaN and leaves lse[row] within its bound.
  sigmoid_ce    term_j = max(x, 0) - x t + log1p(exp(-|x|)) =: a - b + c:  3 e (|a| + |b|) + (F_EXP + F_LOG) e c
                per element; row = sum_j / N: the sum bound over a + |b| + c, + 2 e |row|.  ds = (sig - t) k:
                |k| ((F_EXP + 4) e sig + 6 e |sig - t|) + TINY |k|  (exp, the add and the division are relative
                errors of sig; the two roundings are counted twice, as F_EXP is twice the 1 ulp of a good exp: a
                float32 evaluation with a 1-ulp exp can err by 4 e sig, and the bound is to be twice that).
                t_on = 1, t_off = fp32(0.1) (ViTCELoss(type='sigmoid') with epsilon 0.1).
  soft_ce       T = sum t: sum bound.  dot = sum t s: (C + 2) e sum |t s|.  terms[0] = (l T - dot) / N:
                (|T| B_lse + |L| B_T + B_dot + 2 e (|L T| + |dot|)) / N + 3 e |term|.  ds = k (p T - t): gradient.
                The label is the first arg-max of the target; ranks are exact.
  l2norm        ss = sum x^2 has relative error (D + 2) e; nrm = max(sqrt(ss), eps): ((D + 2) / 2 + 1) e nrm, exact
                on the clamped (all-zero) row; y = x (1 / nrm): ((D + 2) / 2 + 3) e |y|.  l2norm_bwd is handed y and
                nrm: dx = (dy - y dot) / nrm, dot = sum dy y: (|y| B_dot + 4 e (|dy| + |y dot|)) / nrm + u |dx|
                (1 / nrm, the product y dot, the subtraction, the product with 1 / nrm).
  cosine        d = a . b: dot.  na, nb: relative (D + 2) e.  dc = max(sqrt(na nb), eps): relative (D + 4) e or exact.
                cos = d / dc: B_d / dc + (D + 6) e |cos|.  loss = -mean cos: scalar + 2 e |loss|.  The live flag is
                exact (no case has sqrt(na nb) near eps).  cosine_bwd is handed stats:  da = (k / dc) b -
                (k cos / na) a: 5 e (|kb b| + |ka a|).
  clip_logits   alpha = expf(s): F_EXP e alpha.  y = x / |x|: as l2norm without the clamp, inv likewise.  L_ij =
                alpha y_i . t_j: alpha sum_d |y_id t_jd| ((D + 1) + 2 ((D + 2) / 2 + 3)) e + (F_EXP + 2) e |L|.
                The reference of an all-zero row is NaN as in the model this follows (features / features.norm());
                no case has one: clip_norm_kernel's 1 / sqrt(0) is the reference's own behaviour, not a defect.
  clip_ce       row and column lse of L with dx = B_L; terms (l - L_ii) / B as the loss term; out = (rows, columns,
                their sum): scalar.  dL = k (p_row + p_col - 2 [i = j]): the gradient line with two probabilities
                (+ e (p_row + p_col) for their sum).
  clip_logits_bwd  judged on the fp32 operands it is handed (dL, L and the workspace y, inv, alpha of the forward
                launch, taken as float64): an entry point of its own whose inputs are tensors.  d y_i = alpha sum_j
                G_ij t_j: B_dy = (B + 3) e alpha sum_j |G_ij| |t_jd| (the sum and the product with alpha).
                dx = (dy - y <y, dy>) inv: (B_dy + |y| (sum_d |y_d| B_dy_d + (D + 1) e sum |y dy|)
                + 4 e (|dy| + |y <y, dy>|)) inv.  d scale += sum G L: (B^2 + 1) e sum |G L| + 2 e (|fill| + |sum|).
  infonce       x_i0 = q_i . k_i / T, x_ij = q_i . queue_j / T with dx; lse with r = 3, R = 1, n = K + 1; row term
                lse - lp: B_lse + dx_0 + e (|L| + |lp|) + e |term|; out[0] mean: scalar / N.  logits: dx.
                dq = coef (sum_j p_j queue_j + (p_0 - 1) k_i): fused.  Ranks count queue logits ABOVE the positive
                (strict): ambiguous within dx_j + dx_0.
  ntxent        the four lse (R = ceil(tiles / 4) + 5), pos: dx; kl = sum_j (Pb_j - Pa_j)(y_j - x_j) formed as
                wy / zy - wx / zx: for w / z = sum P_j d_j:  sum_j P_j (rel_j |d_j| + dd_j) + (n + 2 + R) e sum P |d|
                + |sum P d| ((n + 1) e + sum_j P_j rel_j), rel_j the relative part of prob, dd_j = dx of its two
                logits + e |d_j|; the two halves add, + e |kl|.  term = (lce_a - pos) + (lce_b - pos) + w kl: the
                parts' bounds + 2 e of the magnitudes.  Gradients: fused with n = 2 x swept rows; each coefficient
                is a sum of probabilities, each with its prob bound, + 4 e of the coefficient's magnitude.

Which case catches which planted defect (test_planted_defect in the host test):
  last column dropped                    softmax 3x5-plain (lse), soft 8x16-plain-random (lse)
  last 128-column slice dropped          infonce 15x256-plain (lse)
  maximum not subtracted                 softmax 3x5-large (lse: the sum overflows)
  label off by one                       softmax 5x64-far_label (terms), sigmoid 5x64-plain (terms)
  self mask missing                      ntxent 8-8-0-plain-w3 (lce_a)
  positive not masked in the CO2 terms   ntxent 8-8-0-plain-w3 (lx)
  1 / N taken as 1 / (N C)               softmax 3x5-plain (ds), sigmoid 3x5-plain (ds)
  slices beyond the 64th ignored         infonce 17x8320-plain (lse)
  column block beyond the first ignored  clip 257x16-plain (lse)
  all-invalid lanes' unit terms left     ntxent 2-2-0-plain-w3 (lce_a)
"""
import functools
import math

import torch

INF = float('inf')


# usage / verdict as in bn_pool_util.py (repeated here: that module imports the package, this one is pure torch)
def _ratios(got, ref, bound):
    """|got - ref| / bound per element (flat).  A bound of 0 admits no error; NaN counts as inf."""
    err, bound = (got.double().flatten() - ref.flatten()).abs(), bound.flatten()
    r = err / bound.clamp_min(1e-300)
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    return torch.where(torch.isnan(err) | ((bound == 0) & (err > 0)), torch.full_like(r, INF), r)


def usage(got, ref, bound):
    """(worst |got - ref| / bound, flat index of that element)."""
    ratio = _ratios(got, ref, bound)
    idx = int(ratio.argmax())
    return float(ratio[idx]), idx


def verdict(what, tensor, ratio, idx):
    """None if the bound holds, else the message the tests raise."""
    if ratio <= 1:
        return None
    return '%s: %s exceeds its bound at flat index %d: error = %.4g x bound' % (what, tensor, idx, ratio)


E = 2.0 ** -24
U_BF16 = 2.0 ** -8
TINY = 2.0 ** -126
F_EXP = 4.0           # unmeasured: accuracy of the hardware exp2 behind __expf, in e relative to the result
F_LOG = 4.0           # unmeasured: accuracy of the hardware log2 behind __logf
ACC_TOL = 1e-3
HEADROOM = 0.5        # the float32 evaluation may use this share of a bound
GLOSS = float(torch.tensor(1.7, dtype=torch.float32))
T_ON, T_OFF = 1.0, float(torch.tensor(0.1, dtype=torch.float32))
NEG = -INF


def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


def _gen(*key):
    return torch.Generator().manual_seed(_seed(*key))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ pieces
def sum_bound(terms, dim=-1, extra=0):
    """(n + 1 + extra) e sum |term| over dim."""
    return (terms.shape[dim] + 1 + extra) * E * terms.abs().sum(dim)


def lse_parts(x, dx=None, rounds=2, rescales=0):
    """x float64 [.., n] (masked entries -inf; they do not count in n) -> L, B_lse [..], p [.., n]."""
    m = x.max(-1, keepdim=True).values
    z = torch.exp(x - m).sum(-1, keepdim=True)
    L = m + torch.log(z)
    p = torch.exp(x - L)
    live = torch.isfinite(x)
    n = live.sum(-1, keepdim=True).double()
    gap = torch.where(live, (x - m).abs(), torch.zeros_like(x))
    trans = (p * (rounds * gap + F_EXP * (1 + rescales) + rescales)).sum(-1, keepdim=True)
    B = E * (m.abs() + L.abs()) + (n + 1) * E + E * trans + F_LOG * E * (1 + torch.log(z).abs())
    if dx is not None:
        B = B + (p * dx).sum(-1, keepdim=True)
    return L.squeeze(-1), B.squeeze(-1), p


def prob_rel(p, x, L, BL, dx=0.0, rounds=2):
    """Relative part of the prob bound (0 where the entry is masked)."""
    live = torch.isfinite(x)
    gap = torch.where(live, (x - L).abs(), torch.zeros_like(x))
    return torch.where(live, rounds * gap * E + BL + F_EXP * E + dx, torch.zeros_like(x))


def prob_bound(p, x, L, BL, dx=0.0, rounds=2):
    return p * prob_rel(p, x, L, BL, dx, rounds) + TINY


def first_argmax(t):
    C = t.shape[-1]
    j = torch.arange(C).expand_as(t)
    return torch.where(t == t.max(-1, keepdim=True).values, j, torch.full_like(j, C)).min(-1).values


def exact_ranks(x, lab):
    """#{j : x_j > x_lab or (x_j == x_lab and j < lab)} per row (x float64 or fp32: exact either way)."""
    sl = x.gather(1, lab.view(-1, 1))
    j = torch.arange(x.shape[1]).view(1, -1)
    return ((x > sl) | ((x == sl) & (j < lab.view(-1, 1)))).sum(1)


def acc_interval(lo_cnt, hi_cnt, k):
    """100 / N x (sure hits), 100 / N x (possible hits), ambiguous rows, for `fewer than k scores above the label`
    with the count known to lie in [lo_cnt, hi_cnt] per row."""
    sure, possible = hi_cnt < k, lo_cnt < k
    n = lo_cnt.shape[0]
    return 100.0 * float(sure.sum()) / n, 100.0 * float(possible.sum()) / n, possible & ~sure


def acc_ok(got, interval):
    return interval[0] - ACC_TOL <= float(got) <= interval[1] + ACC_TOL


# ------------------------------------------------------------------------------------------------ dense-row CE
CE_SHAPES = ((1, 1), (3, 5), (5, 64), (4, 65), (7, 1000), (33, 1001))
CE_KINDS = ('plain', 'large', 'peaked', 'flat', 'far_label', 'offset')
CE_CASES = tuple((s, k) for s in CE_SHAPES for k in CE_KINDS)
BADLABEL_CASES = tuple(((5, 64), k) for k in CE_KINDS)          # row 1's label is C (even kinds) or -1 (odd kinds)
SOFT_SHAPES = ((8, 16), (5, 1001), (3, 1000))
SOFT_TARGETS = ('mixup', 'random')
SOFT_CASES = tuple((s, k, t) for s in SOFT_SHAPES for k in CE_KINDS for t in SOFT_TARGETS)
SOFT_UNALIGNED = ((3, 1000), 'plain', 'mixup')                 # run with every operand 4 bytes off a 16-byte boundary


def ce_id(case):
    return '%dx%d-%s' % (case[0] + tuple(case[1:2])) + ''.join('-' + t for t in case[2:])


def scores(kind, N, C, gen, labels=None):
    """fp32 scores [N, C] of an input family and the int64 labels they were built around."""
    if labels is None:
        labels = torch.randint(0, C, (N,), generator=gen)
    s = torch.randn(N, C, generator=gen) * 3
    rows = torch.arange(N)
    if kind == 'large':
        s = s * 10 + 50
    elif kind == 'peaked':                                     # the peak is the label on even rows only
        pk = torch.where(rows % 2 == 0, labels, torch.randint(0, C, (N,), generator=gen))
        s[rows, pk] = s.max(1).values + 80
    elif kind == 'flat':
        s = torch.full((N, C), 7.25)
    elif kind == 'far_label' and C > 1:
        s[rows, labels] = NEG
        s[rows, labels] = s.max(1).values - 60
    elif kind == 'offset':
        s = s - 1e4
    return s.float(), labels


@functools.lru_cache(maxsize=None)
def ce_data(case):
    (N, C), kind = case
    s, lab = scores(kind, N, C, _gen(N, C, CE_KINDS.index(kind), 1))
    return dict(s=s, labels=lab)


def bad_labels(case):
    (N, C), kind = case
    lab = ce_data(case)['labels'].clone()
    lab[1] = C if CE_KINDS.index(kind) % 2 == 0 else -1
    return lab


@functools.lru_cache(maxsize=None)
def soft_data(case):
    (N, C), kind, tk = case
    gen = _gen(N, C, CE_KINDS.index(kind), SOFT_TARGETS.index(tk), 2)
    if tk == 'mixup':
        y1 = torch.randint(0, C, (N,), generator=gen)
        y2 = y1.flip(0)
        lam, eps = 0.7, 0.1
        off, on = eps / C, 1 - eps + eps / C
        j = torch.arange(C).view(1, -1)
        t = (torch.where(j == y1.view(-1, 1), on, off) * lam + torch.where(j == y2.view(-1, 1), on, off) * (1 - lam))
        t = t.float()
    else:
        t = torch.rand(N, C, generator=gen)
        t = (t / t.sum(1, keepdim=True)).float()
    lab = first_argmax(t)
    s, _ = scores(kind, N, C, gen, lab)
    return dict(s=s, t=t, labels=lab)


def _grad_ce(k, p, pb, t, scale=None, Bscale=None):
    """ds = k (p scale - t) and its bound; pb the prob bound of p."""
    pt = p if scale is None else p * scale
    Bp = pb if scale is None else pb * scale.abs() + p * Bscale + E * pt.abs()        # + the product p T
    ds = k * (pt - t)
    return ds, abs(k) * (Bp + 6 * E * (pt - t).abs())


def _ce_scalars(term, Bterm):
    return term.sum(), Bterm.sum() + sum_bound(term)


@functools.lru_cache(maxsize=None)
def softmax_ref(case):
    (N, C), kind = case
    d = ce_data(case)
    x, lab = d['s'].double(), d['labels']
    L, BL, p = lse_parts(x)
    sl = x.gather(1, lab.view(-1, 1)).squeeze(1)
    term = (L - sl) / N
    Bterm = (BL + E * (L.abs() + sl.abs())) / N + 3 * E * term.abs()
    loss, Bloss = _ce_scalars(term, Bterm)
    cnt = exact_ranks(x, lab)
    onehot = torch.zeros_like(x).scatter_(1, lab.view(-1, 1), 1.0)
    ds, Bds = _grad_ce(GLOSS / N, p, prob_bound(p, x, L.unsqueeze(1), BL.unsqueeze(1)), onehot)
    return dict(lse=(L, BL), terms=(term, Bterm), loss=(loss, Bloss), ds=(ds, Bds),
                acc1=acc_interval(cnt, cnt, 1), acc5=acc_interval(cnt, cnt, 5))


def softmax_eval32(case, defect=None):
    (N, C), kind = case
    d = ce_data(case)
    s, lab = d['s'], d['labels']
    if defect == 'label_off':
        lab = (lab + 1) % C
    body = s[:, :-1] if defect == 'drop_last_col' else s
    m = torch.zeros(N, 1) if defect == 'no_max' else s.max(1, keepdim=True).values
    l = (m + torch.log(torch.exp(body - m).sum(1, keepdim=True))).squeeze(1)
    sl = s.gather(1, lab.view(-1, 1)).squeeze(1)
    invN = torch.tensor(1.0 / N, dtype=torch.float32)
    term = (l - sl) * invN
    cnt = exact_ranks(s, lab)
    k = torch.tensor(GLOSS, dtype=torch.float32) / (N * C if defect == 'invNC' else N)
    onehot = torch.zeros_like(s).scatter_(1, lab.view(-1, 1), 1.0)
    ds = k * (torch.exp(s - l.unsqueeze(1)) - onehot)
    return dict(lse=l, terms=term, loss=term.sum(), ds=ds, acc1=100.0 * float((cnt < 1).sum()) / N,
                acc5=100.0 * float((cnt < 5).sum()) / N)


def _sigmoid_target(lab, C):
    j = torch.arange(C).view(1, -1)
    return torch.where(j == lab.view(-1, 1), torch.tensor(T_ON, dtype=torch.float64),
                       torch.tensor(T_OFF, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def sigmoid_ref(case):
    (N, C), kind = case
    d = ce_data(case)
    x, lab = d['s'].double(), d['labels']
    t = _sigmoid_target(lab, C)
    a, b, c = x.clamp_min(0), x * t, torch.log1p(torch.exp(-x.abs()))
    el = a - b + c
    Bel = 3 * E * (a + b.abs()) + (F_EXP + F_LOG) * E * c
    term = el.sum(1) / N
    Bterm = (Bel.sum(1) + sum_bound(a + b.abs() + c)) / N + 2 * E * term.abs()
    loss, Bloss = _ce_scalars(term, Bterm)
    sig = torch.sigmoid(x)
    k = GLOSS / N
    ds = (sig - t) * k
    Bds = abs(k) * ((F_EXP + 4) * E * sig + 6 * E * (sig - t).abs()) + TINY * abs(k)
    return dict(terms=(term, Bterm), loss=(loss, Bloss), ds=(ds, Bds))


def sigmoid_eval32(case, defect=None):
    (N, C), kind = case
    d = ce_data(case)
    s, lab = d['s'], d['labels']
    if defect == 'label_off':
        lab = (lab + 1) % C
    t = _sigmoid_target(lab, C).float()
    el = s.clamp_min(0) - s * t + torch.log1p(torch.exp(-s.abs()))
    term = el.sum(1) / N
    k = torch.tensor(GLOSS, dtype=torch.float32) / (N * C if defect == 'invNC' else N)
    ds = (1.0 / (1.0 + torch.exp(-s)) - t) * k
    return dict(terms=term, loss=term.sum(), ds=ds)


@functools.lru_cache(maxsize=None)
def soft_ref(case):
    (N, C), kind, tk = case
    d = soft_data(case)
    x, t, lab = d['s'].double(), d['t'].double(), d['labels']
    L, BL, p = lse_parts(x)
    T, BT = t.sum(1), sum_bound(t)
    dot, Bdot = (t * x).sum(1), sum_bound(t * x, extra=1)
    term = (L * T - dot) / N
    Bterm = (T.abs() * BL + L.abs() * BT + Bdot + 2 * E * ((L * T).abs() + dot.abs())) / N + 3 * E * term.abs()
    loss, Bloss = _ce_scalars(term, Bterm)
    cnt = exact_ranks(x, lab)
    ds, Bds = _grad_ce(GLOSS / N, p, prob_bound(p, x, L.unsqueeze(1), BL.unsqueeze(1)), t, T.unsqueeze(1),
                       BT.unsqueeze(1))
    return dict(lse=(L, BL), tsum=(T, BT), terms=(term, Bterm), loss=(loss, Bloss), ds=(ds, Bds),
                acc1=acc_interval(cnt, cnt, 1), acc5=acc_interval(cnt, cnt, 5))


def soft_eval32(case, defect=None):
    (N, C), kind, tk = case
    d = soft_data(case)
    s, t, lab = d['s'], d['t'], d['labels']
    body = s[:, :-1] if defect == 'drop_last_col' else s
    m = s.max(1, keepdim=True).values
    l = (m + torch.log(torch.exp(body - m).sum(1, keepdim=True))).squeeze(1)
    T, dot = t.sum(1), (t * s).sum(1)
    term = (l * T - dot) * torch.tensor(1.0 / N, dtype=torch.float32)
    cnt = exact_ranks(s, lab)
    k = torch.tensor(GLOSS, dtype=torch.float32) / N
    ds = k * (torch.exp(s - l.unsqueeze(1)) * T.unsqueeze(1) - t)
    return dict(lse=l, tsum=T, terms=term, loss=term.sum(), ds=ds, acc1=100.0 * float((cnt < 1).sum()) / N,
                acc5=100.0 * float((cnt < 5).sum()) / N)


# ------------------------------------------------------------------------------------------------ embeddings
EMB_KINDS = ('plain', 'cold', 'unnormalised', 'collapsed', 'duplicate')


def temperature(kind):
    return f32(0.02 if kind == 'cold' else 0.2)


def emb(kind, n, D, gen):
    """fp32 rows [n, D]: unit norm (to fp32 rounding), norm 3 for `unnormalised`, one repeated row for `collapsed`."""
    x = torch.randn(1 if kind == 'collapsed' else n, D, generator=gen).double()
    x = x / x.norm(dim=1, keepdim=True)
    if kind == 'unnormalised':
        x = x * 3
    return x.float().expand(n, D).contiguous()


def dot_dx(a, b, invT=1.0):
    """dx of the logits a . b^T * invT: (D + 3) e sum_d |a_d b_d| invT; a [n, D], b [m, D] float64."""
    return (a.shape[1] + 3) * E * (a.abs() @ b.abs().t()) * invT


# ---- l2norm / cosine
ROW_SHAPES = ((1, 1), (3, 63), (5, 64), (4, 65), (6, 2048))
ROW_KINDS = ('plain', 'unnormalised', 'collapsed')
ROW_CASES = tuple((s, k) for s in ROW_SHAPES for k in ROW_KINDS)
L2_EPS, COS_EPS = f32(1e-12), f32(1e-8)


def row_id(case):
    return '%dx%d-%s' % (case[0] + (case[1],))


@functools.lru_cache(maxsize=None)
def row_data(case):
    """x (= a), b, dy [N, D]; row N // 2 of x is all zero (the eps clamp of both kernels)."""
    (N, D), kind = case
    gen = _gen(N, D, ROW_KINDS.index(kind), 3)
    x, b = emb(kind, N, D, gen), emb('plain', N, D, gen)
    x[N // 2] = 0
    return dict(x=x, b=b, dy=torch.randn(N, D, generator=gen))


def _norm_ref(x, eps=None):
    """nrm, B_nrm, y, B_y of y = x / max(|x|, eps) (eps None: no clamp)."""
    D = x.shape[1]
    nrm = x.norm(dim=1)
    clamped = torch.zeros_like(nrm, dtype=torch.bool) if eps is None else nrm < eps
    nrm = torch.where(clamped, torch.full_like(nrm, eps or 0.0), nrm)
    Bn = torch.where(clamped, torch.zeros_like(nrm), ((D + 2) / 2 + 1) * E * nrm)
    y = x / nrm.unsqueeze(1)
    return nrm, Bn, y, ((D + 2) / 2 + 3) * E * y.abs()


@functools.lru_cache(maxsize=None)
def l2norm_ref(case):
    d = row_data(case)
    x, dy = d['x'].double(), d['dy'].double()
    nrm, Bn, y, By = _norm_ref(x, L2_EPS)
    return dict(norm=(nrm, Bn), y=(y, By))


def l2norm_bwd_ref(dy, y, norm, u=0.0):
    """dx64 and its bound from the fp32 operands the kernel is handed."""
    dy, y, norm = dy.double(), y.double(), norm.double().unsqueeze(1)
    dot = (dy * y).sum(1, keepdim=True)
    Bdot = sum_bound(dy * y).unsqueeze(1)
    dx = (dy - y * dot) / norm
    return dx, (y.abs() * Bdot + 4 * E * (dy.abs() + (y * dot).abs())) / norm + u * dx.abs()


def l2norm_eval32(case, defect=None):
    d = row_data(case)
    x, dy = d['x'], d['dy']
    nrm = torch.sqrt((x * x).sum(1)).clamp_min(L2_EPS)
    y = x * (1.0 / nrm).unsqueeze(1)
    dot = (dy * y).sum(1, keepdim=True)
    dx = (dy - y * dot) * (1.0 / nrm).unsqueeze(1)
    return dict(norm=nrm, y=y, dx=dx, dx_bf16=dx.to(torch.bfloat16).float())


@functools.lru_cache(maxsize=None)
def cosine_ref(case):
    (N, D), kind = case
    d = row_data(case)
    a, b = d['x'].double(), d['b'].double()
    dd, Bd = (a * b).sum(1), sum_bound(a * b)
    na, nb = (a * a).sum(1), (b * b).sum(1)
    den = torch.sqrt(na * nb)
    live = den > COS_EPS
    dc = torch.where(live, den, torch.full_like(den, COS_EPS))
    cs = dd / dc
    Bcs = Bd / dc + (D + 6) * E * cs.abs()
    stats = torch.stack([cs, na, dc, live.double()], 1)
    Bstats = torch.stack([Bcs, (D + 2) * E * na, torch.where(live, (D + 4) * E * dc, torch.zeros_like(dc)),
                          torch.zeros_like(cs)], 1)
    loss = -cs.sum() / N
    Bloss = (Bcs.sum() + sum_bound(cs)) / N + 2 * E * loss.abs()
    return dict(stats=(stats, Bstats), loss=(loss, Bloss))


def cosine_bwd_ref(a, b, stats):
    """da64 and its bound from the fp32 stats the kernel is handed."""
    a, b, st = a.double(), b.double(), stats.double()
    N = a.shape[0]
    k = -GLOSS / N
    kb = (k / st[:, 2]).unsqueeze(1)
    ka = torch.where(st[:, 3] != 0, k * st[:, 0] / st[:, 1].clamp_min(1e-300), torch.zeros(N, dtype=torch.float64))
    ka = ka.unsqueeze(1)
    return kb * b - ka * a, 5 * E * ((kb * b).abs() + (ka * a).abs())


def cosine_eval32(case, defect=None):
    (N, D), kind = case
    d = row_data(case)
    a, b = d['x'], d['b']
    dd, na, nb = (a * b).sum(1), (a * a).sum(1), (b * b).sum(1)
    den = torch.sqrt(na * nb)
    dc = den.clamp_min(COS_EPS)
    live = den > COS_EPS
    stats = torch.stack([dd / dc, na, dc, live.float()], 1)
    k = -torch.tensor(GLOSS, dtype=torch.float32) / N
    kb = (k / dc).unsqueeze(1)
    ka = torch.where(live, k * stats[:, 0] / na, torch.zeros(N)).unsqueeze(1)
    return dict(stats=stats, loss=-stats[:, 0].sum() / N, da=kb * b - ka * a)


# ------------------------------------------------------------------------------------------------ InfoNCE
DIM = 128                                                      # the feature dimension head.hip / ntxent.hip are tiled for
INFONCE_SHAPES = tuple((N, K) for N in (1, 15, 17, 64, 70) for K in (128, 256, 8320))
INFONCE_CASES = tuple((s, k) for i, s in enumerate(INFONCE_SHAPES) for k in ('plain', EMB_KINDS[1 + i % 4]))


def infonce_id(case):
    return '%dx%d-%s' % (case[0] + (case[1],))


@functools.lru_cache(maxsize=None)
def infonce_data(case):
    """q, k [N, 128], queue [128, K], T.  `duplicate`: the queue columns 5, K / 2 + 1, K - 1 hold the keys of rows
    0, 1, 2; `collapsed`: q, k and every queue column are one unit vector."""
    (N, K), kind = case
    gen = _gen(N, K, EMB_KINDS.index(kind), 4)
    q = emb(kind, N, DIM, gen)
    k = q.clone() if kind == 'collapsed' else emb(kind, N, DIM, gen)
    queue = q[:1].expand(K, DIM) if kind == 'collapsed' else emb(kind, K, DIM, gen)
    queue = queue.t().contiguous()
    if kind == 'duplicate':
        for i, col in enumerate((5, K // 2 + 1, K - 1)[:min(N, 3)]):
            queue[:, col] = k[i]
    return dict(q=q, k=k, queue=queue, T=temperature(kind))


def planted_rows(case):
    """Rows whose accuracy the case makes ambiguous on purpose (0 for every kind but `duplicate` / `collapsed`)."""
    kind = case[1]
    n = case[0][0]
    if kind == 'collapsed':
        return n
    if kind != 'duplicate':
        return 0
    return min(n, 3) if len(case[0]) == 2 else 2 * min(2, n // 2)


@functools.lru_cache(maxsize=None)
def infonce_ref(case):
    (N, K), kind = case
    d = infonce_data(case)
    q, k, Q, invT = d['q'].double(), d['k'].double(), d['queue'].double(), 1.0 / d['T']
    x0, xn = (q * k).sum(1, keepdim=True) * invT, q @ Q * invT
    dx0, dxn = (DIM + 3) * E * (q * k).abs().sum(1, keepdim=True) * invT, dot_dx(q, Q.t(), invT)
    x, dx = torch.cat([x0, xn], 1), torch.cat([dx0, dxn], 1)
    L, BL, p = lse_parts(x, dx, rounds=3, rescales=1)
    term = L - x0.squeeze(1)
    Bterm = BL + dx0.squeeze(1) + E * (L.abs() + x0.squeeze(1).abs()) + E * term.abs()
    loss = term.sum() / N
    Bloss = (Bterm.sum() + sum_bound(term)) / N + 2 * E * loss.abs()
    lo, hi = (xn > x0 + (dxn + dx0)).sum(1), (xn >= x0 - (dxn + dx0)).sum(1)
    # dq for a unit upstream gradient: linear in gscale
    coef = invT / N
    rel = prob_rel(p, x, L.unsqueeze(1), BL.unsqueeze(1), dx, rounds=3) + 3 * E
    pn, p0 = p[:, 1:], p[:, :1]
    dq = coef * (pn @ Q.t() + (p0 - 1) * k)
    Bdq = coef * (((K + 2) * E * pn + pn * rel[:, 1:] + TINY) @ Q.abs().t()
                  + k.abs() * (p0 * rel[:, :1] + TINY + (K + 5) * E * (p0 - 1).abs())
                  + 4 * E * (pn @ Q.abs().t() + (p0 - 1).abs() * k.abs()))
    return dict(lse=(L, BL), logits=(x, dx + E * x.abs()), loss=(loss, Bloss), dq=(dq, Bdq),
                acc1=acc_interval(lo, hi, 1), acc5=acc_interval(lo, hi, 5))


def ambiguous_rows(ref):
    return int((ref['acc1'][2] | ref['acc5'][2]).sum()) if 'acc5' in ref else int(ref['acc1'][2].sum())


def infonce_eval32(case, defect=None):
    (N, K), kind = case
    d = infonce_data(case)
    q, k, Q = d['q'], d['k'], d['queue']
    invT = torch.tensor(1.0) / torch.tensor(d['T'])
    x0, xn = (q * k).sum(1, keepdim=True) * invT, (q @ Q) * invT
    seen = xn[:, :-128] if defect == 'drop_last_slice' else xn[:, :64 * 128] if defect == 'finalize64' else xn
    x = torch.cat([x0, seen], 1)
    m = x.max(1, keepdim=True).values
    l = m + torch.log(torch.exp(x - m).sum(1, keepdim=True))
    term = (l - x0).squeeze(1)
    cnt = (xn > x0).sum(1)
    coef = invT / N
    dq = (torch.exp(xn - l) * coef) @ Q.t() + (torch.exp(x0 - l) - 1.0) * coef * k
    return dict(lse=l.squeeze(1), logits=torch.cat([x0, xn], 1), loss=term.sum() / N, dq=dq,
                acc1=100.0 * float((cnt < 1).sum()) / N, acc5=100.0 * float((cnt < 5).sum()) / N)


# ------------------------------------------------------------------------------------------------ CLIP
CLIP_SHAPES = tuple((B, D) for B in (1, 3, 37, 64, 65, 257) for D in (16, 48, 512))
CLIP_CASES = tuple((s, k) for i, s in enumerate(CLIP_SHAPES) for k in ('plain', EMB_KINDS[1 + i % 4]))
CLIP_LO, CLIP_HI = f32(-4.6), f32(4.6)
DSCALE_FILL = 0.25                                             # d logit_scale accumulates into this


@functools.lru_cache(maxsize=None)
def clip_data(case):
    """img, txt [B, D], logit_scale = ln(1 / T).  `duplicate`: txt rows B - 1 - i = txt rows i (i < min(3, B / 2)), so
    column B - 1 - i of the logits equals the positive column of row i."""
    (B, D), kind = case
    gen = _gen(B, D, EMB_KINDS.index(kind), 5)
    img = emb(kind, B, D, gen)
    txt = img.clone() if kind == 'collapsed' else emb(kind, B, D, gen)
    if kind == 'duplicate':
        for i in range(min(3, B // 2)):
            txt[B - 1 - i] = txt[i]
    return dict(img=img, txt=txt, scale=f32(math.log(1.0 / temperature(kind))))


def _two_lse(Lg, BLg):
    Lr, BLr, pr = lse_parts(Lg, BLg)
    Lc, BLc, pc = lse_parts(Lg.t(), BLg.t())
    return Lr, BLr, pr, Lc, BLc, pc


@functools.lru_cache(maxsize=None)
def clip_ref(case):
    (B, D), kind = case
    d = clip_data(case)
    img, txt, s = d['img'].double(), d['txt'].double(), d['scale']
    alpha = math.exp(s)
    ni, _, yi, Byi = _norm_ref(img)
    nt, _, yt, Byt = _norm_ref(txt)
    inv = 1.0 / torch.cat([ni, nt])
    Lg = alpha * yi @ yt.t()
    BLg = alpha * (yi.abs() @ yt.abs().t()) * ((D + 1) + 2 * ((D + 2) / 2 + 3)) * E + (F_EXP + 2) * E * Lg.abs()
    Lr, BLr, pr, Lc, BLc, pc = _two_lse(Lg, BLg)
    diag, Bdiag = Lg.diagonal(), BLg.diagonal()
    out, Bout = [], []
    terms, Bterms = [], []
    for Lx, BLx in ((Lr, BLr), (Lc, BLc)):
        term = (Lx - diag) / B
        Bterm = (BLx + Bdiag + E * (Lx.abs() + diag.abs())) / B + 3 * E * term.abs()
        terms.append(term), Bterms.append(Bterm)
        out.append(term.sum()), Bout.append(Bterm.sum() + sum_bound(term))
    out.append(out[0] + out[1]), Bout.append(Bout[0] + Bout[1] + E * (out[0].abs() + out[1].abs()))
    k = GLOSS / B
    eye = torch.eye(B, dtype=torch.float64)
    pcT = pc.t()
    Bp = (prob_bound(pr, Lg, Lr.unsqueeze(1), BLr.unsqueeze(1), BLg)
          + prob_bound(pc, Lg.t(), Lc.unsqueeze(1), BLc.unsqueeze(1), BLg.t()).t())
    G = k * (pr + pcT - 2 * eye)
    BG = abs(k) * (Bp + E * (pr + pcT) + 6 * E * (pr + pcT - 2 * eye).abs())
    ws = torch.cat([yi.flatten(), yt.flatten(), inv, torch.tensor([alpha], dtype=torch.float64)])
    Bws = torch.cat([Byi.flatten(), Byt.flatten(), ((D + 2) / 2 + 2) * E * inv,
                     torch.tensor([F_EXP * E * alpha], dtype=torch.float64)])
    return dict(ws=(ws, Bws), logits=(Lg, BLg), lse=(torch.cat([Lr, Lc]), torch.cat([BLr, BLc])),
                terms=(torch.cat(terms), torch.cat(Bterms)), out=(torch.stack(out), torch.stack(Bout)), dlogits=(G, BG),
                scale=(torch.tensor(min(max(s, CLIP_LO), CLIP_HI), dtype=torch.float64), torch.zeros((), dtype=torch.float64)))


def clip_bwd_ref(dlogits, logits, ws, B, D):
    """dimg, dtxt, dscale (float64) and their bounds from the fp32 operands clip_logits_bwd is handed."""
    G, Lg, ws = dlogits.double().view(B, B), logits.double().view(B, B), ws.double()
    In, Tn = ws[:B * D].view(B, D), ws[B * D:2 * B * D].view(B, D)
    inv, alpha = ws[2 * B * D:2 * B * D + 2 * B], float(ws[2 * B * D + 2 * B])
    res = {}
    for name, Gm, X, Y, r in (('dimg', G, Tn, In, inv[:B]), ('dtxt', G.t(), In, Tn, inv[B:])):
        dy = alpha * Gm @ X
        Bdy = (B + 3) * E * alpha * (Gm.abs() @ X.abs())
        dot = (Y * dy).sum(1, keepdim=True)
        Bdot = (Y.abs() * Bdy).sum(1, keepdim=True) + sum_bound(Y * dy).unsqueeze(1)
        r = r.unsqueeze(1)
        res[name] = ((dy - Y * dot) * r, (Bdy + Y.abs() * Bdot + 4 * E * (dy.abs() + (Y * dot).abs())) * r)
    tot = (G * Lg).sum()
    res['dscale'] = (DSCALE_FILL + tot, sum_bound((G * Lg).flatten()) + 2 * E * (DSCALE_FILL + tot.abs()))
    return res


def clip_eval32(case, defect=None):
    (B, D), kind = case
    d = clip_data(case)
    img, txt = d['img'], d['txt']
    s = torch.tensor(d['scale'])
    alpha = torch.exp(s)
    ri, rt = 1.0 / torch.sqrt((img * img).sum(1)), 1.0 / torch.sqrt((txt * txt).sum(1))
    yi, yt = img * ri.unsqueeze(1), txt * rt.unsqueeze(1)
    Lg = alpha * (yi @ yt.t())
    lse = []
    for X in (Lg, Lg.t()):
        m = X.max(1, keepdim=True).values
        lse.append((m + torch.log(torch.exp(X - m).sum(1, keepdim=True))).squeeze(1))
    if defect == 'col_block':
        lse[1] = torch.where(torch.arange(B) < 256, lse[1], torch.zeros(B))
    invB = torch.tensor(1.0 / B, dtype=torch.float32)
    terms = [(l - Lg.diagonal()) * invB for l in lse]
    out = torch.stack([terms[0].sum(), terms[1].sum(), terms[0].sum() + terms[1].sum()])
    k = torch.tensor(GLOSS, dtype=torch.float32) / B
    G = k * (torch.exp(Lg - lse[0].unsqueeze(1)) + torch.exp(Lg - lse[1].unsqueeze(0)) - 2 * torch.eye(B))
    ws = torch.cat([yi.flatten(), yt.flatten(), ri, rt, alpha.view(1)])
    res = dict(ws=ws, logits=Lg, lse=torch.cat(lse), terms=torch.cat(terms), out=out, dlogits=G,
               scale=s.clamp(CLIP_LO, CLIP_HI))
    for name, Gm, X, Y, r in (('dimg', G, yt, yi, ri), ('dtxt', G.t(), yi, yt, rt)):
        dy = alpha * (Gm @ X)
        res[name] = (dy - Y * (Y * dy).sum(1, keepdim=True)) * r.unsqueeze(1)
    res['dscale'] = torch.tensor(DSCALE_FILL) + (G * Lg).sum()
    return res


# ------------------------------------------------------------------------------------------------ NT-Xent + CO2
NTX_SHAPES = ((2, 2, 0), (8, 8, 0), (15, 15, 0), (17, 17, 0), (33, 33, 0), (70, 70, 0),       # B, BL, roff
              (8, 32, 16), (5, 23, 9), (17, 70, 34))
NTX_CASES = tuple((s, k, w) for i, s in enumerate(NTX_SHAPES) for k in ('plain', EMB_KINDS[1 + i % 4])
                  for w in (0.0, 3.0))
NTX_ROWSTATS = ('lce_a', 'lce_b', 'lx', 'ly', 'kl', 'pos', 'cnt', 'term')


def ntx_id(case):
    return '%d-%d-%d-%s-w%d' % (case[0] + (case[1], case[2]))


def ntx_rescales(BL):
    return -(-(-(-BL // 16)) // 4) + 5


@functools.lru_cache(maxsize=None)
def ntx_data(case):
    """a, b [B, 128], A, Bl [BL, 128] with A[roff + i] = a_i, Bl[roff + i] = b_i.  `duplicate`: b rows B - 1 - i =
    b rows i (i < min(2, B / 2)): rows i and B - 1 - i each see a column equal to their positive."""
    (B, BL, roff), kind, w = case
    gen = _gen(B, BL, roff, EMB_KINDS.index(kind), 6)
    a = emb(kind, B, DIM, gen)
    b = a.clone() if kind == 'collapsed' else emb(kind, B, DIM, gen)
    if kind == 'duplicate':
        for i in range(min(2, B // 2)):
            b[B - 1 - i] = b[i]
    A = a[:1].expand(BL, DIM).contiguous() if kind == 'collapsed' else emb(kind, BL, DIM, gen)
    Bl = A.clone() if kind == 'collapsed' else emb(kind, BL, DIM, gen)
    A[roff:roff + B], Bl[roff:roff + B] = a, b
    return dict(a=a, b=b, A=A, Bl=Bl, T=temperature(kind))


def _wz(P, x, d, dxx, dd, R):
    """sum_j P_j d_j formed as (sum e_j d_j) / (sum e_j), and its bound."""
    live = torch.isfinite(x)
    m = x.max(1, keepdim=True).values
    gap = torch.where(live, (x - m).abs(), torch.zeros_like(x))
    rel = torch.where(live, 2 * gap * E + (F_EXP * (1 + R) + R) * E + dxx, torch.zeros_like(x))
    n = live.sum(1).double()
    S = (P * d).sum(1)
    Bd = ((P * (rel * d.abs() + dd)).sum(1) + (n + 2 + R) * E * (P * d.abs()).sum(1)
          + S.abs() * ((n + 1) * E + (P * rel).sum(1)) + E * S.abs())
    return S, Bd


@functools.lru_cache(maxsize=None)
def ntx_ref(case):
    (B, BL, roff), kind, w = case
    d = ntx_data(case)
    a, b, A, Bl, invT = d['a'].double(), d['b'].double(), d['A'].double(), d['Bl'].double(), 1.0 / d['T']
    R = ntx_rescales(BL)
    M = torch.zeros(B, BL, dtype=torch.bool)
    M[torch.arange(B), roff + torch.arange(B)] = True
    lg = {n: (u @ V.t() * invT, dot_dx(u, V, invT)) for n, u, V in (('aa', a, A), ('ab', a, Bl), ('ba', b, A), ('bb', b, Bl))}
    msk = lambda t: t.masked_fill(M, NEG)
    zero = lambda t: t.masked_fill(M, 0.0)
    pos = (a * b).sum(1) * invT
    dpos = (DIM + 3) * E * (a * b).abs().sum(1) * invT
    cat = lambda *t: torch.cat(t, 1)
    (aa, daa), (ab, dab), (ba, dba), (bb, dbb) = lg['aa'], lg['ab'], lg['ba'], lg['bb']
    lce_a, Bla, _ = lse_parts(cat(ab, msk(aa)), cat(dab, daa), rescales=R)
    lce_b, Blb, _ = lse_parts(cat(ba, msk(bb)), cat(dba, dbb), rescales=R)
    xx, yy = cat(msk(aa), msk(ab)), cat(msk(ba), msk(bb))
    dxx, dyy = cat(daa, dab), cat(dba, dbb)
    lx, Blx, Pa = lse_parts(xx, dxx, rescales=R)
    ly, Bly, Pb = lse_parts(yy, dyy, rescales=R)
    dd = cat(zero(ba - aa), zero(bb - ab))
    ddd = dxx + dyy + E * dd.abs()
    Sx, Bsx = _wz(Pa, xx, dd, dxx, ddd, R)
    Sy, Bsy = _wz(Pb, yy, dd, dyy, ddd, R)
    kl, Bkl = Sy - Sx, Bsy + Bsx + E * (Sy - Sx).abs()
    term = (lce_a - pos) + (lce_b - pos) + w * kl
    Bterm = Bla + Blb + 2 * dpos + abs(w) * Bkl + 2 * E * (lce_a.abs() + lce_b.abs() + 2 * pos.abs() + (w * kl).abs())
    loss = term.sum() / B
    Bloss = (Bterm.sum() + sum_bound(term)) / B + 2 * E * loss.abs()
    gap = dab + (dpos + E * pos.abs()).unsqueeze(1)
    lo = ((ab > pos.unsqueeze(1) + gap) & ~M).sum(1)
    hi = ((ab >= pos.unsqueeze(1) - gap) & ~M).sum(1)
    cnt, Bcnt = (lo + hi).double() / 2, (hi - lo).double() / 2
    stats = torch.stack([lce_a, lce_b, lx, ly, kl, pos, cnt, term], 1)
    # the count is no rounding matter: `cnt` below judges it (any value between the sure and the possible count)
    Bstats = torch.stack([Bla, Blb, Blx, Bly, Bkl, dpos + E * pos.abs(), torch.full_like(Bcnt, INF), Bterm], 1)
    # gradients for a unit upstream gradient (linear in gscale)
    coef = invT / B
    col = lambda t: t.unsqueeze(1)

    def prob(x, dxv, L, BLv, masked):
        p = torch.exp(x - col(L))
        Bp = prob_bound(p, x, col(L), col(BLv), dxv)
        return (zero(p), zero(Bp)) if masked else (p, Bp)
    e_ab, e_aa = prob(ab, dab, lce_a, Bla, False), prob(aa, daa, lce_a, Bla, True)
    e_ba, e_bb = prob(ba, dba, lce_b, Blb, False), prob(bb, dbb, lce_b, Blb, True)
    pa_aa, pa_ab = prob(aa, daa, lx, Blx, True), prob(ab, dab, lx, Blx, True)
    pb_ba, pb_bb = prob(ba, dba, ly, Bly, True), prob(bb, dbb, ly, Bly, True)
    Mf = M.double()

    def gco(e, hot, plus, minus):
        g = e[0] - hot * Mf + w * (plus[0] - minus[0])
        Bg = e[1] + abs(w) * (plus[1] + minus[1]) + 4 * E * (e[0] + hot * Mf + abs(w) * (plus[0] + minus[0]))
        return g, Bg
    g_aa, g_ab = gco(e_aa, 0, pa_aa, pb_ba), gco(e_ab, 1, pa_ab, pb_bb)
    g_ba, g_bb = gco(e_ba, 1, pb_ba, pa_aa), gco(e_bb, 0, pb_bb, pa_ab)

    def fused(g1, V1, g2, V2, n):
        val = coef * (g1[0] @ V1 + g2[0] @ V2)
        Bv = coef * ((g1[1] + (n + 5) * E * g1[0].abs()) @ V1.abs() + (g2[1] + (n + 5) * E * g2[0].abs()) @ V2.abs())
        return val, Bv
    tr = lambda g: (g[0].t(), g[1].t())
    return dict(rowstats=(stats, Bstats), cnt=(cnt, Bcnt), loss=(loss, Bloss), acc1=acc_interval(lo, hi, 1),
                da=fused(g_aa, A, g_ab, Bl, 2 * BL), db=fused(g_ba, A, g_bb, Bl, 2 * BL),
                dA=fused(tr(g_aa), a, tr(g_ba), b, 2 * B), dB=fused(tr(g_ab), a, tr(g_bb), b, 2 * B))


def ntx_eval32(case, defect=None):
    (B, BL, roff), kind, w = case
    d = ntx_data(case)
    a, b, A, Bl = d['a'], d['b'], d['A'], d['Bl']
    invT = torch.tensor(1.0) / torch.tensor(d['T'])
    M = torch.zeros(B, BL, dtype=torch.bool)
    M[torch.arange(B), roff + torch.arange(B)] = True
    Mce = torch.zeros_like(M) if defect == 'no_self_mask' else M
    aa, ab, ba, bb = (a @ A.t()) * invT, (a @ Bl.t()) * invT, (b @ A.t()) * invT, (b @ Bl.t()) * invT
    pos = (a * b).sum(1) * invT
    cat = lambda *t: torch.cat(t, 1)
    extra = 0.0
    if defect == 'unit_terms':                                 # 8 unit terms per lane group without a valid column
        extra = 8.0 * (4 - -(-(BL % 16) // 4)) if BL % 16 else 0.0

    def lse(x, add=0.0):
        m = x.max(1, keepdim=True).values
        return (m + torch.log(torch.exp(x - m).sum(1, keepdim=True) + add)).squeeze(1)
    lce_a = lse(cat(ab, aa.masked_fill(Mce, NEG)), extra)
    lce_b = lse(cat(ba, bb.masked_fill(Mce, NEG)), extra)
    Mx = torch.zeros_like(M) if defect == 'co2_pos' else M
    xx, yy = cat(aa.masked_fill(M, NEG), ab.masked_fill(Mx, NEG)), cat(ba.masked_fill(Mx, NEG), bb.masked_fill(M, NEG))
    lx, ly = lse(xx), lse(yy)
    dd = cat((ba - aa).masked_fill(M, 0.0), (bb - ab).masked_fill(Mx, 0.0))
    Pa, Pb = torch.exp(xx - lx.unsqueeze(1)), torch.exp(yy - ly.unsqueeze(1))
    kl = (Pb * dd).sum(1) - (Pa * dd).sum(1)
    term = (lce_a - pos) + (lce_b - pos) + w * kl
    cnt = ((ab > pos.unsqueeze(1)) & ~M).sum(1).float()
    stats = torch.stack([lce_a, lce_b, lx, ly, kl, pos, cnt, term], 1)
    coef = invT / B
    keep = (~M).float()
    ex = lambda x, L: torch.exp(x - L.unsqueeze(1))
    hot = M.float()
    g_aa = coef * (keep * ex(aa, lce_a) + w * keep * (ex(aa, lx) - ex(ba, ly)))
    g_ab = coef * (ex(ab, lce_a) - hot + w * keep * (ex(ab, lx) - ex(bb, ly)))
    g_ba = coef * (ex(ba, lce_b) - hot + w * keep * (ex(ba, ly) - ex(aa, lx)))
    g_bb = coef * (keep * ex(bb, lce_b) + w * keep * (ex(bb, ly) - ex(ab, lx)))
    return dict(rowstats=stats, cnt=cnt, loss=term.sum() / B, acc1=100.0 * float((cnt < 0.5).sum()) / B,
                da=g_aa @ A + g_ab @ Bl, db=g_ba @ A + g_bb @ Bl, dA=g_aa.t() @ a + g_ba.t() @ b,
                dB=g_ab.t() @ a + g_bb.t() @ b)
