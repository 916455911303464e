"""The criteria of bn_pool_util.py, tested on the CPU before any kernel is judged by them.

For every case of the tables a float32 torch evaluation of each formula stays within its bound against the float64
reference (slab sums accumulated row by row in float32, with the slab heights the GPU test uses), and no case has
more than AMBIGUOUS_CAP of its elements at the recomputed-mask boundary.  Then eight planted defects: each must
break a criterion on at least one element of at least one case, or the GPU test could not see it either.
"""
import pytest
import torch

import bn_pool_util as U

BN_IDS = [U.case_id(c) for c in U.BN_CASES]


def constants(case):
    d = U.bn_data(case)
    return U.host_constants(d['x'], d['gamma'], d['beta'])


def apply32(x, scale, shift, res, relu, dtype, defect=None):
    """z as float32 arithmetic gives it, stored in dtype.  defect 'next_col': constants of chunk column col + 1;
    'bf16_pre': x s + b rounded to bf16 before the residual is added."""
    if defect == 'next_col':
        scale, shift = torch.roll(scale, -8), torch.roll(shift, -8)
    v = x * scale + shift
    if defect == 'bf16_pre':
        v = v.to(torch.bfloat16).float()
    if res is not None:
        v = v + res
    pos = v > 0
    if relu:
        v = v.clamp_min(0)
    return U.rnd(v, dtype), pos


def slab_sums32(terms, M, nb, rows, drop_last=False, twice=False):
    """Per slab, the float32 sum of every [rows, C] tensor of `terms`, added row by row.  Defects: the last row of
    every slab left out / the second row of every slab added twice."""
    out = torch.zeros(nb, terms[0].shape[1], len(terms))
    for b, (r0, r1) in enumerate(U.slab_rows(M, nb, rows)):
        order = list(range(r0, r1 - 1 if drop_last else r1))
        if twice and r1 - r0 > 1:
            order.insert(1, r0 + 1)
        for k, t in enumerate(terms):
            acc = torch.zeros(t.shape[1])
            for r in order:
                acc = acc + t[r]
            out[b, :, k] = acc
    return out


def stats32(x, M, nb, rows, **defect):
    shift = torch.zeros(nb, x.shape[1])
    d = torch.zeros_like(x)
    for b, (r0, r1) in enumerate(U.slab_rows(M, nb, rows)):
        if r1 > r0:
            shift[b] = x[r0]
            d[r0:r1] = x[r0:r1] - x[r0]
    return shift, slab_sums32([d, d * d], M, nb, rows, **defect)


def masks(case, scale, shift):
    """relu source -> (mask or None, ambiguous or None)"""
    d = U.bn_data(case)
    m2, amb = U.recomputed_mask(d['x'], scale, shift)
    return {0: (None, None), 1: (d['zsrc'] > 0, None), 2: (m2, amb),
            3: (U.unpack_mask(d['maskbits'], d['x'].shape), None)}


def mask32(x, scale, shift):
    return (x * scale + shift) > 0


@pytest.mark.parametrize('case', U.BN_CASES, ids=BN_IDS)
def test_float32_batchnorm_meets_the_bounds(case):
    (M, C, nblocks), kind, dtype = case
    d = U.bn_data(case)
    x, dz, res = d['x'], d['dz'], d['res']
    what = U.case_id(case)
    nb, rows = U.bn_slabs(M, C, nblocks)
    # statistics slabs
    shift_ref, sums_ref, bound = U.stats_ref(x, nb, rows)
    shift, sums = stats32(x, M, nb, rows)
    assert torch.equal(shift, shift_ref)
    msg = U.verdict(what, 'stats slab', *U.usage(sums, sums_ref, bound))
    assert msg is None, msg
    msg = U.verdict(what, 'mean', *U.mean_usage(U.combine_mean(shift, sums, M, rows), x, bound))
    assert msg is None, msg
    mean, invstd, scale, shift_c = constants(case)
    assert all(bool(torch.isfinite(t).all()) for t in (mean, invstd, scale, shift_c))
    # apply
    for relu in (False, True):
        for r in (None, res):
            z, pos = apply32(x, scale, shift_c, r, relu, dtype)
            msg = U.verdict(what, 'z (relu %d, res %d)' % (relu, r is not None),
                            *U.apply_usage(z, x, scale, shift_c, r, relu, dtype))
            assert msg is None, msg
            if relu:
                assert U.mask_mismatch(U.pack_mask(pos), z)[0] == 0
    # backward
    for relu, (mask, amb) in masks(case, scale, shift_c).items():
        if relu == 2:
            share = float(amb.double().mean())
            assert share <= U.AMBIGUOUS_CAP, '%s: %.3f %% of the elements are at the recomputed-mask boundary' % (
                what, 100 * share)
            m32 = mask32(x, scale, shift_c)
        else:
            m32 = mask
        zero = torch.zeros_like(dz)
        g32 = dz if m32 is None else torch.where(m32, dz, zero)
        g = dz if mask is None else torch.where(mask, dz, zero)
        gother = None if amb is None else torch.where(mask, zero, dz)
        sums_ref, bound = U.reduce_ref(g, x, mean, invstd, U.row_groups(M, nb, rows), amb, gother)
        sums = slab_sums32([g32, g32 * (x - mean) * invstd], M, nb, rows)
        msg = U.verdict(what, 'bwd_reduce slab (relu %d)' % relu, *U.usage(sums, sums_ref, bound))
        assert msg is None, msg
        tot = sums.double().sum(0).float()
        msg = U.verdict(what, 'dbeta, dgamma (relu %d)' % relu, *U.param_grad_usage(tot[:, 0], tot[:, 1], sums_ref, bound))
        assert msg is None, msg
        coef = U.host_coef(g, x, d['gamma'], mean, invstd)
        dx = U.rnd(coef[0] * g32 + coef[1] * x + coef[2], dtype)
        msg = U.verdict(what, 'dx (relu %d)' % relu, *U.bwd_apply_usage(dx, dz, x, coef, mask, dtype, amb))
        assert msg is None, msg
        assert U.dres_mismatch(g32, dz, mask, amb)[0] == 0


@pytest.mark.parametrize('case', U.MAXPOOL_CASES, ids=[U.case_id(c) for c in U.MAXPOOL_CASES])
def test_float32_maxpool_meets_the_bounds(case):
    (N, H, W, C), kind, dtype = case
    d = U.pool_data(case)
    x, dy = d['x'], d['dy']
    y_ref, idx_ref = U.maxpool_ref(x)
    yt, it = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    assert torch.equal(y_ref, yt.permute(0, 2, 3, 1))
    # torch's index is h * W + w of the input: the same position as tap r * 3 + s of window (p, q)
    P, Q = U.pool_dims(H, W)
    p, q = torch.arange(P).view(1, P, 1, 1), torch.arange(Q).view(1, 1, Q, 1)
    r, s = idx_ref.long() // 3, idx_ref.long() % 3
    assert torch.equal((2 * p - 1 + r) * W + (2 * q - 1 + s), it.permute(0, 2, 3, 1))
    _, _, dx32 = U.maxpool_bwd_ref(dy, idx_ref, H, W)
    msg = U.verdict(U.case_id(case), 'dx', *U.maxpool_bwd_usage(U.rnd(dx32, dtype), dy, idx_ref, H, W, dtype))
    assert msg is None, msg


@pytest.mark.parametrize('case', U.AVGPOOL_CASES, ids=[U.case_id(c) for c in U.AVGPOOL_CASES])
def test_float32_avgpool_meets_the_bounds(case):
    (N, HW, C), kind, dtype = case
    d = U.pool_data(case)
    x, dy = d['x'], d['dy']
    acc = torch.zeros(N, C)
    for p in range(HW):
        acc = acc + x[:, p]
    inv = torch.tensor(1.0) / torch.tensor(float(HW))
    msg = U.verdict(U.case_id(case), 'y', *U.avgpool_fwd_usage(U.rnd(acc * inv, dtype), x, dtype))
    assert msg is None, msg
    dx = U.rnd((dy * inv).unsqueeze(1).expand(-1, HW, -1), dtype)
    msg = U.verdict(U.case_id(case), 'dx', *U.avgpool_bwd_usage(dx, dy, HW, dtype))
    assert msg is None, msg


def stem_constants(case):
    shape, kind, dtype = case
    x = U.pool_data(case)['x']
    gamma, beta = U.stem_params(shape[3])
    return (gamma,) + U.host_constants(x.reshape(-1, shape[3]), gamma, beta)


def stem32(x, scale, shift, dtype):
    z = U.rnd((x * scale + shift).clamp_min(0), dtype)
    return U.maxpool_ref(z)


@pytest.mark.parametrize('case', U.STEM_CASES, ids=[U.case_id(c) for c in U.STEM_CASES])
def test_float32_bn_relu_maxpool_meets_the_bounds(case):
    (N, H, W, C), kind, dtype = case
    d = U.pool_data(case)
    x, dy = d['x'], d['dy']
    what = U.case_id(case)
    gamma, mean, invstd, scale, shift = stem_constants(case)
    y, idx = stem32(x, scale, shift, dtype)
    msgs, _ = U.stem_fwd_violations(what, y, idx, x, scale, shift, dtype)
    assert not msgs, '\n'.join(msgs)
    g, gother, amb = U.stem_grad(dy, idx, x, scale, shift, dtype)
    share = float(amb.double().mean())
    assert share <= U.AMBIGUOUS_CAP, '%s: %.3f %% of the elements are at the recomputed-mask boundary' % (what, 100 * share)
    x2 = x.reshape(-1, C)
    _, _, acc32 = U.maxpool_bwd_ref(dy, idx, H, W)
    g32 = torch.where(mask32(x2, scale, shift), U.rnd(acc32, dtype).reshape(-1, C), torch.zeros_like(x2))
    for form in (0, 1):
        nb, per = U.stem_layout(N, H, W, C, form)
        groups = U.stem_groups(N, H, W, nb, per)
        assert sorted(torch.cat(groups).tolist()) == list(range(N * H * W))
        sums_ref, bound = U.reduce_ref(g, x2, mean, invstd, groups, amb, gother)
        sums = torch.zeros(nb, C, 2)
        for b, rows in enumerate(groups):
            for r in rows.tolist():
                sums[b, :, 0] = sums[b, :, 0] + g32[r]
                sums[b, :, 1] = sums[b, :, 1] + g32[r] * (x2[r] - mean) * invstd
        msg = U.verdict(what, 'reduce slab, form %d' % form, *U.usage(sums, sums_ref, bound))
        assert msg is None, msg
    coef = U.host_coef(g, x2, gamma, mean, invstd)
    dx = U.rnd(coef[0] * g32 + coef[1] * x2 + coef[2], dtype)
    a, b, c = coef.double()
    ref = [(a * t.double() + b * x2.double() + c, 4 * U.E * ((a * t.double()).abs() + (b * x2.double()).abs() + c.abs()))
           for t in (g, gother)]
    u = U.unit(dtype)
    msg = U.verdict(what, 'dx', *U.usage_either(dx, ref[0][0], ref[0][1] + u * ref[0][0].abs(), ref[1][0],
                                                ref[1][1] + u * ref[1][0].abs(), amb))
    assert msg is None, msg


def test_the_fused_reduce_forms_differ_in_layout():
    assert any(U.stem_layout(*s, 0) != U.stem_layout(*s, 1) for s in U.STEM_SHAPES)


# ------------------------------------------------------------------------------------------------ planted defects
def first_catch(cases, broken):
    """The id of the first case on which broken(case) (a worst usage, or a mismatch count) says 'violated'."""
    for case in cases:
        if broken(case):
            return U.case_id(case)
    return None


@pytest.mark.parametrize('defect', ['drop_last', 'twice'])
def test_a_dropped_or_doubled_slab_row_is_caught(defect):
    def stats_broken(case):
        (M, C, nblocks), _, _ = case
        nb, rows = U.bn_slabs(M, C, nblocks)
        _, sums_ref, bound = U.stats_ref(U.bn_data(case)['x'], nb, rows)
        _, sums = stats32(U.bn_data(case)['x'], M, nb, rows, **{defect: True})
        return U.usage(sums, sums_ref, bound)[0] > 1

    def reduce_broken(case):
        (M, C, nblocks), _, _ = case
        d = U.bn_data(case)
        nb, rows = U.bn_slabs(M, C, nblocks)
        mean, invstd, _, _ = constants(case)
        sums_ref, bound = U.reduce_ref(d['dz'], d['x'], mean, invstd, U.row_groups(M, nb, rows))
        sums = slab_sums32([d['dz'], d['dz'] * (d['x'] - mean) * invstd], M, nb, rows, **{defect: True})
        return U.usage(sums, sums_ref, bound)[0] > 1
    tall = [c for c in U.BN_CASES if c[0][0] > 1]
    for name, broken in (('bn_stats', stats_broken), ('bn_bwd_reduce', reduce_broken)):
        caught = [U.case_id(c) for c in tall if broken(c)]
        # every case with more than one row must see it: a dropped row exceeds the bound ~ 1 / (n^2 e) times
        assert len(caught) == len(tall), '%s with defect %s is caught by %d of %d cases only (first: %s)' % (
            name, defect, len(caught), len(tall), caught[:1])


def test_an_empty_slab_that_is_not_skipped_is_caught():
    def broken(case):
        (M, C, nblocks), _, _ = case
        nb, rows = U.bn_slabs(M, C, nblocks)
        x = U.bn_data(case)['x']
        shift, sums = stats32(x, M, nb, rows)
        return U.mean_usage(U.combine_mean(shift, sums, M, rows, skip_empty=False), x, U.stats_ref(x, nb, rows)[2])[0] > 1
    caught = [U.case_id(c) for c in U.BN_CASES if broken(c)]
    assert caught and all(c.startswith('5x8n4') for c in caught), caught
    print('empty slab not skipped: caught by %s' % caught)


@pytest.mark.parametrize('defect', ['next_col', 'bf16_pre'])
def test_wrong_constants_or_an_early_rounding_are_caught(defect):
    def broken(case):
        d = U.bn_data(case)
        _, _, scale, shift = constants(case)
        z, _ = apply32(d['x'], scale, shift, d['res'], True, case[2], defect)
        return U.apply_usage(z, d['x'], scale, shift, d['res'], True, case[2])[0] > 1
    cases = [c for c in U.BN_CASES if c[0][1] > 8] if defect == 'next_col' else U.BN_CASES
    caught = first_catch(cases, broken)
    assert caught is not None, 'no case sees the defect %s' % defect
    if defect == 'bf16_pre':           # both storage types must see it, not fp32 alone
        for dtype in U.DTYPES:
            c = first_catch([c for c in cases if c[2] == dtype], broken)
            assert c is not None, 'no %s case sees the defect %s (fp32 case %s does)' % (U.DTNAME[dtype], defect, caught)
    print('defect %s: caught first by %s' % (defect, caught))


def test_reversed_mask_bits_are_caught():
    def broken(case):
        d = U.bn_data(case)
        _, _, scale, shift = constants(case)
        z, pos = apply32(d['x'], scale, shift, None, True, case[2])
        rev = U.pack_mask(pos.reshape(-1, 8).flip(1))
        return U.mask_mismatch(rev, z)[0] > 0
    caught = first_catch(U.BN_CASES, broken)
    assert caught is not None, 'no case sees mask bits in reversed order'
    print('reversed mask bits: caught first by %s' % caught)


def test_zero_padding_in_the_maxpool_is_caught():
    def broken(case):
        x = U.pool_data(case)['x']
        y_ref, idx_ref = U.maxpool_ref(x)
        y, idx = U.maxpool_ref(x, pad=0.0)
        return not (torch.equal(y, y_ref) and torch.equal(idx, idx_ref))
    neg = [c for c in U.MAXPOOL_CASES if c[1] == 'negative']
    caught = [U.case_id(c) for c in neg if broken(c)]
    assert len(caught) == len(neg), 'zero padding is caught by %s only, of all negative cases' % caught


def test_the_last_maximum_on_ties_is_caught():
    def broken(case):
        x = U.pool_data(case)['x']
        return not torch.equal(U.maxpool_ref(x, last=True)[1], U.maxpool_ref(x)[1])
    caught = first_catch([c for c in U.MAXPOOL_CASES if c[1] == 'ties'], broken)
    assert caught is not None, 'no ties case tells the last maximum from the first'
    print('last maximum on ties: caught first by %s' % caught)
