"""The criteria of token_util.py, tested on the CPU before any kernel is judged by them.

1. Every reference is the project's own statement of the operation: oracle.mae's random_masking_ids and patchify, the
   gather / scatter / cat expressions of test_masking_and_token_plumbing (tests/test_mae_gpu.py), F.embedding with
   float64 autograd, argmax for the EOT index, nhwc() plus zero padding; and every twin (the kernel's own index
   arithmetic) gives the bits of its reference on every case.
2. Every float32 twin of a summed tensor, in the kernel's documented order, stays within HEADROOM = 0.5 of every
   element's bound on every case.  Every figure is printed as a `FIG host ...` line.
3. The planted defects: each, applied to the twin, exceeds 1.0 of a bound or changes a bit that is compared, on the
   case token_util.py names for it.
4. The bound formula n 2 E (sum |terms| + |initial|) holds for adversarial orders of the same terms: largest first,
   and all of one sign.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_util as U
from oracle import mae as M

LP = pytest.mark.parametrize('lp', U.LPS, ids=('fp32', 'bf16'))
T = torch.from_numpy


def judge(what, ref, got, limit=U.HEADROOM):
    for name, r in ref.items():
        ratio, idx = U.usage(got[name], *r)
        print('FIG host %s %s %.4f of the bound' % (what, name, ratio))
        assert ratio <= limit, '%s: float32 %s uses %.3f of its bound at flat index %d (limit %.2f)' % (
            what, name, ratio, idx, limit)


def same_bits(what, a, b, lp=False):
    for name in b:
        assert np.array_equal(U.wbits(a[name], lp), U.wbits(b[name], lp)), '%s: %s' % (what, name)


def close64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1e-300)


# ------------------------------------------------------------------------------------------------ mae_mask
@pytest.mark.parametrize('case', U.MASK_CASES, ids=U.case_id)
def test_mask_twin_is_the_stable_argsort(case):
    noise = U.mask_data(case)
    for K in U.mask_keeps(case[0]):
        want, got = U.mask_expect(noise, K), U.mask_eval(case, K)
        for name in want:
            assert np.array_equal(got[name], want[name]), '%s K=%d: %s' % (U.case_id(case), K, name)
        assert sorted(got['ids_restore'][0].tolist()) == list(range(case[0])) and got['mask'].sum() == 3 * (case[0] - K)


@pytest.mark.parametrize('L', [L for L in U.MASK_L if L >= 4])
def test_mask_reference_is_random_masking_ids_on_tie_free_rows(L):
    noise = U.mask_data((L, 'uniform'))
    assert all(len(set(r.tolist())) == L for r in noise)
    keep, mask, restore = M.random_masking_ids(T(noise), 0.75)         # len_keep = int(L * 0.25) = L // 4
    want = U.mask_expect(noise, L // 4)
    assert np.array_equal(keep.numpy(), want['ids_keep']) and np.array_equal(restore.numpy(), want['ids_restore'])
    assert np.array_equal(mask.numpy(), want['mask'])


def test_the_mask_kinds_are_what_they_are_named_for():
    n = U.mask_data((513, 'tie256'))
    i = (513 - 257) // 2
    assert (n[:, i] == n[:, i + 256]).all()
    n = U.mask_data((196, 'negzero'))
    assert (np.signbit(n) & (n == 0)).any() and (~np.signbit(n) & (n == 0)).any()
    r = U.mask_eval((196, 'negzero'), 49)['ids_restore'][0]
    z = np.nonzero(n[0] == 0)[0]
    assert (np.diff(r[z]) == 1).all()                                 # the zeros of either sign: ordered by index alone
    n = U.mask_data((196, 'denormal'))
    assert (np.abs(n[n != 0]) < 2.0 ** -126).all() and len(np.unique(n)) == 17
    assert len(np.unique(U.mask_data((196, 'quant4')))) == 4 and len(np.unique(U.mask_data((196, 'equal')))) == 1


# ------------------------------------------------------------------------------------------------ gather, unshuffle
@LP
@pytest.mark.parametrize('case', U.GATHER_CASES, ids=U.case_id)
def test_gather_twin_reference_and_bound(case, lp):
    B, L, K, D, kind = case
    d, ev = U.gather_data(case, lp), U.gather_eval32(case, lp)
    same_bits(U.case_id(case), ev, U.gather_expect(case, lp), lp)
    judge('gather %s %s' % (U.case_id(case), lp), U.gather_ref(case, lp), ev)
    assert all(len(set(r.tolist())) == K for r in d['ids_keep'])
    assert all(np.array_equal(r[k], np.arange(K)) for r, k in zip(d['ids_restore'], d['ids_keep'].astype(np.int64)))
    # the expressions of test_masking_and_token_plumbing
    x, cls, pos, dout, keep = T(d['x']), T(d['cls']), T(d['pos']), T(d['dout']), T(d['ids_keep']).long()
    ref = torch.cat([(cls + pos[0]).expand(B, 1, D), torch.gather(x + pos[1:], 1, keep.unsqueeze(-1).expand(-1, -1, D))], 1)
    dref = torch.zeros(B, L, D).scatter_(1, keep.unsqueeze(-1).expand(-1, -1, D), dout[:, 1:])
    same_bits(U.case_id(case), ev, {'out': ref.numpy(), 'dx': dref.numpy()}, lp)
    assert close64(U.gather_ref(case, lp)['dcls'][0], (dout[:, 0].double().sum(0) + T(d['dcls']).double()).numpy())
    if kind == 'subset':
        assert K < 2 or any((np.diff(r) < 0).any() for r in d['ids_keep'])


@LP
@pytest.mark.parametrize('case', U.UNSHUFFLE_CASES, ids=U.case_id)
def test_unshuffle_twin_reference_and_bound(case, lp):
    B, L, K, D = case
    d, ev = U.unshuffle_data(case, lp), U.unshuffle_eval32(case, lp)
    same_bits(U.case_id(case), ev, U.unshuffle_expect(case, lp), lp)
    ref = U.unshuffle_ref(case, lp)
    judge('unshuffle %s %s' % (U.case_id(case), lp), ref, ev)
    xd, mt, dpos, dd = T(d['x']), T(d['mask_token']), T(d['pos']), T(d['dout'])
    keep, restore = T(d['ids_keep']).long(), T(d['ids_restore']).long()
    x_ = torch.cat([xd[:, 1:], mt.expand(B, L - K, D)], 1)
    x_ = torch.gather(x_, 1, restore.unsqueeze(-1).expand(-1, -1, D))
    refd = torch.cat([xd[:, :1], x_], 1) + dpos
    dref2 = torch.cat([dd[:, :1], torch.gather(dd[:, 1:], 1, keep.unsqueeze(-1).expand(-1, -1, D))], 1)
    same_bits(U.case_id(case), ev, {'out': refd.numpy(), 'dx': dref2.numpy()}, lp)
    mask = (restore >= K).double()
    assert close64(ref['dmask_token'][0], ((dd[:, 1:].double() * mask.unsqueeze(-1)).sum((0, 1)) +
                                           T(d['dmask_token']).double()).numpy())
    if K == L:                                                       # nothing is masked: bound 0, the same bits
        assert not ref['dmask_token'][1].any()
        assert np.array_equal(U.bits(ev['dmask_token']), U.bits(d['dmask_token']))


def test_the_unshuffle_slabs_are_what_the_cases_are_named_for():
    assert [U.unshuffle_slabs(c[0], c[1])[0] for c in U.UNSHUFFLE_CASES] == [1, 1, 2, 1, 7, 4, 33]
    assert U.unshuffle_slabs(3, 42) == (2, 65) and max(U.unshuffle_slabs(B, L)[0] for B, L in ((4096, 4096),)) <= 1024


# ------------------------------------------------------------------------------------------------ patchify
def test_the_loop_cases_pass_the_capped_grid():
    cap = 4096 * 256                                                  # grid_for of vit.hip: blocks x threads
    B, Ln, K, D = U.GATHER_LOOP
    assert B * (K + 1) * D // 8 > cap and B * Ln * D // 8 > cap
    B, Ln, K, D = U.UNSHUFFLE_LOOP
    assert B * (Ln + 1) * D // 8 > cap and np.prod(U.PATCHIFY_LOOP[:4]) > cap and U.RELU_N[-1] // 8 > cap


@pytest.mark.parametrize('which', U.PATCHIFY_INPUTS)
@pytest.mark.parametrize('case', U.PATCHIFY_CASES + ((2, 3, 8, 8, 4), U.PATCHIFY_LOOP), ids=U.case_id)
def test_patchify_twin_and_reference(case, which):
    B, C, H, W, p = case
    if case == U.PATCHIFY_LOOP and which == 'coded':
        return
    img = U.patchify_data(case, which)
    want = U.patchify_expect(img, p)
    assert np.array_equal(U.bits(U.patchify_eval(img, p)), U.bits(want))
    if which == 'coded':                                               # every pixel a distinct value that bf16 holds
        assert len(np.unique(img)) == img.size and np.array_equal(U.q(img, True), img)
    if H == W:
        assert np.array_equal(M.patchify(T(img), p).numpy().reshape(want.shape), want)
    else:                                                              # M.patchify's einsum with h and w apart
        x = torch.einsum('nchpwq->nhwpqc', T(img).reshape(B, C, H // p, p, W // p, p))
        assert np.array_equal(x.reshape(want.shape).numpy(), want)


# ------------------------------------------------------------------------------------------------ prefix tokens, mean2
@LP
@pytest.mark.parametrize('case', U.PREFIX_CASES, ids=U.case_id)
def test_prefix_twin_reference_and_bound(case, lp):
    B, L, NP, C = case
    d, ev = U.prefix_data(case, lp), U.prefix_eval32(case, lp)
    same_bits(U.case_id(case), ev, U.prefix_expect(case, lp), lp)
    ref = U.prefix_ref(case, lp)
    judge('prefix %s %s' % (U.case_id(case), lp), ref, ev)
    x = torch.cat([T(d['prefix'][:NP]).expand(B, NP, C), T(d['x'])], 1) + T(d['pos'])      # deit.py:238-247
    same_bits(U.case_id(case), ev, {'out': x.numpy()}, lp)
    for t in range(NP):
        assert close64(ref['dprefix%d' % t][0], T(d['dout'])[:, t].double().sum(0).numpy() + d['dprefix'][t])
    if L > 200:                                                       # one chunk of 8 past a 256-thread block
        assert 257 in (B * (L + NP) * C // 8, B * L * C // 8)


# ------------------------------------------------------------------------------------------------ embed
@LP
@pytest.mark.parametrize('case', U.EMBED_CASES, ids=U.case_id)
def test_embed_twin_reference_and_bound(case, lp):
    B, Tn, C, V, kind = case
    for dkind in U.EMBED_DOUTS:
        what = 'embed %s %s %s' % (U.case_id(case), dkind, lp)
        d, ev, ref = U.embed_data(case, dkind, lp), U.embed_eval32(case, dkind, lp), U.embed_ref(case, dkind, lp)
        if dkind == 'scattered':                                       # the truncation term may be used in full
            judge(what, {'dpos': ref['dpos']}, ev)
            judge(what, {'dtable': ref['dtable']}, ev, limit=1.0)
            S, bound = ref['dtable']
            count = np.bincount(d['text'][(d['text'] >= 0) & (d['text'] < V)], minlength=V)[:, None]
            trunc = count * 2.0 ** -U.embed_scale_exp(d['dout'], B * Tn)[0]
            assert (np.abs(ev['dtable'] - S) <= trunc + U.HEADROOM * (bound - trunc)).all(), what
        else:
            judge(what, ref, ev)
        text = d['text']
        ok = (text >= 0) & (text < V)
        # F.embedding with float64 autograd; an id out of range has no row: pos alone, and no gradient to the table
        table = T(d['table']).double().requires_grad_(True)
        pos = T(d['pos']).double().requires_grad_(True)
        out = F.embedding(T(np.where(ok, text, 0)), table) * T(ok).unsqueeze(-1) + pos
        out.backward(T(d['dout']).double())
        assert np.array_equal(U.wbits(ev['out'], lp), U.wbits(out.detach().float().numpy(), lp)), what
        assert close64(ref['dtable'][0], table.grad.numpy() + d['dtable']), what
        assert close64(ref['dpos'][0], pos.grad.numpy() + d['dpos']), what
        if dkind == 'zero':                                            # nothing to add: the same bits
            assert np.array_equal(U.bits(ev['dtable']), U.bits(d['dtable']))
            assert np.array_equal(U.bits(ev['dpos']), U.bits(d['dpos']))
        if kind == 'oob':
            assert (text == -1).any() and (B * Tn < 3 or ((text == V).any() and (text == 2 ** 40).any()))
            assert np.array_equal(ev['out'][~ok], np.broadcast_to(d['pos'], ev['out'].shape)[~ok])
        if kind == 'pad':
            assert (text == 0).mean() > 0.6
    assert U.embed_bwd_slabs(70, 2048) == (3, 1) and U.embed_bwd_slabs(3, 24) == (1, 85)


def test_embed_decades_and_the_nan_case():
    case, at = U.EMBED_NAN
    for dkind in ('decades', 'scattered'):
        mag = np.abs(U.embed_data(case, dkind, False)['dout'])
        assert np.quantile(mag, 0.99) > 1e10 * np.quantile(mag, 0.01)
    d = U.embed_data(case, 'normal', False, at)
    assert np.isnan(d['dout']).sum() == 1 and 0 <= d['text'][at[0], at[1]] < case[3]
    ev, ref = U.embed_eval32(case, 'normal', False, nan_at=at), U.embed_ref(case, 'normal', False, at)
    assert np.isnan(ev['dpos'][at[1], at[2]]) and np.isnan(ev['dpos']).sum() == 1
    keep = np.ones(ev['dpos'].shape, bool)
    keep[at[1], at[2]] = False
    assert U.usage(ev['dpos'][keep], ref['dpos'][0][keep], ref['dpos'][1][keep])[0] <= U.HEADROOM
    rows = np.arange(case[3]) != d['text'][at[0], at[1]]
    assert U.usage(ev['dtable'][rows], ref['dtable'][0][rows], ref['dtable'][1][rows])[0] <= U.HEADROOM


# ------------------------------------------------------------------------------------------------ eot_index, rows
@pytest.mark.parametrize('case', U.EOT_CASES, ids=U.case_id)
def test_eot_twin_is_argmax(case):
    for shift in range(len(U.EOT_ROWS)):
        text = U.eot_text(case, shift)
        want = [b * case[1] + int(T(text)[b].argmax()) for b in range(case[0])]        # torch: the first maximum
        assert U.eot_eval(text).tolist() == want == [b * case[1] + int(np.argmax(text[b])) for b in range(case[0])]


def test_the_eot_rows_are_what_they_are_named_for():
    text = np.concatenate([U.eot_text((9, 129), s) for s in (0, 2)])
    idx = U.eot_eval(text) - np.arange(18) * 129
    assert set(idx.tolist()) >= {0, 128, 5, 3, 10}
    assert (text < 0).all(1).any() and (text == 2 ** 40 + 1).any()
    tie = [b for b in range(18) if (text[b] == text[b].max()).sum() == 2]
    assert {tuple(np.nonzero(text[b] == text[b].max())[0]) for b in tie} == {(5, 9), (3, 67), (10, 70)}


@LP
@pytest.mark.parametrize('case', U.ROWS_CASES, ids=U.case_id)
def test_rows_twin(case, lp):
    d, ev = U.rows_data(case, lp), U.rows_eval(case, lp)
    x = T(d['x'])
    assert np.array_equal(ev['out'], x[T(d['gidx']).long()].numpy())
    ref = torch.zeros_like(x)
    ref[T(d['sidx']).long()] = T(d['dout'])
    assert np.array_equal(ev['dx'], ref.numpy())
    assert len(set(d['sidx'].tolist())) == case[0] and (case[0] == 1 or len(set(d['gidx'].tolist())) < case[0])


# ------------------------------------------------------------------------------------------------ layout, colsum, relu
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('case', U.PAD_CASES, ids=U.case_id)
def test_pad_twin_is_nhwc_plus_zero_padding(case):
    lp, C, Cp, pad, ex, skew = case
    want = U.pad_expect(case)
    assert np.array_equal(U.bits(U.pad_eval(case)), U.bits(want))
    ref = torch.zeros(U.PAD_N, U.PAD_H + 2 * pad, U.PAD_W + 2 * pad + ex, Cp)
    ref[:, pad:pad + U.PAD_H, pad:pad + U.PAD_W, :C] = nhwc(T(U.pad_data(C)))
    assert np.array_equal(ref.numpy(), want)


@LP
@pytest.mark.parametrize('case', U.COLSUM_CASES, ids=U.case_id)
def test_colsum_twin_meets_the_bound(case, lp):
    for acc in (0, 1):
        ref = U.colsum_ref(case, lp, acc)
        judge('colsum %s acc=%d %s' % (U.case_id(case), acc, lp), ref, U.colsum_eval32(case, lp, acc))
        d = U.colsum_data(case, lp)
        assert close64(ref['out'][0], T(d['x']).double().sum(0).numpy() + acc * d['out'].astype(np.float64))
    assert U.colsum_slabs(32767) == (512, 64) and U.colsum_slabs(32768) == (128, 256) and U.colsum_slabs(65) == (2, 33)
    assert U.colsum_slabs(64)[0] == 1 and U.colsum_slabs(129)[0] == 3


@LP
@pytest.mark.parametrize('n', U.RELU_N[:2])
def test_relu_twin(n, lp):
    d = U.relu_data(n, lp)
    y, dy = T(d['y'].copy()), T(d['dy'].copy())
    want = torch.where(y > 0, dy, torch.zeros(()))
    got = U.relu_eval(n, lp)
    assert np.array_equal(U.bits(got), U.bits(want.numpy())) and not np.isnan(got).any()
    off = ~(d['y'] > 0)
    assert np.isnan(d['dy'][off]).any() and (d['dy'][off] == -3).any() and (U.bits(got[off]) == 0).all()
    assert np.array_equal(U.q(d['y'], True), d['y'], equal_nan=True)             # bf16 holds every y, the denormals too


# ------------------------------------------------------------------------------------------------ planted defects
def _gather(case, lp, defect=None):
    return U.gather_eval32(case, lp, defect), U.gather_ref(case, lp)


def _unshuffle(case, lp, defect=None):
    return U.unshuffle_eval32(case, lp, defect), U.unshuffle_ref(case, lp)


def _prefix(case, lp, defect=None):
    return U.prefix_eval32(case, lp, defect), U.prefix_ref(case, lp)


def _embed(case, lp, defect=None):
    return U.embed_eval32(case[:-1], case[-1], lp, defect), U.embed_ref(case[:-1], case[-1], lp)


def _colsum(case, lp, defect=None):
    return U.colsum_eval32(case, lp, 0, defect), U.colsum_ref(case, lp, 0)


BOUNDED = [          # what is planted, the twin's switch, family, the case that must catch it, the tensor
    ('cls_grad drops the images from 8 on', 'cls_first_8', _gather, (9, 17, 17, 264, 'mask'), 'dcls'),
    ('mae_unshuffle_bwd drops the last token slab', 'last_slab', _unshuffle, (3, 42, 10, 32), 'dmask_token'),
    ('mae_unshuffle_bwd drops the columns from 256 on', 'cols_256', _unshuffle, (4, 196, 1, 264), 'dmask_token'),
    ('prefix_tokens sums dprefix1 from row 0', 'dprefix1_row0', _prefix, (3, 5, 2, 8), 'dprefix1'),
    ('embed clamps an out-of-range id to V - 1', 'clamp_oob', _embed, (3, 12, 24, 7, 'oob', 'normal'), 'dtable'),
    ('embed never flushes the final run', 'no_final_flush', _embed, (40, 9, 64, 50, 'text', 'normal'), 'dtable'),
    ('colsum drops the rows past a multiple of 8', 'tail_rows', _colsum, (40, 9), 'out'),
]


@LP
@pytest.mark.parametrize('what,defect,family,case,tensor', BOUNDED, ids=[d[1] for d in BOUNDED])
def test_planted_defect(what, defect, family, case, tensor, lp):
    sound, ref = family(case, lp)
    broken, _ = family(case, lp, defect)
    a, b = U.usage(sound[tensor], *ref[tensor])[0], U.usage(broken[tensor], *ref[tensor])[0]
    print('FIG host defect %s: %s %.3g of the bound (sound: %.3f)' % (defect, tensor, b, a))
    assert a <= U.HEADROOM
    assert b > 1.0, '%s goes unnoticed: %s stays at %.3f of its bound' % (what, tensor, b)


def differs(a, b, lp):
    wa, wb = U.wbits(a, lp), U.wbits(b, lp)
    return wa.shape != wb.shape or not np.array_equal(wa, wb)


@LP
def test_planted_defect_in_the_bit_exact_kernels(lp):
    """Each changes a bit of what the GPU test compares bit for bit, on the named case."""
    case = (49, 'quant4')
    for K in U.mask_keeps(49):
        assert not np.array_equal(U.mask_eval(case, K, 'tie_high')['ids_restore'], U.mask_eval(case, K)['ids_restore'])
    case = (49, 'uniform')
    assert not np.array_equal(U.mask_eval(case, 12, 'rank_gt')['mask'], U.mask_eval(case, 12)['mask'])
    case = (3, 5, 2, 8, 'mask')
    assert differs(U.gather_eval32(case, lp, 'pos_src')['out'], U.gather_eval32(case, lp)['out'], lp)
    for which in U.PATCHIFY_INPUTS:
        img = U.patchify_data((2, 3, 8, 12, 4), which)
        for defect in ('swap_hw', 'col_order'):
            assert differs(U.patchify_eval(img, 4, defect), U.patchify_eval(img, 4), lp), defect
    for case, defect in (((3, 42, 10, 32), 'last_slab'), ((4, 196, 1, 264), 'cols_256')):
        assert differs(U.unshuffle_eval32(case, lp, defect)['dx'], U.unshuffle_eval32(case, lp)['dx'], lp), defect
    case = (3, 12, 24, 7, 'oob')
    assert differs(U.embed_eval32(case, 'normal', lp, 'clamp_oob')['out'], U.embed_eval32(case, 'normal', lp)['out'], lp)
    for defect in ('last_max', 'ids_32bit'):
        assert any(not np.array_equal(U.eot_eval(U.eot_text((4, 77), s), defect), U.eot_eval(U.eot_text((4, 77), s)))
                   for s in range(len(U.EOT_ROWS))), defect
    case = (True, 3, 4, 3, 3, 0)
    assert differs(U.pad_eval(case, 'beyond_unwritten'), U.pad_eval(case), True)
    assert differs(U.relu_eval(8, lp, 'ge'), U.relu_eval(8, lp), lp)


# ------------------------------------------------------------------------------------------------ the bound formula
def _terms(kind, n, rng):
    if kind == 'normal':
        return rng.standard_normal(n)
    if kind == 'same_sign':
        return np.abs(rng.standard_normal(n)) + 0.1
    if kind == 'decades':
        return 10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)
    return U.q(rng.standard_normal(n), True).astype(np.float64)           # bf16-valued


@pytest.mark.parametrize('kind', ('normal', 'same_sign', 'decades', 'bf16'))
@pytest.mark.parametrize('n', (1, 2, 8, 257, 4096))
def test_the_sum_bound_holds_for_adversarial_orders(kind, n):
    rng = U._rng('order', kind, n)
    t = _terms(kind, (n, 64), rng).astype(np.float32)
    init = rng.standard_normal(64).astype(np.float32)
    orders = {'as given': t, 'largest first': np.take_along_axis(t, np.argsort(-np.abs(t), axis=0), 0),
              'smallest first': np.take_along_axis(t, np.argsort(np.abs(t), axis=0), 0), 'all of one sign': np.abs(t)}
    for name, terms in orders.items():
        ref, bound = U.sum_ref(terms, init)
        for first in (True, False):                                   # onto the initial value, or the initial value last
            seq = np.concatenate([init[None], terms] if first else [terms, init[None]])
            got = np.cumsum(seq, axis=0, dtype=np.float32)[-1]        # strictly sequential float32 additions
            ratio = U.usage(got, ref, bound)[0]
            print('FIG host order %s %d %s init %s: %.4f of the bound' % (kind, n, name, 'first' if first else 'last', ratio))
            assert ratio <= 1.0
