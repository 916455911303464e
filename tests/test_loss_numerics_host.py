"""The criteria of loss_util.py, tested on the CPU before any kernel is judged by them.

For every case of the tables a float32 torch evaluation of each formula (true exp / log, torch's own summation order)
stays within HEADROOM = 0.5 of every element's bound against the float64 reference; its accuracies lie in the
reference's interval; and no case has an ambiguous row unless its kind is `duplicate` or `collapsed`, and then no more
than were planted.  Two figures are exempt from the 0.5 (not from the bound): a value stored as bf16, whose correctly
rounded store may use the whole u |value| by definition (its fp32 value before the store meets the 0.5), and the
NT-Xent rank count, an integer that may be any value between the sure and the possible count.

Then the planted defects: each, applied to the float32 evaluation, must exceed 1.0 on the named tensor of the named
case, or the GPU test could not see it either.
"""
import pytest
import torch

import loss_util as U

FULL = ('cnt',)                                   # judged against the whole bound, see above


def judge(what, ref, got, limit=U.HEADROOM):
    """Asserts every tensor of `ref` that `got` has; returns {tensor: worst usage}."""
    worst = {}
    for name, r in ref.items():
        if name.startswith('acc'):
            assert U.acc_ok(got[name], r), '%s: %s = %.4f outside [%.4f, %.4f]' % (what, name, got[name], r[0], r[1])
            continue
        ratio, idx = U.usage(got[name], r[0], r[1])
        worst[name] = ratio
        lim = 1.0 if name in FULL else limit
        assert ratio <= lim, '%s: float32 %s uses %.3f of its bound at flat index %d (limit %.2f)' % (
            what, name, ratio, idx, lim)
    return worst


def no_unplanted_ambiguity(what, case, ref):
    amb, planted = U.ambiguous_rows(ref), U.planted_rows(case)
    assert amb <= planted, '%s: %d ambiguous rows, %d planted' % (what, amb, planted)


@pytest.mark.parametrize('case', U.CE_CASES, ids=[U.ce_id(c) for c in U.CE_CASES])
def test_float32_softmax_and_sigmoid_ce_meet_the_bounds(case):
    ref = U.softmax_ref(case)
    judge(U.ce_id(case) + ' softmax_ce', ref, U.softmax_eval32(case))
    assert not (ref['acc1'][2] | ref['acc5'][2]).any()          # dx = 0: ties are exact
    judge(U.ce_id(case) + ' sigmoid_ce', U.sigmoid_ref(case), U.sigmoid_eval32(case))


def test_flat_rows_have_loss_log_c_and_the_lower_index_wins():
    for (N, C) in U.CE_SHAPES:
        case = ((N, C), 'flat')
        ref, lab = U.softmax_ref(case), U.ce_data(case)['labels']
        assert torch.allclose(ref['lse'][0] - 7.25, torch.full((N,), float(torch.log(torch.tensor(float(C)))),
                                                               dtype=torch.float64), atol=1e-12)
        assert ref['acc1'][0] == ref['acc1'][1] == 100.0 * float((lab == 0).sum()) / N
        assert ref['acc5'][0] == 100.0 * float((lab < 5).sum()) / N


@pytest.mark.parametrize('case', U.SOFT_CASES, ids=[U.ce_id(c) for c in U.SOFT_CASES])
def test_float32_soft_ce_meets_the_bounds(case):
    judge(U.ce_id(case) + ' soft_ce', U.soft_ref(case), U.soft_eval32(case))


@pytest.mark.parametrize('case', U.ROW_CASES, ids=[U.row_id(c) for c in U.ROW_CASES])
def test_float32_l2norm_and_cosine_meet_the_bounds(case):
    what, d = U.row_id(case), U.row_data(case)
    (N, D), _ = case
    assert not d['x'][N // 2].any()                             # the clamped row
    ev = U.l2norm_eval32(case)
    judge(what + ' l2norm_fwd', U.l2norm_ref(case), ev)
    dx, B = U.l2norm_bwd_ref(d['dy'], ev['y'], ev['norm'])
    judge(what + ' l2norm_bwd', {'dx': (dx, B)}, ev)
    dx, B = U.l2norm_bwd_ref(d['dy'], ev['y'], ev['norm'], U.U_BF16)
    judge(what + ' l2norm_bwd bf16', {'dx_bf16': (dx, B)}, ev, limit=1.0)
    ev = U.cosine_eval32(case)
    ref = U.cosine_ref(case)
    assert ref['stats'][0][N // 2, 3] == 0 and (N == 1 or ref['stats'][0][:, 3].sum() == N - 1)
    judge(what + ' cosine_fwd', ref, ev)
    da, B = U.cosine_bwd_ref(d['x'], d['b'], ev['stats'])
    judge(what + ' cosine_bwd', {'da': (da, B)}, ev)


@pytest.mark.parametrize('case', U.INFONCE_CASES, ids=[U.infonce_id(c) for c in U.INFONCE_CASES])
def test_float32_infonce_meets_the_bounds(case):
    ref = U.infonce_ref(case)
    judge(U.infonce_id(case) + ' infonce', ref, U.infonce_eval32(case))
    no_unplanted_ambiguity(U.infonce_id(case), case, ref)


@pytest.mark.parametrize('case', U.CLIP_CASES, ids=[U.infonce_id(c) for c in U.CLIP_CASES])
def test_float32_clip_meets_the_bounds(case):
    (B, D), _ = case
    what = U.infonce_id(case)
    ev = U.clip_eval32(case)
    judge(what + ' clip fwd', U.clip_ref(case), ev)
    judge(what + ' clip_logits_bwd', U.clip_bwd_ref(ev['dlogits'], ev['logits'], ev['ws'], B, D), ev)


@pytest.mark.parametrize('case', U.NTX_CASES, ids=[U.ntx_id(c) for c in U.NTX_CASES])
def test_float32_ntxent_meets_the_bounds(case):
    ref = U.ntx_ref(case)
    judge(U.ntx_id(case) + ' ntxent', ref, U.ntx_eval32(case))
    no_unplanted_ambiguity(U.ntx_id(case), case, ref)


def test_the_offset_kind_uses_its_loss_bound_without_exceeding_it():
    """The loss terms cancel at the common offset of -1e4: the float32 evaluation's usage is printed for the record."""
    for (N, C) in U.CE_SHAPES:
        w = judge('offset', U.softmax_ref(((N, C), 'offset')), U.softmax_eval32(((N, C), 'offset')))
        print('FIG host softmax_ce terms %dx%d-offset %.4f of the bound' % (N, C, w['terms']))


SOFTMAX = (U.softmax_ref, U.softmax_eval32)
SIGMOID = (U.sigmoid_ref, U.sigmoid_eval32)
SOFT = (U.soft_ref, U.soft_eval32)
INFONCE = (U.infonce_ref, U.infonce_eval32)
CLIP = (U.clip_ref, U.clip_eval32)
NTX = (U.ntx_ref, U.ntx_eval32)
DEFECTS = [          # what is planted, the evaluation's switch, family, the case that must catch it, the tensor
    ('last column dropped', 'drop_last_col', SOFTMAX, ((3, 5), 'plain'), 'lse'),
    ('last column dropped', 'drop_last_col', SOFT, ((8, 16), 'plain', 'random'), 'lse'),
    ('last 128-column slice dropped', 'drop_last_slice', INFONCE, ((15, 256), 'plain'), 'lse'),
    ('maximum not subtracted', 'no_max', SOFTMAX, ((3, 5), 'large'), 'lse'),
    ('label off by one', 'label_off', SOFTMAX, ((5, 64), 'far_label'), 'terms'),
    ('label off by one', 'label_off', SIGMOID, ((5, 64), 'plain'), 'terms'),
    ('self mask missing', 'no_self_mask', NTX, ((8, 8, 0), 'plain', 3.0), 'rowstats'),
    ('positive not masked in the CO2 terms', 'co2_pos', NTX, ((8, 8, 0), 'plain', 3.0), 'rowstats'),
    ('1/N taken as 1/(N C)', 'invNC', SOFTMAX, ((3, 5), 'plain'), 'ds'),
    ('1/N taken as 1/(N C)', 'invNC', SIGMOID, ((3, 5), 'plain'), 'ds'),
    ('slices beyond the 64th ignored in the InfoNCE finalize', 'finalize64', INFONCE, ((17, 8320), 'plain'), 'lse'),
    ('column block beyond the first ignored in the CLIP column pass', 'col_block', CLIP, ((257, 16), 'plain'), 'lse'),
    ("all-invalid lanes' unit terms left in the NT-Xent sum", 'unit_terms', NTX, ((2, 2, 0), 'plain', 3.0), 'rowstats'),
]


@pytest.mark.parametrize('what,defect,family,case,tensor', DEFECTS, ids=['%s-%d' % (d[1], i) for i, d in enumerate(DEFECTS)])
def test_planted_defect(what, defect, family, case, tensor):
    ref_fn, eval_fn = family
    ref = ref_fn(case)[tensor]
    sound, _ = U.usage(eval_fn(case)[tensor], *ref)
    broken, idx = U.usage(eval_fn(case, defect)[tensor], *ref)
    print('FIG host defect %s: %s %.3g of the bound (sound: %.3f)' % (defect, tensor, broken, sound))
    assert sound <= U.HEADROOM
    assert broken > 1.0, '%s goes unnoticed: %s stays at %.3f of its bound' % (what, tensor, broken)


def test_the_defects_named_by_the_co2_and_lane_cases_hit_the_columns_they_are_named_for():
    """no_self_mask and unit_terms move lce_a (column 0), co2_pos moves lx (column 2) of the row statistics."""
    for defect, case, col in (('no_self_mask', ((8, 8, 0), 'plain', 3.0), 0), ('co2_pos', ((8, 8, 0), 'plain', 3.0), 2),
                              ('unit_terms', ((2, 2, 0), 'plain', 3.0), 0)):
        ref, B = U.ntx_ref(case)['rowstats']
        got = U.ntx_eval32(case, defect)['rowstats']
        assert U.usage(got[:, col], ref[:, col], B[:, col])[0] > 1.0, (defect, col)
