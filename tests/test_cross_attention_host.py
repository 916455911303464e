"""The float64 reference and the rounding model of the cross-attention kernels (cross_attention_util.py) on the CPU: the
fp32 eager result and the rounding model pass the criteria the GPU test applies, no case of the matrix is hollowed out
by underflow, and the criteria see three bugs a cross-attention kernel can have: the accumulator not rescaled when the
running max rises, the last key block skipped, and Tq used where Tk belongs in the dK / dV sweep.
"""
import pytest
import torch

import attention_util as A
import cross_attention_util as X

IDS = [X.case_id(c) for c in X.CASES]
UNDERFLOW_CAP = 0.01           # the project's cap on the share of a tensor's bounds below 2^-100


def test_the_matrix_is_the_one_that_was_set():
    assert len(X.CASES) == 2 * (8 * 2 + 5 * 5)
    assert (64, 75, 196, 'peaked') in X.CASES and (32, 1024, 5, 'negative') in X.CASES
    assert not any(kind in ('peaked', 'ramp', 'vmean') for _, Tq, Tk, kind in X.CASES if (Tq, Tk) in X.PAIRS_EDGE)


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_rounding_model_is_inside_the_bf16_limits(case):
    d = X.case_data(case)
    msgs = []
    for n in A.TENSORS:
        msgs += A.bound_violations(n, d['model'][n], d['ref'][n], d['ref']['b_' + n], A.LIMIT_BF16[n])
    assert not msgs, X.case_id(case) + ':\n' + '\n'.join(msgs)
    assert torch.isfinite(d['model']['lse']).all()
    assert float((d['model']['lse'] - d['ref']['lse']).abs().max()) <= 2.0 ** -40 * max(1.0, float(d['ref']['lse'].abs().max()))


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_fp32_eager_passes_the_fp32_rule(case):
    """The fp32 rule of the GPU test is max(4 x eager error, floor) of the bound: eager itself is inside it, finite, and
    its shapes are those of the operands."""
    DH, Tq, Tk, _ = case
    d = X.case_data(case)
    for n, T in (('out', Tq), ('dq', Tq), ('dk', Tk), ('dv', Tk)):
        assert d['eager'][n].shape == (X.B, T, X.H, DH) and d['ref'][n].shape == (X.B, T, X.H, DH)
        b = d['ref']['b_' + n]
        eager = A.scaled_error(d['eager'][n], d['ref'][n], b)[0]
        assert eager < 2.0 ** -14, '%s %s: eager error %.3g of the bound' % (X.case_id(case), n, eager)
        assert not A.bound_violations(n, d['eager'][n], d['ref'][n], b, max(4 * eager, 16 * 2.0 ** -24))
    assert d['ref']['lse'].shape == (X.B, X.H, Tq)


@pytest.mark.parametrize('case', X.CASES, ids=IDS)
def test_no_case_is_hollowed_out_by_underflow(case):
    """Elements whose bound is below 2^-100 are not compared: at most 1 % of any tensor (largest here: 0.58 %)."""
    ref = X.case_data(case)['ref']
    for n in A.TENSORS:
        share = A.underflow_share(ref['b_' + n])
        assert share <= UNDERFLOW_CAP, '%s: %.2f %% of b_%s below 2^-100' % (X.case_id(case), 100 * share, n)


def _caught(case, defect):
    d = X.case_data(case)
    bad = X.rounding_model(d['q'], d['k'], d['v'], d['dout'], d['scale'], defect=defect)
    res = A.bf16_violations(bad, d['model'], d['ref'])
    return [k for k, v in res.items() if v]


# a case per defect on which the criteria must see it: more than one key block (stale_max), any block at all
# (skip_last_block), fewer queries than keys (kv_sweep_tq)
@pytest.mark.parametrize('defect,case', [
    ('stale_max', (64, 75, 196, 'ramp')),
    ('stale_max', (32, 130, 257, 'plain')),
    ('skip_last_block', (64, 75, 196, 'plain')),
    ('skip_last_block', (32, 5, 1024, 'negative')),
    ('kv_sweep_tq', (64, 75, 196, 'plain')),
    ('kv_sweep_tq', (32, 16, 63, 'negative')),
], ids=lambda x: x if isinstance(x, str) else X.case_id(x))
def test_planted_defects_are_caught(defect, case):
    assert case in X.CASES
    kinds = _caught(case, defect)
    assert 'bound' in kinds, '%s on %s: only %s' % (defect, X.case_id(case), kinds)


def test_the_sound_model_is_not_caught():
    for case in ((64, 75, 196, 'plain'), (32, 1024, 5, 'negative')):
        assert _caught(case, None) == []


def test_equal_lengths_are_the_self_attention_model():
    """Tq = Tk with q, k, v the slices of one qkv: the reference and the model are attention_util's and
    attention_tiled_util's, bit for bit."""
    import attention_tiled_util as TU
    qkv, dout = A.make_inputs('plain', X.B, 75, X.H, 64, 11)
    q, k, v = [qkv[:, :, i].contiguous() for i in range(3)]
    ref, model = X.reference(q, k, v, dout, 0.125), X.rounding_model(q, k, v, dout, 0.125)
    ref0, model0 = A.reference(qkv, dout, 0.125, False), TU.tiled_rounding_model(qkv, dout, 0.125)
    for n in ref0:
        assert torch.equal(ref[n], ref0[n]), n
    for n in model0:
        assert torch.equal(model[n], model0[n]), n
