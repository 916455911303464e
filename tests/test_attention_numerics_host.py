"""Keeps the criteria of tests/test_attention_numerics_gpu.py honest without a GPU (helpers: attention_util.py).

* the closeness caps (rms ratio, disagreement share) hold when the float32 rounding model stands in for a kernel:
  worst over the matrix 0.16 (cap 0.75) and 0.25 % (cap 1 %);
* the float64 rounding model stays inside the a-priori bounds against the float64 reference: worst 1.85 u for
  out / dv (limit 2.25 u), 1.04 u for dq / dk (limit 3.25 u);
* a rounding model with a planted defect (one extra zero key, causal mask off by one, last key dropped, delta
  omitted) is rejected by each criterion on `negative` and / or `ramp`, at T = 17 and T = 208;
* at most 1 % of any bound is below 2^-100 (underflowed probabilities), so the comparison is never vacuous.
"""
import pytest
import torch

import attention_util as A

IDS = [A.case_id(c) for c in A.CASES]


def test_inputs_hold_bf16_values_and_follow_the_recipes():
    for kind in A.KINDS:
        qkv, dout = A.make_inputs(kind, 2, 40, 3, 32, seed=7)
        assert qkv.shape == (2, 40, 3, 3, 32) and dout.shape == (2, 40, 3, 32)
        assert torch.equal(qkv, A.bf16_round(qkv)) and torch.equal(dout, A.bf16_round(dout))
        again, _ = A.make_inputs(kind, 2, 40, 3, 32, seed=7)
        assert torch.equal(qkv, again)

    def scores(kind):
        qkv, _ = A.make_inputs(kind, 2, 40, 3, 32, seed=7)
        return torch.einsum('bihd,bjhd->bhij', qkv[:, :, 0].double(), qkv[:, :, 1].double()) * 32 ** -0.5

    neg, ramp = scores('negative'), scores('ramp')
    assert -60 < neg.min() and neg.max() < -8                   # a leaked score of 0 would own the softmax
    assert abs(float((ramp[..., 1:] - ramp[..., :-1]).mean()) - A.ramp_slope(40)) < 0.1
    assert scores('peaked').abs().max() > 100
    vmean = A.reference(*A.make_inputs('vmean', 2, 40, 3, 32, seed=7), 32 ** -0.5, False)
    assert (vmean['out'].mean() - 3).abs() < 0.2


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_underflow_share(case):
    ref = A.case_data(case)['ref']
    for n in A.TENSORS:
        assert torch.isfinite(ref[n]).all() and torch.isfinite(ref['b_' + n]).all()
        assert A.underflow_share(ref['b_' + n]) <= 0.01, n
    assert torch.isfinite(ref['lse']).all()


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_float64_rounding_model_is_inside_the_a_priori_bounds(case):
    d = A.case_data(case)
    msgs = []
    for n in A.TENSORS:
        msgs += A.bound_violations(n, d['model'][n], d['ref'][n], d['ref']['b_' + n], A.LIMIT_BF16[n])
    assert not msgs, '\n'.join(msgs)
    assert (d['model']['lse'] - d['ref']['lse']).abs().max() < 1e-12


@pytest.mark.parametrize('case', A.CASES, ids=IDS)
def test_caps_hold_for_the_float32_rounding_model(case):
    d = A.case_data(case)
    m32 = A.rounding_model(d['qkv'], d['dout'], d['scale'], case[2], dtype=torch.float32)
    res = A.bf16_violations(m32, d['model'], d['ref'])
    assert not any(res.values()), '\n'.join(sum(res.values(), []))


# defect -> (causal, the kind(s) on which EVERY criterion must reject it at both lengths)
PLANTED = {'zero_key': (False, ('negative',)),
           'drop_last': (False, ('ramp',)),
           'mask_shift': (True, ('negative', 'ramp')),
           'no_delta': (False, ('negative', 'ramp'))}


@pytest.mark.parametrize('T', [17, 208])
@pytest.mark.parametrize('defect', A.DEFECTS)
def test_criteria_reject_a_planted_defect(defect, T):
    causal, kinds = PLANTED[defect]
    for kind in kinds:
        for DH in A.HEAD_DIMS:
            d = A.case_data((DH, T, causal, kind))
            bad = A.rounding_model(d['qkv'], d['dout'], d['scale'], causal, defect=defect)
            res = A.bf16_violations(bad, d['model'], d['ref'])
            for crit in ('bound', 'rms', 'share'):
                assert res[crit], '%s not seen by the %s criterion on %s, T = %d, d = %d' % (defect, crit, kind, T, DH)
            if defect != 'no_delta':                                   # delta only enters dq / dk
                assert any(m.split(': ')[1].startswith('out') for m in res['bound'])
            # the clean model passes the very same calls
            assert not any(A.bf16_violations(d['model'], d['model'], d['ref']).values())
