"""The float64 rounding model of the key-tiled bf16 forward (attention_tiled_util.py) against the float64 reference, on
the CPU: the a-priori limits of the bf16-MFMA kernels hold for an online softmax over key blocks of 64, the criteria see
three bugs a tiled forward can have, and no case of the matrix is hollowed out by underflow.

Measured here: the model uses at most 0.85 of LIMIT_BF16 (dv of d32-T1024-peaked; 1.90 u of 2.25 u), and the share of
elements with a bound below 2^-100 is 0 for every tensor of every case.

The stale max ('stale_max': the accumulator is not rescaled when the running max rises) is caught by `plain` alone, on
every plain case of more than one key block (T >= 128, both head dimensions: 28 cases), by all three criteria; `ramp`,
whose max rises in every block, catches it as well.  test_plain_alone_catches_the_stale_max pins d64-T577-plain.
"""
import pytest
import torch

import attention_tiled_util as TU
import attention_util as A

IDS = [A.case_id(c) for c in TU.CASES]


@pytest.mark.parametrize('case', TU.CASES, ids=IDS)
def test_tiled_model_is_inside_the_bf16_limits(case):
    d = TU.case_data(case)
    msgs = []
    for n in A.TENSORS:
        msgs += A.bound_violations(n, d['model'][n], d['ref'][n], d['ref']['b_' + n], A.LIMIT_BF16[n])
    assert not msgs, A.case_id(case) + ':\n' + '\n'.join(msgs)
    assert torch.isfinite(d['model']['lse']).all()
    assert float((d['model']['lse'] - d['ref']['lse']).abs().max()) <= 2.0 ** -40 * max(1.0, float(d['ref']['lse'].abs().max()))


@pytest.mark.parametrize('case', TU.CASES, ids=IDS)
def test_no_case_is_hollowed_out_by_underflow(case):
    """Elements whose bound is below 2^-100 are not compared; the cap is 1 % per tensor and case, and on the CPU the
    share is 0 for every case of this matrix."""
    ref = TU.case_data(case)['ref']
    for n in A.TENSORS:
        assert A.underflow_share(ref['b_' + n]) == 0.0, '%s: %s' % (A.case_id(case), n)


def _caught(case, defect):
    d = TU.case_data(case)
    bad = TU.tiled_rounding_model(d['qkv'], d['dout'], d['scale'], defect=defect)
    res = A.bf16_violations(bad, d['model'], d['ref'])
    return [k for k, v in res.items() if v]


# a case per defect on which the criteria must see it; the planted bug needs more than one key block (stale_max), any
# block at all (skip_last_block) or a partial last block (pad_zero)
@pytest.mark.parametrize('defect,case', [
    ('stale_max', (64, 257, False, 'ramp')),
    ('stale_max', (32, 578, False, 'ramp')),
    ('skip_last_block', (64, 577, False, 'plain')),
    ('skip_last_block', (32, 1024, False, 'negative')),
    ('pad_zero', (64, 577, False, 'negative')),
    ('pad_zero', (32, 209, False, 'plain')),
], ids=lambda x: x if isinstance(x, str) else A.case_id(x))
def test_planted_defects_are_caught(defect, case):
    assert case in TU.CASES
    kinds = _caught(case, defect)
    assert 'bound' in kinds, '%s on %s: only %s' % (defect, A.case_id(case), kinds)


def test_plain_alone_catches_the_stale_max():
    kinds = _caught((64, 577, False, 'plain'), 'stale_max')
    assert kinds == ['bound', 'rms', 'share'], kinds


def test_a_whole_last_block_has_no_padding_to_miscount():
    """pad_zero is invisible where the last block is whole: the model is then the sound one, bit for bit."""
    d = TU.case_data((64, 256, False, 'plain'))
    bad = TU.tiled_rounding_model(d['qkv'], d['dout'], d['scale'], defect='pad_zero')
    for n in A.TENSORS + ('lse',):
        assert torch.equal(bad[n], d['model'][n])


def test_one_block_is_the_dense_model_up_to_the_place_of_the_division():
    """T <= 64 is one block: running max = row max, so the tiled model differs from attention_util.rounding_model only in
    rounding exp(s - m) instead of exp(s - m) / z; both are within the limits of the same reference."""
    d = TU.case_data((64, 17, False, 'plain'))
    dense = A.rounding_model(d['qkv'], d['dout'], d['scale'], False)
    assert float((dense['lse'] - d['model']['lse']).abs().max()) <= 2.0 ** -40
    for n in A.TENSORS:
        assert not A.bound_violations(n, dense[n], d['ref'][n], d['ref']['b_' + n], A.LIMIT_BF16[n])
