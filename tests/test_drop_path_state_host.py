"""``hnn.DropPathState`` / ``hnn.DropPathModel`` under the four models that draw a keep table — everything that needs no
GPU and launches nothing: the rows' keep probabilities, where the seed is drawn in the host generator's stream, the
64-bit step, the refusals, and that nothing of the state reaches ``state_dict()``."""
import numpy as np
import pytest
import torch

import drop_path_state_util as U
from passl_amd.hip import config as hip_config
from passl_amd.hip import nn as hnn

CPU = torch.device('cpu')
MASK64 = 2 ** 64 - 1


def _build(name, rate=None, seed=None):
    hip_config.set_device('cpu')
    hip_config.set_compute_dtype(torch.float32)
    if seed is not None:
        torch.manual_seed(seed)
    return U.build(name, rate)


def _next_randint():
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


@pytest.mark.parametrize('case', U.CASES, ids=U.IDS)
def test_keep_probs_are_the_reference_ladder_of_the_owning_blocks(case):
    model = _build(case.name)
    st = model._drop_path
    want = U.expected_keep_probs(case.name)
    assert type(st) is hnn.DropPathState and st.keep_probs == want
    owners = U.owning_blocks(case.name, model)
    assert len(st.blocks) == len(owners) and all(a is b for a, b in zip(st.blocks, owners))
    assert len(want) == case.rows * len(owners)
    if case.name == 'mae':
        assert want[0] == want[1] == 1.0                       # block 0 owns rows although it never drops
    else:
        assert all(p < 1.0 for p in want)
    # a block's rows are its slice of the table, in network order; a block that cannot drop owns none
    table = torch.arange(len(want) * U.BATCH, dtype=torch.float32).view(len(want), U.BATCH)
    k = 0
    for blk in U.trunk_blocks(case.name, model):
        got = model._drop_path_rows(table, blk)
        if any(blk is o for o in owners):
            assert torch.equal(got, table[k] if case.rows == 1 else table[k:k + case.rows])
            k += case.rows
        else:
            assert got is None
        assert model._drop_path_rows(None, blk) is None
    assert k == len(want)
    # the constructor of the state draws nothing
    before = torch.random.get_rng_state()
    hnn.DropPathState(want, seed=1)
    hnn.DropPathState.for_blocks(owners, case.rows)
    assert torch.equal(before, torch.random.get_rng_state())


@pytest.mark.parametrize('case', [c for c in U.CASES if c.name != 'mae'], ids=[n for n in U.IDS if n != 'mae'])
def test_seed_is_drawn_after_the_weights(case, monkeypatch):
    """A model with stochastic depth initialises as one without; its seed is the generator's next draw plus the rank."""
    monkeypatch.setenv('RANK', '3')
    plain = _build(case.name, rate=0., seed=41)
    want_seed = _next_randint() + 3
    dropping = _build(case.name, seed=41)
    assert plain._drop_path is None and plain.drop_path_draws == 0
    a, b = plain.state_dict(), dropping.state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert dropping._drop_path.seed == want_seed & MASK64
    # exactly one draw: the generators stand at the same place after both constructors and that draw
    torch.manual_seed(41)
    _build(case.name, rate=0.)
    _next_randint()
    after_plain = torch.random.get_rng_state()
    _build(case.name, seed=41)
    assert torch.equal(after_plain, torch.random.get_rng_state())


def test_mae_seed_is_drawn_in_front_of_the_weights(monkeypatch):
    from passl_amd.modules.vit import trunc_normal_
    monkeypatch.delenv('RANK', raising=False)
    model = _build('mae', seed=41)
    torch.manual_seed(41)
    want_seed = _next_randint()
    cls = torch.zeros(1, 1, U.MAE_SMALL['embed_dim'])
    trunc_normal_(cls, std=0.02)
    assert model._drop_path.seed == want_seed
    assert torch.equal(model.cls_token.detach(), cls)
    # without stochastic depth nothing is drawn in front of the class token
    torch.manual_seed(41)
    trunc_normal_(cls, std=0.02)
    assert torch.equal(_build('mae', rate=0., seed=41).cls_token.detach(), cls)


@pytest.mark.parametrize('case', U.CASES, ids=U.IDS)
def test_seed_and_step_are_64_bit_before_any_device_state(case):
    model = _build(case.name)
    model.set_drop_path_seed(2 ** 64 - 1, 2 ** 63 + 5)
    assert model.drop_path_step() == 2 ** 63 + 5
    assert model._drop_path.seed == 2 ** 64 - 1
    model.set_drop_path_seed(2 ** 64 + 9, 7)
    assert model._drop_path.seed == 9 and model.drop_path_step() == 7
    st = model._drop_path
    assert st._dp_step is None and st._dp_keep_prob is None and st.table(U.BATCH) is None and st.draws == 0
    assert model.drop_path_table(U.BATCH) is None and model.drop_path_draws == 0


@pytest.mark.parametrize('case', U.CASES, ids=U.IDS)
def test_injected_tables_are_validated_and_never_drawn(case):
    model = _build(case.name)
    rows = len(U.expected_keep_probs(case.name))
    model.train()
    for shape in ((rows + 1, U.BATCH), (rows, U.BATCH + 1), (U.BATCH, rows + 7), (rows * U.BATCH,)):
        with pytest.raises(ValueError):
            model._drop_path_keep(U.BATCH, CPU, torch.ones(shape))
    given = torch.ones(U.BATCH, rows, dtype=torch.float64).t()             # not fp32, not contiguous
    got = model._drop_path_keep(U.BATCH, CPU, given)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (rows, U.BATCH)
    assert torch.equal(got, torch.ones(rows, U.BATCH))
    model.eval()
    assert model._drop_path_keep(U.BATCH, CPU) is None
    with pytest.raises(ValueError):
        model._drop_path_keep(U.BATCH, CPU, torch.ones(rows, U.BATCH))     # a table in evaluation mode
    plain = _build(case.name, rate=0.).train()
    assert plain._drop_path_keep(U.BATCH, CPU) is None
    with pytest.raises(ValueError):
        plain._drop_path_keep(U.BATCH, CPU, torch.ones(rows, U.BATCH))     # a table to a model that cannot drop
    # nothing above drew a table or made device state
    assert model.drop_path_draws == 0 and model._drop_path._dp_step is None and model.drop_path_step() == 0


@pytest.mark.parametrize('case', U.CASES, ids=U.IDS)
def test_state_is_not_in_the_state_dict(case):
    plain, model = _build(case.name, rate=0.), _build(case.name)
    st = model._drop_path
    assert not isinstance(st, torch.nn.Module)
    assert '_drop_path' not in model._modules and '_drop_path' not in model._buffers
    assert list(model.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in model.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert [n for n, _ in model.named_modules()] == [n for n, _ in plain.named_modules()]
    assert not [k for k in model.state_dict() if 'drop_path' in k or '_dp' in k]
    assert np.float32(st.keep_probs[-1]) == np.float32(model._drop_path.blocks[-1].keep_prob)
