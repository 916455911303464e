"""``hnn.DropPathState`` under the four models that draw a keep table, on the device: the table of every training
forward is the Philox table of (the reference ladder's keep probabilities, seed, step) bit for bit, the device tensors
are allocated once, every block receives its own rows, and evaluation mode touches nothing."""
import numpy as np
import pytest
import torch

import drop_path_state_util as U
import droppath_util as DP
from passl_amd.hip import config as hip_config

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
SEED, STEP = 12345, 7


def _build(name):
    """-> (forward(x): one forward under no_grad in the model's current mode, the model that owns the state)."""
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    torch.manual_seed(5)
    if name == 'mae':
        from passl_amd.modeling import build_model
        wrapper = build_model(dict(name='MAE_FINETUNE',
                                   architecture=dict(name='MAE_ViT', drop_path_rate=U.MAE_RATE, **U.MAE_SMALL),
                                   head=dict(name='VisionTransformerClsHead', num_classes=16,
                                             in_channels=U.MAE_SMALL['embed_dim'])))
        return (lambda x: wrapper(x, mode='extract')), wrapper.backbone       # extract: refresh + backbone(x), no_grad
    model = U.build(name)

    def forward(x):
        with torch.no_grad():
            return model(x)
    return forward, model


def _spy(case, model):
    """-> seen: per trunk block and forward, what the block received as its keep argument: None, or (a copy taken
    at the call, its address, its shape)."""
    seen = []
    for blk in U.trunk_blocks(case.name, model):
        def fwd(*a, _f=blk.forward, **k):
            keep = a[case.keep_arg] if len(a) > case.keep_arg else k.get('keep', k.get('keep_row'))
            seen.append(None if keep is None else (keep.clone(), keep.data_ptr(), tuple(keep.shape)))
            return _f(*a, **k)
        blk.forward = fwd
    return seen


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('case', U.CASES, ids=U.IDS)
def test_training_forwards_draw_the_philox_table_and_hand_out_its_rows(case):
    forward, model = _build(case.name)
    probs = U.expected_keep_probs(case.name)
    blocks, owners = U.trunk_blocks(case.name, model), U.owning_blocks(case.name, model)
    seen = _spy(case, model)
    x = torch.randn(U.BATCH, 3, *case.hw, generator=torch.Generator().manual_seed(6)).to(DEV)
    model.train()
    model.set_drop_path_seed(SEED, STEP)
    assert model.drop_path_step() == STEP and model.drop_path_draws == 0 and model.drop_path_table(U.BATCH) is None
    ptrs, state_ptrs = [], []
    for k in range(2):
        del seen[:]
        out = forward(x)
        assert bool(torch.isfinite(out.float()).all())
        table = model.drop_path_table(U.BATCH)
        want = DP.keep_table(probs, U.BATCH, SEED, STEP + k)
        assert tuple(table.shape) == want.shape and table.dtype == torch.float32 and table.is_contiguous()
        assert np.array_equal(_bits(table.cpu().numpy()), _bits(want))
        assert model.drop_path_step() == STEP + 1 + k and model.drop_path_draws == 1 + k
        ptrs.append(table.data_ptr())
        state_ptrs.append((model._drop_path._dp_step.data_ptr(), model._drop_path._dp_keep_prob.data_ptr()))
        # every block received its own rows of THIS table, the others nothing
        assert len(seen) == len(blocks)
        row = 0
        for blk, got in zip(blocks, seen):
            if not any(blk is o for o in owners):
                assert got is None
                continue
            copy, ptr, shape = got
            assert shape == ((U.BATCH,) if case.rows == 1 else (case.rows, U.BATCH))
            assert ptr == table.data_ptr() + 4 * U.BATCH * row
            assert np.array_equal(_bits(copy.cpu().numpy().reshape(case.rows, U.BATCH)), _bits(want[row:row + case.rows]))
            row += case.rows
        assert row == len(probs)
    assert ptrs[0] == ptrs[1] and state_ptrs[0] == state_ptrs[1]
    # set_drop_path_seed refills the counter in place
    model.set_drop_path_seed(SEED, STEP + 2)
    assert model._drop_path._dp_step.data_ptr() == state_ptrs[0][0] and model.drop_path_step() == STEP + 2
    # evaluation mode: no draw, no table handed to any block, nothing moves
    last = model.drop_path_table(U.BATCH).clone()
    model.eval()
    del seen[:]
    forward(x)
    assert all(got is None for got in seen)
    assert model.drop_path_step() == STEP + 2 and model.drop_path_draws == 2
    assert model.drop_path_table(U.BATCH).data_ptr() == ptrs[0] and torch.equal(model.drop_path_table(U.BATCH), last)
