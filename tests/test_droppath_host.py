"""Stochastic depth (drop_path_rate) of the fine-tuning ViT — everything that needs no GPU: the Philox restatement
against published known answers, the committed fixtures, the constructor, the YAML key."""
import os

import numpy as np
import pytest
import torch

import droppath_util as DP
from passl_amd.hip import config as hip_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SMALL = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4)


def test_philox_restatement_matches_known_answer_vectors():
    DP.check_known_answers()
    # the table definition: a slot with keep_prob 1 never drops, one with keep_prob 0.5 drops about half
    t = DP.keep_table([1.0, 0.5], 4096, seed=(5 << 32) + 7, step=(1 << 33) + 3)
    assert t.dtype == np.float32 and t.shape == (2, 4096) and np.all(t[0] == 1)
    assert set(np.unique(t[1])) == {0.0, 1.0} and 0.45 < t[1].mean() < 0.55
    assert not np.array_equal(t, DP.keep_table([1.0, 0.5], 4096, seed=(5 << 32) + 7, step=(1 << 33) + 4))
    assert not np.array_equal(t, DP.keep_table([1.0, 0.5], 4096, seed=(6 << 32) + 7, step=(1 << 33) + 3))


@pytest.mark.parametrize('name,depth,rate', [('mae_ft_dp_small', 4, 0.3), ('mae_ft_dp_vit_b', 12, 0.1)])
def test_fixtures_hold_tables_that_drop_something(name, depth, rate):
    """What tests/golden/make_golden_mae_finetune_droppath.py asserts when it writes the files, on the committed files:
    a fixture whose tables are all ones would test nothing."""
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    N, _hw, steps, _classes = [int(v) for v in z['meta']]
    assert float(z['rate']) == rate and steps == 2 and N == 8
    for s in range(steps):
        keep = z['s%d_keep' % s]
        assert keep.shape == (2 * depth, N) and keep.dtype == np.float32
        assert np.all((keep == 0) | (keep == 1))
        assert np.all(keep[:2] == 1)                      # block 0: the ladder starts at zero
    dropped = z['s0_keep'] == 0
    assert dropped.sum() >= 5 and dropped.any(axis=1).sum() >= 3
    # and dropping is visible in what the fixture records (the distances the GPU test's discrimination check relies on)
    f, f0 = z['s0_feat_head'], z['s0_feat_head_nodrop']
    assert np.abs(f - f0).max() / np.abs(f0).max() > 0.1
    assert abs(float(z['s0_loss']) - float(z['s0_loss_nodrop'])) / abs(float(z['s0_loss_nodrop'])) > 3e-3


def test_fixture_adds_no_state_dict_entry():
    a = np.load(os.path.join(GOLDEN, 'mae_ft_dp_vit_b.npz'))['keys']
    b = np.load(os.path.join(GOLDEN, 'mae_ft_vit_b.npz'))['keys']
    assert [str(k) for k in a] == [str(k) for k in b]


def test_constructor_builds_the_reference_ladder():
    hip_config.set_device('cpu')
    from passl_amd.modeling.backbones.mae import MAE_ViT
    plain = MAE_ViT(embed_dim=768, depth=12, num_heads=12, patch_size=16, qkv_bias=True, mlp_ratio=4)
    m = MAE_ViT(embed_dim=768, depth=12, num_heads=12, patch_size=16, qkv_bias=True, mlp_ratio=4, drop_path_rate=0.1)
    ladder = np.linspace(0, 0.1, 12, dtype=np.float64)
    want = torch.linspace(0, 0.1, 12, dtype=torch.float32).numpy()
    assert np.allclose(want, ladder, atol=1e-7)
    for i, blk in enumerate(m.blocks):
        assert np.float32(blk.drop_path) == want[i], i
        assert np.float32(blk.keep_prob) == np.float32(1.0) - want[i], i
    assert m.blocks[0].drop_path == 0. and m.blocks[0].keep_prob == 1.
    assert all(blk.drop_path == 0. for blk in plain.blocks)
    # nothing new in the state_dict, nothing registered as a buffer
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert m.drop_path_step() == 0 and plain.drop_path_step() == 0


def test_constructor_argument_errors():
    hip_config.set_device('cpu')
    from passl_amd.modeling.backbones.mae import Block, MAE_ViT
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            MAE_ViT(drop_path_rate=bad, **SMALL)
    with pytest.raises(ValueError):
        Block(128, 4, drop_path=1.0)
    with pytest.raises(NotImplementedError):
        MAE_ViT(drop_rate=0.1, **SMALL)
    with pytest.raises(NotImplementedError):
        MAE_ViT(attn_drop_rate=0.1, drop_path_rate=0.1, **SMALL)


def test_seed_follows_the_global_generator_and_the_rank(monkeypatch):
    hip_config.set_device('cpu')
    from passl_amd.modeling.backbones.mae import MAE_ViT

    def seed_of(manual, rank=None):
        if rank is None:
            monkeypatch.delenv('RANK', raising=False)
        else:
            monkeypatch.setenv('RANK', str(rank))
        torch.manual_seed(manual)
        return MAE_ViT(drop_path_rate=0.2, **SMALL)._drop_path.seed
    a = seed_of(3)
    assert a == seed_of(3) and a != seed_of(4)
    assert seed_of(3, rank=2) == (a + 2) & (2 ** 64 - 1)          # an unseeded run: ranks still differ
    # a model without stochastic depth leaves the generator alone (weight initialisation of every existing recipe)
    torch.manual_seed(3)
    w0 = MAE_ViT(**SMALL).pos_embed.detach().clone()
    torch.manual_seed(3)
    assert torch.equal(w0, MAE_ViT(drop_path_rate=0., **SMALL).pos_embed.detach())
    m = MAE_ViT(drop_path_rate=0.2, **SMALL)
    m.set_drop_path_seed(12345, step=7)
    assert m._drop_path.seed == 12345 and m.drop_path_step() == 7


def test_droppath_yaml_loads_and_builds():
    hip_config.set_device('cpu')
    from passl_amd.modeling import build_model
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_droppath_synthetic.yaml'), [])
    assert cfg.model.architecture.drop_path_rate == 0.1
    base = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_synthetic.yaml'), [])
    arch = dict(cfg.model.architecture)
    arch.pop('drop_path_rate')
    assert arch == dict(base.model.architecture) and dict(cfg.optimizer) == dict(base.optimizer)
    model = build_model(cfg.model)
    assert type(model).__name__ == 'MAE_FINETUNE' and model.backbone.drop_path_rate == 0.1
    assert np.float32(model.backbone.blocks[-1].drop_path) == np.float32(0.1)
    assert not getattr(model, 'graph_safe', False)
