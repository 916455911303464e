"""Random erasing on the MI355X: 'const' against the reference's erased regions bit for bit (tolerance 0), hand-made
box tables in both modes and both aliasing forms, the 'pixel' normals against their float64 restatement, and the wiring
into the loaders, the fine-tuning step and the Trainer."""
import os
import random

import numpy as np
import pytest
import torch

import random_erasing_util as RU

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
ERASE_YAML = os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_erase_synthetic.yaml')

# |kernel - float64 restatement| inside a box: the last-place errors of logf / sqrtf / sincospif on values up to |z| ~ 5.
# The bound is 4 x the largest deviation MEASURED on the MI355X over the four shapes of test_hand_made_tables_both_modes
# and the 12 288 values of test_pixel_moments_and_identity (both print it), and may never exceed 1e-4: a wrong word, a
# swapped sine / cosine or a shifted counter is off by O(1).  PIXEL_DEV_MEASURED = None: NOT MEASURED YET — the bound
# then stands at the cap.  (Without a GPU: the kernel's source built for the host is within 2.9e-7 of the restatement.)
PIXEL_DEV_MEASURED = None
PIXEL_BOUND = 1e-4 if PIXEL_DEV_MEASURED is None else 4 * PIXEL_DEV_MEASURED
assert PIXEL_BOUND <= 1e-4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _table(rows):
    return torch.tensor(np.asarray(rows, dtype=np.int32).reshape(-1, 4), device=DEV)


# ---------------------------------------------------------------------------------------------- 1. 'const' vs the reference
@pytest.mark.parametrize('case', RU.CASES, ids=lambda c: 'seed%d' % c[0])
def test_const_reproduces_the_reference_regions(case):
    """RandomErasing(mode='const') under random.Random(seed): the result equals the slice assignment over the regions
    the reference's class erased (tests/golden/random_erasing_boxes.npz) bit for bit; the input is bit-unchanged and
    the result is another tensor.  (15, 17): 765 elements per sample, the scalar form."""
    from passl_amd.datasets.preprocess import RandomErasing
    seed, (B, H, W), kw, _erased, _rejected = case
    z = np.load(os.path.join(GOLDEN, 'random_erasing_boxes.npz'))
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, W, generator=gen)
    xd = x.to(DEV)
    fn = RandomErasing(mode='const', rng=random.Random(seed), seed=1, **kw)
    keys = ['boxes_%d' % seed] + (['boxes_%d_second' % seed] if seed == RU.SECOND_CALL_SEED else [])
    for n, key in enumerate(keys):
        got = fn(xd)
        want = x.clone()
        for b, (top, left, h, w) in enumerate(z[key].tolist()):
            want[b, :, top:top + h, left:left + w] = 0.
        assert got.data_ptr() != xd.data_ptr()
        assert torch.equal(_bits(got.cpu()), _bits(want)), key
        assert fn.step == n + 1
    assert torch.equal(_bits(xd.cpu()), _bits(x))


# ---------------------------------------------------------------------------------------------- 2. hand-made tables
def _boxes(H, W):
    """(top, left, h, w): empty by h = 0, empty by w = 0, all zeros, the two (H-1) x (W-1) boxes, 1 x 1 at the four
    corners, odd left and w crossing 16-byte chunks, one row, one column, the whole image."""
    return [(1, 1, 0, 2), (1, 1, 2, 0), (0, 0, 0, 0), (0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1),
            (0, 0, 1, 1), (0, W - 1, 1, 1), (H - 1, 0, 1, 1), (H - 1, W - 1, 1, 1),
            (1, 1, max(H - 2, 1), min(W - 1, 7)), (H // 2, min(3, W - 1), 2, min(W - min(3, W - 1), 5)),
            (H // 2, 0, 1, W), (0, W // 2, H, 1), (0, 0, H, W)]


def _check(x, xd, table, mode, seed, step):
    """One out-of-place and one in-place launch against the restatement -> the largest deviation inside the boxes."""
    from passl_amd.datasets.preprocess import RandomErasing
    from passl_amd.hip import ops
    B, C, H, W = x.shape
    RandomErasing.validate(table, H, W)                      # no out-of-range box is ever sent to the device
    td = _table(table)
    got = ops.random_erase(xd, td, mode, seed, step)
    assert got.data_ptr() != xd.data_ptr()
    ref, m = RU.erase_ref(x.numpy(), table, mode, seed, step)
    g = got.cpu().numpy()
    assert np.array_equal(g[~m].view(np.int32), x.numpy()[~m].view(np.int32))       # outside: the bits of x
    dev = float(np.abs(g[m].astype(np.float64) - ref[m]).max()) if m.any() else 0.
    if mode == 0:
        assert dev == 0. and not np.signbit(g[m]).any()
    inplace = xd.clone()
    assert ops.random_erase(inplace, td, mode, seed, step, out=inplace) is inplace
    assert torch.equal(_bits(inplace), _bits(got))
    return dev


@pytest.mark.parametrize('shape', [(8, 3, 32, 32), (6, 3, 37, 53), (7, 1, 5, 3), (1, 3, 16, 20)])
def test_hand_made_tables_both_modes(shape):
    """Outside the box the result is bit-equal to x; inside it is 0 (mode 0) or the float64 restatement of the normal
    within PIXEL_BOUND (mode 1); in place gives the bits of out of place; x is never written.  (6, 3, 37, 53) and
    (7, 1, 5, 3): samples that do not start on 16-byte boundaries, the scalar form; (8, 3, 32, 32): three workgroups per
    sample."""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen)
    xd = x.to(DEV)
    boxes = _boxes(H, W)
    worst = 0.
    for first in range(0, len(boxes), B):
        table = np.array([boxes[(first + b) % len(boxes)] for b in range(B)], dtype=np.int32)
        assert _check(x, xd, table, 0, 0, 0) == 0.
        worst = max(worst, _check(x, xd, table, 1, 0x9e3779b97f4a7c15, first + (1 << 40)))
    print('pixel: largest |kernel - float64| over %s: %.3e (bound %.3e)' % (shape, worst, PIXEL_BOUND))
    assert worst <= PIXEL_BOUND
    assert torch.equal(_bits(xd.cpu()), _bits(x))


def test_misaligned_views_take_the_scalar_form():
    """C*H*W % 4 == 0 but the pointers are not 16-byte aligned: single floats, the same values."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 3, 8, 8, generator=gen)
    buf = torch.zeros(x.numel() + 1, device=DEV)
    xd = buf[1:].view(2, 3, 8, 8)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4
    table = np.array([[1, 1, 5, 6], [0, 3, 8, 2]], dtype=np.int32)
    got = ops.random_erase(xd, _table(table), 1, 7, 3)
    ref, m = RU.erase_ref(x.numpy(), table, 1, 7, 3)
    g = got.cpu().numpy()
    assert np.array_equal(g[~m].view(np.int32), x.numpy()[~m].view(np.int32))
    assert float(np.abs(g[m] - ref[m]).max()) <= PIXEL_BOUND
    aligned = ops.random_erase(x.to(DEV), _table(table), 1, 7, 3)
    assert torch.equal(_bits(aligned), _bits(got))           # the value is defined by position, not by the chunking


def test_refuses_bad_arguments_and_clamps_the_table():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib = L.load()
    x = torch.randn(4, 3, 8, 8, device=DEV)
    out = torch.empty_like(x)
    t = _table([[0, 0, 2, 2]] * 4)
    p, q, tb, st = x.data_ptr(), out.data_ptr(), t.data_ptr(), L.stream()

    def call(x_=p, out_=q, t_=tb, B=4, C=3, H=8, W=8, mode=0):
        return lib.passl_hip_random_erase(x_, out_, t_, B, C, H, W, mode, 1, 0, st)
    assert call() == 0 and call(out_=p) == 0
    assert call(x_=None) == -1 and call(out_=None) == -1 and call(t_=None) == -1
    assert call(B=-1) == -1 and call(C=0) == -1 and call(H=0) == -1 and call(W=-3) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(C=1 << 11, H=1 << 10, W=1 << 10) == -1        # C*H*W = 2^31
    assert call(B=0) == 0
    with pytest.raises(L.PasslHipError):
        ops.random_erase(torch.zeros(2, 3, 8, 8), torch.zeros(2, 4, dtype=torch.int32), 0, 0, 0)     # host tensors
    # whatever the table holds, no access leaves the tensor: every box is clamped to the image
    x = torch.randn(4, 3, 8, 8, device=DEV)
    wild = _table([[-3, -2, 6, 5], [6, 5, 100, 100], [2, 2, -4, 3], [2 ** 31 - 1, 0, 2 ** 31 - 1, 2 ** 31 - 1]])
    got = ops.random_erase(x, wild, 0, 0, 0).cpu()
    want = x.cpu().clone()
    want[0, :, 0:6, 0:5] = 0.                                 # top/left clamped to 0, the extent kept
    want[1, :, 6:8, 5:8] = 0.
    assert torch.equal(_bits(got), _bits(want))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. 'pixel'
def test_pixel_moments_and_identity():
    """The GPU's own values over 16 whole samples of 3 x 16 x 16: mean within 5 / sqrt(n), variance within
    5 sqrt(2 / n) of (0, 1), as for the host restatement, and within PIXEL_BOUND of it value for value; the same
    (seed, step) gives the same bits on two launches; sample b of a B = 8 launch equals sample b of a B = 3 launch with
    the same box; step + 1 differs."""
    from passl_amd.hip import ops
    a = RU.MOMENT_ARGS
    B, C, H, W = a['B'], 3, 16, 16
    x = torch.zeros(B, C, H, W, device=DEV)
    full = np.array([[0, 0, H, W]] * B, dtype=np.int32)
    got = ops.random_erase(x, _table(full), 1, a['seed'], a['step'])
    z = got.cpu().numpy().astype(np.float64).reshape(-1)
    n = z.size
    ref = np.concatenate([RU.normals(a['seed'], a['step'], b, a['E']) for b in range(B)])
    dev = float(np.abs(z - ref).max())
    print('gpu normals: mean %.4f var %.4f max |z| %.2f; largest |kernel - float64| %.3e (bound %.3e)'
          % (z.mean(), z.var(), np.abs(z).max(), dev, PIXEL_BOUND))
    assert n == 12288 and np.isfinite(z).all()
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert dev <= PIXEL_BOUND
    again = ops.random_erase(x, _table(full), 1, a['seed'], a['step'])
    assert torch.equal(_bits(again), _bits(got))
    box = [3, 2, 9, 11]
    b8 = ops.random_erase(x[:8], _table([box] * 8), 1, a['seed'], a['step'])
    b3 = ops.random_erase(x[:3], _table([box] * 3), 1, a['seed'], a['step'])
    assert torch.equal(_bits(b8[:3]), _bits(b3))
    assert torch.equal(_bits(b8[:, :, 3:12, 2:13]), _bits(got[:8, :, 3:12, 2:13]))     # nor on the box
    nxt = ops.random_erase(x, _table(full), 1, a['seed'], a['step'] + 1)
    assert not (nxt == got).any()
    other = ops.random_erase(x, _table(full), 1, a['seed'] + 1, a['step'])
    assert not (other == got).any()


# ---------------------------------------------------------------------------------------------- 4. wiring
FT_ARCH = dict(name='MAE_ViT', patch_size=16, embed_dim=768, depth=12, num_heads=12, qkv_bias=True, mlp_ratio=4)
SMALL = dict(FT_ARCH, embed_dim=128, depth=4, num_heads=4, img_size=64)


def _spy_on_ops(monkeypatch):
    """-> calls: the name of every public function of passl_amd.hip.ops, in call order (the spy of
    tests/test_mixup_gpu.py)."""
    import types
    from passl_amd.hip import ops
    calls = []
    for name, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith('_') and fn.__module__ == ops.__name__:
            def wrapped(*a, _f=fn, _n=name, **k):
                calls.append(_n)
                return _f(*a, **k)
            monkeypatch.setattr(ops, name, wrapped)
    return calls


def _build_finetune(arch, classes, dtype):
    from oracle.mae import finetune_state
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    model = build_model(dict(name='MAE_FINETUNE', architecture=dict(arch),
                             head=dict(name='VisionTransformerClsHead', num_classes=classes,
                                       in_channels=arch['embed_dim'])))
    keys_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(dict(finetune_state(keys_shapes)), strict=False)
    assert not missing and not unexpected
    return model


def _loader(eraser, ring=0):
    from passl_amd.datasets.synthetic import HostRingLoader, SyntheticLabeled, SyntheticLoader
    ds = SyntheticLabeled(num_samples=16, image_size=64, num_classes=16, seed=3)
    loader = SyntheticLoader(ds, 8, DEV, batch_transform=eraser)
    return HostRingLoader(loader, ring=ring) if ring else loader


def test_step_launches_one_erase_in_front_and_nothing_else_moves(monkeypatch):
    import mixup_util as MU
    from passl_amd.datasets.preprocess import Mixup, RandomErasing
    torch.manual_seed(1)
    model = _build_finetune(dict(SMALL), 16, torch.float32)
    model.train()
    plain_loader = _loader(None)
    eraser = RandomErasing(prob=1., mode='pixel', rng=random.Random(0), seed=1)
    erase_loader = _loader(eraser)
    ring_loader = _loader(RandomErasing(prob=1., mode='pixel', rng=random.Random(0), seed=1), ring=3)
    calls = _spy_on_ops(monkeypatch)

    def run(loader, **kw):
        del calls[:]
        x, y = next(iter(loader))
        out = model(x, y, mode='train', **kw)
        out['loss'].backward()
        return list(calls)
    plain = run(plain_loader)
    assert 'random_erase' not in plain and plain == run(plain_loader)       # without the entry: what it launched before
    erased = run(erase_loader)
    assert erased == ['random_erase'] + plain and eraser.step == 1
    assert run(ring_loader) == ['random_erase'] + plain
    # with a mixup_fn as well: erasing first (the loader), then the collate-time mix (the same draw in both runs)
    mixed_plain = run(plain_loader, mixup_fn=Mixup(num_classes=16, rng=np.random.RandomState(0), **MU.RECIPE))
    mixed = run(erase_loader, mixup_fn=Mixup(num_classes=16, rng=np.random.RandomState(0), **MU.RECIPE))
    assert mixed[:3] == ['random_erase', 'batch_mix', 'mixup_target']
    assert mixed == ['random_erase'] + mixed_plain


def test_loader_yields_erased_batches_and_keeps_its_cache():
    """The yielded batch differs from the cached one exactly inside the drawn boxes; the cached batch stays
    bit-unchanged; labels are passed through."""
    from passl_amd.datasets.preprocess import RandomErasing
    loader = _loader(RandomErasing(prob=.5, mode='pixel', rng=random.Random(21), seed=5))
    twin = RandomErasing(prob=.5, mode='pixel', rng=random.Random(21), seed=5)
    cached = [(_bits(x).clone(), y.clone()) for x, y in loader._cache]
    assert len(loader) == 2 and len(loader._cache) == 1
    for x, y in loader:
        cx, cy = loader._cache[0]
        table = twin.draw(8, 64, 64)
        m = torch.from_numpy(RU.box_mask(table, 3, 64, 64))
        assert m.any() and not m.all()
        assert x.data_ptr() != cx.data_ptr() and y is cy
        assert torch.equal((_bits(x) != _bits(cx)).cpu(), m)
    assert loader.batch_transform.step == 2
    for (x, y), (bx, by) in zip(loader._cache, cached):
        assert torch.equal(_bits(x), bx) and torch.equal(y, by)


def test_trainer_runs_erase_config_end_to_end(tmp_path):
    """configs/mae/mae_vit_b_finetune_erase_synthetic.yaml through the v110 Trainer, shrunk to the small ViT of the other
    fine-tuning tests: three steps, finite losses; every batch the step received differs from the cached batch exactly
    inside the boxes drawn from Python's global `random` stream."""
    from passl_amd.engine.trainer import Trainer
    from passl_amd.utils.config import get_config
    cfg = get_config(ERASE_YAML,
                     ['dataloader.train.sampler.batch_size=8', 'dataloader.train.dataset.num_samples=24',
                      'dataloader.train.dataset.image_size=64', 'dataloader.train.dataset.num_classes=16',
                      'model.architecture.embed_dim=128', 'model.architecture.depth=4', 'model.architecture.num_heads=4',
                      'model.head.in_channels=128', 'model.head.num_classes=16',
                      'epochs=1', 'output_dir=%s' % tmp_path, 'log_config.interval=1'])
    cfg.timestamp = ''
    cfg.model.architecture['img_size'] = 64                  # (a key the YAML does not carry: overrides cannot add one)
    torch.manual_seed(5)
    tr = Trainer(cfg)
    fn = tr.train_dataloader.batch_transform
    assert type(tr.model).__name__ == 'MAE_FINETUNE' and tr.iters_per_epoch == 3 and tr.mixup_fn is None
    assert type(fn).__name__ == 'RandomErasing' and (fn.prob, fn.mode, fn.step) == (0.25, 'pixel', 0)
    cached = tr.train_dataloader._cache[0][0]
    before = _bits(cached).clone()
    losses, diffs = [], []
    step = tr.train_step

    def train_step(data):
        diffs.append((_bits(data[0]) != before).cpu())
        out = step(data)
        losses.append(float(out['loss'].detach()))
        return out
    tr.train_step = train_step
    random.seed(5)
    tr.train()
    print('losses', losses)
    assert tr.current_iter == 3 and len(losses) == 3 and fn.step == 3
    assert all(np.isfinite(v) and 0 < v < 20 for v in losses)
    twin = type(fn)(prob=0.25, mode='pixel', max_count=1, rng=random.Random(5), seed=0)
    erased = 0
    for d in diffs:
        m = torch.from_numpy(RU.box_mask(twin.draw(8, 64, 64), 3, 64, 64))
        erased += int(m.any())
        assert torch.equal(d, m)
    assert erased >= 1
    assert torch.equal(_bits(cached), before)
    del tr
    torch.cuda.empty_cache()
