"""Random resized crop + flip + normalise on the MI355X: the kernel against the reference's PIL path bit for bit
(tests/golden/crop_resize_small.npz, tolerance 0), against the numpy restatement on the shapes where it takes another
path, clamping and guard rows, and the wiring into the loaders, a step plan and the fine-tuning step."""
import copy
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import crop_resize_util as CU

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NORM = (CU.MEAN, CU.STD, float(np.float32(CU.SCALE)))

CROP_TF = [dict(name='MAERandCropImage', size=32, scale=[0.2, 1.0], interpolation='bicubic', backend='pil'),
           dict(name='RandomHorizontalFlip'),
           dict(name='NormalizeImage', scale='1.0/255.0', mean=list(CU.MEAN), std=list(CU.STD), order='hwc'),
           dict(name='ToCHWImage')]


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'crop_resize_small.npz'))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """fp32 device tensor == fp32 numpy array, bit for bit."""
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))


def _table(t):
    return torch.tensor(np.asarray(t, dtype=np.int32).reshape(-1, 8), device=DEV)


def _raw_call(src, out_ptr, table, S, B=None):
    """The entry point itself, on an output address of the caller's choice."""
    from passl_amd.hip import lib as L
    consts = (C.c_float * 7)(*CU.MEAN, *CU.STD, CU.SCALE)
    B = src.shape[0] if B is None else B
    return L.load().passl_hip_crop_resize_norm(src.data_ptr(), out_ptr, table.data_ptr(), B, src.shape[1], src.shape[2],
                                               S, C.cast(consts, C.c_void_p), L.stream())


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('key', ['a', 'a_second', 'b', 'c'])
def test_kernel_equals_the_reference_pil_path(golden, key):
    """ops.crop_resize_norm on the golden sources and tables = the fp32 CHW batches the reference's classes produced
    through Pillow, bit for bit; the source is bit-unchanged and the result is a tensor of its own."""
    from passl_amd.hip import ops
    src = torch.from_numpy(golden['src_' + key[0]]).to(DEV)
    before = src.clone()
    got = ops.crop_resize_norm(src, _table(golden['table_' + key]), 32, *NORM)
    want = golden['f32_' + key]
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    print('%s: %d of %d values differ' % (key, int((g.view(np.int32) != want.view(np.int32)).sum()), want.size))
    assert _same(got, want)
    assert torch.equal(src, before)


def test_single_float_form_equals_the_16_byte_form(golden):
    """An output that is not 16-byte aligned takes the single-float stores: the same bits (case (a))."""
    src = torch.from_numpy(golden['src_a']).to(DEV)
    n = 8 * 3 * 32 * 32
    buf = torch.zeros(n + 4, device=DEV)
    assert (buf.data_ptr() + 4) % 16 == 4
    assert _raw_call(src, buf.data_ptr() + 4, _table(golden['table_a']), 32) == 0
    assert _same(buf[1:n + 1].view(8, 3, 32, 32), golden['f32_a'])
    assert float(buf[0]) == 0. and not buf[n + 1:].any()


# ---------------------------------------------------------------------------------------------- 2. other paths
@pytest.mark.parametrize('shape', [(3, 50, 70, 27), (3, 50, 70, 36), (2, 256, 256, 224), (2, 23, 9, 32)],
                         ids=lambda s: '%dx%dx%d_to_%d' % s)
def test_kernel_equals_the_restatement_on_other_shapes(shape):
    """S = 27: single floats, a last band of 11 rows.  S = 36: 16-byte stores, a last band of 4 rows.  256 -> 224: the
    recipe's shape (14 bands, rows of 7 coefficients).  23 x 9 -> 32: up-scaling only.  Boxes: the whole source, one
    pixel, one row, one column, a corner, an inner box; both flip values."""
    from passl_amd.hip import ops
    B, Hs, Ws, S = shape
    src = CU.block_noise(sum(shape), B, Hs, Ws)
    boxes = [(0, 0, Hs, Ws, 1), (Hs - 1, Ws - 1, 1, 1, 0), (Hs // 2, 0, 1, Ws, 1), (0, Ws // 3, Hs, 1, 0),
             (Hs - 5, Ws - 4, 5, 4, 1), (3, 2, Hs - 7, Ws - 5, 0)]
    sd = torch.from_numpy(src).to(DEV)
    for first in range(0, len(boxes), B):
        table = np.zeros((B, 8), dtype=np.int32)
        for b in range(B):
            table[b, :5] = boxes[(first + b) % len(boxes)]
        _u8, want = CU.crop_resize_norm_ref(src, table, S)
        got = ops.crop_resize_norm(sd, _table(table), S, *NORM)
        assert _same(got, want), (shape, table.tolist())
    assert torch.equal(sd.cpu(), torch.from_numpy(src))


def test_other_constants_are_used():
    from passl_amd.hip import ops
    src = CU.block_noise(1, 2, 20, 24)
    table = np.array([[1, 2, 17, 20, 1, 0, 0, 0], [0, 0, 20, 24, 0, 0, 0, 0]], dtype=np.int32)
    mean, std, scale = (0.5, 0.25, 0.125), (0.5, 2.0, 0.3), 1.0 / 128.0
    _u8, want = CU.crop_resize_norm_ref(src, table, 16, scale, mean, std)
    got = ops.crop_resize_norm(torch.from_numpy(src).to(DEV), _table(table), 16, mean, std, scale)
    assert _same(got, want)


# ---------------------------------------------------------------------------------------------- 3. clamping, B = 0
def test_wild_table_stays_inside_the_tensors_and_is_clamped(golden):
    """Boxes that lie partly or wholly outside the source: the result equals the restatement on the clamped box
    (crop_resize_util.clamp_box), and one sample of guard floats on either side of ``out`` stays as it was."""
    src = torch.from_numpy(golden['src_a']).to(DEV)                      # 8 x 40 x 56
    big = 2 ** 31 - 1
    wild = np.array([[-3, -2, 20, 30, 1, 0, 0, 0], [30, 40, 100, 100, 0, 0, 0, 0], [5, 5, -4, 0, 1, 0, 0, 0],
                     [big, 0, big, big, 7, 0, 0, 0], [0, big, 1, big, 0, 0, 0, 0], [-big - 1, -big - 1, -big - 1, big, 0, 0, 0, 0],
                     [39, 55, 5, 5, -1, 0, 0, 0], [0, 0, 40, 56, 0, 9, 9, 9]], dtype=np.int32)
    n, guard = 8 * 3 * 32 * 32, 3 * 32 * 32
    buf = torch.full((n + 2 * guard,), -7.5, device=DEV)
    assert _raw_call(src, buf.data_ptr() + 4 * guard, _table(wild), 32) == 0
    torch.cuda.synchronize()
    assert (buf[:guard] == -7.5).all() and (buf[guard + n:] == -7.5).all()
    _u8, want = CU.crop_resize_norm_ref(golden['src_a'], wild, 32)
    assert _same(buf[guard:guard + n].view(8, 3, 32, 32), want)
    assert torch.equal(src.cpu(), torch.from_numpy(golden['src_a']))


def test_empty_batch_launches_nothing(golden):
    from passl_amd.hip import ops
    src = torch.from_numpy(golden['src_a']).to(DEV)
    buf = torch.full((64,), 3.25, device=DEV)
    assert _raw_call(src, buf.data_ptr(), _table(golden['table_a']), 32, B=0) == 0
    torch.cuda.synchronize()
    assert (buf == 3.25).all()
    out = ops.crop_resize_norm(src[:0], torch.zeros(0, 8, dtype=torch.int32, device=DEV), 32, *NORM)
    assert tuple(out.shape) == (0, 3, 32, 32) and out.dtype == torch.float32


# ---------------------------------------------------------------------------------------------- 4. wiring
def _golden_loader(golden, ring=0, extra=()):
    """build_dataloader on a SyntheticRawLabeled source of case (a)'s shape, its resident images replaced by the
    golden sources (a loader has no other way in)."""
    from passl_amd.datasets import build_dataloader
    ds = dict(name='SyntheticRawLabeled', num_samples=24, source_h=40, source_w=56, image_size=32, num_classes=16, seed=3,
              transforms=copy.deepcopy(CROP_TF) + list(extra))
    block = dict(dataset=ds, sampler=dict(batch_size=8), loader=dict(host_ring=ring) if ring else {})
    loader, _mix = build_dataloader(block, DEV)
    src = torch.from_numpy(golden['src_a'])
    if ring:
        assert all(h[0].dtype == torch.uint8 and tuple(h[0].shape) == (8, 40, 56, 3) for h in loader._host)
        for h in loader._host:
            h[0].copy_(src)
    else:
        assert len(loader._cache) == 1 and loader._cache[0][0].dtype == torch.uint8
        loader._cache[0][0].copy_(src)
    return loader


@pytest.mark.parametrize('ring', [0, 3])
def test_loader_path_equals_case_a(golden, ring):
    """SyntheticRawLabeled 40 x 56 -> 32 through build_dataloader, random.seed(5) and np.random.seed(5): the first two
    batches are the reference's first and second call; the resident uint8 batch stays as it was.  ring = 3: the
    HostRingLoader moves the uint8 images and applies the same pipeline to the slot."""
    loader = _golden_loader(golden, ring)
    random.seed(5)
    np.random.seed(5)
    it = iter(loader)
    for key in ('a', 'a_second'):
        x, y = next(it)
        assert x.dtype == torch.float32 and tuple(x.shape) == (8, 3, 32, 32) and y.dtype == torch.int64
        assert _same(x, golden['f32_' + key]), key
    assert loader.batch_transform.step == 2
    if not ring:
        assert torch.equal(loader._cache[0][0].cpu(), torch.from_numpy(golden['src_a']))


def test_replayed_plan_steps_receive_fresh_tables(golden):
    """The crop runs in the loader, in front of the recorded step: a plan recorded on another batch is replayed on the
    loader's first two batches, and what the replayed launches read is the reference's first and second call."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    loader = _golden_loader(golden)

    def step(x, y):
        return dict(seen=ops.clone(x), labels=ops.clone(y))
    sp = StepPlan(step, warmup=0, strict=True)
    x0 = torch.zeros(8, 3, 32, 32, device=DEV)
    y0 = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert torch.equal(sp.run(x0, y0)['seen'], x0)                        # the recording call
    assert sp.failed is None and sp.captured and not sp.foreign
    random.seed(5)
    np.random.seed(5)
    it = iter(loader)
    seen = [sp.run(*next(it))['seen'] for _ in range(2)]
    torch.cuda.synchronize()
    assert sp.replays == 2
    assert _same(seen[0], golden['f32_a']) and _same(seen[1], golden['f32_a_second'])
    assert not torch.equal(_bits(seen[0]), _bits(seen[1]))
    del sp
    torch.cuda.empty_cache()


def test_finetune_step_on_the_pipeline_output(golden):
    """One fine-tuning step of a depth-2, width-64 MAE_ViT at 32 x 32 on the loader's batch: its loss has the bits of the
    loss on the golden fp32 batch fed directly; with RandomErasing in the list the eraser runs after the crop, once."""
    from oracle.mae import finetune_state
    from passl_amd.datasets.preprocess import DeviceCropPipeline, RandomErasing
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    arch = dict(name='MAE_ViT', img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=2, qkv_bias=True, mlp_ratio=4)
    model = build_model(dict(name='MAE_FINETUNE', architecture=arch,
                             head=dict(name='VisionTransformerClsHead', num_classes=16, in_channels=64)))
    keys_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(dict(finetune_state(keys_shapes)), strict=False)
    assert not missing and not unexpected
    model.train()
    loader = _golden_loader(golden)
    random.seed(5)
    np.random.seed(5)
    x, y = next(iter(loader))

    def loss_of(img):
        out = model(img, y, mode='train')
        out['loss'].backward()
        return out['loss'].detach().clone().reshape(1)
    got = loss_of(x)
    want = loss_of(torch.from_numpy(golden['f32_a']).to(DEV))
    print('loss on the pipeline output %.6f, on the golden batch %.6f' % (float(got), float(want)))
    assert np.isfinite(float(got)) and torch.equal(_bits(got), _bits(want))
    # crop -> erase: the chained loader yields the crop's batch, erased inside the eraser's boxes only
    chained = _golden_loader(golden, extra=[dict(name='RandomErasing', prob=1., mode='const', seed=1)])
    crop, eraser = chained.batch_transform.stages
    assert isinstance(crop, DeviceCropPipeline) and isinstance(eraser, RandomErasing)
    random.seed(5)
    np.random.seed(5)
    state = random.getstate()
    xe, _ = next(iter(chained))
    # the eraser drew from `random` after the crop's 16 randint draws of this batch: restate both
    random.setstate(state)
    np.random.seed(5)
    assert np.array_equal(crop.draw(8, 40, 56), golden['table_a'])
    boxes = eraser.draw(8, 32, 32)
    want = torch.from_numpy(golden['f32_a']).clone()
    for b, (top, left, h, w) in enumerate(boxes.tolist()):
        want[b, :, top:top + h, left:left + w] = 0.
    assert (boxes[:, 2] > 0).any() and torch.equal(_bits(xe.cpu()), _bits(want))
    assert (crop.step, eraser.step) == (1, 1)
