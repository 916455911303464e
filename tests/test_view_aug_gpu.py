"""Colour jitter, grayscale, blur and solarise of resident two-view batches on the MI355X: the kernels of csrc/view_aug.hip
and passl_hip_crop_resize_u8 against what the reference's classes produced through Pillow (tests/golden/view_aug_small.npz,
tests/golden/crop_resize_small.npz) and against the numpy restatement (tests/view_aug_util.py) where the kernels take
another path; the loaders, a step plan and a MoCo-v3 step.  Tolerance 0 everywhere."""
import copy
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import crop_resize_util as CU
import view_aug_util as VU

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NORM = (CU.MEAN, CU.STD, float(np.float32(CU.SCALE)))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'view_aug_small.npz'))


def _same(got, want):
    return np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))


def _tables(samples):
    from passl_amd.datasets.preprocess import DeviceViewPipeline
    crop, table = DeviceViewPipeline.encode(samples)
    DeviceViewPipeline.validate(table)
    return torch.from_numpy(crop).to(DEV), torch.from_numpy(table).to(DEV), table


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(img, samples, normalize=None):
    """The launches of run_view behind the crop, on uint8 images [B, H, W, 3]: -> (result, sums)."""
    from passl_amd.hip import ops
    _c, t, host = _tables(samples)
    x = _dev(img)
    sums = ops.view_gray_sum(x, t) if (host[:, 6] >= 0).any() else None
    r_max = int(host[:, 2].max())
    if r_max < 0:
        return ops.view_pointwise(x, t, sums, 0, normalize), sums
    y = ops.gaussian_blur_u8(ops.view_pointwise(x, t, sums, 1, None), t, r_max)
    return ops.view_pointwise(y, t, None, 2, normalize), sums


def _ref(img, samples):
    return np.stack([VU.apply_ops(img[b], s[1]) for b, s in enumerate(samples)])


BOX = (0, 0, 1, 1)


# ---------------------------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize('view', [1, 2])
def test_kernels_equal_the_reference_stage_by_stage(golden, view):
    """On the golden sources and OBSERVED decisions: the crop, the image after the jitter, after the grayscale, after
    the blur / solarisation and the final fp32 view equal what the reference's classes produced, bit for bit."""
    from passl_amd.hip import ops
    st, samples = golden['stages_%d' % view], VU.golden_samples(golden, view)
    crop_t, table, host = _tables(samples)
    src = _dev(golden['src'])
    u8 = ops.crop_resize_u8(src, crop_t, 32)
    assert torch.equal(u8.cpu(), torch.from_numpy(st[0])) and torch.equal(src.cpu(), torch.from_numpy(golden['src']))
    for upto, stage in ((VU.OP_HUE, 1), (VU.OP_GRAY, 2)):                # the list cut behind the jitter / the grayscale
        cut = [(s[0], [o for o in s[1] if o[0] <= upto], False) for s in samples]
        got, _ = _run(st[0], cut)
        assert torch.equal(got.cpu(), torch.from_numpy(st[stage])), stage
    noflip = [(s[0], s[1], False) for s in samples]
    got, _ = _run(st[0], noflip)
    assert torch.equal(got.cpu(), torch.from_numpy(st[3]))
    got, sums = _run(st[0], samples, NORM)
    assert _same(got, golden['f32_%d' % view])
    if view == 1:
        assert (host[:, 2] == 0).any() and (host[:, 2] == 1).any() and (host[:, 2] < 0).any()
    want = [VU.contrast_mean_sum(st[0][b], s[1]) for b, s in enumerate(samples)]
    assert any(want) and sums.cpu().tolist() == want


@pytest.mark.parametrize('view', [1, 2])
def test_pipeline_equals_the_reference_views(golden, view):
    """DeviceViewPipeline on the observed samples (crop, gray sum, pointwise, blur, pointwise) = the reference's view."""
    from passl_amd.datasets.preprocess import build_view_pipeline
    pipe = build_view_pipeline(_view_cfg(view))
    got = pipe(_dev(golden['src']), VU.golden_samples(golden, view))
    assert _same(got, golden['f32_%d' % view]) and pipe.step == 1


@pytest.mark.parametrize('key', ['a', 'a_second', 'b', 'c'])
def test_crop_resize_u8_equals_the_crop_golden(key):
    from passl_amd.hip import ops
    z = np.load(os.path.join(GOLDEN, 'crop_resize_small.npz'))
    src = _dev(z['src_' + key[0]])
    got = ops.crop_resize_u8(src, _dev(z['table_' + key]), 32)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(z['u8_' + key]))


# ---------------------------------------------------------------------------------------------- 2. the restatement
@pytest.fixture(scope='module')
def colours():
    return VU.all_colours()


def test_hue_over_all_colours(colours):
    """All 2^24 colours as one [1, 4096, 4096, 3] image through the uint8 output, hue shift 37."""
    ops_ = [(VU.OP_HUE, 37)]
    got, _ = _run(colours[None], [(BOX, ops_, False)])
    want = VU.hue(colours, 37)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))


def test_gray_hue_saturation_over_all_colours(colours):
    """Grayscale, then hue, then saturation 1.3 (a factor outside [0, 1]) over all colours; the restatement runs on the
    distinct colours behind the grayscale."""
    ops_ = [(VU.OP_GRAY, 0), (VU.OP_HUE, 200), (VU.OP_SATURATION, 1.3)]
    got, _ = _run(colours[None], [(BOX, ops_, False)])
    g = VU.gray(colours)
    lut = VU.apply_ops(np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2), ops_[1:])[:, 0]
    assert torch.equal(got[0].cpu(), torch.from_numpy(lut[g]))


TILE = 32
BLUR_SHAPES = [(1, 1), (7, 2), (3, 5), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (TILE - 1, TILE + 1),
               (TILE + 1, TILE), (224, 224)]


@pytest.mark.parametrize('hw', BLUR_SHAPES, ids=lambda s: '%dx%d' % s)
def test_blur_equals_the_restatement(hw):
    """r = 0 and r = 1 mixed within one batch, non-blurred samples bit-equal to their input; one sample at 224 x 224."""
    from passl_amd.hip import ops
    H, W = hw
    radii = [1.9] if H == 224 else [0.3, 1.9, None, 1.42, 1.41, None]
    img = np.random.RandomState(H * 1000 + W).randint(0, 256, (len(radii), H, W, 3)).astype(np.uint8)
    samples = [(BOX, [(VU.OP_BLUR, r)] if r is not None else [], False) for r in radii]
    _c, t, host = _tables(samples)
    assert sorted(set(host[:, 2].tolist())) == ([1] if H == 224 else [-1, 0, 1])
    x = _dev(img)
    got = ops.gaussian_blur_u8(x, t, 1)
    assert torch.equal(got.cpu(), torch.from_numpy(_ref(img, samples))) and torch.equal(x.cpu(), torch.from_numpy(img))
    for b, r in enumerate(radii):
        if r is None:
            assert torch.equal(got[b].cpu(), torch.from_numpy(img[b]))
    with pytest.raises(Exception, match='envelope'):
        ops.gaussian_blur_u8(x, t, 2)


@pytest.mark.parametrize('S', [33, 224])
def test_contrast_equals_the_restatement(S):
    """The contrast entry first, in the middle and last, beside a sample without one: the mean is taken over the image as
    it stands when contrast is reached."""
    img = CU.block_noise(S, 4, S, S)
    lists = [[(VU.OP_CONTRAST, 1.4), (VU.OP_BRIGHTNESS, 0.7)],
             [(VU.OP_SATURATION, 1.2), (VU.OP_CONTRAST, 0.6), (VU.OP_HUE, 250)],
             [(VU.OP_BRIGHTNESS, 1.3), (VU.OP_GRAY, 0), (VU.OP_CONTRAST, 1.39)],
             [(VU.OP_BRIGHTNESS, 0.9)]]
    samples = [(BOX, o, False) for o in lists]
    got, sums = _run(img, samples)
    assert sums.cpu().tolist() == [VU.contrast_mean_sum(img[b], o) for b, o in enumerate(lists)]
    assert torch.equal(got.cpu(), torch.from_numpy(_ref(img, samples)))


@pytest.mark.parametrize('S,offset', [(33, 0), (33, 1), (32, 1), (32, 0)])
def test_fp32_output_forms(S, offset):
    """Odd S and an ``out`` that is not 16-byte aligned take the single-float stores; both forms equal the restatement,
    flips included, and the floats around ``out`` stay as they were."""
    from passl_amd.hip import ops
    img = CU.block_noise(40 + S, 3, S, S)
    samples = [(BOX, [(VU.OP_SOLARIZE, 0)], True), (BOX, [], False), (BOX, [(VU.OP_BRIGHTNESS, 1.2)], True)]
    _c, t, _h = _tables(samples)
    n = 3 * 3 * S * S
    buf = torch.full((n + 64,), 3.25, device=DEV)
    out = buf[8 + offset:8 + offset + n].view(3, 3, S, S)
    assert (out.data_ptr() % 16 == 0) == (offset == 0)
    consts = C.cast((C.c_float * 7)(*CU.MEAN, *CU.STD, CU.SCALE), C.c_void_p)
    ops.view_pointwise_into(_dev(img), t, None, 0, out, consts)
    want = np.stack([VU.view_ref(img[b], s[1], s[2], CU.SCALE, CU.MEAN, CU.STD)[1] for b, s in enumerate(samples)])
    assert _same(out, want)
    assert (buf[:8 + offset] == 3.25).all() and (buf[8 + offset + n:] == 3.25).all()


def test_wild_table_stays_inside_the_tensors():
    """Counts, indices, radii and codes far outside their ranges: the kernels clamp them; guard bytes on either side of
    every output stay as they were."""
    from passl_amd.hip import lib as L
    S, B = 33, 2
    img = _dev(CU.block_noise(9, B, S, S))
    wild = np.full((B, 24), 0x7fffffff, dtype=np.int32)
    wild[1] = -0x7fffffff
    wild[1, 0], wild[1, 2], wild[1, 6] = 100, 77, 3
    t = _dev(wild)
    n = B * S * S * 3
    guard8 = torch.full((n + 128,), 7, dtype=torch.uint8, device=DEV)
    guardf = torch.full((n + 128,), 3.25, device=DEV)
    sums = torch.full((B + 2,), -5, dtype=torch.int64, device=DEV)
    lib = L.load()
    consts = C.cast((C.c_float * 7)(*CU.MEAN, *CU.STD, CU.SCALE), C.c_void_p)
    assert lib.passl_hip_view_gray_sum(img.data_ptr(), t.data_ptr(), sums[1:].data_ptr(), B, S, S, L.stream()) == 0
    assert lib.passl_hip_view_pointwise(img.data_ptr(), t.data_ptr(), sums[1:].data_ptr(), guard8[64:].data_ptr(), None, B, S,
                                        S, 0, None, L.stream()) == 0
    assert lib.passl_hip_view_pointwise(img.data_ptr(), t.data_ptr(), None, None, guardf[64:].data_ptr(), B, S, S, 2, consts,
                                        L.stream()) == 0
    torch.cuda.synchronize()
    assert (guard8[:64] == 7).all() and (guard8[64 + n:] == 7).all()
    assert (guardf[:64] == 3.25).all() and (guardf[64 + n:] == 3.25).all() and sums[0] == -5 and sums[-1] == -5
    guard8.fill_(7)
    assert lib.passl_hip_gaussian_blur_u8(img.data_ptr(), guard8[64:].data_ptr(), t.data_ptr(), B, S, S, 1, L.stream()) == 0
    torch.cuda.synchronize()
    assert (guard8[:64] == 7).all() and (guard8[64 + n:] == 7).all()


# ---------------------------------------------------------------------------------------------- 3. wiring
def _view_cfg(view, S=32):
    crop = {'MAERandCropImage': dict(size=S, scale=[0.2, 1.0], interpolation='bicubic', backend='pil')}
    jit = dict(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1)
    tail = [{'RandomHorizontalFlip': None},
            {'NormalizeImage': dict(scale='1.0/255.0', mean=list(CU.MEAN), std=list(CU.STD), order='hwc')},
            {'ToCHWImage': None}]
    if view == 1:
        mid = [{'ColorJitter': dict(p=0.7, **jit)}, {'RandomGrayscale': dict(p=0.3)},
               {'SimCLRGaussianBlur': dict(sigma=[.1, 2.], p=0.6)}]
    else:
        mid = [{'RandomApply': dict(transforms=[{'ColorJitter': dict(p=1.0, **jit)}], p=0.7)},
               {'RandomGrayscale': dict(p=0.3)}, {'BYOLSolarize': dict(p=0.5)}]
    return [crop] + mid + tail


def _golden_loader(golden, ring=0):
    from passl_amd.datasets import build_dataloader
    tf = [{'TwoViewsTransform': dict(base_transform1=_view_cfg(1), base_transform2=_view_cfg(2))}]
    ds = dict(name='SyntheticRawTwoView', num_samples=24, source_h=40, source_w=56, image_size=32, seed=3, transform=tf)
    loader, _mix = build_dataloader(dict(dataset=ds, sampler=dict(batch_size=8),
                                         loader=dict(host_ring=ring) if ring else {}), DEV)
    src = torch.from_numpy(golden['src'])
    for slot in (loader._host if ring else loader._cache):
        assert len(slot) == 1 and slot[0].dtype == torch.uint8 and tuple(slot[0].shape) == (8, 40, 56, 3)
        slot[0].copy_(src)
    return loader


def _final_views(golden, suffix):
    """The two fp32 views of a call from the restatement applied to the observed decisions."""
    out = []
    for v in (1, 2):
        views = []
        for b, (box, ops_, flip) in enumerate(VU.golden_samples(golden, v, suffix)):
            top, left, h, w = box
            u8 = CU.resize_u8(golden['src'][b, top:top + h, left:left + w], 32)
            views.append(VU.view_ref(u8, ops_, flip, CU.SCALE, CU.MEAN, CU.STD)[1])
        out.append(np.stack(views))
    return out


@pytest.mark.parametrize('ring', [0, 3])
def test_loader_yields_the_two_views_of_the_reference(golden, ring):
    """SyntheticRawTwoView through build_dataloader, random.seed(0) and np.random.seed(0): the first batch is the
    reference's first call (its fp32 views), the second batch its second call (the restatement on the observed
    decisions, whose final uint8 images are the golden's); both views come from the SAME resident images."""
    loader = _golden_loader(golden, ring)
    random.seed(0)
    np.random.seed(0)
    it = iter(loader)
    xq, xk = next(it)
    assert xq.dtype == xk.dtype == torch.float32 and tuple(xq.shape) == tuple(xk.shape) == (8, 3, 32, 32)
    assert _same(xq, golden['f32_1']) and _same(xk, golden['f32_2'])
    xq, xk = next(it)
    w1, w2 = _final_views(golden, '_second')
    assert _same(xq, w1) and _same(xk, w2)
    assert loader.batch_transform.step == 2
    if not ring:
        assert torch.equal(loader._cache[0][0].cpu(), torch.from_numpy(golden['src']))


def test_replayed_plan_steps_receive_fresh_views(golden):
    """The pipelines run in the loader, in front of the recorded step: a plan recorded on other tensors is replayed on
    the loader's first two batches, and what the replayed launches read are the reference's first and second call."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    loader = _golden_loader(golden)

    def step(xq, xk):
        return dict(q=ops.clone(xq), k=ops.clone(xk))
    sp = StepPlan(step, warmup=0, strict=True)
    x0 = torch.zeros(8, 3, 32, 32, device=DEV)
    sp.run(x0, x0.clone())
    assert sp.failed is None and sp.captured and not sp.foreign
    random.seed(0)
    np.random.seed(0)
    it = iter(loader)
    seen = [sp.run(*next(it)) for _ in range(2)]
    torch.cuda.synchronize()
    assert sp.replays == 2
    assert _same(seen[0]['q'], golden['f32_1']) and _same(seen[0]['k'], golden['f32_2'])
    w1, w2 = _final_views(golden, '_second')
    assert _same(seen[1]['q'], w1) and _same(seen[1]['k'], w2)
    del sp
    torch.cuda.empty_cache()


def test_mocov3_step_on_the_two_views_eager_and_under_a_step_plan():
    """MoCo-v3 (a depth-2 ViT at 64 x 64) on the two views of a SyntheticRawTwoView loader built from the recipe's
    block: three steps run eagerly and through a StepPlan wrapper give the same losses bit for bit, on views that differ
    from step to step.  (MoCo-v3's step holds ATen launches, so a strict plan hands the step back to eager launches:
    either way the loader's launches run live, in front of the step.)"""
    import yaml
    import mocov3_util as U
    from oracle import mocov3 as O
    from passl_amd.datasets import build_dataloader
    from passl_amd.hip.replay import StepPlan
    with open(os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_views_synthetic.yaml')) as f:
        block = copy.deepcopy(yaml.safe_load(f)['DataLoader']['Train'])
    S = O.SMALL['img_size']
    block['dataset'].update(num_samples=64, source_h=72, source_w=80, image_size=S)
    for v in ('base_transform1', 'base_transform2'):
        block['dataset']['transform'][0]['TwoViewsTransform'][v][0]['MAERandCropImage']['size'] = S
    block['sampler'] = dict(batch_size=8)
    results = {}
    for mode in ('eager', 'plan'):
        oracle = O.MoCoV3Oracle(O.SMALL, seed=0, max_steps=10, **U.SOLVER)
        model, opt = U.build_product(O.SMALL, torch.float32, max_steps=10)
        U.load_oracle_state(model, oracle)
        model.train()
        loader, _ = build_dataloader(copy.deepcopy(block), DEV)
        random.seed(4)
        np.random.seed(4)

        def full_step(xq, xk):
            return dict(loss=U.product_step(model, opt, xq, xk).detach().reshape(1))
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'))
        losses, firsts = [], []
        it = iter(loader)
        for _ in range(3):
            xq, xk = next(it)
            assert tuple(xq.shape) == (8, 3, S, S) and not torch.equal(xq, xk)
            firsts.append(xq[0, 0, 0, :4].clone())
            losses.append(sp.run(xq, xk)['loss'].clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.captured or sp.failed is not None
            print('step plan: captured %s, refused: %s' % (sp.captured, sp.failed))
        results[mode] = (torch.cat(losses).cpu(), torch.stack(firsts).cpu())
        del sp, model, opt, loader
        torch.cuda.empty_cache()
    (la, fa), (lb, fb) = results['eager'], results['plan']
    print('losses eager %s, under the plan %s' % (la.tolist(), lb.tolist()))
    assert torch.isfinite(la).all() and torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(fa, fb) and not torch.equal(fa[0], fa[1])
