"""Mixup / CutMix and soft-target cross-entropy on the MI355X: the batch mix bit for bit (tolerance 0: its arithmetic
is fully specified), the mixed target, the soft-target cross-entropy against float64, parity of two fine-tuning steps
with the reference run under its own Mixup (tests/golden/mae_ft_mix_*.npz), CELoss, the unchanged paths, the Trainer on
the recipe YAML."""
import os

import numpy as np
import pytest
import torch

import mixup_util as MU

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NEW_OPS = ('batch_mix', 'mixup_target', 'soft_ce_fwd', 'soft_ce_bwd')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _params():
    return np.load(os.path.join(GOLDEN, 'mixup_params.npz'))


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# ---------------------------------------------------------------------------------------------- 1. batch_mix
def _boxes(H, W):
    return [(0, H // 2, 0, W // 3), (H // 2, H, W // 3, W), (0, H, 0, 1), (0, 1, 0, W), (H - 1, H, W - 1, W),
            (H // 3, H // 3 + 1, W // 2, W // 2 + 1), (2, 2, 1, min(5, W)), (0, 0, 0, 0), (0, H, 0, W), (1, H - 1, 1, W - 2)]


@pytest.mark.parametrize('shape', [(8, 3, 64, 64), (6, 3, 37, 53), (5, 3, 16, 20), (7, 1, 5, 3), (128, 3, 224, 224)])
def test_batch_mix_bit_for_bit(shape):
    """Mode 0 against fl(fl(x lam) + fl(x' (1 - lam))) evaluated on the CPU, mode 1 against the slice assignment; the
    input is bit-unchanged afterwards.  (6, 3, 37, 53) and (7, 1, 5, 3): samples that do not start on 16-byte
    boundaries, the scalar form; odd B: the middle sample is its own partner."""
    from passl_amd.hip import ops
    B, C, H, W = shape
    big = B * C * H * W > 1 << 22
    gen = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=gen)
    xd = x.to(DEV)
    for lam in ([0.531506] if big else [0.531506, 0.0000531, 0.9774, 0.5, 1.0 / 3.0]):
        got = ops.batch_mix(xd, lam)
        assert got.data_ptr() != xd.data_ptr()
        assert torch.equal(_bits(got.cpu()), _bits(MU.batch_mix_ref(x, lam))), lam
    boxes = _boxes(H, W)
    for box in (boxes[:2] + boxes[4:5] if big else boxes):
        got = ops.batch_mix(xd, 0.25, box)
        assert torch.equal(_bits(got.cpu()), _bits(MU.batch_mix_ref(x, box=box))), box
    assert torch.equal(_bits(xd.cpu()), _bits(x))


def test_batch_mix_reproduces_the_reference_batches():
    """The strided slice of the result equals what the reference's Mixup produced (x_mixed[:, :, ::8, ::8] of
    tests/golden/mixup_params.npz) bit for bit, for all 12 seeds with the fixture's parameters."""
    from passl_amd.hip import ops
    z = _params()
    gen = torch.Generator().manual_seed(909)
    x = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
    for s in MU.PARAM_SEEDS:
        box = tuple(int(v) for v in z['box'][s]) if z['use_cutmix'][s] else None
        got = ops.batch_mix(x, float(z['lam'][s]), box)
        assert np.array_equal(got[:, :, ::8, ::8].cpu().numpy().view(np.int32), z['x_mixed_sub'][s].view(np.int32)), s


def test_batch_mix_refuses_bad_arguments():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib = L.load()
    x = torch.randn(4, 3, 8, 8, device=DEV)
    out = torch.empty_like(x)
    p, q, st = x.data_ptr(), out.data_ptr(), L.stream()

    def call(x_=p, out_=q, B=4, C=3, H=8, W=8, box=(0, 0, 0, 0), mode=0):
        return lib.passl_hip_batch_mix(x_, out_, B, C, H, W, 0.5, 0.5, box[0], box[1], box[2], box[3], mode, st)
    assert call() == 0
    assert call(out_=p) == -1                                 # in place
    assert call(x_=None) == -1 and call(out_=None) == -1
    assert call(B=0) == -1 and call(C=-1) == -1 and call(H=0) == -1 and call(W=0) == -1
    assert call(mode=2) == -1 and call(mode=-1) == -1
    for box in ((0, 9, 0, 4), (-1, 4, 0, 4), (0, 4, 0, 9), (0, 4, -1, 4), (5, 4, 0, 4), (0, 4, 5, 4)):
        assert call(box=box, mode=1) == -1, box
    with pytest.raises(L.PasslHipError):
        ops.batch_mix(torch.zeros(2, 3, 8, 8), 0.5)           # a host tensor
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. mixup_target
TARGET_BOUND = 4 * 2.0 ** -24          # three fp32 roundings of values <= 1 and the cast


def test_mixup_target_vs_reference_and_float64():
    from passl_amd.hip import ops
    z = _params()
    y = torch.from_numpy(z['labels']).to(DEV)
    for s in MU.PARAM_SEEDS:
        t = ops.mixup_target(y, 16, float(z['lam'][s]), 0.1)
        assert t.dtype == torch.float32 and t.shape == (8, 16)
        err = float(np.abs(t.cpu().numpy().astype(np.float64) - z['target'][s]).max())
        assert err <= TARGET_BOUND, (s, err)
    gen = torch.Generator().manual_seed(3)
    for N, C in [(128, 1000), (6, 1001), (2, 3), (10, 1)]:
        lab = torch.randint(0, C, (N,), generator=gen)
        for lam, eps in [(0.3, 0.1), (1.0, 0.1), (0.0, 0.0), (0.77, 0.5)]:
            t = ops.mixup_target(lab.to(DEV), C, lam, eps).cpu().numpy().astype(np.float64)
            err = float(np.abs(t - MU.mixup_target_ref(lab.numpy(), C, lam, eps)).max())
            assert err <= TARGET_BOUND, (N, C, lam, eps, err)
        onehot = ops.mixup_target(lab.to(DEV), C, 1.0, 0.0).cpu()
        assert torch.equal(onehot, torch.nn.functional.one_hot(lab, C).float())
    bad = torch.tensor([1, 2, 16, 3, 4, 5], device=DEV)
    t = ops.mixup_target(bad, 16, 0.6, 0.1).cpu()
    rows = torch.isnan(t).all(dim=1)
    assert rows.tolist() == [False, False, True, True, False, False]      # row 2 and its partner 6 - 1 - 2
    assert not torch.isnan(t[~rows]).any()


# ---------------------------------------------------------------------------------------------- 3. soft_ce
def _soft_case(N, C, kind, gen):
    s = torch.randn(N, C, generator=gen) * 3
    if kind == 'mixup':
        lab = torch.randint(0, C, (N,), generator=gen)
        t = torch.from_numpy(MU.mixup_target_ref(lab.numpy(), C, 0.531506, 0.1)).float()
    else:
        t = torch.rand(N, C, generator=gen) * 2
    return s, t


@pytest.mark.parametrize('kind', ['mixup', 'random'])
@pytest.mark.parametrize('N,C', [(8, 16), (128, 1000), (256, 1000), (5, 1001)])
def test_soft_ce_vs_float64(N, C, kind):
    """The bounds tests/test_clas_gpu.py uses for softmax_ce_fwd / bwd.  (5, 1001): rows that are not 16-byte aligned."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(N * 31 + C)
    s, t = _soft_case(N, C, kind, gen)
    loss, a1, a5, grad = MU.soft_ce_ref(s, t)
    sd, td = s.to(DEV), t.to(DEV)
    out, lse, tsum = ops.soft_ce_fwd(sd, td)
    print(N, C, kind, 'loss', float(out[0]), loss, 'acc', float(out[1]), a1, float(out[2]), a5)
    assert abs(float(out[0]) - loss) < 2e-5 * max(1.0, loss)
    assert abs(float(out[1]) - a1) < 1e-3 and abs(float(out[2]) - a5) < 1e-3
    assert relmax(tsum, t.double().sum(dim=1)) < 1e-6
    ds = ops.soft_ce_bwd(sd, td, lse, tsum, torch.tensor([0.7], device=DEV))
    err = relmax(ds, grad * 0.7)
    print(N, C, kind, 'grad err / max', err)
    assert err < 1e-5
    # two runs: the same bits
    out2, lse2, tsum2 = ops.soft_ce_fwd(sd, td)
    ds2 = ops.soft_ce_bwd(sd, td, lse2, tsum2, torch.tensor([0.7], device=DEV))
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(lse), _bits(lse2))
    assert torch.equal(_bits(ds), _bits(ds2))


@pytest.mark.parametrize('N,C', [(8, 16), (128, 1000)])
def test_soft_ce_on_one_hot_is_softmax_ce(N, C):
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(N + C)
    s = (torch.randn(N, C, generator=gen) * 3).to(DEV)
    lab = torch.randint(0, C, (N,), generator=gen).to(DEV)
    hard, _lse = ops.softmax_ce_fwd(s, lab)
    soft, _lse2, _tsum = ops.soft_ce_fwd(s, ops.mixup_target(lab, C, 1.0, 0.0))
    assert abs(float(soft[0]) - float(hard[0])) < 2e-5 * max(1.0, float(hard[0]))
    assert float(soft[1]) == float(hard[1]) and float(soft[2]) == float(hard[2])


def test_soft_ce_accuracy_takes_the_lower_index_on_ties():
    from passl_amd.hip import ops
    s = torch.zeros(4, 16)
    s[:, 3] = 2.0
    s[:, 9] = 1.0
    t = torch.zeros(4, 16)
    t[0, 3] = t[0, 9] = 0.5            # tie: label 3, the top score -> a hit
    t[1, 9] = t[1, 12] = 0.5           # tie: label 9, rank 1 -> top-5 only
    t[2, 12] = 0.6                     # label 12: scores 0 tie with 11 lower indices besides the two above -> no hit
    t[2, 3] = 0.4
    t[3, 0] = t[3, 3] = 0.5            # tie: label 0, score 0, rank 2 -> top-5 only
    out, _lse, _tsum = ops.soft_ce_fwd(s.to(DEV), t.to(DEV))
    _loss, a1, a5, _g = MU.soft_ce_ref(s, t)
    assert (a1, a5) == (25.0, 75.0)
    assert float(out[1]) == 25.0 and float(out[2]) == 75.0


def test_soft_ce_autograd_node():
    from passl_amd.modeling.heads.clas_head import _SoftCEFn
    gen = torch.Generator().manual_seed(11)
    s, t = _soft_case(16, 40, 'mixup', gen)
    _loss, _a1, _a5, grad = MU.soft_ce_ref(s, t)
    sd = s.to(DEV).requires_grad_(True)
    loss, acc1, acc5 = _SoftCEFn.apply(sd, t.to(DEV))
    assert not acc1.requires_grad and not acc5.requires_grad
    (loss * 3.0).sum().backward()
    assert relmax(sd.grad, grad * 3.0) < 1e-5


# ---------------------------------------------------------------------------------------------- 4. CELoss
def _spy_on_ops(monkeypatch):
    """-> calls: the name of every public function of passl_amd.hip.ops, in call order."""
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


def test_celoss_on_the_device(monkeypatch):
    """epsilon = 0.1 on integer labels = the reference's LabelSmoothingCrossEntropy(0.1); a soft label without epsilon =
    its SoftTargetCrossEntropy (values recorded in mixup_params.npz); integer labels without epsilon launch what they
    launched before."""
    from passl_amd.loss.celoss import CELoss
    z = _params()
    scores = torch.from_numpy(z['scores']).to(DEV)
    y = torch.from_numpy(z['labels']).to(DEV)
    want = float(z['ce_label_smoothing'])
    got = float(CELoss(epsilon=0.1)(scores, y)['CELoss'])
    print('CELoss(0.1)', got, want)
    assert abs(got - want) < 2e-5 * max(1.0, want)
    assert abs(float(CELoss(epsilon=0.1)(scores, y.view(-1, 1))['CELoss']) - want) < 2e-5 * max(1.0, want)
    soft = torch.from_numpy(z['target'][11]).to(DEV)
    want = float(z['ce_soft_target'])
    got = float(CELoss()({'logits': scores}, soft)['CELoss'])
    print('CELoss() on a soft label', got, want)
    assert abs(got - want) < 2e-5 * max(1.0, want)
    # a soft label with epsilon: (1 - eps) t + eps / C
    want = MU.soft_ce_ref(scores, soft.double() * 0.8 + 0.2 / 16)[0]
    assert abs(float(CELoss(epsilon=0.2)(scores, soft)['CELoss']) - want) < 2e-5 * max(1.0, want)
    # gradient through the smoothed loss
    sd = scores.clone().requires_grad_(True)
    CELoss(epsilon=0.1)(sd, y)['CELoss'].backward()
    grad = MU.soft_ce_ref(scores, torch.from_numpy(MU.mixup_target_ref(z['labels'], 16, 1., 0.1)))[3]
    assert relmax(sd.grad, grad) < 1e-5
    calls = _spy_on_ops(monkeypatch)
    sd = scores.clone().requires_grad_(True)
    CELoss()(sd, y)['CELoss'].backward()
    assert calls == ['softmax_ce_fwd', 'softmax_ce_bwd']


# ---------------------------------------------------------------------------------------------- 5. fine-tuning parity
FT_ARCH = dict(name='MAE_ViT', patch_size=16, embed_dim=768, depth=12, num_heads=12, qkv_bias=True, mlp_ratio=4)
SMALL = dict(FT_ARCH, embed_dim=128, depth=4, num_heads=4, img_size=64)
FT_WATCH = ['backbone.cls_token', 'backbone.pos_embed', 'backbone.patch_embed.proj.weight',
            'backbone.blocks.0.attn.qkv.weight', 'backbone.blocks.1.mlp.fc2.bias', 'backbone.blocks.1.norm2.weight',
            'backbone.fc_norm.weight', 'backbone.fc_norm.bias', 'head.fc_cls.weight', 'head.fc_cls.bias']
FT_SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05)


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
    return model, keys_shapes


def _run_finetune_golden(name, arch, dtype, tol, discriminate):
    """The harness of tests/test_droppath_gpu.py::_run_finetune_golden with ``mixup_fn=Mixup(..., rng=RandomState(seed))``
    reseeded per step as the fixture says; same bounds (step 1 at the x 20 that harness allows).  discriminate (fp32):
    step 0 must also be FAR from the same step without mixing and with hard labels (s0_*_plain) — features by more
    than 3 x their bound, loss by more than 2 x its bound."""
    from passl_amd.datasets.preprocess import Mixup
    from passl_amd.solver.optimizer import AdamW
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    N, hw, steps, classes = [int(v) for v in z['meta']]
    torch.manual_seed(0)
    model, keys_shapes = _build_finetune(arch, classes, dtype)
    assert ['%s:%s' % (k, 'x'.join(map(str, s))) for k, s in keys_shapes] == [str(k) for k in z['keys']]
    model.train()
    opt = AdamW(FT_SOLVER['lr'], beta1=FT_SOLVER['beta1'], beta2=FT_SOLVER['beta2'],
                weight_decay=FT_SOLVER['weight_decay'], parameters=list(model.parameters()))
    seen = {}
    head_fwd = model.head.forward

    def spy(x):
        seen['feat'] = x.detach()
        seen['score'] = head_fwd(x)
        return seen['score']
    model.head.forward = spy
    fn = Mixup(num_classes=classes, **MU.RECIPE)

    def mix(x, y):
        seen['x_mixed'], seen['target'] = fn(x, y)
        return seen['x_mixed'], seen['target']
    gen = torch.Generator().manual_seed(909)
    report, bad = [], []

    def check(what, got, ref, bound, rel=False, at_least=False):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        scale = max(float(np.max(np.abs(ref))), 1e-12) if rel else 1.0
        err = float(np.max(np.abs(got - ref))) / scale
        line = '%-52s %s %.3e  bound %.3e' % (what, 'dist' if at_least else 'err', err, bound)
        report.append(line)
        if not (err > bound if at_least else err <= bound):
            bad.append(line)

    st = hw // 8
    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        xd = x.to(DEV)
        fn.rng = np.random.RandomState(int(z['seeds'][s]))
        out = model(xd, y.to(DEV), mode='train', mixup_fn=mix)
        opt.clear_grad()
        out['loss'].backward()
        pre = 's%d_' % s
        k = 1.0 if s == 0 else 20.0
        # the mix itself: the reference's batch bit for bit, its target to the kernel's bound, the input untouched
        assert torch.equal(_bits(xd.cpu()), _bits(x))
        assert np.array_equal(seen['x_mixed'][:, :, ::st, ::st].cpu().numpy().view(np.int32),
                              z[pre + 'x_mixed_sub'].view(np.int32)), s
        t = seen['target'].cpu().numpy().astype(np.float64)
        assert np.array_equal(t.argmax(axis=1), z[pre + 'target_argmax'])
        check(pre + 'target max', t.max(axis=1), z[pre + 'target_max'], TARGET_BOUND)
        check(pre + 'loss', float(out['loss'].detach()), z[pre + 'loss'], tol['loss'] * k, rel=True)
        if s == 0:
            feat = seen['feat'].float().cpu()[:, :8].numpy()
            check(pre + 'acc1', float(out['acc1']), z[pre + 'acc1'], 1e-6)
            check(pre + 'acc5', float(out['acc5']), z[pre + 'acc5'], 1e-6)
            check(pre + 'feat[:, :8]', feat, z[pre + 'feat_head'], tol['feat'], rel=True)
            check(pre + 'score[:, :8]', seen['score'].detach().float().cpu()[:, :8].numpy(), z[pre + 'score_head'],
                  tol['feat'], rel=True)
            ps = dict(model.named_parameters())
            for n in FT_WATCH:
                check(pre + 'gradnorm/' + n, ps[n].grad.double().norm().item(), z[pre + 'gradnorm/' + n], tol['grad'], rel=True)
            if discriminate:
                check(pre + 'feat[:, :8] vs the plain step', feat, z['s0_feat_head_plain'], 3 * tol['feat'], rel=True,
                      at_least=True)
                check(pre + 'loss vs the plain step', float(out['loss'].detach()), z['s0_loss_plain'], 2 * tol['loss'],
                      rel=True, at_least=True)
        opt.step()
        if s == 0:
            ps = dict(model.named_parameters())
            for n in FT_WATCH:
                check(pre + 'pnorm/' + n, ps[n].detach().double().norm().item(), z[pre + 'pnorm/' + n], tol['param'], rel=True)
    print('\n'.join(report))                                  # every figure, before the assertion
    assert not bad, 'parity violations:\n' + '\n'.join(bad)


def test_finetune_mix_golden_small_fp32():
    _run_finetune_golden('mae_ft_mix_small', dict(SMALL), torch.float32, MU.FT_TOL_F32, True)


def test_finetune_mix_golden_vit_b_fp32():
    _run_finetune_golden('mae_ft_mix_vit_b', dict(FT_ARCH), torch.float32, MU.FT_TOL_F32, True)


def test_finetune_mix_golden_vit_b_bf16():
    """The bf16 bounds are wider than what mixing changes in the loss: this run discriminates on nothing but the mixed
    batch and target themselves; it shows that the bf16 path runs the same computation within the project's bf16
    bounds.  The parity claim is the fp32 run above."""
    _run_finetune_golden('mae_ft_mix_vit_b', dict(FT_ARCH), torch.bfloat16, MU.FT_TOL_BF16, False)


# ---------------------------------------------------------------------------------------------- 6. unchanged paths
def test_no_mixup_fn_and_test_mode_launch_what_they_launched(monkeypatch):
    from passl_amd.datasets.preprocess import Mixup
    torch.manual_seed(1)
    model, _ = _build_finetune(dict(SMALL), 16, torch.float32)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
    y = torch.randint(0, 16, (8,), generator=gen).to(DEV)
    fn = Mixup(num_classes=16, rng=np.random.RandomState(0), **MU.RECIPE)
    calls = _spy_on_ops(monkeypatch)

    def run(**kw):
        del calls[:]
        out = model(x, y, **kw)
        if isinstance(out, dict):
            out['loss'].backward()
        return list(calls)
    model.train()
    plain = run(mode='train')
    assert not set(plain) & set(NEW_OPS) and plain.count('softmax_ce_fwd') == 1 and plain.count('softmax_ce_bwd') == 1
    assert run(mode='train', mixup_fn=None) == plain
    # with a mixup_fn: two launches in front, the soft-target loss in place of the integer one, nothing else moves
    mixed = run(mode='train', mixup_fn=fn)
    assert mixed[:2] == ['batch_mix', 'mixup_target']
    swap = {'soft_ce_fwd': 'softmax_ce_fwd', 'soft_ce_bwd': 'softmax_ce_bwd'}
    assert [swap.get(c, c) for c in mixed[2:]] == plain
    # mode='test' never mixes; neither does a model in eval mode
    model.eval()
    state = fn.rng.get_state()[1].copy()
    tested = run(mode='test', mixup_fn=fn)
    assert not set(tested) & set(NEW_OPS)
    del calls[:]
    model(x, mode='test')
    assert list(calls) == tested
    assert not set(run(mode='train', mixup_fn=fn)) & set(NEW_OPS)
    assert np.array_equal(fn.rng.get_state()[1], state)       # and nothing was drawn


def test_unmixed_step_returns_the_batch_itself():
    from passl_amd.datasets.preprocess import Mixup
    x = torch.randn(4, 3, 8, 8, device=DEV)
    y = torch.tensor([1, 0, 3, 2], device=DEV)
    xm, t = Mixup(0.8, 1.0, prob=0., label_smoothing=0.1, num_classes=4, rng=np.random.RandomState(0))(x, y)
    assert xm is x
    want = MU.mixup_target_ref(y.cpu().numpy(), 4, 1., 0.1)
    assert float(np.abs(t.cpu().numpy().astype(np.float64) - want).max()) <= TARGET_BOUND


# ---------------------------------------------------------------------------------------------- 7. end to end
def _train_recipe(tmp_path, seed):
    from passl_amd.engine.trainer import Trainer
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml'),
                     ['dataloader.train.sampler.batch_size=8', 'dataloader.train.dataset.num_samples=32', 'epochs=1',
                      'output_dir=%s' % tmp_path, 'log_config.interval=2', 'seed=%d' % seed])
    cfg.timestamp = ''
    np.random.seed(seed)
    torch.manual_seed(seed)
    tr = Trainer(cfg)
    assert type(tr.model).__name__ == 'MAE_FINETUNE' and tr.iters_per_epoch == 4
    assert type(tr.mixup_fn).__name__ == 'Mixup' and tr.mixup_fn.num_classes == 1000
    losses = []
    step = tr.train_step

    def train_step(data):
        out = step(data)
        losses.append(float(out['loss'].detach()))
        return out
    tr.train_step = train_step
    w0 = tr.model.head.fc_cls.weight.detach().clone()
    tr.train()
    assert tr.current_iter == 4 and len(losses) == 4
    assert float((tr.model.head.fc_cls.weight.detach() - w0).abs().max()) > 0
    assert tr.model.backbone.drop_path_step() == 4
    del tr
    torch.cuda.empty_cache()
    return losses


def test_trainer_runs_recipe_config_end_to_end(tmp_path):
    """configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml through the v110 Trainer: finite, changing loss; the same
    seeds log the same losses (mixing parameters from numpy's global stream, stochastic depth from torch's)."""
    a = _train_recipe(tmp_path / 'a', 5)
    b = _train_recipe(tmp_path / 'b', 5)
    print('losses', a)
    assert all(np.isfinite(v) and 0 < v < 20 for v in a) and len(set(a)) == 4
    assert a == b
