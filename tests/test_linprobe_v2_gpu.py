"""The v2 linear-probe recipes (tasks/ssl/simsiam lp, tasks/ssl/mocov3 lp) on a real MI355X: the MomentumLARC kernel
against its rule, whole probe steps + the evaluation pass of the product loops against the golden vectors produced by
the reference's own models / loss / metric / optimizers / schedule / loops (tests/golden/make_golden_linprobe_v2.py),
the pre-training -> probe weight hand-over, and the v2 Engine driving the recipe from a yaml."""
import os
import pickle
from functools import partial
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import linprobe_v2_util as U                                  # noqa: E402
from oracle import linprobe_v2 as L                           # noqa: E402
from passl_amd.hip import config as hip_config                # noqa: E402
from passl_amd.hip import nn as hnn                           # noqa: E402

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = hnn.Linear(40, 24)
        self.b = hnn.Linear(24, 16)
        self.c = hnn.Linear(16, 8)


@pytest.mark.parametrize('clip, wd, tc, lr', [(False, 0.0, 0.001, 1.6), (True, 1e-3, 0.02, 0.05), (False, 1e-2, 0.02, 0.3)])
def test_larc_kernel_matches_the_rule(clip, wd, tc, lr):
    """passl_hip_larc_momentum_dev over an arena of six tensors (one with zero norm: raw gradient, no decay) vs the
    rule of passl/optimizer/momentum_larc.py restated in fp64, three steps with a changing rate.  (A norm per tensor:
    the element-wise float64 bounds are in test_flat_numerics_gpu.py.)"""
    from passl_amd.hip.nn import EncoderArena
    from passl_amd.solver.optimizer import MomentumLARC
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    torch.manual_seed(5)
    toy = _Toy().to(DEV)
    with torch.no_grad():
        for q in toy.parameters():
            q.copy_(torch.randn(q.shape) * 0.1)
        toy.b.bias.zero_()
    arena = EncoderArena(toy, trainable=True)
    rates = [lr, lr * 0.7, lr * 0.2]
    it = iter(rates)
    opt = MomentumLARC(learning_rate=lr, momentum=0.9, weight_decay=wd, trust_coefficient=tc, clip=clip,
                       parameters=list(toy.parameters()))
    opt.get_lr = lambda: next(it)
    names = [n for n, _ in toy.named_parameters()]
    ref = L.LinearProbeOracle.__new__(L.LinearProbeOracle)
    ref.optimizer, ref.mu, ref.wd, ref.tc, ref.clip, ref.eps = 'MomentumLARC', 0.9, wd, tc, clip, 1e-8
    ref.exp_avg, ref.step_count = {}, 0
    ref.lr_value = lambda s: rates[s]
    ref.st = {n: p.detach().double().cpu() for n, p in toy.named_parameters()}
    gen = torch.Generator().manual_seed(9)
    for s in range(3):
        grads = {n: torch.randn(ref.st[n].shape, generator=gen, dtype=torch.float64) * (0.05 if s else 1.0)
                 for n in names}
        opt.clear_grad()
        for n, p in toy.named_parameters():
            p.grad.copy_(grads[n].float())
        opt.step()
        ref.update(grads)
        torch.cuda.synchronize()
        for n, p in toy.named_parameters():
            assert rel_l2(p.detach(), ref.st[n]) < 5e-6, (s, n, rel_l2(p.detach(), ref.st[n]))
    assert float(ref.st['b.bias'].abs().max()) > 0          # the zero-norm tensor moved by its raw gradient


def _build(kind, classes, dtype):
    from passl_amd.models import simsiam_resnet50_linearprobe
    from passl_amd.models.mocov3 import MoCoV3LinearProbe
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(0)
    if kind == 'simsiam':
        return simsiam_resnet50_linearprobe(class_num=classes)
    c = U.VIT_SMALL
    return MoCoV3LinearProbe(img_size=c['img_size'], patch_size=c['patch_size'], embed_dim=c['embed_dim'],
                             depth=c['depth'], num_heads=c['num_heads'], mlp_ratio=c['mlp_ratio'], qkv_bias=True,
                             class_num=classes, norm_layer=partial(hnn.LayerNorm, epsilon=1e-6))


def _trainer(name, model, steps_per_epoch):
    """The attributes the loops read, with the optimizer / schedule of the golden case built by the product's own
    classes."""
    from passl_amd.loss import build_loss
    from passl_amd.metric import build_metrics
    from passl_amd.solver.lr_scheduler import TimmCosine
    from passl_amd.solver.optimizer import Momentum, MomentumLARC
    c = U.CASES[name]
    sched = TimmCosine(**c['sched'])
    o = dict(c['opt'])
    klass = MomentumLARC if o.pop('optimizer') == 'MomentumLARC' else Momentum
    opt = klass(sched, parameters=list(model.parameters()), **o)
    spec = [{'CELoss': {'weight': 1.0}}]
    mspec = [{'TopkAcc': {'topk': [1, 5]}}]
    return SimpleNamespace(model=model, optimizer=opt, lr_scheduler=sched, lr_decay_unit=c['sched']['decay_unit'],
                           accum_steps=1, grad_reducer=None, print_batch_step=1, mode='train', validating=True,
                           cur_epoch_id=1, train_loss_func=build_loss(spec), eval_loss_func=build_loss(spec),
                           train_metric_func=build_metrics(mspec), eval_metric_func=build_metrics(mspec),
                           config={'Global': {}})


class _Batches(list):
    @property
    def dataset(self):
        return range(sum(b[0].shape[0] for b in self))


def _run_case(name, dtype, tol):
    from passl_amd.engine.loops import ClassificationEvaluationLoop, ClassificationTrainingEpochLoop
    z, N, S, classes, steps = U.load(name)
    kind = U.CASES[name]['kind']
    oracle = U.make_oracle(name, classes)
    model = _build(kind, classes, dtype)
    missing, unexpected = model.load_state_dict({k: v.float() for k, v in oracle.st.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    tr = _trainer(name, model, None)
    loop = ClassificationTrainingEpochLoop(tr, epochs=U.CASES[name]['sched']['epochs'])
    train, ev = U.batches(N, S, classes, steps)
    model.train()
    head = L.HEAD[kind]
    ps = dict(model.named_parameters())
    lines = []
    for s, (x, y) in enumerate(train):
        pre = 's%d_' % s
        amp = 4.0 ** s
        lr = tr.optimizer.get_lr()
        assert abs(lr - float(z[pre + 'lr'])) < 1e-12, (s, lr, float(z[pre + 'lr']))
        w0 = {n: ps[n].detach().clone() for n in head}
        grads = {}
        step_fn = tr.optimizer.step

        def spy():
            for n in head:
                grads[n] = ps[n].grad.detach().clone()
            step_fn()
        tr.optimizer.step = spy
        loop.global_step += 1
        out, ld = loop.train_one_step([x.to(DEV), y.to(DEV)])
        tr.optimizer.step = step_fn
        torch.cuda.synchronize()
        e_loss = abs(float(ld['loss']) - float(z[pre + 'loss']))
        e_sc = float((out.detach()[:, :8].double().cpu() - torch.as_tensor(z[pre + 'scores_head'])).abs().max())
        lines.append('step %d lr %.6f  loss err %.2e  scores err %.2e' % (s, lr, e_loss, e_sc))
        assert e_loss < tol['loss'] * amp and e_sc < tol['scores'] * amp, lines
        if tol['exact_topk']:
            assert abs(float(ld['top1']) - float(z[pre + 'top1'])) < 1e-6, (s, float(ld['top1']), float(z[pre + 'top1']))
            assert abs(float(ld['top5']) - float(z[pre + 'top5'])) < 1e-6
            assert float(ld['metric']) == float(ld['top1'])
        for n in head:
            eg = rel_l2(grads[n], z[pre + 'grad/' + n])
            ed = rel_l2(ps[n].detach() - w0[n], z[pre + 'delta/' + n])
            lines.append('   %-12s grad rel %.2e  update rel %.2e' % (n, eg, ed))
            assert eg < tol['grad'] * amp and ed < tol['delta'] * amp, lines
    res = ClassificationEvaluationLoop(tr).eval_one_dataset(_Batches([[x.to(DEV), y.to(DEV)] for x, y in ev]))
    for k in ('CELoss', 'loss', 'top1', 'top5', 'metric'):
        bound = tol['eval_loss'] if 'oss' in k else (1e-6 if tol['exact_topk'] else 0.13)
        lines.append('eval %-8s %.5f (reference %.5f)' % (k, res[k], float(z['eval_' + k])))
        assert abs(res[k] - float(z['eval_' + k])) < bound, lines
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    with open(os.path.join(ROOT, 'gpurun_out', 'parity_%s_%s.txt' % (name, str(dtype).replace('torch.', ''))), 'w') as f:
        f.write('\n'.join(lines) + '\n')


FP32 = dict(loss=5e-5, scores=5e-4, grad=2e-4, delta=1e-3, eval_loss=5e-3, exact_topk=True)
# bf16 frozen encoder (smoke bounds, as tests/test_clas_gpu.py's TOL_BF16): 53 conv layers with FIXED BatchNorm
# statistics do not re-normalise bf16 rounding, a few per cent of the feature range reach the classifier (the frozen
# layers themselves are bounded per layer, teacher-forced, in tests/test_layers_gpu.py); classifier, loss and update fp32
BF16 = dict(loss=2.5e-1, scores=1.5, grad=3e-1, delta=5e-1, eval_loss=1.0, exact_topk=False)


@pytest.mark.parametrize('name', sorted(U.CASES))
def test_probe_steps_and_evaluation_match_the_reference_run_fp32(name):
    _run_case(name, torch.float32, FP32)


def test_probe_steps_bf16_stay_near_the_reference_run():
    """bf16 compute (the MoCo-v3 recipe's FP16 O1 block): only the frozen encoder runs in bf16 — scores and loss
    stay within bf16 feature noise of the fp32 reference run."""
    _run_case('lp_simsiam_r50', torch.bfloat16, BF16)


def test_pretrain_checkpoint_feeds_the_probe(tmp_path):
    """SimSiamPretain.save writes <prefix>_encoder.pdparams (simsiam.py:113-126), MoCoV3Pretrain.save
    <prefix>_base_encoder.pdparams (mocov3.py:247-262); the probes' load_pretrained takes them: every frozen tensor
    equals the pre-trained one, the classifier keeps its own initialisation, and the probe's features are the
    pre-trained encoder's evaluation-mode features."""
    from passl_amd.models import build_model
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    torch.manual_seed(1)
    pre = build_model(dict(name='simsiam_resnet50_pretrain'))
    gen = torch.Generator().manual_seed(3)
    pre.train()
    for _ in range(2):                         # move the running statistics away from (0, 1)
        pre([torch.randn(8, 3, 64, 64, generator=gen).to(DEV), torch.randn(8, 3, 64, 64, generator=gen).to(DEV)])
    prefix = str(tmp_path / 'simsiam' / 'latest')
    pre.save(prefix)
    with open(prefix + '_encoder.pdparams', 'rb') as f:
        enc = pickle.load(f)
    assert 'conv1.weight' in enc and 'layer4.2.bn3._variance' in enc and not any(k.startswith('fc') for k in enc)
    probe = build_model(dict(name='simsiam_resnet50_linearprobe', class_num=1000))
    fc0 = probe.fc.weight.detach().clone()
    probe.load_pretrained(prefix + '_encoder')
    sd_pre, sd = pre.state_dict(), probe.state_dict()
    for k in enc:
        assert torch.equal(sd[k], sd_pre['encoder.' + k]), k
    assert torch.equal(probe.fc.weight, fc0)
    x = torch.randn(4, 3, 64, 64, generator=gen).to(DEV)
    probe.train()                               # BatchNorm stays on its running statistics
    s1 = probe(x)
    probe.eval()
    assert torch.equal(s1, probe(x))
    # MoCo-v3
    v3 = build_model(dict(name='mocov3_vit_base_pretrain'))
    p3 = str(tmp_path / 'mocov3' / 'latest')
    v3.save(p3)
    lp3 = build_model(dict(name='mocov3_vit_base_linearprobe', class_num=1000))
    lp3.load_pretrained(p3 + '_base_encoder')
    sd_pre, sd = v3.state_dict(), lp3.state_dict()
    n_checked = 0
    for k, v in sd.items():
        if not k.startswith('head.'):
            assert torch.equal(v, sd_pre['base_encoder.' + k]), k
            n_checked += 1
    assert n_checked > 100 and float(lp3.head.bias.abs().max()) == 0.0
    with torch.no_grad():
        xi = torch.randn(2, 3, 224, 224, generator=gen).to(DEV)
        v3.arena_q.refresh()
        f_pre = v3.base_encoder.forward_features(xi)
        lp3.arena_q.refresh()
        f_lp = lp3.forward_features(xi)
    assert torch.equal(f_pre, f_lp)


def test_v2_engine_trains_and_evaluates_the_simsiam_probe_from_yaml(tmp_path):
    """Engine(config).train() on configs/v2/simsiam_resnet50_lp_synthetic.yaml (the reference yaml's blocks over the
    synthetic labeled source): two epochs of ClassificationTrainingEpochLoop with the evaluation pass after each,
    checkpoints (epoch_N / latest / best) whose .pdstates carry the metric, the schedule stepped per epoch, only the
    classifier moving; the same run twice is bit-identical; Engine(mode='eval') evaluates a saved model to the same
    numbers."""
    from passl.engine.engine import Engine
    from passl_amd.utils.checkpoint import load_pickle
    from passl_amd.utils.config import get_config

    def run(out_dir):
        cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'simsiam_resnet50_lp_synthetic.yaml'),
                         ['Global.epochs=2', 'Global.output_dir=%s' % out_dir, 'Global.print_batch_step=1',
                          'Model.class_num=40', 'DataLoader.Train.dataset.num_classes=40',
                          'DataLoader.Eval.dataset.num_classes=40',
                          'DataLoader.Train.dataset.num_samples=48', 'DataLoader.Train.dataset.image_size=64',
                          'DataLoader.Train.sampler.batch_size=16', 'DataLoader.Eval.dataset.num_samples=40',
                          'DataLoader.Eval.dataset.image_size=64', 'DataLoader.Eval.sampler.batch_size=16'])
        cfg.DataLoader.Train.dataset.num_batches_cached = 3
        cfg.DataLoader.Eval.dataset.num_batches_cached = 3
        eng = Engine(cfg, mode='train')
        frozen0 = eng.model.arena_k.flat.clone()
        w0 = eng.model.fc.weight.detach().clone()
        lrs = []
        inner = eng.train_loop.train_one_step

        def spy(batch):
            lrs.append(eng.optimizer.get_lr())
            return inner(batch)
        eng.train_loop.train_one_step = spy
        eng.train()
        assert eng.global_step == 6 and len(lrs) == 6
        assert lrs[:3] == [1.6] * 3 and all(abs(v - 0.8) < 1e-12 for v in lrs[3:])       # per-epoch cosine, T_max 2
        assert torch.equal(frozen0, eng.model.arena_k.flat) and not torch.equal(w0, eng.model.fc.weight)
        return eng

    e1 = run(str(tmp_path / 'a'))
    d = os.path.join(str(tmp_path / 'a'), 'simsiam_resnet50_linearprobe')
    for stem in ('epoch_1', 'epoch_2', 'latest', 'best'):
        for ext in ('.pdparams', '.pdopt', '.pdstates'):
            assert os.path.exists(os.path.join(d, stem + ext)), (stem, ext, os.listdir(d))
    st = load_pickle(os.path.join(d, 'latest.pdstates'))
    assert st['epoch'] == 2 and st['global_step'] == 6 and 0.0 <= st['top1'] <= st['top5'] <= 1.0 and 'CELoss' in st
    latest = e1.validate_loop.latest_model_metric
    best = e1.validate_loop.best_model_metric
    assert best['metric'] >= latest['metric'] and abs(latest['loss'] - latest['CELoss']) < 1e-12
    e2 = run(str(tmp_path / 'b'))
    assert torch.equal(e1.model.arena_q.flat, e2.model.arena_q.flat)
    assert e1.validate_loop.latest_model_metric == e2.validate_loop.latest_model_metric
    # evaluation-only engine over the saved model
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'simsiam_resnet50_lp_synthetic.yaml'),
                     ['Global.pretrained_model=%s' % os.path.join(d, 'latest'), 'Model.class_num=40',
                      'DataLoader.Eval.dataset.num_classes=40', 'DataLoader.Eval.dataset.num_samples=40',
                      'DataLoader.Eval.dataset.image_size=64', 'DataLoader.Eval.sampler.batch_size=16'])
    cfg.DataLoader.Eval.dataset.num_batches_cached = 3
    ev = Engine(cfg, mode='eval')
    assert ev.optimizer is None and ev.train_loop is None
    res = ev.eval()
    assert res == latest, (res, latest)
