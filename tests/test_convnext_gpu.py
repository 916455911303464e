"""ConvNeXt (passl_amd/models/convnext.py) on the HIP path against the run of the reference's own convnext.py
(tests/golden/convnext_small.npz, convnext_small_dp.npz; tests/golden/make_golden_convnext.py), and as a whole step:
evaluation mode, save / load, eager against a strict step plan, the YAML through the Engine.

fp32: logits, loss and EACH parameter gradient (relative to that gradient's own maximum) within the project's fp32
bound of 1e-3 of the fixture for both drop-path cases, and every parameter after two AdamW steps within the same
bound.  bf16: the loss within 3e-2, the bound of the ViT bf16 tests (tests/test_mae_v2_gpu.py, test_droppath_gpu.py)."""
import math
import os

import numpy as np
import pytest
import torch

import convnext_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(rate, dtype=torch.float32, seed=1):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    model = PM.build_model(dict(name='ConvNeXt', drop_path_rate=rate, **MU.MODEL))
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(MU.fixture_state(keys), strict=False)
    assert not missing and not unexpected
    return model


def _optimizer(model):
    from passl_amd.solver.optimizer import AdamW
    s = MU.SOLVER
    return AdamW(s['lr'], beta1=s['beta1'], beta2=s['beta2'], epsilon=s['epsilon'], weight_decay=s['weight_decay'],
                 parameters=list(model.parameters()))


def _relmax(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _two_steps(name, dtype):
    """-> (fixture, logits of step 0, losses, gradients of step 0, the model after two steps)."""
    from passl_amd.loss.celoss import CELoss
    fx = MU.load(name)
    model = _model(float(fx['rate']), dtype).train()
    opt, celoss = _optimizer(model), CELoss()
    losses, grads, logits0 = [], {}, None
    for step, (x, y) in enumerate(MU.batches()):
        keep = torch.from_numpy(fx['s%d_keep' % step]) if ('s%d_keep' % step) in fx else None
        logits = model(x.to(DEV), drop_path_keep=keep)
        loss = celoss(logits, y.to(DEV))['CELoss']
        opt.clear_grad()
        loss.backward()
        if step == 0:
            logits0 = logits.detach().clone()
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return fx, logits0, losses, grads, model


@pytest.mark.parametrize('name', sorted(MU.CASES))
def test_fp32_matches_the_reference_run(name):
    fx, logits, losses, grads, model = _two_steps(name, torch.float32)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (MU.BATCH, MU.MODEL['class_num'])
    worst = {'logits': _relmax(logits, fx['s0_logits'])}
    for s in range(MU.STEPS):
        worst['loss%d' % s] = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
    params = dict(model.named_parameters())
    assert sorted('s0_grad/' + n for n in params) == sorted(k for k in fx if k.startswith('s0_grad/'))
    for n in params:
        worst['grad ' + n] = _relmax(grads[n], fx['s0_grad/' + n])
        worst['final ' + n] = _relmax(params[n].detach(), fx['final/' + n])
    for k in ('logits', 'loss0', 'loss1'):
        print('%s %-8s %.3e' % (name, k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('%s worst %-6s %.3e (%s)' % (name, kind, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v <= TOL_F32}
    assert not bad, bad


def test_fp32_parity_sees_the_branch_and_the_keep_table():
    """The comparison discriminates: without the reference's keep table the logits are far outside the bound."""
    fx = MU.load('convnext_small_dp')
    model = _model(0.5).train()
    x, _ = MU.batches()[0]
    keep = torch.from_numpy(fx['s0_keep'])
    assert (keep == 0).any()
    with torch.no_grad():
        other = model(x.to(DEV), drop_path_keep=torch.ones_like(keep))
    assert _relmax(other, fx['s0_logits']) > 10 * TOL_F32


@pytest.mark.parametrize('name', sorted(MU.CASES))
def test_bf16_loss(name):
    fx, logits, losses, _grads, _model_ = _two_steps(name, torch.bfloat16)
    assert bool(torch.isfinite(logits).all())
    for s in range(MU.STEPS):
        err = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
        print('%s bf16 loss%d %.3e (bound %.0e)' % (name, s, err, TOL_BF16_LOSS))
        assert err <= TOL_BF16_LOSS


def test_evaluation_mode_ignores_drop_path_rate():
    x = MU.batches()[0][0].to(DEV)
    dropping, plain = _model(0.5).eval(), _model(0.0, seed=2).eval()
    with torch.no_grad():
        a, b = dropping(x), plain(x)
    assert torch.equal(_bits(a), _bits(b))
    assert dropping.drop_path_draws == 0 and dropping.drop_path_step() == 0
    dropping.train()
    with torch.no_grad():
        c = dropping(x)
    assert dropping.drop_path_draws == 1 and dropping.drop_path_step() == 1
    assert dropping.drop_path_table(MU.BATCH).shape == (4, MU.BATCH)
    assert bool(torch.isfinite(c).all())


def test_state_dict_round_trip_through_save_and_load_pretrained(tmp_path):
    model = _model(0.0)
    path = str(tmp_path / 'convnext')
    model.save(path)
    assert os.path.exists(path + '.pdparams')
    other = _model(0.0, seed=5)
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    other.load_pretrained(path)
    a, b = model.state_dict(), other.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x = MU.batches()[0][0].to(DEV)
    with torch.no_grad():
        assert torch.equal(_bits(model.eval()(x)), _bits(other.eval()(x)))
    with pytest.raises(ValueError):
        other.load_pretrained(str(tmp_path / 'missing'))


def test_eager_and_plan_replayed_steps_are_bit_identical():
    """Four steps with rate 0.5: the draw and every launch of the step are the library's own (strict plan, nothing
    foreign), the counter lives on the device so each replay draws a fresh keep table, and losses and parameters equal
    the eager twin's bit for bit."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.loss.celoss import CELoss
    steps, seed = 4, (0x2201 << 32) + 7
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(MU.BATCH, 3, MU.HEIGHT, MU.WIDTH, generator=gen).to(DEV),
                torch.randint(0, MU.MODEL['class_num'], (MU.BATCH,), generator=gen).to(DEV)) for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        model = _model(0.5).train()
        model.set_drop_path_seed(seed)
        opt, celoss = _optimizer(model), CELoss()

        def full_step(x, y):
            loss = celoss(model(x), y)['CELoss']
            opt.clear_grad()
            loss.backward(ops.ones_like_cached(loss))
            opt.step()
            return dict(loss=loss, keep=model.drop_path_table(MU.BATCH))
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, tables = [], []
        for x, y in batches:
            out = sp.run(x, y)
            losses.append(out['loss'].detach().clone().reshape(1))
            tables.append(out['keep'].detach().clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        assert model.drop_path_step() == steps
        results[mode] = (torch.cat(losses).cpu(), torch.stack(tables).cpu(),
                         model.arena_q.flat[:model.arena_q.n_train].clone().cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, ta, fa), (lb, tb, fb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(ta, tb) and torch.equal(_bits(fa), _bits(fb))
    assert all(math.isfinite(float(v)) for v in lb)
    assert len({tuple(t.flatten().tolist()) for t in tb}) >= 2, 'the keep table must differ from step to step'
    import droppath_util as DP
    _rates, keep_prob = MU.ladder(0.5)
    for s in range(steps):
        assert np.array_equal(tb[s].numpy(), DP.keep_table(keep_prob, MU.BATCH, seed, s)), 'step %d' % s


def test_engine_trains_the_convnext_yaml(tmp_path):
    """configs/v2/convnext_base_synthetic.yaml at a reduced size through the Engine (Model overridden to the small
    ConvNeXt, 64-pixel images, bf16, two steps): finite losses, TimmCosine's first two rates, one draw per pass."""
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N, steps = 8, 2
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'convnext_base_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'Global.eval_during_train=False', 'LRScheduler.warmup_epoch=1',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 4), 'DataLoader.Train.dataset.image_size=64',
                      'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=64',
                      'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'convnext_base' and cfg['Model']['drop_path_rate'] == 0.5
    cfg['Model'] = dict(name='ConvNeXt', drop_path_rate=cfg['Model']['drop_path_rate'], **MU.MODEL)
    cfg['Global']['max_train_step'] = steps
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'ConvNeXt' and eng.model.drop_path_rate == 0.5
    assert type(eng.lr_scheduler).__name__ == 'TimmCosine'
    assert type(eng.train_loss_func.loss_func[0]).__name__ == 'CELoss'
    assert eng.model.arena_q.dtype == torch.bfloat16
    lrs, losses = [], []
    inner = eng.train_loop.train_one_step

    def spy(batch):
        lrs.append(eng.optimizer.get_lr())
        out, ld = inner(batch)
        losses.append(float(ld['loss'].detach().float().reshape(())))
        return out, ld
    eng.train_loop.train_one_step = spy
    eng.train()
    print('lr', lrs, 'loss', losses)
    assert eng.global_step == steps and len(losses) == steps
    assert all(math.isfinite(v) and v > 0 for v in losses)
    # warmup_start_lr 0 over one epoch of 4 steps towards 4e-3: step 0 runs at 0, step 1 at a quarter of the peak
    assert lrs[0] == 0.0 and abs(lrs[1] - 4e-3 / 4) < 1e-12
    assert eng.model.drop_path_draws == steps and eng.model.drop_path_step() == steps
