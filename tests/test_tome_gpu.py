"""Token merging on the v2 VisionTransformer (passl_amd/models/utils/tome.py) against the run of the reference's own
tome.py on its own ViT (tests/golden/tome_small.npz; tests/golden/make_golden_tome.py), and the patched model's contract.

fp32: every layer's decisions from the trace equal the reference's; logits, losses, EACH parameter gradient (relative to
that gradient's own maximum, large tensors on the fixture's sample) and every parameter after two AdamW steps within the
project's fp32 bound of 1e-3.  Measured on an MI355X: logits 7.4e-7, losses 1.4e-7 / 2.3e-6, worst gradient 1.5e-6, worst
parameter 5.2e-7; prop_attn logits 5.3e-7 (7.1e-2 without the key bias).
bf16: equal decisions in both steps (the fixture's seed keeps every decision 4 x clear of what bf16 qkv changes: gap
4.995e-3, change 1.174e-3), losses within the 3e-2 of the bf16 model tests.  Measured: 2.5e-3 / 1.6e-3.
The model is driven as the v2 loops drive it: forward, loss, clear_grad, backward, step; VisionTransformer.forward
refreshes the arena's compute-dtype operands and data-gradient packs from the updated weights."""
import math
import os

import numpy as np
import pytest
import torch

import tome_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(dtype=torch.float32, tome_cfg=None, seed=None, **over):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(1)
    cfg = dict(dict(name='VisionTransformer', **MU.MODEL), **over)
    if tome_cfg is not None:
        cfg['tome'] = tome_cfg
    model = PM.build_model(cfg)
    if seed is not None:
        keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        missing, unexpected = model.load_state_dict(MU.fixture_state(keys, seed), strict=False)
        assert not missing and not unexpected
    return model


def _optimizer(model):
    from passl_amd.solver.optimizer import AdamW
    s = MU.SOLVER
    named = list(model.named_parameters())
    skip = {n for n, _ in named if any(nd in n for nd in MU.NO_DECAY)}
    groups = [{'params': [p for n, p in named if n not in skip]},
              {'params': [p for n, p in named if n in skip], 'weight_decay': 0.0}]
    return AdamW(s['lr'], beta1=s['beta1'], beta2=s['beta2'], epsilon=s['epsilon'], weight_decay=s['weight_decay'],
                 parameters=groups)


def _relmax(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _decisions(fx, tag):
    """[(dest int64 [B, T], node_idx, src rows)] of the merging layers of a recorded pass."""
    out = []
    i = 0
    for r, T in zip(fx['r'].tolist(), fx['t_in'].tolist()):
        if r > 0:
            pre = '%s/layer%d/' % (tag, i)
            out.append((MU.dest_from_indices(T, fx[pre + 'unm_idx'], fx[pre + 'src_idx'], fx[pre + 'dst_idx']),
                        fx[pre + 'node_max'], fx[pre + 'node_idx'], fx[pre + 'src_idx']))
            i += 1
    return out


def _check_trace(trace, fx, tag, what):
    want = _decisions(fx, tag)
    assert len(trace) == len(want), '%s: %d merging layers traced, %d recorded' % (what, len(trace), len(want))
    for i, ((dest, nmax, nidx), (wd, wmax, widx, src)) in enumerate(zip(trace, want)):
        assert np.array_equal(dest.cpu().numpy().astype(np.int64), wd), '%s: layer %d decisions differ' % (what, i)
        got_idx = np.take_along_axis(nidx.cpu().numpy().astype(np.int64), src, axis=1)
        assert np.array_equal(got_idx, np.take_along_axis(widx, src, axis=1)), '%s: layer %d partners differ' % (what, i)
        err = float(np.abs(nmax.cpu().numpy()[:, 1:] - wmax[:, 1:]).max())
        print('%s layer %d: node_max off by %.3e' % (what, i, err))


def _two_steps(dtype):
    """-> (fixture, logits of step 0, losses, gradients of step 0, the model after two steps, the trace of each step)."""
    from passl_amd.loss.celoss import CELoss
    fx = MU.load(MU.FIXTURE)
    model = _model(dtype, tome_cfg=dict(r=list(MU.R), prop_attn=False), seed=int(fx['seed'])).train()
    assert model.r == MU.R
    opt, celoss = _optimizer(model), CELoss()
    losses, grads, logits0, traces = [], {}, None, []
    for step, (x, y) in enumerate(MU.batches()):
        model._tome_info['trace'] = []
        logits = model(x.to(DEV))
        traces.append(model._tome_info.pop('trace'))
        loss = celoss(logits, y.to(DEV))['CELoss']
        opt.clear_grad()
        loss.backward()
        if step == 0:
            logits0 = logits.detach().clone()
            grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return fx, logits0, losses, grads, model, traces


def test_apply_patch_keeps_the_state_dict():
    from passl_amd.models.utils import tome
    model = _model(seed=3)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in model.named_parameters()]
    tome.apply_patch(model)
    assert model.r == 0 and type(model).__name__ == 'ToMeVisionTransformer'
    after = model.state_dict()
    assert list(after) == list(before) and [n for n, _ in model.named_parameters()] == names
    for k in before:
        assert torch.equal(after[k], before[k]), k
    model.r = (16, -1)
    assert model.r == (16, -1) and list(model.state_dict()) == list(before)
    tome.apply_patch(model, prop_attn=True)                         # again: only the switch changes
    assert model._tome_info['prop_attn'] is True and type(model).__name__ == 'ToMeVisionTransformer'


def test_r_zero_is_the_unpatched_model_bit_for_bit():
    from passl_amd.loss.celoss import CELoss
    from passl_amd.models.utils import tome
    x, y = MU.batches()[0]
    res = []
    for patched in (False, True):
        model = _model(seed=3).train()
        if patched:
            tome.apply_patch(model)
            model.r = 0
        logits = model(x.to(DEV))
        CELoss()(logits, y.to(DEV))['CELoss'].backward()
        torch.cuda.synchronize()
        res.append((logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    (la, ga), (lb, gb) = res
    assert torch.equal(_bits(la), _bits(lb))
    assert sorted(ga) == sorted(gb)
    for n in ga:
        assert torch.equal(_bits(ga[n]), _bits(gb[n])), n


def test_fp32_matches_the_reference_run():
    fx, logits, losses, grads, model, traces = _two_steps(torch.float32)
    for step, trace in enumerate(traces):
        _check_trace(trace, fx, 's%d' % step, 'fp32 step %d' % step)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (MU.BATCH, MU.MODEL['class_num'])
    worst = {'logits': _relmax(logits, fx['s0_logits'])}
    for s in range(MU.STEPS):
        worst['loss%d' % s] = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
    params = dict(model.named_parameters())
    assert sorted('s0_grad/' + n for n in params) == sorted(k for k in fx if k.startswith('s0_grad/'))
    init = MU.fixture_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()], int(fx['seed']))
    for n in params:
        g, ref = MU.sample(grads[n]).cpu(), torch.from_numpy(fx['s0_grad/' + n])
        got, fin = MU.sample(params[n]).cpu(), torch.from_numpy(fx['final/' + n])
        assert g.shape == ref.shape and got.shape == fin.shape, n
        gz, g = MU.zero_grad_part(n, g)
        if gz is not None:
            # softmax ignores a shift of a row of scores: both sides compute rounding noise for the key third of the
            # bias, which AdamW turns into steps of +-lr (tests/test_cait_gpu.py)
            scale = float(grads[n.rsplit('.', 1)[0] + '.weight'].abs().max())
            assert float(gz.abs().max()) <= TOL_F32 * scale, n
            pz, got = MU.zero_grad_part(n, got)
            iz, _ = MU.zero_grad_part(n, MU.sample(init[n]))
            assert float((pz - iz).abs().max()) <= 1.01 * MU.STEPS * MU.SOLVER['lr'], n
            ref, fin = MU.zero_grad_part(n, ref)[1], MU.zero_grad_part(n, fin)[1]
        worst['grad ' + n] = _relmax(g, ref)
        worst['final ' + n] = _relmax(got, fin)
    for k in ('logits', 'loss0', 'loss1'):
        print('fp32 %-8s %.3e' % (k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('fp32 worst %-6s %.3e (%s)' % (kind, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v <= TOL_F32}
    assert not bad, bad


def test_fp32_parity_sees_a_wrong_schedule():
    """The comparison discriminates: with r = [3, 4, 0] in place of [4, 3, 0] the logits are far outside the bound."""
    fx = MU.load(MU.FIXTURE)
    model = _model(tome_cfg=dict(r=[3, 4, 0]), seed=int(fx['seed'])).eval()
    with torch.no_grad():
        other = model(MU.batches()[0][0].to(DEV))
        model.r = list(MU.R)
        same = model(MU.batches()[0][0].to(DEV))
    assert _relmax(same, fx['s0_logits']) <= TOL_F32 < 10 * TOL_F32 < _relmax(other, fx['s0_logits'])


def test_bf16_decisions_and_losses():
    fx, logits, losses, _grads, _m, traces = _two_steps(torch.bfloat16)
    assert float(fx['gap']) >= 4 * float(fx['change'])
    for step, trace in enumerate(traces):
        _check_trace(trace, fx, 's%d' % step, 'bf16 step %d' % step)
    assert bool(torch.isfinite(logits).all())
    for s in range(MU.STEPS):
        err = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
        print('bf16 loss%d %.3e (bound %.0e)' % (s, err, TOL_BF16_LOSS))
        assert err <= TOL_BF16_LOSS


def test_prop_attn_evaluates_under_no_grad_and_refuses_gradients():
    fx = MU.load(MU.FIXTURE)
    model = _model(tome_cfg=dict(r=list(MU.R), prop_attn=True), seed=int(fx['seed'])).eval()
    x = MU.batches()[0][0].to(DEV)
    model._tome_info['trace'] = []
    with torch.no_grad():
        logits = model(x)
    _check_trace(model._tome_info.pop('trace'), fx, 'prop', 'prop_attn')
    err = _relmax(logits, fx['prop/logits'])
    print('prop_attn logits %.3e; without the key bias they would be off by %.3e' % (
        err, _relmax(fx['s0_logits'], fx['prop/logits'])))
    assert err <= TOL_F32
    assert _relmax(fx['s0_logits'], fx['prop/logits']) > 10 * TOL_F32          # the bias matters in this fixture
    assert tuple(model._tome_info['size'].shape) == (MU.BATCH, int(fx['t_final']))
    assert float(model._tome_info['size'].sum()) == MU.BATCH * MU.TOKENS
    with pytest.raises(NotImplementedError):
        model(x)
    model.train()
    with pytest.raises(NotImplementedError):
        model(x)


def test_dropout_with_merging_in_training_raises():
    model = _model(tome_cfg=dict(r=2), drop_rate=0.1)
    x = MU.batches()[0][0].to(DEV)
    model.train()
    with pytest.raises(NotImplementedError):
        model(x)
    model.eval()                                    # evaluation: dropout is off, merging runs
    with torch.no_grad():
        assert bool(torch.isfinite(model(x)).all())
    model.train()
    model.r = 0                                     # r = 0: the unpatched path with its dropout
    assert bool(torch.isfinite(model(x)).all())


def test_vit_base_r16_forward_and_backward():
    """The shape envelope: ViT-B/16 at 224, r = 16: 197 tokens shrink to 11 over the 12 blocks."""
    import passl.models as PM
    from passl_amd.models.utils import tome
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(1)
    model = PM.build_model(dict(name='ViT_base_patch16_224', class_num=16, tome=dict(r=16))).train()
    assert tome.token_schedule(197, tome.parse_r(12, model.r))[2] == 11
    model._tome_info['trace'] = []
    logits = model(torch.randn(2, 3, 224, 224, device=DEV))
    logits.float().square().mean().backward()
    torch.cuda.synchronize()
    trace = model._tome_info.pop('trace')
    assert [tuple(d.shape) for d, _, _ in trace] == [(2, T) for T in range(197, 20, -16)]
    assert [int(d.max()) for d, _, _ in trace] == [T - 17 for T in range(197, 36, -16)] + [10]    # the clamp: r = 10
    assert tuple(model._tome_info['size'].shape) == (2, 11) and float(model._tome_info['size'].sum()) == 2 * 197
    assert tuple(logits.shape) == (2, 16) and bool(torch.isfinite(logits).all())
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(model.blocks[0].attn.qkv.weight.grad.abs().max()) > 0


def test_engine_trains_the_tome_yaml(tmp_path):
    """configs/v2/vit_base_sup_tome_synthetic.yaml shrunk to the fixture model through the Engine: its `tome` entry reaches
    the model, four steps with a finite, changing loss, and the evaluation loop."""
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N = 8
    S = MU.MODEL['img_size']
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_sup_tome_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'Global.accum_steps=1', 'LRScheduler.warmup_steps=1',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 2), 'DataLoader.Train.dataset.image_size=%d' % S,
                      'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=%d' % S,
                      'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'ViT_base_patch16_224' and cfg['Model']['drop_rate'] == 0.0
    assert dict(cfg['Model']['tome']) == {'r': 16, 'prop_attn': False}
    cfg['Model'] = dict(dict(name='VisionTransformer', **MU.MODEL), tome=dict(cfg['Model']['tome']))
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'ToMeVisionTransformer' and eng.model.r == 16
    assert eng.model.arena_q.dtype == torch.bfloat16
    losses = []
    inner = eng.train_loop.train_one_step

    def spy(batch):
        out, ld = inner(batch)
        losses.append(float(ld['loss'].detach().float().reshape(())))
        return out, ld
    eng.train_loop.train_one_step = spy
    eng.train()
    print('loss', losses)
    assert eng.global_step == 4 and len(losses) == 4
    assert all(math.isfinite(v) and v > 0 for v in losses) and len(set(losses)) > 1
    assert tuple(eng.model._tome_info['size'].shape)[1] == 37 - 16 - 10 - 5          # r = 16 clamped to 18, 10, 5: 16, 10, 5
    metric = eng.validate_loop.latest_model_metric
    assert metric and all(math.isfinite(v) for v in metric.values()), metric
