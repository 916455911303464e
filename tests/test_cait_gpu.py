"""CaiT (passl_amd/models/cait.py) on the HIP path against the run of the reference's own cait.py
(tests/golden/cait_small.npz, cait_small_dp.npz; tests/golden/make_golden_cait.py), and as a whole step: evaluation
mode, save / load, eager against a strict step plan, the YAML through the Engine.

fp32: logits, loss and EACH parameter gradient (relative to that gradient's own maximum) within the project's fp32
bound of 1e-3 of the fixture for both drop-path cases, and every recorded parameter after two AdamW steps (no-decay names
of the config, no clipping) within the same bound.  Parameters whose gradient is analytically zero — every proj_l.bias,
the key third of a trunk qkv.bias, ClassAttn's k.bias — are held to AdamW's +-lr per step around their initial value,
their gradient to zero at the scale of the layer's other gradients.  bf16: the losses within 3e-2."""
import math
import os

import numpy as np
import pytest
import torch

import cait_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(rate, dtype=torch.float32, seed=1, **over):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    model = PM.build_model(dict(dict(name='Cait', drop_path_rate=rate, **MU.MODEL), **over))
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(MU.fixture_state(keys), strict=False)
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


def _two_steps(name, dtype, perturb=None):
    """-> (fixture, logits of step 0, losses, gradients of step 0, the model after two steps)."""
    from passl_amd.loss.celoss import CELoss
    fx = MU.load(name)
    model = _model(float(fx['rate']), dtype).train()
    if perturb is not None:
        perturb(model)
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


def _zero_part(name, t):
    """The analytically-zero part of a gradient / parameter and the rest (None when all of it is zero)."""
    if name.endswith('attn.qkv.bias'):
        D = t.numel() // 3
        return t[D:2 * D], torch.cat([t[:D], t[2 * D:]])
    return t, None


@pytest.mark.parametrize('name', sorted(MU.CASES))
def test_fp32_matches_the_reference_run(name):
    fx, logits, losses, grads, model = _two_steps(name, torch.float32)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (MU.BATCH, MU.MODEL['num_classes'])
    worst = {'logits': _relmax(logits, fx['s0_logits'])}
    for s in range(MU.STEPS):
        worst['loss%d' % s] = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
    params = dict(model.named_parameters())
    assert sorted('s0_grad/' + n for n in params) == sorted(k for k in fx if k.startswith('s0_grad/'))
    zero = set(MU.zero_grad_names(params))
    init = MU.fixture_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    for n in params:
        g, ref = grads[n].detach().cpu(), torch.from_numpy(fx['s0_grad/' + n])
        got = params[n].detach().cpu()
        fin = torch.from_numpy(fx['final/' + n]) if ('final/' + n) in fx else None
        if n in zero:
            # softmax is invariant to a constant added to a row of scores: what both sides compute for these is rounding
            # noise, which AdamW turns into steps of +-lr in either direction (tests/test_swin_gpu.py, test_mocov3_gpu.py)
            gz, g = _zero_part(n, g)
            _rz, ref = _zero_part(n, ref)
            scale = float(grads[n.rsplit('.', 1)[0] + '.weight'].abs().max())       # the same layer's weight gradient
            assert float(gz.abs().max()) <= TOL_F32 * scale, n
            pz, got = _zero_part(n, got)
            iz, _ = _zero_part(n, init[n])
            assert float((pz - iz).abs().max()) <= 1.01 * MU.STEPS * MU.SOLVER['lr'], n
            if fin is not None:
                _fz, fin = _zero_part(n, fin)
            if g is None:
                continue
        if float(ref.abs().max()) == 0.0:                    # a block dropped for every sample of the batch
            assert float(g.abs().max()) == 0.0, n
        else:
            worst['grad ' + n] = _relmax(g, ref)
        if fin is not None:
            worst['final ' + n] = _relmax(got, fin)
    for k in ('logits', 'loss0', 'loss1'):
        print('%s %-8s %.3e' % (name, k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('%s worst %-6s %.3e (%s)' % (name, kind, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v <= TOL_F32}
    assert not bad, bad


def test_fp32_parity_sees_the_keep_table_and_the_head_mixes():
    """The comparison discriminates: with two entries of the reference's keep table swapped, or with one proj_w.weight
    transposed, the logits are far outside the bound."""
    fx = MU.load('cait_small_dp')
    model = _model(0.5).train()
    x, _ = MU.batches()[0]
    keep = torch.from_numpy(fx['s0_keep'])
    assert (keep == 0).any() and tuple(keep.shape) == (2 * MU.MODEL['depth'], MU.BATCH)
    row = int(np.flatnonzero(keep[:, 0].numpy() != keep[:, 1].numpy())[0])
    swapped = keep.clone()
    swapped[row] = keep[row].flip(0)
    with torch.no_grad():
        same = model(x.to(DEV), drop_path_keep=keep)
        other = model(x.to(DEV), drop_path_keep=swapped)
    assert _relmax(same, fx['s0_logits']) <= TOL_F32 < 10 * TOL_F32 < _relmax(other, fx['s0_logits'])
    plain = _model(0.0).eval()
    ref = MU.load('cait_small')['s0_logits']
    with torch.no_grad():
        assert _relmax(plain(x.to(DEV)), ref) <= TOL_F32
        w = plain.blocks[1].attn.proj_w.weight
        w.copy_(w.t().clone())
        plain.sync_runtime_state()
        assert _relmax(plain(x.to(DEV)), ref) > 10 * TOL_F32


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
    assert plain.train()(x).requires_grad and plain.drop_path_draws == 0       # rate 0: no draw in training either
    dropping.train()
    with torch.no_grad():
        c = dropping(x)
    assert dropping.drop_path_draws == 1 and dropping.drop_path_step() == 1
    assert dropping.drop_path_table(MU.BATCH).shape == (2 * MU.MODEL['depth'], MU.BATCH)   # the token-only blocks: none
    assert bool(torch.isfinite(c).all())


def test_state_dict_round_trip_through_save_and_load_pretrained(tmp_path):
    model = _model(0.0)
    path = str(tmp_path / 'cait')
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
    # finetune=True: a square grid's position table is resized (bicubic) and a head of another size is dropped
    sq = _model(0.0, img_size=(16, 16), num_classes=5)
    sq.save(str(tmp_path / 'sq'))
    big = _model(0.0, img_size=(24, 24), num_classes=8)
    head = big.head.weight.detach().clone()
    big.load_pretrained(str(tmp_path / 'sq'), finetune=True)
    assert tuple(big.pos_embed.shape) == (1, 36, MU.MODEL['embed_dim']) and torch.equal(big.head.weight, head)
    want = torch.nn.functional.interpolate(sq.pos_embed.detach().cpu().reshape(1, 4, 4, -1).permute(0, 3, 1, 2),
                                           size=(6, 6), mode='bicubic', align_corners=False)
    assert torch.allclose(big.pos_embed.detach().cpu(), want.permute(0, 2, 3, 1).flatten(1, 2))
    assert torch.equal(big.cls_token, sq.cls_token)


def test_reset_classifier_builds_a_new_head():
    model = _model(0.0).eval()
    x = MU.batches()[0][0].to(DEV)
    model.reset_classifier(16)
    assert model.get_classifier() is model.head and model.num_classes == 16
    with torch.no_grad():
        assert tuple(model(x).shape) == (MU.BATCH, 16)
    model.reset_classifier(0)
    with torch.no_grad():
        assert tuple(model(x).shape) == (MU.BATCH, model.num_features)


def test_large_factories_are_refused_by_the_library_when_run():
    """576 tokens: the model builds (tests/test_cait_host.py holds its keys) and the first attention raises the library's
    unsupported error; nothing falls back."""
    from passl_amd.hip.lib import PasslHipError
    model = _model(0.0, img_size=(96, 96), depth=1, depth_token_only=1).eval()          # 24 x 24 = 576 patch tokens
    with torch.no_grad(), pytest.raises(PasslHipError):
        model(torch.randn(1, 3, 96, 96, device=DEV))
    heads = _model(0.0, embed_dim=16 * 48, num_heads=16, depth=1, depth_token_only=1).eval()
    with torch.no_grad(), pytest.raises(PasslHipError):
        heads(MU.batches()[0][0].to(DEV))


def test_eager_and_plan_replayed_steps_are_bit_identical():
    """Four steps with rate 0.5: the draw and every launch of the step are the library's own (strict plan, nothing
    foreign), the counter lives on the device so each replay draws a fresh keep table, and losses and parameters equal
    the eager twin's bit for bit."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.loss.celoss import CELoss
    steps, seed = 4, (0x2103 << 32) + 7
    gen = torch.Generator().manual_seed(3)
    H, W = MU.MODEL['img_size']
    batches = [(torch.randn(MU.BATCH, 3, H, W, generator=gen).to(DEV),
                torch.randint(0, MU.MODEL['num_classes'], (MU.BATCH,), generator=gen).to(DEV)) for _ in range(steps)]
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
    for s in range(steps):
        assert np.array_equal(tb[s].numpy(), DP.keep_table(MU.keep_probs(0.5), MU.BATCH, seed, s)), 'step %d' % s


def test_engine_trains_and_evaluates_the_cait_yaml(tmp_path):
    """configs/v2/cait_s24_224_synthetic.yaml shrunk to the fixture model (16-pixel images, bf16) through the Engine: two
    epochs with a finite, changing loss, the no-decay groups of the YAML, one draw per training pass, and the evaluation
    loop."""
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N = 8
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'cait_s24_224_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'LRScheduler.warmup_epoch=1',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 2), 'DataLoader.Train.dataset.image_size=16',
                      'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=16',
                      'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'cait_s24_224' and cfg['Model']['drop_path_rate'] == 0.1
    assert list(cfg['Optimizer']['no_weight_decay_name']) == MU.NO_DECAY
    cfg['Model'] = dict(dict(name='Cait', drop_path_rate=0.1, drop_rate=0.0, **MU.MODEL), img_size=16)
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'Cait' and type(eng.optimizer).__name__ == 'AdamW'
    assert eng.model.arena_q.dtype == torch.bfloat16
    decays = {n: wd for rows in eng.optimizer._param_table for n, _s, wd in rows}
    assert sorted(set(decays.values())) == [0.0, 0.05]
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
    assert eng.model.drop_path_draws == 4 and eng.model.drop_path_step() == 4
    metric = eng.validate_loop.latest_model_metric                           # eval_during_train: once per epoch
    assert metric and all(math.isfinite(v) for v in metric.values()), metric
