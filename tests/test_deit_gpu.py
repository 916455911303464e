"""DeiT (passl_amd/models/deit.py) on the HIP path against the run of the reference's own deit.py
(tests/golden/deit_small.npz, deit_long.npz; tests/golden/make_golden_deit.py), and as a whole step: the routing of
``hnn.attention``, evaluation mode, the eight factories, eager against a strict step plan, the YAML through the Engine.

fp32: logits, loss and EACH parameter gradient (relative to that gradient's own maximum) within the project's fp32
bound of 1e-3 of the fixture, and every recorded parameter after two AdamW steps (no-decay names of the config, no
clipping) within the same bound.  The key third of a qkv.bias, whose gradient is analytically zero, is held to AdamW's
+-lr per step around its initial value, its gradient to zero at the scale of the layer's weight gradient.  bf16: the
losses within 3e-2.

The 226- and 227-token fixtures ('plain' and 'dist' of deit_long) are refused by the dense attention kernels: they pass
only through the key-tiled ones (csrc/attention_tiled.hip), forward and backward."""
import math
import os

import numpy as np
import pytest
import torch

import deit_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2
ALL_CASES = [(name, tag) for name, cases in MU.CASES.items() for tag in cases]
CASE_IDS = ['%s-%s' % c for c in ALL_CASES]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(cls_name, args, rate, dtype=torch.float32, seed=1, **over):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    model = PM.build_model(dict(dict(name=cls_name, drop_path_rate=rate, **args), **over))
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


def _fixture(name, tag):
    fx = MU.load(name)
    return {k[len(tag) + 1:]: v for k, v in fx.items() if k.startswith(tag + '/')}


def _two_steps(name, tag, dtype):
    """-> (fixture of the case, logits of step 0, losses, gradients of step 0, the model after two steps)."""
    from passl_amd.loss.celoss import CELoss
    cls_name, args, rate = MU.CASES[name][tag]
    fx = _fixture(name, tag)
    model = _model(cls_name, args, rate, dtype).train()
    opt, celoss = _optimizer(model), CELoss()
    losses, grads, logits0 = [], {}, None
    for step, (x, y) in enumerate(MU.batches(args)):
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
    """The analytically-zero part of a qkv.bias (its key third) and the rest."""
    D = t.numel() // 3
    return t[D:2 * D], torch.cat([t[:D], t[2 * D:]])


@pytest.mark.parametrize('name,tag', ALL_CASES, ids=CASE_IDS)
def test_fp32_matches_the_reference_run(name, tag):
    fx, logits, losses, grads, model = _two_steps(name, tag, torch.float32)
    args = MU.CASES[name][tag][1]
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (MU.BATCH, args['class_num'])
    worst = {'logits': _relmax(logits, fx['s0_logits'])}
    for s in range(MU.STEPS):
        worst['loss%d' % s] = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
    params = dict(model.named_parameters())
    assert sorted('s0_grad/' + n for n in params) == sorted(k for k in fx if k.startswith('s0_grad/'))
    zero = set(MU.zero_grad_names(params))
    init = MU.fixture_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    for n in params:
        g, ref = grads[n].detach().cpu().flatten(), torch.from_numpy(fx['s0_grad/' + n]).flatten()
        got = params[n].detach().cpu().flatten()
        fin = torch.from_numpy(fx['final/' + n]).flatten() if ('final/' + n) in fx else None
        if n in zero:
            # softmax is invariant to a constant added to a row of scores: what both sides compute for the key third is
            # rounding noise, which AdamW turns into steps of +-lr in either direction (tests/test_cait_gpu.py)
            gz, g = _zero_part(n, g)
            _rz, ref = _zero_part(n, ref)
            scale = float(grads[n.rsplit('.', 1)[0] + '.weight'].abs().max())       # the same layer's weight gradient
            assert float(gz.abs().max()) <= TOL_F32 * scale, n
            pz, got = _zero_part(n, got)
            iz, _ = _zero_part(n, init[n].flatten())
            assert float((pz - iz).abs().max()) <= 1.01 * MU.STEPS * MU.SOLVER['lr'], n
            if fin is not None:
                _fz, fin = _zero_part(n, fin)
        if float(ref.abs().max()) == 0.0:                    # a block dropped for every sample of the batch
            assert float(g.abs().max()) == 0.0, n
        else:
            worst['grad ' + n] = _relmax(g, ref)
        if fin is not None:
            worst['final ' + n] = _relmax(got, fin)
    for k in ('logits', 'loss0', 'loss1'):
        print('FIG %s/%s %-8s %.3e' % (name, tag, k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('FIG %s/%s worst %-6s %.3e (%s)' % (name, tag, kind, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v <= TOL_F32}
    assert not bad, bad


@pytest.mark.parametrize('name,tag', ALL_CASES, ids=CASE_IDS)
def test_bf16_loss(name, tag):
    fx, logits, losses, _grads, _model_ = _two_steps(name, tag, torch.bfloat16)
    assert bool(torch.isfinite(logits).all())
    for s in range(MU.STEPS):
        err = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
        print('FIG %s/%s bf16 loss%d %.3e (bound %.0e)' % (name, tag, s, err, TOL_BF16_LOSS))
        assert err <= TOL_BF16_LOSS


def test_fp32_parity_sees_the_keep_table_and_the_distillation_token():
    """The comparison discriminates: with two entries of the reference's keep table swapped, or with cls_token and
    dist_token exchanged, the logits are far outside the bound."""
    fx = _fixture('deit_small', 'dp5')
    model = _model('DeitVisionTransformer', MU.SMALL, 0.5).train()
    x, _ = MU.batches(MU.SMALL)[0]
    keep = torch.from_numpy(fx['s0_keep'])
    assert (keep == 0).any() and tuple(keep.shape) == (2 * MU.SMALL['depth'], MU.BATCH)
    row = int(np.flatnonzero(keep[:, 0].numpy() != keep[:, 1].numpy())[0])
    swapped = keep.clone()
    swapped[row] = keep[row].flip(0)
    with torch.no_grad():
        same = model(x.to(DEV), drop_path_keep=keep)
        other = model(x.to(DEV), drop_path_keep=swapped)
    assert _relmax(same, fx['s0_logits']) <= TOL_F32 < 10 * TOL_F32 < _relmax(other, fx['s0_logits'])
    dist = _model('DistilledVisionTransformer', MU.LONG, 0.0).eval()
    ref = _fixture('deit_long', 'dist')['s0_logits']
    xl = MU.batches(MU.LONG)[0][0].to(DEV)
    with torch.no_grad():
        assert _relmax(dist(xl), ref) <= TOL_F32
        c = dist.cls_token.detach().clone()
        dist.cls_token.copy_(dist.dist_token)
        dist.dist_token.copy_(c)
        dist.sync_runtime_state()
        assert _relmax(dist(xl), ref) > 10 * TOL_F32


def test_attention_routing_changes_nothing_up_to_the_dense_limit():
    """hnn.attention at T = 208 is ops.attention_fwd / _bwd bit for bit; at T = 209 it is the tiled pair; causal or
    key_bias beyond the limit raises by name."""
    from passl_amd.hip import nn as hnn, ops
    from passl_amd.hip.lib import PasslHipError
    B, H, DH = 2, 3, 64
    gen = torch.Generator().manual_seed(8)
    assert ops.ATTENTION_MAX_TOKENS == 208 and ops.ATTENTION_TILED_MAX_TOKENS == 1024
    for T, fwd, bwd in ((208, ops.attention_fwd, ops.attention_bwd), (209, ops.attention_tiled_fwd, ops.attention_tiled_bwd)):
        for dtype in (torch.float32, torch.bfloat16):
            qkv = torch.randn(B * T, 3 * H * DH, generator=gen).to(DEV, dtype).requires_grad_()
            dout = torch.randn(B * T, H * DH, generator=gen).to(DEV, dtype)
            out = hnn.attention(qkv, B, T, H, DH, DH ** -0.5)
            out.backward(dout)
            want, lse = fwd(qkv.detach(), B, T, H, DH, DH ** -0.5)
            assert torch.equal(_bits(out.detach()), _bits(want))
            assert torch.equal(_bits(qkv.grad), _bits(bwd(qkv.detach(), want, dout, lse, B, T, H, DH, DH ** -0.5)))
    qkv = torch.randn(B * 209, 3 * H * DH, generator=gen).to(DEV)
    with pytest.raises(PasslHipError):
        ops.attention_fwd(qkv, B, 209, H, DH, 0.125)                       # the dense kernels still refuse it
    with pytest.raises(NotImplementedError, match='causal'):
        hnn.attention(qkv, B, 209, H, DH, 0.125, causal=True)
    with pytest.raises(NotImplementedError, match='key_bias'):
        hnn.attention(qkv, B, 209, H, DH, 0.125, key_bias=torch.zeros(B, 209, device=DEV))
    with pytest.raises(PasslHipError):
        hnn.attention(torch.zeros(1025, 3 * H * DH, device=DEV), 1, 1025, H, DH, 0.125)


def test_evaluation_mode_ignores_drop_path_rate():
    x = MU.batches(MU.SMALL)[0][0].to(DEV)
    dropping, plain = _model('DeitVisionTransformer', MU.SMALL, 0.5).eval(), \
        _model('DeitVisionTransformer', MU.SMALL, 0.0, seed=2).eval()
    with torch.no_grad():
        a, b = dropping(x), plain(x)
    assert torch.equal(_bits(a), _bits(b))
    assert dropping.drop_path_draws == 0 and dropping.drop_path_step() == 0
    assert plain.train()(x).requires_grad and plain.drop_path_draws == 0       # rate 0: no draw in training either
    dropping.train()
    with torch.no_grad():
        c = dropping(x)
    assert dropping.drop_path_draws == 1 and dropping.drop_path_step() == 1
    assert dropping.drop_path_table(MU.BATCH).shape == (2 * MU.SMALL['depth'], MU.BATCH)
    assert bool((dropping.drop_path_table(MU.BATCH)[:2] == 1).all())           # block 0: rate 0, keep probability 1
    assert bool(torch.isfinite(c).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('factory', MU.FACTORIES)
def test_every_factory_trains_and_evaluates(factory, dtype):
    """One image through the full-size model: a training forward and backward with a gradient for every parameter, then
    an evaluation forward.  The two 384-pixel factories run 577 / 578 tokens through the key-tiled kernels."""
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(3)
    model = getattr(PM, factory)(class_num=16, drop_path_rate=0.1).train()
    size = 384 if factory.endswith('384') else 224
    x = torch.randn(1, 3, size, size, device=DEV)
    logits = model(x)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (1, 16)
    logits.square().sum().backward()
    torch.cuda.synchronize()
    assert model.drop_path_draws == 1
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(model.blocks[-1].attn.qkv.weight.grad.abs().max()) > 0
    assert float(model.pos_embed.grad.abs().max()) > 0 and float(model.cls_token.grad.abs().max()) > 0
    if 'distilled' in factory:
        assert float(model.dist_token.grad.abs().max()) > 0 and float(model.head_dist.weight.grad.abs().max()) > 0
    with torch.no_grad():
        out = model.eval()(x)
    assert bool(torch.isfinite(out).all()) and model.drop_path_draws == 1


def test_eager_and_plan_replayed_steps_of_the_long_distilled_model_are_bit_identical():
    """Four steps of the 227-token distilled model with rate 0.5: every launch of the step is the library's own (strict
    plan, nothing foreign: the tiled attention pair, the prefix-token pair, the logit mean), the counter lives on the
    device so each replay draws a fresh keep table, and losses and parameters equal the eager twin's bit for bit."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.loss.celoss import CELoss
    steps, seed = 4, (0x2012 << 32) + 7
    gen = torch.Generator().manual_seed(3)
    S = MU.LONG['img_size']
    batches = [(torch.randn(MU.BATCH, MU.LONG['in_chans'], S, S, generator=gen).to(DEV),
                torch.randint(0, MU.LONG['class_num'], (MU.BATCH,), generator=gen).to(DEV)) for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        model = _model('DistilledVisionTransformer', MU.LONG, 0.5).train()
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
    probs = [float(np.float32(1.0) - np.float32(r)) for r in MU.block_rates(0.5, MU.LONG['depth']) for _ in range(2)]
    for s in range(steps):
        assert np.array_equal(tb[s].numpy(), DP.keep_table(probs, MU.BATCH, seed, s)), 'step %d' % s


def test_engine_trains_and_evaluates_the_deit_yaml(tmp_path):
    """configs/v2/deit_base_patch16_224_synthetic.yaml shrunk to the distilled long model over the source's three channels
    (60-pixel images, 4-pixel patches: 227 tokens; bf16) through the Engine: two epochs with a finite, changing loss, the no-decay groups of the YAML, one draw per
    training pass, and the evaluation loop."""
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N, S = 8, 60
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'deit_base_patch16_224_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'LRScheduler.warmup_epoch=1',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 2), 'DataLoader.Train.dataset.image_size=%d' % S,
                      'DataLoader.Train.dataset.num_classes=8', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=%d' % S,
                      'DataLoader.Eval.dataset.num_classes=8', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'DeiT_base_patch16_224' and cfg['Model']['drop_path_rate'] == 0.1
    assert list(cfg['Optimizer']['no_weight_decay_name']) == MU.NO_DECAY
    cfg['Model'] = dict(name='DistilledVisionTransformer', drop_path_rate=0.1, drop_rate=0.0,
                        **dict(MU.LONG, in_chans=3, img_size=S, patch_size=4))
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'DistilledVisionTransformer' and type(eng.optimizer).__name__ == 'AdamW'
    assert eng.model.pos_embed.shape[1] == 227
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
