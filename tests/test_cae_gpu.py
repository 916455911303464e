"""CAE pre-training (passl_amd/models/cae.py, engine/loops/cae_pretrain_loop.py) on the HIP path against the run of the
reference's own cae.py (tests/golden/cae_small.npz; tests/golden/make_golden_cae.py), and as a whole step: a strict step
plan against its eager twin, and the loop.

fp32: the first rows of logits, latent_pred and latent_target, loss_main / loss_aux / loss of both steps, EACH parameter
gradient of step 0 (relative to that gradient's own maximum, which the fixture records) and every student and teacher
parameter after two clipped AdamW steps within the project's fp32 bound of 1e-3 of the fixture.  The gradient of a
regressor block's ``norm1_k_cross.bias`` is analytically zero (softmax does not see a constant added to every key); it
is held to the bound relative to the same layer's weight gradient, on both sides, instead of to its own noise.
Measured (fp32): logits, latents and losses within 8e-7, parameters after the two steps within 4e-5 of the fixture.
bf16: the losses within 3e-2, the bound of the other bf16 model tests.
Model m1 has dual_path_ema 0; m2 has 0.5 and a decoder of another width (encoder_to_decoder and its norm run, on the
teacher's output too)."""
import math
from functools import partial

import numpy as np
import pytest
import torch

import cae_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402
from passl_amd.hip import nn as hnn                         # noqa: E402

DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _build(name, dtype=torch.float32, seed=1):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    model = PM.CAEPretrain(norm_layer=partial(hnn.LayerNorm, epsilon=MU.NORM_EPS), args=MU.args_of(name), **MU.MODEL_KW)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(MU.fixture_state(keys), strict=False)
    assert not unexpected and set(missing) == {'encoder.pos_embed', 'teacher_network.pos_embed'}, (missing, unexpected)
    return model


def _optimizer(model):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm
    from passl_amd.engine.loops.cae_pretrain_loop import param_groups
    from passl_amd.solver.optimizer import AdamW
    s = MU.SOLVER
    groups = param_groups(model, s['weight_decay'])
    names = {id(p): n for n, p in model.named_parameters()}
    no_decay, _decay = MU.decay_groups([(n, tuple(p.shape)) for n, p in model.named_parameters()
                                        if 'teacher' not in n and p.requires_grad])
    assert sorted(names[id(p)] for p in groups[0]['params']) == sorted(no_decay)
    return AdamW(s['lr'], beta1=s['beta1'], beta2=s['beta2'], epsilon=s['epsilon'], parameters=groups,
                 grad_clip=ClipGradByGlobalNorm.like_clip_grad_norm_(s['clip_grad']))


def _relmax(got, ref, scale=None):
    got = torch.as_tensor(got).double().cpu().reshape(-1)
    ref = torch.as_tensor(np.asarray(ref)).double().reshape(-1)
    got = got[:ref.numel()] if got.numel() > ref.numel() else got
    assert got.numel() == ref.numel()
    scale = float(ref.abs().max()) if scale is None else float(scale)
    return float((got - ref).abs().max()) / max(scale, 1e-30)


def _two_steps(name, dtype):
    from passl_amd.engine.loops.cae_pretrain_loop import forward_backward
    fx = {k[len(name) + 1:]: v for k, v in MU.load().items() if k.startswith(name + '/')}
    masks = MU.load()['masks']
    model = _build(name, dtype).train()
    opt = _optimizer(model)
    w = MU.SOLVER['dual_loss_weight']
    losses, first = [], {}
    for step, (imgs, mask, labels) in enumerate(MU.batches(masks)):
        opt.clear_grad()
        if step == 0:                       # the model's outputs, then the step itself through the loop's function
            with torch.no_grad():
                model.eval()
                logits, lp, lt = model(imgs.to(DEV), mask.float().to(DEV), num_masked=MU.NM)
                model.train()
            first = dict(logits=logits.clone(), latent_pred=lp.clone(), latent_target=lt.clone())
        lm, mse = forward_backward(model, imgs.to(DEV), mask.float().to(DEV), labels.to(DEV), MU.NM, w)
        if step == 0:
            first['grads'] = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
        opt.step()
        losses.append((float(lm.detach()), w * float(mse.detach())))
    torch.cuda.synchronize()
    return fx, first, losses, model


@pytest.mark.parametrize('name', list(MU.MODELS))
def test_cae_fp32_matches_the_reference_run(name):
    fx, first, losses, model = _two_steps(name, torch.float32)
    C = MU.args_of(name).decoder_embed_dim
    assert first['logits'].dtype == torch.float32 and tuple(first['logits'].shape) == (MU.BATCH * MU.NM, MU.VOCAB)
    assert tuple(first['latent_pred'].shape) == tuple(first['latent_target'].shape) == (MU.BATCH, MU.NM, C)
    worst = {'logits': _relmax(first['logits'][:MU.ROWS], fx['s0_logits']),
             'latent_pred': _relmax(first['latent_pred'][:, :MU.ROWS], fx['s0_latent_pred']),
             'latent_target': _relmax(first['latent_target'][:, :MU.ROWS], fx['s0_latent_target'])}
    for s, (lm, la) in enumerate(losses):
        for k, v in (('loss_main', lm), ('loss_aux', la), ('loss', lm + la)):
            ref = float(fx['s%d_%s' % (s, k)])
            worst['%s%d' % (k, s)] = abs(v - ref) / abs(ref)
    params = dict(model.named_parameters())
    student = {n: p for n, p in params.items() if p.requires_grad}
    assert sorted('s0_grad/' + n for n in student) == sorted(k for k in fx if k.startswith('s0_grad/')), \
        'the trainable parameters differ'
    assert sorted('final/' + n for n in params) == sorted(k for k in fx if k.startswith('final/'))
    for n in student:
        if n.endswith('norm1_k_cross.bias'):
            # a constant added to every key moves every score of a query row alike and the softmax does not see it:
            # this gradient is analytically zero, what either side computes for it is rounding noise (the key third of a
            # qkv.bias in the DeiT, CaiT and ConvMAE model tests is the same case) — both are held to the bound relative
            # to the same layer's weight gradient
            scale = float(fx['s0_gmax/' + n[:-len('bias')] + 'weight'])
            assert float(first['grads'][n].abs().max()) <= TOL_F32 * scale, n
            assert float(fx['s0_gmax/' + n]) <= TOL_F32 * scale, n
            continue
        worst['grad ' + n] = _relmax(first['grads'][n], fx['s0_grad/' + n], fx['s0_gmax/' + n])
    for n, p in params.items():
        worst['final ' + n] = _relmax(p.detach(), fx['final/' + n])
    for k in [k for k in worst if not k.startswith(('grad ', 'final '))]:
        print('FIG cae_%s %-14s %.3e' % (name, k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('FIG cae_%s worst %-6s %.3e (%s)' % (name, kind, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v <= TOL_F32}
    assert not bad, bad
    assert sorted(n for n in student if n.endswith(('q_bias', 'v_bias')))       # the biases are parameters with gradients
    assert not any(n.endswith('qkv.bias') for n in params)


def test_teacher_lags_the_student_by_one_step_at_ema_0():
    """After step 2's forward the teacher holds the student's parameters of step 2's forward = after ONE update."""
    from passl_amd.engine.loops.cae_pretrain_loop import forward_backward
    masks = MU.load()['masks']
    model = _build('m1').train()
    opt = _optimizer(model)
    o, n = model._enc
    snaps = []
    for imgs, mask, labels in MU.batches(masks):
        opt.clear_grad()
        snaps.append(model.arena_q.flat[o:o + n].clone())                       # the student before this step's update
        forward_backward(model, imgs.to(DEV), mask.float().to(DEV), labels.to(DEV), MU.NM, 2.0)
        opt.step()
    assert torch.equal(model.arena_k.flat[:n], snaps[1]), 'the teacher is not the student after one step'
    assert not torch.equal(snaps[1], snaps[0]) and not torch.equal(model.arena_q.flat[o:o + n], snaps[1])


def test_evaluation_mode_launches_no_ema():
    masks = MU.load()['masks']
    model = _build('m2').eval()
    with torch.no_grad():
        model.arena_q.flat[:model.arena_q.n_train].mul_(1.5)                     # student and teacher now differ
    before = model.arena_k.flat.clone()
    imgs, mask, _labels = MU.batches(masks)[0]
    with torch.no_grad():
        logits, _lp, _lt = model(imgs.to(DEV), mask.float().to(DEV), num_masked=MU.NM)
    assert bool(torch.isfinite(logits).all())
    assert torch.equal(model.arena_k.flat, before)
    model.train()
    with torch.no_grad():
        model(imgs.to(DEV), mask.float().to(DEV), num_masked=MU.NM)
    assert not torch.equal(model.arena_k.flat, before), 'training mode must update the teacher'


def test_a_bool_mask_and_no_count_give_the_same_outputs():
    masks = MU.load()['masks']
    model = _build('m1').eval()
    imgs, mask, _labels = MU.batches(masks)[0]
    with torch.no_grad():
        a = model(imgs.to(DEV), mask.float().to(DEV), num_masked=MU.NM)
        b = model(imgs.to(DEV), mask.to(DEV))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize('name', list(MU.MODELS))
def test_cae_bf16_losses(name):
    fx, first, losses, _model = _two_steps(name, torch.bfloat16)
    assert bool(torch.isfinite(first['logits']).all())
    for s, (lm, la) in enumerate(losses):
        for k, v in (('loss_main', lm), ('loss_aux', la), ('loss', lm + la)):
            ref = float(fx['s%d_%s' % (s, k)])
            err = abs(v - ref) / abs(ref)
            print('FIG cae_%s bf16 %s%d %.3e (bound %.0e)' % (name, k, s, err, TOL_BF16_LOSS))
            assert err <= TOL_BF16_LOSS


def test_cae_eager_and_plan_replayed_steps_are_bit_identical():
    """Four pre-training steps with images, mask and labels as the plan's inputs and a different mask each step: every
    launch of the step is the library's own (strict plan, nothing foreign), and losses and student and teacher
    parameters equal the eager twin's bit for bit."""
    from passl_amd.engine.loops.cae_pretrain_loop import forward_backward
    from passl_amd.hip.replay import StepPlan
    steps = 4
    gen = torch.Generator().manual_seed(3)
    masks = MU.block_masks(steps * MU.BATCH, seed=5)
    batches = []
    for s in range(steps):
        m = torch.from_numpy(masks[s * MU.BATCH:(s + 1) * MU.BATCH]).bool()
        ids = torch.randint(0, MU.VOCAB, (MU.BATCH, MU.L), generator=gen)
        batches.append((torch.randn(MU.BATCH, 3, MU.IMG, MU.IMG, generator=gen).to(DEV), m.float().to(DEV),
                        ids[m].to(DEV)))
    assert len({tuple(b[1].flatten().tolist()) for b in batches}) == steps, 'the mask must differ from step to step'
    results = {}
    for mode in ('eager', 'plan'):
        model = _build('m2').train()
        opt = _optimizer(model)

        def full_step(x, mask, labels):
            opt.clear_grad()
            lm, mse = forward_backward(model, x, mask, labels, MU.NM, 2.0)
            opt.step()
            return dict(loss_main=lm, mse=mse)
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses = []
        for b in batches:
            out = sp.run(*b)
            losses.append(torch.cat([out['loss_main'].detach().reshape(1), out['mse'].detach().reshape(1)]).clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        results[mode] = (torch.stack(losses).cpu(), model.arena_q.flat[:model.arena_q.n_train].clone().cpu(),
                         model.arena_k.flat.clone().cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, qa, ka), (lb, qb, kb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(qa), _bits(qb)) and torch.equal(_bits(ka), _bits(kb))
    assert all(math.isfinite(float(v)) for v in lb.flatten())


def test_the_loop_runs_two_iterations():
    from passl_amd.datasets.synthetic import SyntheticLoader, SyntheticMaskedTokens
    from passl_amd.engine.loops.cae_pretrain_loop import build_optimizer, train_one_epoch
    from passl_amd.models.cae import cae_pretrain_args
    model = _build('m1').train()
    args = cae_pretrain_args(lr=1e-3, warmup_epochs=1, epochs=2, clip_grad=3.0, print_freq=1, num_mask_patches=MU.NM)
    ds = SyntheticMaskedTokens(num_samples=2 * MU.BATCH, image_size=MU.IMG, patch_size=MU.PATCH, vocab_size=MU.VOCAB,
                               num_mask_patches=MU.NM, min_mask_patches_per_block=4, num_batches_cached=2, seed=3)
    loader = SyntheticLoader(ds, MU.BATCH, torch.device(DEV))
    assert len(loader) == 2 and ds.num_masked == MU.NM
    seen = []
    for images, mask, labels in loader:
        assert mask.dtype == torch.float32 and tuple(mask.shape) == (MU.BATCH, MU.L)
        assert labels.dtype == torch.int64 and tuple(labels.shape) == (MU.BATCH * MU.NM,)
        assert bool((mask.sum(1) == MU.NM).all())
        seen.append(mask.clone())
    assert not torch.equal(seen[0], seen[1])
    opt, _sched = build_optimizer(model, args, len(loader))
    before = model.arena_q.flat.clone()
    lines = []
    out = train_one_epoch(model, loader, opt, 1, args, log=lines.append)
    assert len(lines) == 2 and math.isfinite(out['loss']) and out['loss'] > 0
    assert abs(out['loss'] - (out['loss_main'] + out['loss_aux'])) < 1e-6 * out['loss']
    assert out['lr'] > 0 and not torch.equal(model.arena_q.flat, before)
    with pytest.raises(NotImplementedError):
        train_one_epoch(model, loader, opt, 0, cae_pretrain_args(target_mode='rgb'))
    with pytest.raises(NotImplementedError):
        train_one_epoch(model, loader, opt, 0, cae_pretrain_args(dual_loss_type='kld'))
