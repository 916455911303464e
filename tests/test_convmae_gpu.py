"""ConvMAE (passl_amd/models/convmae/) on the HIP path against the run of the reference's own conv_mae.py and
conv_vit.py (tests/golden/convmae_small.npz, convvit_small.npz, convvit_small_dp.npz;
tests/golden/make_golden_convmae.py), and as a whole step: a strict step plan against its eager twin, and one training
step and one evaluation of each full-size factory.

fp32: mask and ids_restore exactly; pred / logits, loss and EACH parameter gradient (relative to that gradient's own
maximum, which the fixture records next to the gradient's first elements) within the project's fp32 bound of 1e-3 of
the fixture, and every parameter after two AdamW steps within the same bound.  The product embeds and decodes the kept
patches only (gather, then GEMM) where the reference computes all patches and then gathers: the same bound covers it.
The key third of a qkv.bias, whose gradient is analytically zero, is held to AdamW's +-lr per step around its initial
value instead, as in the DeiT and CaiT model tests.
bf16: the losses within 3e-2, the bound of the other bf16 model tests."""
import math
from functools import partial

import numpy as np
import pytest
import torch

import convmae_model_util as MU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config              # noqa: E402
from passl_amd.hip import nn as hnn                         # noqa: E402

DEV = 'cuda'
TOL_F32 = 1e-3
TOL_BF16_LOSS = 3e-2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _build(kind, dtype=torch.float32, seed=1, **kw):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    norm = partial(hnn.LayerNorm, epsilon=MU.NORM_EPS)
    if kind == 'mae':
        model = PM.MaskedAutoencoderConvViT(norm_layer=norm, **MU.MAE_MODEL)
    else:
        model = PM.ConvViT(norm_layer=norm, **dict(MU.VIT_MODEL, **kw))
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(MU.fixture_state(keys), strict=False)
    assert not unexpected and set(missing) <= {'decoder_pos_embed'}, (missing, unexpected)
    return model


def _optimizer(model):
    from passl_amd.solver.optimizer import AdamW
    s = MU.SOLVER
    return AdamW(s['lr'], beta1=s['beta1'], beta2=s['beta2'], epsilon=s['epsilon'], weight_decay=s['weight_decay'],
                 parameters=list(model.parameters()))


def _relmax(got, ref, scale=None):
    """max |got - ref| over the recorded elements, relative to `scale` (default: the recorded maximum)."""
    got = torch.as_tensor(got).double().cpu().reshape(-1)
    ref = torch.as_tensor(np.asarray(ref)).double().reshape(-1)
    got = got[:ref.numel()] if got.numel() > ref.numel() else got
    assert got.numel() == ref.numel()
    scale = float(ref.abs().max()) if scale is None else float(scale)
    return float((got - ref).abs().max()) / max(scale, 1e-30)


def _zero_part(t):
    """The analytically-zero part of a qkv.bias (its key third) and the rest."""
    D = t.numel() // 3
    return t[D:2 * D], torch.cat([t[:D], t[2 * D:]])


def _compare(name, fx, prefix, head, losses, grads, model):
    worst = dict(head)
    for s in range(MU.STEPS):
        ref = float(fx[prefix + 's%d_loss' % s])
        worst['loss%d' % s] = abs(losses[s] - ref) / abs(ref)
    params = dict(model.named_parameters())
    assert sorted(prefix + 's0_grad/' + n for n in params) == \
        sorted(k for k in fx if k.startswith(prefix + 's0_grad/')), 'the trainable parameters differ'
    init = MU.fixture_state([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    for n in params:
        g, gref = grads[n].detach().cpu().flatten(), torch.from_numpy(fx[prefix + 's0_grad/' + n]).flatten()
        got, fin = params[n].detach().cpu().flatten(), torch.from_numpy(fx[prefix + 'final/' + n]).flatten()
        if n.endswith('attn.qkv.bias'):
            # softmax is invariant to a constant added to a row of scores: the gradient of the key third of a qkv.bias
            # is analytically zero, what both sides compute for it is rounding noise, and AdamW turns noise into steps
            # of +-lr in either direction (tests/test_deit_gpu.py, test_cait_gpu.py treat it the same way)
            (gz, g), (_rz, gref) = _zero_part(g), _zero_part(gref)
            scale = float(grads[n.rsplit('.', 1)[0] + '.weight'].abs().max())       # the same layer's weight gradient
            assert float(gz.abs().max()) <= TOL_F32 * scale, n
            (pz, got), (_fz, fin) = _zero_part(got), _zero_part(fin)
            iz, _ = _zero_part(init[n].flatten())
            assert float((pz - iz).abs().max()) <= 1.01 * MU.STEPS * MU.SOLVER['lr'], n
            worst['grad ' + n] = _relmax(g, gref)
        else:
            worst['grad ' + n] = _relmax(g, gref, fx[prefix + 's0_gmax/' + n])
        worst['final ' + n] = _relmax(got, fin)
    for k in list(head) + ['loss0', 'loss1']:
        print('FIG %s%s %-8s %.3e' % (name, prefix, k, worst[k]))
    for kind in ('grad', 'final'):
        k = max((k for k in worst if k.startswith(kind + ' ')), key=worst.get)
        print('FIG %s%s worst %-6s %.3e (%s)' % (name, prefix, kind, worst[k], k))
    return {k: v for k, v in worst.items() if not v <= TOL_F32}


# ------------------------------------------------------------------------------------------------ masked autoencoder
def _mae_two_steps(dtype):
    fx = MU.load('convmae_small')
    model = _build('mae', dtype).train()
    opt = _optimizer(model)
    losses, first = [], {}
    for step, (imgs, _y, noise) in enumerate(MU.batches()):
        loss, pred, mask = model(imgs.to(DEV), MU.MASK_RATIO, noise=noise.to(DEV))
        opt.clear_grad()
        loss.backward()
        if step == 0:
            first = dict(pred=pred.detach().clone(), mask=mask.detach().clone(),
                         grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return fx, first, losses, model


def test_convmae_fp32_matches_the_reference_run():
    fx, first, losses, model = _mae_two_steps(torch.float32)
    assert first['pred'].dtype == torch.float32 and tuple(first['pred'].shape) == (MU.BATCH, MU.L, MU.P)
    assert np.array_equal(first['mask'].cpu().numpy(), fx['s0_mask'])
    pred = first['pred'][:, :MU.PRED_ROWS].cpu()
    head = {'pred': _relmax(pred, fx['s0_pred'])}
    bad = _compare('convmae_small', fx, '', head, losses, first['grads'], model)
    assert not bad, bad
    assert 'pos_embed' in dict(model.named_parameters()), 'conv_mae.py leaves pos_embed trainable'
    assert float(first['grads']['pos_embed'].abs().max()) > 0
    assert 'decoder_pos_embed' not in dict(model.named_parameters())


def test_convmae_masking_is_the_reference_ranking():
    """ops.mae_mask on the fixture's noise gives the reference's ids_restore and mask (no ties in the noise)."""
    from passl_amd.hip import ops
    hip_config.set_device('gpu')
    fx = MU.load('convmae_small')
    ids_keep, ids_restore, mask = ops.mae_mask(torch.from_numpy(fx['s0_noise']).to(DEV), MU.K)
    assert np.array_equal(ids_restore.cpu().numpy(), fx['s0_ids_restore'])
    assert np.array_equal(mask.cpu().numpy(), fx['s0_mask'])
    assert int((mask == 0).sum()) == MU.BATCH * MU.K


def test_convmae_parity_sees_the_mask():
    """The comparison discriminates: with another mask the prediction is far outside the bound (the loss of an
    untrained model hardly depends on which patches are removed; the prediction does)."""
    fx = MU.load('convmae_small')
    model = _build('mae').train()
    imgs, _y, noise = MU.batches()[0]
    with torch.no_grad():
        _loss, pred, mask = model(imgs.to(DEV), MU.MASK_RATIO, noise=noise.flip(1).to(DEV))
    assert not np.array_equal(mask.cpu().numpy(), fx['s0_mask'])
    assert _relmax(pred[:, :MU.PRED_ROWS].cpu(), fx['s0_pred']) > 10 * TOL_F32


def test_convmae_bf16_loss():
    fx, first, losses, _model = _mae_two_steps(torch.bfloat16)
    assert bool(torch.isfinite(first['pred']).all())
    for s in range(MU.STEPS):
        err = abs(losses[s] - float(fx['s%d_loss' % s])) / abs(float(fx['s%d_loss' % s]))
        print('FIG convmae_small bf16 loss%d %.3e (bound %.0e)' % (s, err, TOL_BF16_LOSS))
        assert err <= TOL_BF16_LOSS


def test_convmae_eager_and_plan_replayed_steps_are_bit_identical():
    """Four pre-training steps: every launch of the step is the library's own (strict plan, nothing foreign), the noise
    is drawn afresh at every replay (a live host call), and losses, masks and parameters equal the eager twin's bit
    for bit."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    steps = 4
    gen = torch.Generator().manual_seed(3)
    batches = [torch.randn(MU.BATCH, 3, MU.IMG, MU.IMG, generator=gen).to(DEV) for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        model = _build('mae').train()
        opt = _optimizer(model)
        torch.manual_seed(77)
        torch.cuda.manual_seed(77)                       # the noise of random_masking

        def full_step(x):
            loss, _pred, mask = model(x, MU.MASK_RATIO)
            opt.clear_grad()
            loss.backward(ops.ones_like_cached(loss))
            opt.step()
            return dict(loss=loss, mask=mask)
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, masks = [], []
        for x in batches:
            out = sp.run(x)
            losses.append(out['loss'].detach().clone().reshape(1))
            masks.append(out['mask'].detach().clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        results[mode] = (torch.cat(losses).cpu(), torch.stack(masks).cpu(),
                         model.arena_q.flat[:model.arena_q.n_train].clone().cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, ma, fa), (lb, mb, fb) = results['eager'], results['plan']
    assert torch.equal(ma, mb), 'the replayed steps drew other masks than the eager ones'
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(fa), _bits(fb))
    assert all(math.isfinite(float(v)) for v in lb)
    assert len({tuple(m.flatten().tolist()) for m in mb}) == steps, 'the mask must differ from step to step'


# ------------------------------------------------------------------------------------------------ classifier
def _keep_table(fx, prefix, step):
    """The reference's keep decisions as the model's table [2 * blocks, B]: block 0 (p = 0) owns two rows of ones."""
    k = prefix + 's%d_keep' % step
    if k not in fx:
        return None
    keep = torch.from_numpy(fx[k])
    return torch.cat([torch.ones(2, keep.shape[1]), keep], 0)


def _vit_two_steps(name, prefix, pool, dtype):
    from passl_amd.loss.celoss import CELoss
    fx = MU.load(name)
    model = _build('vit', dtype, drop_path_rate=float(fx['rate']), global_pool=pool).train()
    opt, celoss = _optimizer(model), CELoss()
    losses, grads, logits0 = [], {}, None
    for step, (x, y, _noise) in enumerate(MU.batches()):
        logits = model(x.to(DEV), drop_path_keep=_keep_table(fx, prefix, step))
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


@pytest.mark.parametrize('prefix,pool', MU.POOLS, ids=[p[0].strip('/') for p in MU.POOLS])
@pytest.mark.parametrize('name', sorted(MU.VIT_CASES))
def test_convvit_fp32_matches_the_reference_run(name, prefix, pool):
    fx, logits, losses, grads, model = _vit_two_steps(name, prefix, pool, torch.float32)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (MU.BATCH, MU.VIT_MODEL['num_classes'])
    names = set(dict(model.named_parameters()))
    assert ('fc_norm.weight' in names) == pool and ('norm.weight' in names) == (not pool)
    bad = _compare(name, fx, prefix, {'logits': _relmax(logits, fx[prefix + 's0_logits'])}, losses, grads, model)
    assert not bad, bad


def test_convvit_parity_sees_the_keep_table():
    fx = MU.load('convvit_small_dp')
    model = _build('vit', drop_path_rate=0.5).train()
    keep = _keep_table(fx, 'tok/', 0)
    assert (keep == 0).any()
    x = MU.batches()[0][0].to(DEV)
    with torch.no_grad():
        other = model(x, drop_path_keep=torch.ones_like(keep))
    assert _relmax(other, fx['tok/s0_logits']) > 10 * TOL_F32


@pytest.mark.parametrize('name', sorted(MU.VIT_CASES))
def test_convvit_bf16_loss(name):
    fx, logits, losses, _grads, _model_ = _vit_two_steps(name, 'tok/', False, torch.bfloat16)
    assert bool(torch.isfinite(logits).all())
    for s in range(MU.STEPS):
        err = abs(losses[s] - float(fx['tok/s%d_loss' % s])) / abs(float(fx['tok/s%d_loss' % s]))
        print('FIG %s bf16 loss%d %.3e (bound %.0e)' % (name, s, err, TOL_BF16_LOSS))
        assert err <= TOL_BF16_LOSS


def test_convvit_evaluation_mode_ignores_drop_path_rate():
    x = MU.batches()[0][0].to(DEV)
    dropping, plain = _build('vit', drop_path_rate=0.5).eval(), _build('vit', seed=2).eval()
    with torch.no_grad():
        a, b = dropping(x), plain(x)
    assert torch.equal(_bits(a), _bits(b))
    assert dropping.drop_path_draws == 0
    dropping.train()
    with torch.no_grad():
        c = dropping(x)
    assert dropping.drop_path_draws == 1 and dropping.drop_path_step() == 1
    assert dropping.drop_path_table(MU.BATCH).shape == (2 * sum(MU.STAGES['depth']), MU.BATCH)
    assert bool(torch.isfinite(c).all())


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_factories_train_and_evaluate_in_bf16():
    """One training step and one evaluation of convmae_convvit_base_patch16 and convvit_base_patch16 at batch 2."""
    import passl.models as PM
    from passl_amd.loss.celoss import CELoss
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 224, 224, generator=gen).to(DEV)
    y = torch.tensor([3, 977]).to(DEV)

    model = PM.convmae_convvit_base_patch16(norm_pix_loss=True).train()
    opt = _optimizer(model)
    before = model.arena_q.flat[:model.arena_q.n_train].clone()
    loss, pred, mask = model(x, 0.75)
    opt.clear_grad()
    loss.backward()
    opt.step()
    assert tuple(pred.shape) == (2, 196, 768) and tuple(mask.shape) == (2, 196) and int(mask.sum()) == 2 * 147
    assert math.isfinite(float(loss)) and float(loss) > 0
    g = model.arena_q.grads
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert not torch.equal(before, model.arena_q.flat[:model.arena_q.n_train])
    model.eval()
    with torch.no_grad():
        loss2, _p, _m = model(x, 0.75)
    assert math.isfinite(float(loss2))
    del model, opt, before, g
    torch.cuda.empty_cache()

    model = PM.convvit_base_patch16(drop_path_rate=0.1).train()
    opt = _optimizer(model)
    logits = model(x)
    loss = CELoss()(logits, y)['CELoss']
    opt.clear_grad()
    loss.backward()
    opt.step()
    assert tuple(logits.shape) == (2, 1000) and logits.dtype == torch.float32
    assert math.isfinite(float(loss)) and model.drop_path_draws == 1
    assert bool(torch.isfinite(model.arena_q.grads).all())
    model.eval()
    with torch.no_grad():
        out = model(x)
    assert bool(torch.isfinite(out).all()) and model.drop_path_draws == 1


# ------------------------------------------------------------------------------------------------ the YAML
def test_trainer_trains_the_convmae_yaml(tmp_path):
    """configs/mae/convmae_convvit_b_synthetic.yaml at a reduced size through the v110 Trainer (64-pixel images, a
    4 x 4 patch grid, small widths, bf16, three epochs of eight iterations over one cached batch): AdamW, the warm-up,
    and a loss that falls."""
    import os
    from passl_amd.engine.trainer import Trainer
    from passl_amd.utils.config import get_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_config(os.path.join(root, 'configs/mae/convmae_convvit_b_synthetic.yaml'),
                     ['dataloader.train.sampler.batch_size=8', 'dataloader.train.dataset.image_size=64',
                      'dataloader.train.dataset.num_samples=64', 'epochs=3', 'model.architecture.num_heads=2',
                      'model.architecture.decoder_embed_dim=64', 'model.architecture.decoder_depth=1',
                      'model.architecture.decoder_num_heads=2', 'lr_scheduler.warmup_steps=1',
                      'lr_scheduler.learning_rate.learning_rate=2e-3', 'lr_scheduler.end_lr=2e-3',
                      'output_dir=%s' % tmp_path, 'log_config.interval=4'])
    arch = cfg.model.architecture
    assert arch.name == 'ConvMAE' and list(arch.embed_dim) == [256, 384, 768] and list(arch.depth) == [2, 2, 11]
    assert cfg.model.mask_ratio == 0.75 and arch.norm_pix_loss is True and cfg.optimizer.beta2 == 0.95
    arch.img_size, arch.embed_dim, arch.depth = [64, 16, 8], [16, 24, 64], [1, 1, 2]
    cfg.timestamp = ''
    tr = Trainer(cfg)
    assert type(tr.model.backbone).__name__ == 'ConvMAE' and tr.model.arena_q.dtype == torch.bfloat16
    assert tr.optimizer.type == 'adamw' and tr.iters_per_epoch == 8
    data = next(iter(tr.train_dataloader))
    tr.model.train()
    l0 = float(tr.model(*data)['loss'].detach())
    tr.train()
    assert tr.current_iter == 24
    l1 = float(tr.outputs['loss'].detach())
    assert np.isfinite(l1) and l1 < l0, (l0, l1)           # one cached batch: it must be fitted
