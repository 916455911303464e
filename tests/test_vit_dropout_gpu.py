"""``VisionTransformer(drop_rate=...)`` on the MI355X: logits and every parameter gradient against a float64 ViT fed the
host masks of the same (seed, step, sites) — tests/dropout_util.py —, the step counter, evaluation mode, the refusal of
a stale backward, eager versus plan-replayed steps, and the supervised ViT YAML through the Engine."""
import math
import os
from functools import partial

import numpy as np
import pytest
import torch

import dropout_util as DU

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config      # noqa: E402

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 17 tokens.  16 classes: the GEMM kernels write 16-byte rows, so a head needs a multiple of 8 (10 classes construct
# and then fail at the first forward with or without dropout)
ARCH = dict(img_size=64, patch_size=16, embed_dim=64, depth=2, num_heads=2, class_num=16)
RATE, BATCH, EPS = 0.1, 3, 1e-5
SEED = (0x51 << 32) + 0x7e57
# tests/test_mae_gpu.py TOL_F32 for a ViT of this size in fp32: predictions and gradients, relative to max |reference|
TOL = dict(pred=1e-3, grad=1e-3)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _model(drop_rate=RATE, seed=1):
    import passl.models as PM
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    torch.manual_seed(seed)
    model = PM.VisionTransformer(drop_rate=drop_rate, **ARCH)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():                     # the constructor's head and class token are zeros: give them a signal
        for n, p in model.named_parameters():
            if n.startswith('head') or n == 'cls_token':
                p.copy_(torch.randn(p.shape, generator=gen).to(DEV) * 0.1)
    model.sync_runtime_state()
    return model


def _relmax(got, ref):
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def test_logits_and_gradients_against_float64_with_the_host_masks():
    model = _model().train()
    step0 = (1 << 32) + 4                                          # the pass below runs at step0 + 1
    model.set_dropout_seed(SEED, step=step0)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(BATCH, 3, 64, 64, generator=gen)
    w = torch.randn(BATCH, ARCH['class_num'], generator=gen)
    out = model(x.to(DEV))
    assert out.dtype == torch.float32 and tuple(out.shape) == (BATCH, ARCH['class_num'])
    (out * w.to(DEV)).sum().backward()
    step = model.dropout_step()
    assert step == step0 + 1

    def reference(site_shift):
        params = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
        ref = DU.vit_fp64(params, x, ARCH['depth'], ARCH['num_heads'], ARCH['patch_size'], EPS,
                          drop=DU.site_dropper(RATE, SEED, step, site_shift))
        (ref * w.double()).sum().backward()
        return ref.detach(), params
    ref, params = reference(0)
    got = out.detach().double().cpu()
    err = _relmax(got, ref)
    print('logits: %.3e of max (bound %.0e)' % (err, TOL['pred']))
    worst = {}
    for n, p in model.named_parameters():
        assert params[n].grad is not None and p.grad is not None, n
        worst[n] = _relmax(p.grad.double().cpu(), params[n].grad)
        print('grad %-28s %.3e of max' % (n, worst[n]))
    assert err < TOL['pred']
    assert all(v < TOL['grad'] for v in worst.values()), {n: v for n, v in worst.items() if v >= TOL['grad']}
    # the comparison discriminates: the masks of the neighbouring site numbers, or no masks at all, are far outside
    shifted, _ = reference(1)
    print('site ids shifted by one: %.3e of max' % _relmax(got, shifted))
    assert _relmax(got, shifted) > 10 * TOL['pred']
    plain = DU.vit_fp64({k: v.detach() for k, v in params.items()}, x, ARCH['depth'], ARCH['num_heads'],
                        ARCH['patch_size'], EPS)
    assert _relmax(got, plain) > 10 * TOL['pred']


def test_step_counter_eval_mode_and_stale_backward():
    model = _model().train()
    model.set_dropout_seed(SEED)
    x = torch.randn(BATCH, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    outs = []
    for k in range(1, 4):
        outs.append(model(x).detach().clone())
        assert model.dropout_step() == k
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])      # step 1, 2, 3: other masks
    thr = model._dropout.thr
    assert not np.array_equal(DU.keep_mask(8 * 1024, SEED, 1, 0, thr), DU.keep_mask(8 * 1024, SEED, 2, 0, thr))
    model.set_dropout_seed(SEED)                                   # the same seed and step: the same bits again
    assert torch.equal(_bits(model(x).detach()), _bits(outs[0]))
    # evaluation: no advance, no mask — bit-equal to a model built without dropout holding the same weights
    model.eval()
    plain = _model(drop_rate=0.0, seed=2)
    plain.load_state_dict(model.state_dict())
    for m in (plain.eval(), plain.train()):
        assert torch.equal(_bits(model(x).detach()), _bits(m(x).detach()))
    assert model.dropout_step() == 1 and plain.dropout_step() == 0
    # two training forwards before a backward: the counter has moved past the first one's masks
    model.train()
    first = model(x)
    model(x)
    with pytest.raises(RuntimeError, match='dropout backward of training pass'):
        first.sum().backward()


# ---------------------------------------------------------------------------------------------- replay
def _tiny_step_model(dim, heads, classes, B, T, seed):
    """pos_drop, two Blocks with dropout, LayerNorm over the class rows, a Linear head, the sigmoid cross entropy: the
    smallest step with every dropout launch that records without a foreign launch (as tests/test_droppath_gpu.py's)."""
    from passl_amd.hip import nn
    from passl_amd.loss.celoss import _SigmoidCEFn
    from passl_amd.modules.vit import Block, trunc_normal_

    class Tiny(nn.Layer):
        def __init__(self):
            super().__init__()
            norm = partial(nn.LayerNorm, epsilon=1e-6)
            self.state = nn.DropoutState(RATE, seed=seed)
            self.pos_drop = nn.Dropout(RATE).bind(self.state, 0)
            self.blocks = torch.nn.ModuleList([Block(dim, heads, 4., qkv_bias=True, norm_layer=norm, drop=RATE)
                                               for _ in range(2)])
            for i, blk in enumerate(self.blocks):
                blk.bind_dropout(self.state, 1 + 3 * i)
            self.norm = norm(dim)
            self.head = nn.Linear(dim, classes)
            with torch.no_grad():
                for m in self.modules():
                    if isinstance(m, nn.Linear):
                        trunc_normal_(m.weight, std=0.02)
            self.arena_q = nn.EncoderArena(self, trainable=True)
            self.cls_rows = (torch.arange(B, dtype=torch.int32, device=DEV) * T).contiguous()

        def forward(self, x, labels):
            self.arena_q.refresh()
            self.state.begin_pass(x.device)
            x = self.pos_drop(x)
            seen = x
            for blk in self.blocks:
                x = blk(x, B, T)
            scores = self.head(self.norm(nn.gather_rows(x, self.cls_rows)), out_f32=True)
            return dict(loss=_SigmoidCEFn.apply(scores, labels, 1.0, 0.0), pos_drop=seen)
    return Tiny()


def test_eager_and_plan_replayed_steps_are_bit_identical():
    """The advance launch and every mask launch are recorded with their argument bytes; the counter lives on the device,
    so each replay draws the masks of the next step: losses, parameters and the zero pattern after pos_drop equal the
    eager twin's, and the pattern is the restatement's for steps 1, 2, 3, 4."""
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    B, T, dim, classes, steps = 16, 17, 128, 16, 4
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(B * T, dim, generator=gen).to(DEV), torch.randint(0, classes, (B,), generator=gen).to(DEV))
               for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        torch.manual_seed(9)
        model = _tiny_step_model(dim, 4, classes, B, T, SEED)
        model.train()
        opt = AdamW(1e-3, weight_decay=0.05, parameters=list(model.parameters()))

        def full_step(x, y):
            out = model(x, y)
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            opt.step()
            return out
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, seen = [], []
        for x, y in batches:
            out = sp.run(x, y)
            losses.append(out['loss'].detach().clone().reshape(1))
            seen.append(out['pos_drop'].detach().clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        assert model.state.step() == steps
        results[mode] = (torch.cat(losses).cpu(), torch.stack(seen).cpu(),
                         model.arena_q.flat[:model.arena_q.n_train].clone().cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, sa, fa), (lb, sb, fb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(fa), _bits(fb)) and torch.equal(_bits(sa), _bits(sb))
    thr, _factor = DU.thr_factor(RATE)
    for s in range(steps):
        keep = DU.keep_mask(B * T * dim, SEED, s + 1, 0, thr)
        assert np.array_equal(sb[s].reshape(-1).numpy() != 0, keep), 'step %d' % (s + 1)


# ---------------------------------------------------------------------------------------------- the YAML
def test_engine_trains_the_supervised_vit_yaml(tmp_path):
    """configs/v2/vit_base_sup_synthetic.yaml at a reduced size through the Engine: ViTCELoss, ViTLRScheduler, AdamW
    with global-norm clipping, two accumulated micro-batches per step, bf16 compute (FP16 O2) — two steps, four
    training passes, a finite loss."""
    from passl.engine.engine import Engine
    from passl_amd.utils.config import get_config
    N, steps = 8, 2
    cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_sup_synthetic.yaml'),
                     ['Global.epochs=2', 'Global.output_dir=%s' % tmp_path, 'Global.print_batch_step=1',
                      'Global.eval_during_train=False', 'LRScheduler.warmup_steps=3',
                      'DataLoader.Train.dataset.num_samples=%d' % (N * 4), 'DataLoader.Train.dataset.image_size=64',
                      'DataLoader.Train.dataset.num_classes=16', 'DataLoader.Train.sampler.batch_size=%d' % N,
                      'DataLoader.Eval.dataset.num_samples=%d' % N, 'DataLoader.Eval.dataset.image_size=64',
                      'DataLoader.Eval.dataset.num_classes=16', 'DataLoader.Eval.sampler.batch_size=%d' % N])
    assert cfg['Model']['name'] == 'ViT_base_patch16_224' and cfg['Model']['drop_rate'] == 0.1
    cfg['Model'] = dict(name='VisionTransformer', drop_rate=cfg['Model']['drop_rate'], qkv_bias=True, epsilon=1e-6,
                        representation_size=64, **ARCH)
    cfg['Global']['max_train_step'] = steps
    eng = Engine(cfg, mode='train')
    assert type(eng.model).__name__ == 'VisionTransformer' and eng.model.drop_rate == 0.1
    assert type(eng.lr_scheduler).__name__ == 'ViTLRScheduler' and eng.lr_scheduler.warmup_steps == 3
    assert type(eng.train_loss_func.loss_func[0]).__name__ == 'ViTCELoss' and eng.accum_steps == 2
    assert eng.optimizer._clip is not None
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
    assert lrs[0] == 0.0 and abs(lrs[1] - 3e-3 / 3) < 1e-15            # last_epoch 0, then lr_step(1)
    assert eng.model.dropout_step() == steps * 2                       # one advance per micro-batch
