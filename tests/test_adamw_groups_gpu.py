"""AdamW parameter groups on the MI355X: the grouped kernel bit for bit against the flat kernel (a uniform table =
the flat launch; every segment = the flat kernel on that slice alone), refused arguments, parity with the reference's
fine-tuning runs with layer-wise lr decay (tests/golden/mae_ft_lrd_small.npz: the v2 rule through AdamW(param_groups_lrd),
the v110 rule through build_optimizer), replay from a step plan while the schedule moves, state_dict round trip and the
Trainer on the YAML."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import lrd_util

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mae_ft_lrd_small.npz')
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3
STEPS = 3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _buffers(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen).to(DEV)
    grads = [(torch.randn(n, generator=gen) * 10 ** torch.empty(n).uniform_(-4, 0, generator=gen)).to(DEV)
             for _ in range(STEPS)]
    return p, grads


def _hyper(t, lr):
    return torch.tensor([lr, B1 ** t, B2 ** t, 0.0], dtype=torch.float32, device=DEV)


def _cuts(n, n_seg, gen):
    """n_seg ascending segment ends, multiples of 4, the last one n."""
    inner = torch.randperm(n // 4 - 1, generator=gen)[:n_seg - 1] + 1
    return sorted((inner * 4).tolist()) + [n]


# ---------------------------------------------------------------------------------------------- 1. uniform = flat
@pytest.mark.parametrize('n_seg', [1, 3, 300])
@pytest.mark.parametrize('n', [8, 4104, 2 ** 20 + 24])
def test_uniform_table_equals_the_flat_kernel_bit_for_bit(n, n_seg):
    """Every multiplier 1.0 and one decay: p / m / v after 3 consecutive steps carry the bits of ops.adamw_dev.
    (n = 8 holds two float4: its tables have min(n_seg, 2) segments.)"""
    from passl_amd.hip import ops
    n_seg = min(n_seg, n // 4)
    gen = torch.Generator().manual_seed(n + n_seg)
    table = ops.adamw_groups_table(_cuts(n, n_seg, gen), [1.0] * n_seg, [0.05] * n_seg, n, DEV)
    p0, grads = _buffers(n, 11)
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    for t, g in enumerate(grads, 1):
        lr = LR * (1.0 - 0.1 * t)
        ops.adamw_dev(pa, g, ma, va, _hyper(t, lr), B1, B2, EPS, 0.05, 0.5)
        ops.adamw_groups_dev(pb, g, mb, vb, table, _hyper(t, lr), B1, B2, EPS, 0.5)
        assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
    assert not torch.equal(pa, p0)


@pytest.mark.parametrize('n', [1, 3, 4099, 2 ** 20 + 27, 2 ** 21 + 2 ** 19 + 27])
def test_scalars_by_value_and_from_device_memory_give_equal_bits_with_a_tail(n):
    """ops.adamw (lr, beta^t by value) against ops.adamw_dev (the same floats, rounded to fp32, read from device memory)
    on an n that is no multiple of 4: the last n % 4 elements take the flat kernel's scalar tail, which no
    variant-against-variant test reaches (their n are multiples of 4).  Tail only (1, 3), a tail after 1024 float4
    (4099), after 1025 workgroups of one grid round (2**20 + 27) and after the capped grid of 2048 workgroups went
    round more than once (2**21 + 2**19 + 27 = 655366 float4 > 2048 * 256)."""
    from passl_amd.hip import ops
    p0, grads = _buffers(n, 13)
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    for t, g in enumerate(grads, 1):
        lr = LR * (1.0 - 0.1 * t)
        ops.adamw(pa, g, ma, va, lr, B1, B2, EPS, 0.05, B1 ** t, B2 ** t, 0.5)
        ops.adamw_dev(pb, g, mb, vb, _hyper(t, lr), B1, B2, EPS, 0.05, 0.5)
        assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
    assert not torch.equal(pa[-1:], p0[-1:]) and bool((ma[-(n & 3):] != 0).all())      # the tail was updated


# ---------------------------------------------------------------------------------------------- 2. groups = slices
LENGTHS = [4, 8, 12, 1000, 4096, 4100, 65540]


@pytest.mark.parametrize('grad_scale', [1.0, 1.0 / 3.0])
@pytest.mark.parametrize('n_seg', [1, 2, 7, 300, 5000])
def test_groups_equal_the_flat_kernel_per_slice_bit_for_bit(n_seg, grad_scale):
    """Segment s of the grouped launch = passl_hip_adamw on that slice alone with lr = fp32(lr) * fp32(scale_s) and
    wd_s: no tolerance.  m and v do not depend on (lr, wd): they also equal one flat launch over the whole buffer.
    The kernel has no segment limit (the table stays in global memory): 5000 segments run like 7."""
    from passl_amd.hip import ops
    gen = torch.Generator().manual_seed(n_seg)
    if n_seg <= 2:
        lens = [4100, 65540][:n_seg]
    elif n_seg == 7:
        lens = [LENGTHS[i] for i in torch.randperm(7, generator=gen).tolist()]
    else:
        # every length occurs; short ones dominate (boundaries inside one wave), the 65540s keep whole tiles apart
        w = torch.tensor([0.3, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05])
        lens = LENGTHS + [LENGTHS[i] for i in torch.multinomial(w, n_seg - 7, replacement=True, generator=gen).tolist()]
        lens = [lens[i] for i in torch.randperm(n_seg, generator=gen).tolist()]
    ends = np.cumsum(lens).tolist()
    n = ends[-1]
    scales = torch.empty(n_seg).uniform_(0.01, 1.0, generator=gen).tolist()
    scales[0] = 1.0
    wds = [[0.0, 0.05, 0.3][i] for i in torch.randint(0, 3, (n_seg,), generator=gen).tolist()]
    table = ops.adamw_groups_table(ends, scales, wds, n, DEV)
    p0, grads = _buffers(n, 5 + n_seg)
    pa, pb = p0.clone(), p0.clone()
    ma, va, mb, vb, mf, vf = (torch.zeros(n, device=DEV) for _ in range(6))
    scratch = p0.clone()
    for t, g in enumerate(grads, 1):
        lr = LR * (1.0 - 0.1 * t)
        b1p, b2p = B1 ** t, B2 ** t
        off = 0
        for end, sc, wd in zip(ends, scales, wds):
            ops.adamw(pa[off:end], g[off:end], ma[off:end], va[off:end], float(np.float32(lr) * np.float32(sc)), B1, B2,
                      EPS, wd, b1p, b2p, grad_scale)
            off = end
        ops.adamw(scratch, g, mf, vf, lr, B1, B2, EPS, 0.0, b1p, b2p, grad_scale)
        ops.adamw_groups_dev(pb, g, mb, vb, table, _hyper(t, lr), B1, B2, EPS, grad_scale)
        assert torch.equal(_bits(pa), _bits(pb)), 'step %d: %d elements differ' % (t, int((pa != pb).sum()))
        assert torch.equal(_bits(ma), _bits(mb)) and torch.equal(_bits(va), _bits(vb))
        assert torch.equal(_bits(mf), _bits(mb)) and torch.equal(_bits(vf), _bits(vb))
    assert not torch.equal(pa, p0)


# ---------------------------------------------------------------------------------------------- 3. bad arguments
def test_bad_arguments_are_refused_before_any_launch():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    fn = L.load().passl_hip_adamw_groups_dev
    n = 4104
    p0, grads = _buffers(n + 4, 3)
    p, g = p0.clone(), grads[0]
    m, v = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    t = ops.adamw_groups_table([8, 4104], [1.0, 0.5], [0.05, 0.0], n, DEV)
    hyper = _hyper(1, LR)
    good = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, t['seg_end'].data_ptr(),
            t['seg_lr_scale'].data_ptr(), t['seg_wd'].data_ptr(), 2, hyper.data_ptr(), B1, B2, EPS, 1.0, L.stream()]

    def call(**kw):
        a = list(good)
        for i, val in kw.items():
            a[int(i[1:])] = val
        return fn(*a)
    for i in (0, 1, 2, 3, 5, 6, 7, 9):
        assert call(**{'a%d' % i: None}) == L.EINVAL, i                              # NULL pointers
    assert call(a4=-4) == L.EINVAL and call(a4=4102) == L.EINVAL                     # n < 0, n % 4
    assert call(a8=0) == L.EINVAL and call(a8=-1) == L.EINVAL                        # n_seg <= 0
    for i in (0, 1, 2, 3):
        assert call(**{'a%d' % i: good[i] + 4}) == L.EINVAL, i                       # not 16-byte aligned
    assert call(a5=good[5] + 4) == L.EINVAL                                          # int64 table not 8-byte aligned
    assert call(a4=0) == L.OK                                                        # nothing to do
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(p0)) and not m.any() and not v.any()          # nothing was launched
    with pytest.raises(L.PasslHipError):
        ops.adamw_groups_dev(p[:n].cpu(), g[:n], m[:n], v[:n], t, hyper, B1, B2, EPS)   # no host fall-back
    with pytest.raises(ValueError):
        ops.adamw_groups_dev(p, g, m, v, t, hyper, B1, B2, EPS)                      # the table of another buffer
    assert call() == L.OK
    torch.cuda.synchronize()
    assert not torch.equal(p[:n], p0[:n]) and torch.equal(_bits(p[n:]), _bits(p0[n:]))   # ... and bounded by n


# ---------------------------------------------------------------------------------------------- 4. reference parity
FT_ARCH = dict(name='MAE_ViT', patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4, img_size=64)
FT_TOL_F32 = dict(loss=1e-3, param=1e-4)              # tests/test_droppath_gpu.py (= tests/test_mae_gpu.py), unchanged
FT_TOL_BF16 = dict(loss=3e-2, param=1e-2)


def _build_finetune(dtype, classes=16):
    from oracle.mae import finetune_state
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(dtype)
    model = build_model(dict(name='MAE_FINETUNE', architecture=dict(FT_ARCH),
                             head=dict(name='VisionTransformerClsHead', num_classes=classes, in_channels=128)))
    keys_shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    missing, unexpected = model.load_state_dict(dict(finetune_state(keys_shapes)), strict=False)
    assert not missing and not unexpected
    return model, keys_shapes


def _optimizer(run, model, z):
    lr, wd, ld = float(z['lr']), float(z['weight_decay']), float(z['layer_decay'])
    if run == 'A':
        from passl_amd.solver.lr_decay import param_groups_lrd
        from passl_amd.solver.optimizer import AdamW
        return AdamW(lr, beta1=B1, beta2=B2, weight_decay=wd,
                     parameters=param_groups_lrd(model, wd, {'pos_embed', 'cls_token', 'dist_token'}, ld))
    from passl_amd.solver.builder import build_optimizer
    return build_optimizer(dict(name='AdamW', beta1=B1, beta2=B2, weight_decay=wd, layer_decay=ld), lr, [model])


def _run_lrd_golden(run, dtype, tol, parity):
    """The harness of tests/test_droppath_gpu.py::_run_finetune_golden for the runs with parameter groups.  Loss (every
    step; x 20 after the first update, as there) and pnorm (after the first update) at the project's bounds.  parity
    (fp32): dnorm of every watched parameter with a multiplier != 1 within 1/10 of its relative gap to the uniform run U
    in the fixture, every element-wise stored tensor within D / 10 of the reference (D = its distance to U in the
    fixture) — and the product's own distance to U LARGER than those bounds: the test sees the feature."""
    z = np.load(GOLDEN)
    N, hw, steps, classes = [int(v) for v in z['meta']]
    torch.manual_seed(0)
    model, keys_shapes = _build_finetune(dtype, classes)
    assert ['%s:%s' % (k, 'x'.join(map(str, s))) for k, s in keys_shapes] == [str(k) for k in z['keys']]
    model.train()
    opt = _optimizer(run, model, z)
    want_table = lrd_util.tables(z)[run]
    assert [(s, w) for _n, s, w in opt.param_table()] == [(s, w) for _n, s, w in want_table]
    watch, elem = [str(n) for n in z['watch']], [str(n) for n in z['elementwise']]
    ps = dict(model.named_parameters())
    gen = torch.Generator().manual_seed(909)
    report, bad = [], []

    def check(what, err, bound, at_least=False):
        line = '%-64s %s %.3e  bound %.3e' % (what, 'dist' if at_least else 'err', err, bound)
        report.append(line)
        if not (err > bound if at_least else err <= bound):
            bad.append(line)

    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        out = model(x.to(DEV), y.to(DEV), mode='train')
        opt.clear_grad()
        out['loss'].backward()
        before = {n: ps[n].detach().double().clone() for n in watch}
        opt.step()
        pre = '%s_s%d_' % (run, s)
        ref_loss = float(z[pre + 'loss'])
        check(pre + 'loss', abs(float(out['loss'].detach()) - ref_loss) / abs(ref_loss), tol['loss'] * (1.0 if s == 0 else 20.0))
        for n in watch:
            after = ps[n].detach().double()
            if s == 0:
                ref = float(z[pre + 'pnorm/' + n])
                check(pre + 'pnorm/' + n, abs(after.norm().item() - ref) / ref, tol['param'])
            if not parity or not lrd_util.treated_differently(z, run, n)[0]:
                continue
            dn, ref, ref_u = (after - before[n]).norm().item(), float(z[pre + 'dnorm/' + n]), float(z['U_s%d_dnorm/%s' % (s, n)])
            bound = lrd_util.dnorm_gap(z, run, s, n) / 10.0
            check(pre + 'dnorm/' + n, abs(dn - ref) / ref, bound)
            check(pre + 'dnorm/' + n + ' vs uniform', abs(dn - ref_u) / ref_u, bound, at_least=True)
        for n in elem if parity else []:
            got = ps[n].detach().double().cpu().numpy()
            bound = lrd_util.elem_dist(z, run, s, n) / 10.0
            check(pre + 'p/' + n, float(np.max(np.abs(got - z[pre + 'p/' + n]))), bound)
            check(pre + 'p/' + n + ' vs uniform', float(np.max(np.abs(got - z['U_s%d_p/%s' % (s, n)]))), bound, at_least=True)
    print('\n'.join(report))                                  # every figure, before the assertion
    assert not bad, 'parity violations:\n' + '\n'.join(bad)


@pytest.mark.parametrize('run', ['A', 'B'])
def test_finetune_layer_decay_golden_fp32(run):
    """fp32 is the parity claim.  Measured maxima (MI355X) are recorded in DESIGN.md, 'AdamW parameter groups'."""
    _run_lrd_golden(run, torch.float32, FT_TOL_F32, True)


def test_finetune_layer_decay_golden_bf16():
    """The bf16 path runs the same update within the project's bf16 bounds (loss, pnorm); no parity claim."""
    _run_lrd_golden('A', torch.bfloat16, FT_TOL_BF16, False)


# ---------------------------------------------------------------------------------------------- 5. replay
def _tiny_step_model(dim, heads, classes, B, T):
    """Two Blocks, LayerNorm over the class rows, a Linear head, softmax cross entropy: the smallest step that records
    without a foreign launch (tests/test_droppath_gpu.py::_tiny_step_model without stochastic depth)."""
    from passl_amd.hip import nn
    from passl_amd.modeling.backbones.mae import Block, trunc_normal_
    from passl_amd.modeling.heads.clas_head import _SoftmaxCEFn

    class Tiny(nn.Layer):
        def __init__(self):
            super().__init__()
            norm = partial(nn.LayerNorm, epsilon=1e-6)
            self.blocks = torch.nn.ModuleList([Block(dim, heads, 4., qkv_bias=True, norm_layer=norm) for _ in range(2)])
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
            for blk in self.blocks:
                x = blk(x, B, T)
            scores = self.head(self.norm(nn.gather_rows(x, self.cls_rows)), out_f32=True)
            loss, _a1, _a5 = _SoftmaxCEFn.apply(scores, labels)
            return dict(loss=loss)
    return Tiny()


def _tiny_groups(model):
    """Block 0 at 0.25, block 1 at 0.5, norm and head at 1; 1-D parameters without decay."""
    groups = {}
    for n, p in model.named_parameters():
        scale = {'blocks.0': 0.25, 'blocks.1': 0.5}.get(n[:8], 1.0)
        key = (scale, p.ndim == 1)
        groups.setdefault(key, {'lr_scale': scale, 'weight_decay': 0.0 if p.ndim == 1 else 0.05, 'params': []})
        groups[key]['params'].append(p)
    return list(groups.values())


def test_step_plan_replays_grouped_adamw_while_the_schedule_moves():
    """The grouped launch is recorded like its neighbours: the replayed steps read the learning rate of THEIR step from
    device memory and the table from the recorded pointers — parameters and losses equal the eager twin's, bit for bit."""
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.lr_scheduler import CosineAnnealingDecay
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    B, T, dim, classes, steps = 16, 17, 128, 16, 4              # one warm-up step, then 3 steps through the plan
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(B * T, dim, generator=gen).to(DEV), torch.randint(0, classes, (B,), generator=gen).to(DEV))
               for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        torch.manual_seed(9)
        model = _tiny_step_model(dim, 4, classes, B, T)
        model.train()
        sched = CosineAnnealingDecay(1e-3, T_max=6)
        opt = AdamW(sched, weight_decay=0.05, parameters=_tiny_groups(model))
        assert opt._tables[0] is not None and opt._tables[0]['n_seg'] >= 4

        def full_step(x, y):
            out = model(x, y)
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            opt.step()
            return out
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, lrs, flats = [], [], []
        for x, y in batches:
            lrs.append(opt.get_lr())
            out = sp.run(x, y)
            sched.step()
            losses.append(out['loss'].detach().clone().reshape(1))
            flats.append(model.arena_q.flat[:model.arena_q.n_train].clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        assert len(set(lrs)) == steps                            # the schedule moved at every step
        results[mode] = (torch.cat(losses).cpu(), torch.stack(flats).cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, fa), (lb, fb) = results['eager'], results['plan']
    assert torch.equal(_bits(la), _bits(lb))
    for s in range(steps):
        assert torch.equal(_bits(fa[s]), _bits(fb[s])), 'parameters differ after step %d' % s
    assert not torch.equal(fa[steps - 1], fa[steps - 2])


# ---------------------------------------------------------------------------------------------- 6. state_dict
def test_state_dict_round_trip_gives_identical_bits():
    from passl_amd.solver.lr_decay import param_groups_lrd
    from passl_amd.solver.optimizer import AdamW
    gen = torch.Generator().manual_seed(21)
    data = [(torch.randn(8, 3, 64, 64, generator=gen).to(DEV), torch.randint(0, 16, (8,), generator=gen).to(DEV))
            for _ in range(3)]

    def make():
        torch.manual_seed(0)
        model, _ = _build_finetune(torch.float32)
        model.train()
        return model, AdamW(LR, weight_decay=0.05, parameters=param_groups_lrd(model, 0.05, {'pos_embed', 'cls_token'}, 0.65))

    def step(model, opt, x, y):
        out = model(x, y, mode='train')
        opt.clear_grad()
        out['loss'].backward()
        opt.step()

    m1, o1 = make()
    for x, y in data[:2]:
        step(m1, o1, x, y)
    sd, weights = o1.state_dict(), {k: v.detach().clone() for k, v in m1.state_dict().items()}
    assert sorted(sd) == ['moment1_0', 'moment2_0', 't'] and sd['t'] == 2        # the table is not state
    step(m1, o1, *data[2])
    m2, o2 = make()
    m2.load_state_dict(weights)
    o2.set_state_dict(sd)
    step(m2, o2, *data[2])
    a, b = m1.arena_q, m2.arena_q
    assert torch.equal(_bits(a.flat[:a.n_train]), _bits(b.flat[:b.n_train]))
    assert torch.equal(_bits(o1._m[0]), _bits(o2._m[0])) and torch.equal(_bits(o1._v[0]), _bits(o2._v[0]))


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_trainer_runs_layer_decay_config_end_to_end(tmp_path, monkeypatch):
    """configs/mae/mae_vit_b_finetune_lrd_synthetic.yaml through the v110 Trainer + hook bus for 2 iterations: the
    optimizer is the grouped one (ViT-B ladder of 14 multipliers) and every iteration is one grouped launch."""
    from passl_amd.engine.trainer import Trainer
    from passl_amd.hip import ops
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_lrd_synthetic.yaml'),
                     ['dataloader.train.sampler.batch_size=8', 'dataloader.train.dataset.num_samples=16', 'epochs=1',
                      'output_dir=%s' % tmp_path, 'log_config.interval=1'])
    cfg.timestamp = ''
    tr = Trainer(cfg)
    assert type(tr.model).__name__ == 'MAE_FINETUNE' and tr.iters_per_epoch == 2
    assert tr.optimizer.grouped
    table = tr.optimizer.param_table()
    scales = sorted({s for _n, s, _w in table})
    assert len(scales) == 14 and scales[0] == 0.65 ** 13 and scales[-1] == 1.0
    assert {w for _n, _s, w in table} == {0.0, 0.05}
    calls = []
    real = ops.adamw_groups_dev
    monkeypatch.setattr(ops, 'adamw_groups_dev', lambda *a, **k: (calls.append(a[4]['n_seg']), real(*a, **k))[1])
    monkeypatch.setattr(ops, 'adamw_dev', lambda *a, **k: pytest.fail('the flat launch ran'))
    w0 = tr.model.head.fc_cls.weight.detach().clone()
    tr.train()
    assert tr.current_iter == 2 and len(calls) == 2
    loss = float(tr.outputs['loss'].detach())
    assert np.isfinite(loss) and 0 < loss < 20
    assert float((tr.model.head.fc_cls.weight.detach() - w0).abs().max()) > 0
