"""Stochastic depth (drop_path_rate) of the fine-tuning ViT on the MI355X: the Philox draw kernel bit for bit, the
streaming add / backward kernels, the autograd node, parity with the reference run with stochastic depth
(tests/golden/mae_ft_dp_*.npz, tables injected), eval mode / rate 0, reproducibility, replay from a step plan and the
Trainer on the YAML."""
import os
from functools import partial

import numpy as np
import pytest
import torch

import droppath_util as DP

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------- 1. the draw
def test_draw_is_philox4x32_10_bit_for_bit():
    """passl_hip_drop_path_draw against the numpy restatement of its definition (droppath_util.keep_table), itself
    checked against the published Philox4x32-10 known-answer vectors first.  Three launches with IDENTICAL arguments
    give three different tables — the counter lives on the device and the launch advances it."""
    from passl_amd.hip import ops
    DP.check_known_answers()
    slots, B = 24, 256
    keep_prob = np.array([1.0, 1.0] + [0.9, 0.5, 0.75, 0.97, 0.25, 1.0, 0.6, 0.999, 0.01, 0.8, 0.5] * 2,
                         dtype=np.float32)
    assert keep_prob.shape == (slots,)
    seed, step0 = (0x1234 << 32) + 0x9abcdef1, (3 << 32) + 0xfffffffe       # the low word wraps at the third launch
    kp = torch.from_numpy(keep_prob).to(DEV)
    step = torch.tensor([step0], dtype=torch.int64, device=DEV)
    keep = torch.full((slots, B), -1.0, dtype=torch.float32, device=DEV)
    tables = []
    for _ in range(3):
        ops.drop_path_draw(keep, kp, seed, step)
        tables.append(keep.cpu().numpy().copy())
    assert int(step.item()) == step0 + 3
    for i, t in enumerate(tables):
        want = DP.keep_table(keep_prob, B, seed, step0 + i)
        assert np.array_equal(t, want), 'launch %d: %d of %d entries differ' % (i, int((t != want).sum()), t.size)
        assert np.all(t[keep_prob >= 1.0] == 1) and 0 < (t == 0).sum() < t.size
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])
    # a seed with the top bit set passes through the signed argument unchanged
    big = (1 << 63) + 12345
    step.fill_(0)
    ops.drop_path_draw(keep, kp, big, step)
    assert np.array_equal(keep.cpu().numpy(), DP.keep_table(keep_prob, B, big, 0))


# ---------------------------------------------------------------------------------------------- 2. add / bwd kernels
def _keep_pattern(B):
    k = torch.ones(B, dtype=torch.float32)
    k[1::3] = 0.0                                   # both values present for every B >= 2; sample 0 kept, 1 dropped
    return k


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,T,C', [(8, 17, 128), (5, 197, 768), (128, 197, 768)])
def test_add_and_bwd_kernels_bit_for_bit(B, T, C, dtype):
    """out = residual + keep[b] * (branch / keep_prob) and dbranch = keep[b] * (dy / keep_prob): fp32 arithmetic, IEEE
    division, one rounding — equal to torch's evaluation of the same formula on the GPU.  The divisor is handed to torch
    as a device tensor: with a Python scalar torch's GPU division multiplies by a rounded reciprocal instead, which is
    not the division the reference performs (the smallest shape is also checked against torch's CPU division).  Rows of
    a dropped sample are not read: NaN planted there changes nothing.  (For those rows the backward formula gives a
    zero with the sign of dy and the kernel writes +0: compared as values; every kept row is compared as bits.)"""
    from passl_amd.hip import ops
    keep_prob = float(np.float32(1.0) - np.float32(0.3))
    gen = torch.Generator().manual_seed(B * 1000 + T)
    branch = torch.randn(B * T, C, generator=gen).to(DEV).to(dtype)
    res = torch.randn(B * T, C, generator=gen).to(DEV).to(dtype)
    dy = torch.randn(B * T, C, generator=gen).to(DEV).to(dtype)
    keep = _keep_pattern(B).to(DEV)
    rows = keep.repeat_interleave(T)[:, None]                 # the factor of every row
    kp = torch.tensor(keep_prob, dtype=torch.float32, device=DEV)
    want_out = (res.float() + rows * (branch.float() / kp)).to(dtype)
    want_db = (rows * (dy.float() / kp)).to(dtype)
    out = ops.drop_path_add(branch, res, keep, keep_prob, B, T)
    db = ops.drop_path_bwd(dy, keep, keep_prob, B, T)
    kept = rows[:, 0] != 0
    assert torch.equal(_bits(out), _bits(want_out))
    assert torch.equal(db, want_db) and torch.equal(_bits(db[kept]), _bits(want_db[kept]))
    assert torch.equal(_bits(out[~kept]), _bits(res[~kept])) and not db[~kept].any()
    if B * T * C <= 8 * 17 * 128:
        cpu = (res.cpu().float() + rows.cpu() * (branch.cpu().float() / keep_prob)).to(dtype)
        assert torch.equal(_bits(out.cpu()), _bits(cpu))
    # dropped samples' rows are not read
    branch2, dy2 = branch.clone(), dy.clone()
    branch2[~kept] = float('nan')
    dy2[~kept] = float('nan')
    out2 = ops.drop_path_add(branch2, res, keep, keep_prob, B, T)
    db2 = ops.drop_path_bwd(dy2, keep, keep_prob, B, T)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(db2), _bits(db))
    # keep_prob == 1 with everything kept is a plain add
    ones = torch.ones(B, dtype=torch.float32, device=DEV)
    assert torch.equal(_bits(ops.drop_path_add(branch, res, ones, 1.0, B, T)), _bits((res.float() + branch.float()).to(dtype)))


def test_kernels_refuse_bad_arguments():
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    x = torch.zeros(4 * 3, 16, device=DEV)
    keep = torch.ones(4, device=DEV)
    for kp in (0.0, 1.5, -0.1, float('nan')):
        with pytest.raises(L.PasslHipError):
            ops.drop_path_add(x, x, keep, kp, 4, 3)
        with pytest.raises(L.PasslHipError):
            ops.drop_path_bwd(x, keep, kp, 4, 3)
    y = torch.zeros(4 * 3, 12, device=DEV)                        # C % 8 != 0
    with pytest.raises(L.PasslHipError):
        ops.drop_path_add(y, y, keep, 0.9, 4, 3)
    with pytest.raises(L.PasslHipError):
        ops.drop_path_add(x.cpu(), x, keep, 0.9, 4, 3)            # no host fall-back


# ---------------------------------------------------------------------------------------------- 3. autograd node
def test_autograd_node_matches_torch_autograd():
    from passl_amd.hip import nn
    B, T, C = 6, 17, 128
    keep_prob = float(np.float32(1.0) - np.float32(0.2))
    gen = torch.Generator().manual_seed(5)
    keep = _keep_pattern(B).to(DEV)
    rows = keep.repeat_interleave(T)[:, None]
    kp = torch.tensor(keep_prob, dtype=torch.float32, device=DEV)
    g = torch.randn(B * T, C, generator=gen).to(DEV)
    leaves = []
    for _ in range(2):
        gen2 = torch.Generator().manual_seed(6)
        leaves.append([torch.randn(B * T, C, generator=gen2).to(DEV).requires_grad_(True) for _ in range(2)])
    (b1, r1), (b2, r2) = leaves
    out1 = nn.drop_path_add(b1, r1, keep, keep_prob, B, T)
    out2 = r2 + rows * (b2 / kp)
    assert torch.equal(_bits(out1.detach()), _bits(out2.detach()))
    out1.backward(g)
    out2.backward(g)
    kept = rows[:, 0] != 0
    assert torch.equal(_bits(r1.grad), _bits(r2.grad)) and torch.equal(_bits(r1.grad), _bits(g))
    assert torch.equal(b1.grad, b2.grad)                                    # values: the zeros of dropped rows
    assert torch.equal(_bits(b1.grad[kept]), _bits(b2.grad[kept])) and not b1.grad[~kept].any()


# ---------------------------------------------------------------------------------------------- 4. golden parity
FT_SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05)
FT_ARCH = dict(name='MAE_ViT', patch_size=16, embed_dim=768, depth=12, num_heads=12, qkv_bias=True, mlp_ratio=4)
FT_WATCH = ['backbone.cls_token', 'backbone.pos_embed', 'backbone.patch_embed.proj.weight',
            'backbone.blocks.0.attn.qkv.weight', 'backbone.blocks.1.mlp.fc2.bias', 'backbone.blocks.1.norm2.weight',
            'backbone.fc_norm.weight', 'backbone.fc_norm.bias', 'head.fc_cls.weight', 'head.fc_cls.bias']
FT_TOL_F32 = dict(loss=1e-3, feat=1e-3, grad=2e-3, param=1e-4)              # tests/test_mae_gpu.py, unchanged
FT_TOL_BF16 = dict(loss=3e-2, feat=6e-2, grad=8e-2, param=1e-2)


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
    """The harness of tests/test_mae_gpu.py::_run_finetune_golden with the reference's keep table of every step passed
    as ``drop_path_keep=``; same bounds.  discriminate (fp32): step 0 must also be FAR from the same step with nothing
    dropped (s0_*_nodrop) — features by more than 3 x their bound, loss by more than 2 x its bound; the reference's own
    distances are 230 x / 700 x (features) and 4.9 x / 3.6 x (loss) for the small / ViT-B case."""
    from passl_amd.solver.optimizer import AdamW
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    N, hw, steps, classes = [int(v) for v in z['meta']]
    torch.manual_seed(0)
    model, keys_shapes = _build_finetune(dict(arch, drop_path_rate=float(z['rate'])), classes, dtype)
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

    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        keep = torch.from_numpy(z['s%d_keep' % s]).to(DEV)
        out = model(x.to(DEV), y.to(DEV), mode='train', drop_path_keep=keep)
        opt.clear_grad()
        out['loss'].backward()
        pre = 's%d_' % s
        k = 1.0 if s == 0 else 20.0
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
                check(pre + 'feat[:, :8] vs nothing dropped', feat, z['s0_feat_head_nodrop'], 3 * tol['feat'], rel=True,
                      at_least=True)
                check(pre + 'loss vs nothing dropped', float(out['loss'].detach()), z['s0_loss_nodrop'], 2 * tol['loss'],
                      rel=True, at_least=True)
        opt.step()
        if s == 0:
            ps = dict(model.named_parameters())
            for n in FT_WATCH:
                check(pre + 'pnorm/' + n, ps[n].detach().double().norm().item(), z[pre + 'pnorm/' + n], tol['param'], rel=True)
    assert model.backbone.drop_path_step() == 0               # injected tables: no draw, the counter does not move
    print('\n'.join(report))                                  # every figure, before the assertion
    assert not bad, 'parity violations:\n' + '\n'.join(bad)


def test_finetune_droppath_golden_small_fp32():
    _run_finetune_golden('mae_ft_dp_small', dict(FT_ARCH, embed_dim=128, depth=4, num_heads=4, img_size=64),
                         torch.float32, FT_TOL_F32, True)


def test_finetune_droppath_golden_vit_b_fp32():
    """fp32 is the parity claim: against the distance to the step with nothing dropped (loss 3.6e-3, features 0.70 of
    their maximum, gradient norms 0.6 - 2.8 %) the fp32 bounds discriminate on loss, features and gradients."""
    _run_finetune_golden('mae_ft_dp_vit_b', dict(FT_ARCH), torch.float32, FT_TOL_F32, True)


def test_finetune_droppath_golden_vit_b_bf16():
    """The bf16 bounds (loss 3e-2, features 6e-2, gradients 8e-2) are wider than what dropping changes in the loss
    (3.6e-3) and in the watched gradient norms (0.6 - 2.8 %): this run discriminates on the features only (0.70 of
    their maximum against a bound of 0.06).  It shows that the bf16 path runs the same computation within the
    project's bf16 bounds; the parity claim is the fp32 run above."""
    _run_finetune_golden('mae_ft_dp_vit_b', dict(FT_ARCH), torch.bfloat16, FT_TOL_BF16, False)


# ---------------------------------------------------------------------------------------------- 5. eval mode, rate 0
SMALL = dict(FT_ARCH, embed_dim=128, depth=4, num_heads=4, img_size=64)


def _spy_on_blocks(model, monkeypatch):
    """-> calls: the index of the block inside whose forward every ops.drop_path_add launch happened."""
    from passl_amd.hip import ops
    calls, cur = [], [None]
    real = ops.drop_path_add

    def add(*a, **k):
        calls.append(cur[0])
        return real(*a, **k)
    monkeypatch.setattr(ops, 'drop_path_add', add)
    for i, blk in enumerate(model.backbone.blocks):
        def fwd(*a, _f=blk.forward, _i=i, **k):
            cur[0] = _i
            try:
                return _f(*a, **k)
            finally:
                cur[0] = None
        blk.forward = fwd
    return calls


def test_eval_mode_and_rate_zero_keep_the_fused_path(monkeypatch):
    torch.manual_seed(1)
    dropper, _ = _build_finetune(dict(SMALL, drop_path_rate=0.3), 16, torch.float32)
    plain, _ = _build_finetune(dict(SMALL), 16, torch.float32)
    plain.load_state_dict(dropper.state_dict())
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
    y = torch.randint(0, 16, (8,), generator=gen).to(DEV)
    calls_d = _spy_on_blocks(dropper, monkeypatch)
    # eval: bit-identical scores, no draw, no launch of the new op
    dropper.eval()
    plain.eval()
    a, b = dropper(x, mode='test'), plain(x, mode='test')
    assert torch.equal(_bits(a.float()), _bits(b.float()))
    assert dropper.backbone.drop_path_step() == 0 and dropper.backbone.drop_path_table(8) is None and not calls_d
    with pytest.raises(ValueError):
        dropper(x, y, mode='train', drop_path_keep=torch.ones(8, 8, device=DEV))      # a table in eval mode
    # train: block 0 never calls the op, every other block twice per forward; one draw per forward
    dropper.train()
    for n in (1, 2):
        del calls_d[:]
        dropper(x, y, mode='train')['loss'].backward()
        assert calls_d == [1, 1, 2, 2, 3, 3]
        assert dropper.backbone.drop_path_step() == n
    t = dropper.backbone.drop_path_table(8).cpu().numpy()
    assert t.shape == (8, 8) and np.all(t[:2] == 1) and np.all((t == 0) | (t == 1))
    # rate 0 in train mode: no counter, no table, no launch of the new op, the loss of the fused path
    monkeypatch.undo()
    calls_p = _spy_on_blocks(plain, monkeypatch)
    plain.train()
    out = plain(x, y, mode='train')
    out['loss'].backward()
    assert not calls_p and plain.backbone.drop_path_step() == 0 and plain.backbone.drop_path_table(8) is None
    assert plain.backbone._drop_path is None                  # no state at all, so no device tensor either
    # a table of the wrong shape is refused before anything is launched
    with pytest.raises(ValueError):
        dropper(x, y, mode='train', drop_path_keep=torch.ones(6, 8, device=DEV))
    assert dropper.backbone.drop_path_step() == 2


# ---------------------------------------------------------------------------------------------- 6. reproducibility
def _three_steps(seed):
    from passl_amd.solver.optimizer import AdamW
    torch.manual_seed(seed)
    model, _ = _build_finetune(dict(SMALL, drop_path_rate=0.3), 16, torch.float32)
    model.train()
    opt = AdamW(1e-3, weight_decay=0.05, parameters=list(model.parameters()))
    gen = torch.Generator().manual_seed(77)
    losses, tables = [], []
    for _ in range(3):
        x = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
        y = torch.randint(0, 16, (8,), generator=gen).to(DEV)
        out = model(x, y, mode='train')
        opt.clear_grad()
        out['loss'].backward()
        opt.step()
        losses.append(out['loss'].detach().clone().reshape(1))
        tables.append(model.backbone.drop_path_table(8).clone())
    assert model.backbone.drop_path_step() == 3
    return torch.cat(losses).cpu(), torch.stack(tables).cpu(), model.backbone._drop_path.seed


def test_same_seed_same_masks_and_losses():
    la, ta, sa = _three_steps(123)
    lb, tb, sb = _three_steps(123)
    lc, tc, sc = _three_steps(124)               # what torch.manual_seed(seed + rank) gives the next rank
    assert sa == sb and torch.equal(ta, tb) and torch.equal(_bits(la), _bits(lb))
    assert sa != sc and not torch.equal(ta, tc)
    assert not torch.equal(ta[0], ta[1]) and not torch.equal(ta[1], ta[2])      # a new table at every step
    assert (ta == 0).any() and (ta[:, :2] == 1).all()
    # the tables are the definition's: seed and step are all that goes in
    kp = [float(np.float32(1.0) - p) for p in torch.linspace(0, 0.3, 4, dtype=torch.float32).numpy() for _ in range(2)]
    for s in range(3):
        assert np.array_equal(ta[s].numpy(), DP.keep_table(kp, 8, sa, s))


# ---------------------------------------------------------------------------------------------- 7. replay
def _tiny_step_model(dim, heads, classes, B, T, seed):
    """Two Blocks with stochastic depth, LayerNorm over the class rows, a Linear head, softmax cross entropy: the
    smallest step that records without a foreign launch (the fine-tuning model itself is not ``graph_safe``: its
    pooling backward launches framework kernels)."""
    from passl_amd.hip import nn, ops
    from passl_amd.modeling.backbones.mae import Block, trunc_normal_
    from passl_amd.modeling.heads.clas_head import _SoftmaxCEFn

    class Tiny(nn.Layer):
        def __init__(self):
            super().__init__()
            norm = partial(nn.LayerNorm, epsilon=1e-6)
            self.blocks = torch.nn.ModuleList([Block(dim, heads, 4., qkv_bias=True, norm_layer=norm, drop_path=p)
                                               for p in (0.3, 0.4)])
            self.norm = norm(dim)
            self.head = nn.Linear(dim, classes)
            with torch.no_grad():
                for m in self.modules():
                    if isinstance(m, nn.Linear):
                        trunc_normal_(m.weight, std=0.02)
            self.arena_q = nn.EncoderArena(self, trainable=True)
            self.keep_prob = torch.tensor([b.keep_prob for b in self.blocks for _ in range(2)], device=DEV)
            self.keep = torch.zeros(4, B, device=DEV)
            self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
            self.cls_rows = (torch.arange(B, dtype=torch.int32, device=DEV) * T).contiguous()

        def forward(self, x, labels):
            self.arena_q.refresh()
            ops.drop_path_draw(self.keep, self.keep_prob, seed, self.step)
            for i, blk in enumerate(self.blocks):
                x = blk(x, B, T, self.keep[2 * i:2 * i + 2])
            scores = self.head(self.norm(nn.gather_rows(x, self.cls_rows)), out_f32=True)
            loss, _a1, _a5 = _SoftmaxCEFn.apply(scores, labels)
            return dict(loss=loss)
    return Tiny()


def test_step_plan_replays_draw_fresh_tables():
    """A recorded step plan replays the draw launch with the recorded argument bytes and still gets a new table every
    step (seed by value, counter on the device): tables and losses equal the eager twin's, bit for bit."""
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.float32)
    B, T, dim, classes, steps, seed = 16, 17, 128, 16, 4, (7 << 32) + 99
    gen = torch.Generator().manual_seed(3)
    batches = [(torch.randn(B * T, dim, generator=gen).to(DEV), torch.randint(0, classes, (B,), generator=gen).to(DEV))
               for _ in range(steps)]
    results = {}
    for mode in ('eager', 'plan'):
        torch.manual_seed(9)
        model = _tiny_step_model(dim, 4, classes, B, T, seed)
        model.train()
        opt = AdamW(1e-3, weight_decay=0.05, parameters=list(model.parameters()))

        def full_step(x, y):
            out = model(x, y)
            opt.clear_grad()
            out['loss'].backward(ops.ones_like_cached(out['loss']))
            opt.step()
            return out
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'plan'), strict=True)
        losses, tables = [], []
        for x, y in batches:
            out = sp.run(x, y)
            losses.append(out['loss'].detach().clone().reshape(1))
            tables.append(model.keep.clone())
        torch.cuda.synchronize()
        if mode == 'plan':
            assert sp.failed is None, sp.failed
            assert not sp.foreign, sp.foreign
            assert sp.captured and sp.replays >= 2
            print('step plan:', sp.info)
        assert int(model.step.item()) == steps
        results[mode] = (torch.cat(losses).cpu(), torch.stack(tables).cpu())
        del sp, model, opt
        torch.cuda.empty_cache()
    (la, ta), (lb, tb) = results['eager'], results['plan']
    for s in range(1, steps):
        assert not torch.equal(tb[s], tb[s - 1]), 'step %d replayed the table of step %d' % (s, s - 1)
    assert torch.equal(ta, tb) and (tb == 0).any()
    assert torch.equal(_bits(la), _bits(lb))
    kp = [float(np.float32(1.0) - np.float32(p)) for p in (0.3, 0.3, 0.4, 0.4)]
    for s in range(steps):
        assert np.array_equal(tb[s].numpy(), DP.keep_table(kp, B, seed, s))


# ---------------------------------------------------------------------------------------------- 8. end to end
def test_trainer_runs_droppath_config_end_to_end(tmp_path):
    """configs/mae/mae_vit_b_finetune_droppath_synthetic.yaml through the v110 Trainer + hook bus: one draw per
    iteration, finite loss, the head learns."""
    from passl_amd.engine.trainer import Trainer
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_droppath_synthetic.yaml'),
                     ['dataloader.train.sampler.batch_size=8', 'dataloader.train.dataset.num_samples=32', 'epochs=1',
                      'output_dir=%s' % tmp_path, 'log_config.interval=2'])
    cfg.timestamp = ''
    tr = Trainer(cfg)
    assert type(tr.model).__name__ == 'MAE_FINETUNE' and tr.iters_per_epoch == 4
    assert tr.model.backbone.drop_path_rate == 0.1
    w0 = tr.model.head.fc_cls.weight.detach().clone()
    tr.train()
    assert tr.current_iter == 4
    loss = float(tr.outputs['loss'].detach())
    assert np.isfinite(loss) and 0 < loss < 20 and 'acc1' in tr.outputs
    assert float((tr.model.head.fc_cls.weight.detach() - w0).abs().max()) > 0
    assert tr.model.backbone.drop_path_step() == 4
    t = tr.model.backbone.drop_path_table(8).cpu().numpy()
    assert t.shape == (24, 8) and np.all(t[:2] == 1) and np.all((t == 0) | (t == 1))
