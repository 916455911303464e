"""Generate tests/golden/mixup_params.npz and tests/golden/mae_ft_mix_*.npz by EXECUTING THE REFERENCE's own files under
the paddle shim (oracle/ref_runner.py): class Mixup (passl_v110/datasets/preprocess/mixup.py), SoftTargetCrossEntropy /
LabelSmoothingCrossEntropy (tasks/ssl/mae/util/loss.py), and MAE_FINETUNE's backbone and head as in
make_golden_mae_finetune.py (same state, inputs, AdamW rule and recorded quantities).

    python tests/golden/make_golden_mixup.py [mixup_params] [mae_ft_mix_small] [mae_ft_mix_vit_b]

mixup_params: for numpy seeds 0..11 the reference's Mixup(0.8, 1.0, prob=1, switch_prob=.5, mode='batch',
num_classes=16) on x = randn(8, 3, 64, 64), y = randint(0, 16, (8,)) from Generator().manual_seed(909): kind, final
lambda, box (cutmix_bbox_and_lam is wrapped to record it), the float64 target and x_mixed[:, :, ::8, ::8].  For two of
the seeds a second consecutive call is recorded as well (the stream continues).  The float32 restatement of the
kernel's definition (tests/mixup_util.py) must equal the reference's x_mixed bit for bit on every seed, or nothing is
written.  Also the two losses of util/loss.py on scores = randn(8, 16) drawn after the batch.

mae_ft_mix_*: two steps at drop-path rate 0; step 0 mixes under numpy seed 0 (mixup), step 1 under seed 2 (CutMix):
reference Mixup -> backbone -> head -> SoftTargetCrossEntropy -> backward -> AdamW.  Step 0 is also recorded without
mixing, with hard labels (s0_loss_plain / s0_feat_head_plain); the mixed step must be farther from it than 2 x the fp32
loss bound and 3 x the fp32 feature bound of the GPU test, or the next seed of the same kind is taken (the seeds used
are written into the file).  Only parameters, targets, strided slices, scores and norms are stored."""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import mixup_util as MU                            # noqa: E402
from oracle import ref_runner                      # noqa: E402
from oracle.mae import MAEOracle, finetune_state   # noqa: E402

SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05)        # mae_vit_b_finetune.yaml:58-62
ARCH_YAML = dict(name='MAE_ViT', patch_size=16, embed_dim=768, depth=12, num_heads=12, qkv_bias=True, mlp_ratio=4)
CASES = {
    'mae_ft_mix_small': dict(arch=dict(ARCH_YAML, embed_dim=128, depth=4, num_heads=4, img_size=64), classes=16, N=8),
    'mae_ft_mix_vit_b': dict(arch=dict(ARCH_YAML), classes=1000, N=8),
}
WATCH = ['backbone.cls_token', 'backbone.pos_embed', 'backbone.patch_embed.proj.weight', 'backbone.blocks.0.attn.qkv.weight',
         'backbone.blocks.1.mlp.fc2.bias', 'backbone.blocks.1.norm2.weight', 'backbone.fc_norm.weight',
         'backbone.fc_norm.bias', 'head.fc_cls.weight', 'head.fc_cls.bias']


def _load_file(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_runner.REF_ROOT, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    ns = ref_runner.load()
    mix = _load_file('_ref_mixup', 'passl_v110', 'datasets', 'preprocess', 'mixup.py')
    loss = _load_file('_ref_mae_loss', 'tasks', 'ssl', 'mae', 'util', 'loss.py')
    return ns, mix, loss


class Recorder:
    """One reference Mixup whose every call leaves (use_cutmix, final lam, box) behind."""

    def __init__(self, mod, **kw):
        self.mod = mod
        self.fn = mod.Mixup(**kw)
        self.last = None
        params0 = self.fn._params_per_batch

        def params():
            lam, use_cutmix = params0()
            self.last = [bool(use_cutmix), float(lam), (0, 0, 0, 0)]
            return lam, use_cutmix
        self.fn._params_per_batch = params

    def __call__(self, x, y):
        box0 = self.mod.cutmix_bbox_and_lam

        def box(*a, **k):
            (yl, yh, xl, xh), lam = box0(*a, **k)
            self.last[1] = float(lam)
            self.last[2] = (int(yl), int(yh), int(xl), int(xh))
            return (yl, yh, xl, xh), lam
        self.mod.cutmix_bbox_and_lam = box
        try:
            xm, t = self.fn(x.clone(), y)          # the reference's CutMix writes into its argument
        finally:
            self.mod.cutmix_bbox_and_lam = box0
        return xm, t, tuple(self.last)


def restated(x, use_cutmix, lam, box):
    return MU.batch_mix_ref(x, lam, box if use_cutmix else None)


def make_params():
    _ns, mix, loss = load_reference()
    gen = torch.Generator().manual_seed(909)
    x = torch.randn(8, 3, 64, 64, generator=gen)
    y = torch.randint(0, 16, (8,), generator=gen)
    scores = torch.randn(8, 16, generator=gen)
    out = dict(labels=y.numpy().copy(), scores=scores.numpy().copy())
    kinds, lams, boxes, targets, subs = [], [], [], [], []
    second = []
    for seed in MU.PARAM_SEEDS:
        np.random.seed(seed)
        rec = Recorder(mix, num_classes=16, **MU.RECIPE)
        xm, t, (use_cutmix, lam, box) = rec(x, y)
        assert torch.equal(xm.view(torch.int32), restated(x, use_cutmix, lam, box).view(torch.int32)), seed
        if use_cutmix:
            assert box[1] > box[0] and box[3] > box[2], (seed, box)
        kinds.append(use_cutmix)
        lams.append(lam)
        boxes.append(box)
        targets.append(t.double().numpy().copy())
        subs.append(xm[:, :, ::8, ::8].numpy().copy())
        print('seed %2d  %s  lam %.6f  box %s' % (seed, 'cutmix' if use_cutmix else 'mixup ', lam, box))
        if seed in MU.SECOND_CALL_SEEDS:
            _xm2, _t2, (c2, l2, b2) = rec(x, y)
            second.append((c2, l2) + tuple(b2))
            print('         second call: %s  lam %.6f  box %s' % ('cutmix' if c2 else 'mixup ', l2, b2))
    assert any(kinds) and not all(kinds)
    out.update(use_cutmix=np.array(kinds), lam=np.array(lams, dtype=np.float64),
               box=np.array(boxes, dtype=np.int64), target=np.stack(targets), x_mixed_sub=np.stack(subs),
               second_seeds=np.array(MU.SECOND_CALL_SEEDS, dtype=np.int64),
               second_use_cutmix=np.array([s[0] for s in second]),
               second_lam=np.array([s[1] for s in second], dtype=np.float64),
               second_box=np.array([s[2:] for s in second], dtype=np.int64))
    out['ce_label_smoothing'] = np.float64(loss.LabelSmoothingCrossEntropy(0.1)(scores, y).item())
    out['ce_soft_target'] = np.float64(loss.SoftTargetCrossEntropy()(scores, torch.from_numpy(targets[11])).item())
    print('LabelSmoothingCrossEntropy(0.1) %.6f   SoftTargetCrossEntropy(seed-11 target) %.6f' % (
        out['ce_label_smoothing'], out['ce_soft_target']))
    np.savez_compressed(os.path.join(HERE, 'mixup_params.npz'), **out)


def _acc(scores, target, k):
    lab = target.argmax(axis=1)
    top = np.argsort(-scores, axis=1, kind='stable')[:, :k]
    return 100.0 * float((top == lab[:, None]).any(axis=1).mean())


def run_case(name, arch, classes, N):
    torch.manual_seed(0)
    ns, mix, loss_mod = load_reference()
    crit = loss_mod.SoftTargetCrossEntropy()
    cfg = dict(name='MAE_FINETUNE', architecture=copy.deepcopy(arch),
               head=dict(name='VisionTransformerClsHead', num_classes=classes, in_channels=arch['embed_dim']))
    model = ns.build_model(cfg)
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    st = finetune_state(keys_shapes)
    with torch.no_grad():
        for k, v in sd.items():
            v.copy_(st[k])
    model.train()
    opt = MAEOracle(dict(img_size=32, patch_size=16, embed_dim=32, depth=1, decoder_embed_dim=32, decoder_depth=1,
                         mlp_ratio=1.0), **SOLVER)              # (its AdamW rule only; the state comes from the model)
    hw = arch.get('img_size', 224)
    gen = torch.Generator().manual_seed(909)
    feats = {}
    model.head.register_forward_pre_hook(lambda mod, args: feats.update(x=args[0].detach().clone()))
    out = {}
    seeds = []
    for s, seed in enumerate(MU.FT_SEEDS):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        if s == 0:
            with torch.no_grad():
                res = model(x, y, mode='train')
            out['s0_loss_plain'] = np.float64(res['loss'].item())
            out['s0_feat_head_plain'] = feats['x'][:, :8].numpy().copy()
        want_cutmix = s == 1
        while True:
            np.random.seed(seed)
            rec = Recorder(mix, num_classes=classes, **MU.RECIPE)
            xm, t, (use_cutmix, lam, box) = rec(x, y)
            if use_cutmix != want_cutmix:
                seed += 1
                continue
            assert torch.equal(xm.view(torch.int32), restated(x, use_cutmix, lam, box).view(torch.int32))
            for p in model.parameters():
                p.grad = None
            scores = model.head(model.backbone_forward(xm))
            loss = crit(scores, t)
            if s == 0:
                f, f0 = feats['x'][:, :8].numpy(), out['s0_feat_head_plain']
                d_loss = abs(loss.item() - out['s0_loss_plain']) / abs(out['s0_loss_plain'])
                d_feat = np.abs(f - f0).max() / np.abs(f0).max()
                print(name, 'seed', seed, 'mixed vs plain: loss %.2e rel, feat %.2e of max' % (d_loss, d_feat))
                if not (d_loss > 2 * MU.FT_TOL_F32['loss'] and d_feat > 3 * MU.FT_TOL_F32['feat']):
                    seed += 1
                    continue
            break
        seeds.append(seed)
        loss.backward()
        ps = dict(model.named_parameters())
        grads = {n: ps[n].grad.detach().clone() for n in ps if ps[n].grad is not None}
        opt.st = {n: p.detach().clone() for n, p in model.state_dict().items()}
        opt.apply_adamw(grads)
        with torch.no_grad():
            for n, p in model.state_dict().items():
                p.copy_(opt.st[n])
        pre = 's%d_' % s
        sc, tn = scores.detach().double().numpy(), t.double().numpy()
        out[pre + 'use_cutmix'] = np.bool_(use_cutmix)
        out[pre + 'lam'] = np.float64(lam)
        out[pre + 'box'] = np.array(box, dtype=np.int64)
        out[pre + 'target_argmax'] = tn.argmax(axis=1).astype(np.int64)
        out[pre + 'target_max'] = tn.max(axis=1)
        out[pre + 'x_mixed_sub'] = xm[:, :, ::hw // 8, ::hw // 8].numpy().copy()
        out[pre + 'loss'] = np.float64(loss.item())
        out[pre + 'acc1'] = np.float64(_acc(sc, tn, 1))
        out[pre + 'acc5'] = np.float64(_acc(sc, tn, 5))
        out[pre + 'feat_head'] = feats['x'][:, :8].numpy().copy()
        out[pre + 'score_head'] = scores.detach()[:, :8].numpy().copy()
        for n in WATCH:
            out[pre + 'gradnorm/' + n] = np.float64(grads[n].double().norm().item())
            out[pre + 'pnorm/' + n] = np.float64(opt.st[n].double().norm().item())
        print(name, 'step', s, 'seed', seed, 'cutmix' if use_cutmix else 'mixup', 'lam %.6f box %s loss %.6f acc1 %.1f '
              'acc5 %.1f' % (lam, box, out[pre + 'loss'], out[pre + 'acc1'], out[pre + 'acc5']))
    out['meta'] = np.array([N, hw, len(seeds), classes], dtype=np.int64)
    out['seeds'] = np.array(seeds, dtype=np.int64)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)


if __name__ == '__main__':
    assert ref_runner.available(), 'needs the reference tree'
    for name in (sys.argv[1:] or ['mixup_params'] + list(CASES)):
        if name == 'mixup_params':
            make_params()
        else:
            run_case(name, **CASES[name])
