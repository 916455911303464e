"""Generate tests/golden/mae_ft_dp_*.npz by EXECUTING THE REFERENCE's fine-tuning sources WITH STOCHASTIC DEPTH —
MAE_FINETUNE over MAE_ViT(drop_path_rate=r) (passl_v110/modeling/backbones/mae.py:190-314; DropPath :32-50, the ladder
linspace(0, r, depth) :234, its two uses per Block :186-187) — the twin of make_golden_mae_finetune.py: same state
(oracle.mae.finetune_state), inputs (Generator().manual_seed(909)), AdamW rule and recorded quantities.

    python tests/golden/make_golden_mae_finetune_droppath.py

The paddle shim (oracle/ref_runner.py) has paddle.rand and paddle.linspace but no paddle.floor: this script adds
``paddle.floor = torch.floor`` to the loaded shim module at run time and wraps ``paddle.rand`` to record the draws.
Every training forward draws 2 * (depth - 1) vectors of length N (block 0 holds Identity); the keep table of the step is
``floor(float32(1 - p_i) + u)``, stored as s<k>_keep [2 * depth, N] (row 2i = attention branch of block i, row 2i + 1 =
its MLP branch, ones for block 0) — what the product's ``drop_path_keep=`` takes.  Step 0 is also run with every DropPath
in eval mode (s0_loss_nodrop / s0_feat_head_nodrop): the distance a test must be able to see."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_runner                      # noqa: E402
from oracle.mae import MAEOracle, finetune_state   # noqa: E402

SOLVER = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05)        # mae_vit_b_finetune.yaml:58-62
ARCH_YAML = dict(name='MAE_ViT', patch_size=16, embed_dim=768, depth=12, num_heads=12, qkv_bias=True, mlp_ratio=4)
CASES = {
    'mae_ft_dp_small': dict(arch=dict(ARCH_YAML, embed_dim=128, depth=4, num_heads=4, img_size=64, drop_path_rate=0.3),
                            classes=16, N=8, steps=2),
    # the yaml's architecture as written (ViT-B/16, 224^2: 197 tokens), 1000 classes, the recipe's rate
    'mae_ft_dp_vit_b': dict(arch=dict(ARCH_YAML, drop_path_rate=0.1), classes=1000, N=8, steps=2),
}
WATCH = ['backbone.cls_token', 'backbone.pos_embed', 'backbone.patch_embed.proj.weight', 'backbone.blocks.0.attn.qkv.weight',
         'backbone.blocks.1.mlp.fc2.bias', 'backbone.blocks.1.norm2.weight', 'backbone.fc_norm.weight',
         'backbone.fc_norm.bias', 'head.fc_cls.weight', 'head.fc_cls.bias']


def check_table(keep, depth, N, first_step):
    """What a fixture must satisfy to test anything (tests/test_droppath_host.py re-asserts it on the committed files)."""
    assert keep.shape == (2 * depth, N) and keep.dtype == np.float32
    assert np.all((keep == 0) | (keep == 1))
    assert np.all(keep[:2] == 1)
    if first_step:
        dropped = keep == 0
        assert dropped.sum() >= 5 and dropped.any(axis=1).sum() >= 3, (int(dropped.sum()), int(dropped.any(axis=1).sum()))


def run_case(name, arch, classes, N, steps):
    torch.manual_seed(0)
    ns = ref_runner.load()
    paddle = sys.modules['paddle']
    if not hasattr(paddle, 'floor'):
        paddle.floor = torch.floor
    draws = []
    rand0 = paddle.rand

    def rand(shape, *a, **k):
        u = rand0(shape, *a, **k)
        draws.append(u.detach().clone().reshape(-1))
        return u
    paddle.rand = rand
    try:
        _run(ns, draws, name, arch, classes, N, steps)
    finally:
        paddle.rand = rand0


def _run(ns, draws, name, arch, classes, N, steps):
    cfg = dict(name='MAE_FINETUNE', architecture=copy.deepcopy(arch),
               head=dict(name='VisionTransformerClsHead', num_classes=classes, in_channels=arch['embed_dim']))
    model = ns.build_model(cfg)
    depth = arch['depth']
    ladder = torch.linspace(0, arch['drop_path_rate'], depth, dtype=torch.float32).numpy()
    keep_prob = (np.float32(1.0) - ladder).astype(np.float32)
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
    # one DropPath layer per block (used for both of its branches), Identity in block 0
    droppers = [m for m in model.modules() if type(m).__name__ == 'DropPath']
    assert len(droppers) == depth - 1, len(droppers)
    out = {}
    for s in range(steps):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, classes, (N,), generator=gen)
        if s == 0:
            # the same step with nothing dropped (DropPath.forward reads self.training); draws nothing
            for d in droppers:
                d.training = False
            with torch.no_grad():
                res = model(x, y, mode='train')
            for d in droppers:
                d.training = True
            assert not draws
            out['s0_loss_nodrop'] = np.float64(res['loss'].item())
            out['s0_feat_head_nodrop'] = feats['x'][:, :8].numpy().copy()
        for p in model.parameters():
            p.grad = None
        scores = {}
        h = model.head.fc_cls.register_forward_hook(lambda mod, a, o: scores.update(s=o.detach().clone()))
        del draws[:]
        res = model(x, y, mode='train')
        h.remove()
        assert len(draws) == 2 * (depth - 1) and all(u.numel() == N for u in draws), len(draws)
        keep = np.ones((2 * depth, N), dtype=np.float32)
        for j, u in enumerate(draws):                    # draw j belongs to table row j + 2 (forward order)
            kp = keep_prob[(j + 2) // 2]
            keep[j + 2] = np.floor((kp + u.numpy().astype(np.float32)).astype(np.float32))
        check_table(keep, depth, N, s == 0)
        res['loss'].backward()
        ps = dict(model.named_parameters())
        grads = {n: ps[n].grad.detach().clone() for n in ps if ps[n].grad is not None}
        opt.st = {n: p.detach().clone() for n, p in model.state_dict().items()}
        opt.apply_adamw(grads)
        with torch.no_grad():
            for n, p in model.state_dict().items():
                p.copy_(opt.st[n])
        pre = 's%d_' % s
        out[pre + 'keep'] = keep
        out[pre + 'loss'] = np.float64(res['loss'].item())
        out[pre + 'acc1'] = np.float64(float(res['acc1']))
        out[pre + 'acc5'] = np.float64(float(res['acc5']))
        out[pre + 'feat_head'] = feats['x'][:, :8].numpy().copy()
        out[pre + 'score_head'] = scores['s'][:, :8].numpy().copy()
        for n in WATCH:
            out[pre + 'gradnorm/' + n] = np.float64(grads[n].double().norm().item())
            out[pre + 'pnorm/' + n] = np.float64(opt.st[n].double().norm().item())
        dropped = keep == 0
        print(name, 'step', s, 'loss %.6f acc1 %.1f acc5 %.1f  dropped %d of %d in %d rows' % (
            out[pre + 'loss'], out[pre + 'acc1'], out[pre + 'acc5'], int(dropped.sum()), 2 * (depth - 1) * N,
            int(dropped.any(axis=1).sum())))
        if s == 0:
            f, f0 = out['s0_feat_head'], out['s0_feat_head_nodrop']
            print(name, 'step 0 dropped vs not: loss %.2e rel, feat %.2e of max' % (
                abs(out['s0_loss'] - out['s0_loss_nodrop']) / abs(out['s0_loss_nodrop']),
                np.abs(f - f0).max() / np.abs(f0).max()))
    out['meta'] = np.array([N, hw, steps, classes], dtype=np.int64)
    out['rate'] = np.float64(arch['drop_path_rate'])
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)


if __name__ == '__main__':
    assert ref_runner.available(), 'needs the reference tree'
    for name in (sys.argv[1:] or list(CASES)):
        run_case(name, **CASES[name])
