"""Generate tests/golden/mae_ft_lrd_small.npz by EXECUTING THE REFERENCE's fine-tuning sources WITH ITS PARAMETER GROUPS
— the twin of make_golden_mae_finetune_droppath.py: same model sources (MAE_FINETUNE over MAE_ViT,
passl_v110/modeling/backbones/mae.py:190-314), same state (oracle.mae.finetune_state), same inputs
(Generator().manual_seed(909)); drop-path 0, 3 steps, lr 1e-3, wd 0.05, layer_decay 0.65.

    python tests/golden/make_golden_mae_finetune_lrd.py

Three runs, each from the same state, all through the reference's own optimizer passl/optimizer/adamw.py (loaded by
oracle/ref_runner_v2.load_solver; its one kernel call ``_C_ops.adamw`` is answered by ref_runner_v2._adamw_op):
  A  the v2 rule: tasks/ssl/mae/util/lr_decay.py (loaded from the reference tree at run time) called on
     ``model.backbone`` with {'pos_embed', 'cls_token', 'dist_token'} as main_finetune.py:478-484 does, plus the head as
     two groups at the top id (multiplier 1; weight decayed, bias not);
  B  the v110 rule: get_parameter_groups / LayerDecayValueAssigner of passl_v110/solver/builder.py:91-159 (the module
     is executed from the tree) called on the whole model with ``num_layers = len(backbone.blocks)`` (the reference's
     MAE_ViT has no get_num_layers()); the group's ``learning_rate`` is fed to the optimizer as ``lr_scale``
     [Paddle-semantics: a group's learning_rate is a multiplier];
  U  one uniform group: what AdamW over a plain parameter list does.
Stored per run and step: the loss; pnorm and dnorm = |p_after - p_before| (float64) of the WATCH parameters; p_after and
min / max |gradient| of the ELEMENTWISE ones; and the tables (name, multiplier, decay per parameter) of A and B.
tests/lrd_util.check_golden states what the file must satisfy; it is asserted here before the file is written."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_runner, ref_runner_v2       # noqa: E402
from oracle.mae import finetune_state              # noqa: E402
import lrd_util                                    # noqa: E402

SOLVER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
LAYER_DECAY = 0.65
ARCH = dict(name='MAE_ViT', patch_size=16, embed_dim=128, depth=4, num_heads=4, qkv_bias=True, mlp_ratio=4, img_size=64)
CLASSES, N, STEPS = 16, 8, 3
WATCH = ['backbone.cls_token', 'backbone.pos_embed', 'backbone.patch_embed.proj.weight',
         'backbone.blocks.0.attn.qkv.weight', 'backbone.blocks.0.norm1.weight', 'backbone.blocks.1.attn.proj.bias',
         'backbone.blocks.1.norm2.weight', 'backbone.blocks.2.mlp.fc1.weight', 'backbone.blocks.3.attn.proj.weight',
         'backbone.blocks.3.norm1.weight', 'backbone.fc_norm.weight', 'backbone.fc_norm.bias', 'head.fc_cls.weight',
         'head.fc_cls.bias']
# stored element by element (<= 4 K elements each): every one is treated differently from run U in both rules, and
# none has a gradient element below 1e-4 of the tensor's largest at any step of any run (lrd_util.check_golden (c))
ELEMENTWISE = ['backbone.cls_token', 'backbone.blocks.0.norm1.weight', 'backbone.blocks.1.attn.proj.bias',
               'backbone.blocks.1.norm2.weight', 'backbone.blocks.3.norm1.weight', 'backbone.fc_norm.weight']


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_rules():
    """-> (the reference's v2 lr_decay module, its v110 solver/builder module), executed from the tree."""
    import paddle
    lrd = _load_file('ref_mae_lr_decay', os.path.join(ref_runner.REF_ROOT, 'tasks', 'ssl', 'mae', 'util', 'lr_decay.py'))
    if 'paddle.nn.clip' not in sys.modules:                 # builder.py:18 imports two classes the rule never uses
        clip = types.ModuleType('paddle.nn.clip')
        clip.ClipGradByGlobalNorm = clip.ClipGradByNorm = None
        sys.modules['paddle.nn.clip'] = clip
        paddle.nn.clip = clip
    ref_runner._pkg(ref_runner.PKG + '.solver', os.path.join(ref_runner.REF_ROOT, 'passl_v110', 'solver'))
    builder = importlib.import_module(ref_runner.PKG + '.solver.builder')
    return lrd, builder


def build(ns):
    torch.manual_seed(0)
    model = ns.build_model(dict(name='MAE_FINETUNE', architecture=dict(ARCH),
                                head=dict(name='VisionTransformerClsHead', num_classes=CLASSES,
                                          in_channels=ARCH['embed_dim'])))
    sd = model.state_dict()
    keys_shapes = [(k, tuple(v.shape)) for k, v in sd.items()]
    st = finetune_state(keys_shapes)
    with torch.no_grad():
        for k, v in sd.items():
            v.copy_(st[k])
    model.train()
    return model, keys_shapes


def groups_of(run, model, lrd, builder):
    wd = SOLVER['weight_decay']
    if run == 'A':
        groups = lrd.param_groups_lrd(model.backbone, wd, no_weight_decay_list={'pos_embed', 'cls_token', 'dist_token'},
                                      layer_decay=LAYER_DECAY)
        head = list(model.head.named_parameters())
        groups.append({'lr_scale': 1.0, 'weight_decay': wd, 'params': [p for _n, p in head if p.ndim != 1]})
        groups.append({'lr_scale': 1.0, 'weight_decay': 0., 'params': [p for _n, p in head if p.ndim == 1]})
        return groups
    if run == 'B':
        num_layers = len(model.backbone.blocks)
        assigner = builder.LayerDecayValueAssigner(list(LAYER_DECAY ** (num_layers + 1 - i)
                                                        for i in range(num_layers + 2)))
        groups = builder.get_parameter_groups(dict(weight_decay=wd), model, get_num_layer=assigner.get_layer_id,
                                              get_layer_scale=assigner.get_scale)
        return [{'lr_scale': g['learning_rate'], 'weight_decay': g['weight_decay'], 'params': g['params']}
                for g in groups]
    return [{'params': list(model.parameters())}]


def run_one(run, ns, solver, lrd, builder, out):
    model, keys_shapes = build(ns)
    groups = groups_of(run, model, lrd, builder)
    named = list(model.named_parameters())
    if run != 'U':
        of = {}
        for g in groups:
            for p in g['params']:
                assert id(p) not in of
                of[id(p)] = (g['lr_scale'], g['weight_decay'])
        assert len(of) == len(named)
        out['table_names'] = np.array([n for n, _p in named])
        out['table_%s_scale' % run] = np.array([of[id(p)][0] for _n, p in named], dtype=np.float64)
        out['table_%s_wd' % run] = np.array([of[id(p)][1] for _n, p in named], dtype=np.float64)
    opt = solver.adamw.AdamW(groups, **SOLVER)
    ps = dict(named)
    hw = ARCH['img_size']
    gen = torch.Generator().manual_seed(909)
    for s in range(STEPS):
        x = torch.randn(N, 3, hw, hw, generator=gen)
        y = torch.randint(0, CLASSES, (N,), generator=gen)
        for p in model.parameters():
            p.grad = None
        res = model(x, y, mode='train')
        res['loss'].backward()
        before = {n: ps[n].detach().clone() for n in WATCH}
        opt.step()
        pre = '%s_s%d_' % (run, s)
        out[pre + 'loss'] = np.float64(res['loss'].item())
        for n in WATCH:
            after = ps[n].detach()
            out[pre + 'pnorm/' + n] = np.float64(after.double().norm().item())
            out[pre + 'dnorm/' + n] = np.float64((after.double() - before[n].double()).norm().item())
        for n in ELEMENTWISE:
            assert ps[n].numel() <= 4096
            g = ps[n].grad.detach().abs()
            out[pre + 'p/' + n] = ps[n].detach().numpy().copy()
            out[pre + 'gmin/' + n] = np.float64(g.min().item())
            out[pre + 'gmax/' + n] = np.float64(g.max().item())
        print(run, 'step', s, 'loss %.6f' % out[pre + 'loss'])
    return keys_shapes


def survey(out):
    """min|g| / max|g| of every stored tensor (choosing ELEMENTWISE) and the figures of conditions (a) and (b)."""
    for n in ELEMENTWISE:
        r = min(float(out['%s_s%d_gmin/%s' % (run, s, n)]) / float(out['%s_s%d_gmax/%s' % (run, s, n)])
                for run in lrd_util.RUNS for s in range(STEPS))
        print('min|g|/max|g| %-40s %.2e' % (n, r))
    for run in ('A', 'B'):
        for n in WATCH:
            gaps = ['%.3f' % lrd_util.dnorm_gap(out, run, s, n) for s in range(STEPS)]
            d = ['%.2e' % lrd_util.elem_dist(out, run, s, n) for s in range(STEPS)] if n in ELEMENTWISE else ''
            print(run, '%-40s dnorm gap to U %s  D %s' % (n, gaps, d))


if __name__ == '__main__':
    assert ref_runner.available() and ref_runner_v2.available(), 'needs the reference tree'
    ns = ref_runner.load()
    solver = ref_runner_v2.load_solver(ref_runner_v2.load())
    lrd, builder = load_rules()
    out = {}
    for run in lrd_util.RUNS:
        keys_shapes = run_one(run, ns, solver, lrd, builder, out)
    out['meta'] = np.array([N, ARCH['img_size'], STEPS, CLASSES], dtype=np.int64)
    out['lr'] = np.float64(SOLVER['lr'])
    out['weight_decay'] = np.float64(SOLVER['weight_decay'])
    out['layer_decay'] = np.float64(LAYER_DECAY)
    out['watch'] = np.array(WATCH)
    out['elementwise'] = np.array(ELEMENTWISE)
    out['keys'] = np.array(['%s:%s' % (k, 'x'.join(map(str, s_))) for k, s_ in keys_shapes])
    survey(out)
    lrd_util.check_golden(out)
    path = os.path.join(HERE, 'mae_ft_lrd_small.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
