"""What AdamW parameter groups cost on the MI355X (DESIGN.md "AdamW parameter groups"): the grouped launch against the
flat one on the same bytes, and a whole fine-tuning step with and without ``layer_decay``.

    python tools/adamw_groups_bench.py kernels [--out profiles/adamw_groups_kernels.txt]
    python tools/adamw_groups_bench.py step    [--out profiles/adamw_groups_step.txt]

kernels: the ViT-B/16 fine-tuning arena (MAE_FINETUNE, 1000 classes: about 86 M fp32 elements; parameters, gradients
and both moments = 1.4 GB, far more than the last-level cache holds) updated by passl_hip_adamw_groups_dev with the
table build_optimizer makes for ``layer_decay: 0.65`` and by passl_hip_adamw_dev — the update every recipe ran before —
on the same buffers.  Device events around windows of back-to-back launches, the two kernels alternating inside every
repetition; the median of the repetitions is compared.  The grouped kernel moves the same bytes plus a table of a few
KB, so the target is parity, and its margin is the flat kernel's own max - min over the repetitions of this run, no
more.  Exit status 1 when the grouped median lies above the flat median by more than that.

step: configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml at batch 128 bf16 (stochastic depth, Mixup) with the
optimizer build_optimizer makes of the YAML as written and of the YAML plus ``layer_decay: 0.65``, and a third model with
the YAML's optimizer again as a control (models built later in a process are not equally fast), all alive in one
process, windows of eager steps alternating.  No bound."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYER_DECAY = 0.65


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n            # ms per call


def _recipe(overrides=()):
    from passl_amd.utils.config import get_config
    return get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml'), list(overrides))


def _model(cfg):
    from passl_amd.modeling import build_model
    mc = dict(cfg.model)
    mc['architecture'] = dict(cfg.model.architecture)
    mc['head'] = dict(cfg.model.head)
    model = build_model(mc)
    model.train()
    return model


def kernels(args):
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.solver.builder import build_optimizer
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    cfg = _recipe()
    torch.manual_seed(0)
    model = _model(cfg)
    ocfg = dict(cfg.optimizer, layer_decay=LAYER_DECAY)
    opt = build_optimizer(ocfg, 1e-3, [model])
    table, arena = opt._tables[0], model.arena_q
    n = arena.n_train
    p, m, v = arena.flat[:n], opt._m[0], opt._v[0]
    g = arena.grads
    g.copy_(torch.randn(n, generator=torch.Generator().manual_seed(1)).to(g.device) * 1e-3)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 0.0], dtype=torch.float32, device=p.device)
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, float(cfg.optimizer.weight_decay)
    variants = [('passl_hip_adamw_dev (flat)', lambda _i: ops.adamw_dev(p, g, m, v, hyper, b1, b2, eps, wd, 1.0)),
                ('passl_hip_adamw_groups_dev', lambda _i: ops.adamw_groups_dev(p, g, m, v, table, hyper, b1, b2, eps, 1.0))]
    times = {name: [] for name, _f in variants}
    for _name, f in variants:                       # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.reps):
        for name, f in variants:                    # alternating: drift hits both alike
            times[name].append(_window(f, args.launches))
    nbytes = n * 4 * 7                              # p, g, m, v read; p, m, v written
    lines = ['ViT-B/16 fine-tuning arena: %d fp32 elements, %d parameters in %d segments (layer_decay %.2f, weight decay '
             '%.2f / 0); %.2f GB moved per launch; %d repetitions x %d launches per window, alternating'
             % (n, len(arena.param_slices), table['n_seg'], LAYER_DECAY, wd, nbytes / 1e9, args.reps, args.launches),
             '%-30s %10s %10s %10s %12s' % ('launch', 'median us', 'min us', 'max us', 'GB/s (median)')]
    med = {}
    for name, _f in variants:
        ts = times[name]
        med[name] = statistics.median(ts)
        lines.append('%-30s %10.2f %10.2f %10.2f %12.0f' % (name, med[name] * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                                                            nbytes / (med[name] * 1e-3) / 1e9))
    flat, grp = (med[name] for name, _f in variants)
    spread = max(times[variants[0][0]]) - min(times[variants[0][0]])
    ok = grp - flat <= spread
    lines.append('grouped - flat = %+.2f us (%+.2f %%); margin = the flat kernel\'s max - min = %.2f us: %s'
                 % ((grp - flat) * 1e3, 100 * (grp / flat - 1), spread * 1e3, 'HOLDS' if ok else 'MISSED'))
    return lines, ok


def step(args):
    from passl_amd.datasets.preprocess import build_mixup
    from passl_amd.hip import config as hip_config
    from passl_amd.solver.builder import build_optimizer
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    cfg = _recipe()
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    block = [dict(b) for b in cfg.dataloader.train.dataset.batch_transforms]
    runs = {}
    variants = (('optimizer as in the recipe YAML', {}), ('+ layer_decay %.2f' % LAYER_DECAY, dict(layer_decay=LAYER_DECAY)),
                ('as in the YAML, a third model (control)', {}))
    for name, extra in variants:
        torch.manual_seed(0)
        model = _model(cfg)
        opt = build_optimizer(dict(cfg.optimizer, **extra), 1e-3, [model])
        assert (opt._tables[0] is not None) == bool(extra)
        mixup_fn = build_mixup(block)
        mixup_fn.rng = np.random.RandomState(0)

        def one(_i, model=model, opt=opt, mixup_fn=mixup_fn):
            out = model(x, y, mode='train', mixup_fn=mixup_fn)
            opt.clear_grad()
            out['loss'].backward()
            opt.step()
        runs[name] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.reps):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, drop_path_rate 0.1, Mixup, batch %d, bf16, eager steps; %d repetitions x %d steps per '
             'window, alternating' % (B, args.reps, args.steps), '%-40s %10s %9s %9s' % ('', 'median ms', 'min ms', 'max ms')]
    med = []
    for r in runs:
        ts = times[r]
        med.append(statistics.median(ts))
        lines.append('%-40s %10.3f %9.3f %9.3f' % (r, med[-1], min(ts), max(ts)))
    t0 = times[list(runs)[0]]
    lines.append('layer_decay - YAML = %+.3f ms per step (%+.2f %%); control - YAML = %+.3f ms (%+.2f %%: what a model built '
                 'later in the process costs by itself); spread of the first model\'s windows %.2f %%'
                 % (med[1] - med[0], 100 * (med[1] / med[0] - 1), med[2] - med[0], 100 * (med[2] / med[0] - 1),
                    100 * (max(t0) - min(t0)) / med[0]))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('adamw_groups_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
