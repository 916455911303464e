"""What global-norm gradient clipping costs on the MI355X (DESIGN.md "Global-norm gradient clipping"): the sum-of-squares
pass against a copy of the same bytes, the clip variants of the AdamW update against the existing kernels on the same
buffers, and a whole fine-tuning step with and without ``grad_clip``.

    python tools/grad_clip_bench.py kernels [--out profiles/grad_clip_kernels.txt]
    python tools/grad_clip_bench.py step    [--out profiles/grad_clip_step.txt]

kernels: the ViT-B/16 fine-tuning arena (MAE_FINETUNE, 1000 classes: about 86 M fp32 elements, 346 MB of gradients — more
than the last-level cache holds).  Device events around windows of back-to-back launches, the variants alternating inside
every repetition; medians are compared.
  * passl_hip_grad_sumsq over the whole gradient buffer (one set) against passl_hip_copy_bytes of the same byte count out
    of the same buffer.  The bound was set before anything was measured: the pass is not slower than that copy, which
    moves twice the traffic.  Exit status 1 when it is missed.  The finalize launch is timed next to it.
  * passl_hip_adamw_clip_dev against passl_hip_adamw_dev, and passl_hip_adamw_groups_clip_dev (the table of
    ``layer_decay: 0.65``, one set per group) against passl_hip_adamw_groups_dev.  The clip variants move the same bytes
    plus one coefficient per segment: the target is parity, reported next to the flat kernel's own max - min over the
    repetitions of this run.

step: configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml at batch 128 bf16 (stochastic depth, Mixup) with the YAML's
optimizer, with the same optimizer + ``grad_clip=ClipGradByGlobalNorm.like_clip_grad_norm_(1.0)`` (the MAE recipe's
--clip_grad), and a third model with the YAML's optimizer again as a control (models built later in a process are not
equally fast), all alive in one process, windows of eager steps alternating.  No bound."""
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


def _alternate(variants, args):
    times = {name: [] for name, _f in variants}
    for _name, f in variants:                       # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.reps):
        for name, f in variants:                    # alternating: drift hits both alike
            times[name].append(_window(f, args.launches))
    return times


def _rows(variants, times, nbytes):
    lines, med = [], {}
    for name, _f in variants:
        ts = times[name]
        med[name] = statistics.median(ts)
        lines.append('%-36s %10.2f %10.2f %10.2f %12.0f' % (name, med[name] * 1e3, min(ts) * 1e3, max(ts) * 1e3,
                                                            nbytes[name] / (med[name] * 1e-3) / 1e9))
    return lines, med


def kernels(args):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    from passl_amd.solver.lr_decay import LayerDecayValueAssigner, get_parameter_groups
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    cfg = _recipe()
    torch.manual_seed(0)
    model = _model(cfg)
    wd = float(cfg.optimizer.weight_decay)
    arena = model.arena_q
    n = arena.n_train
    flat = AdamW(1e-3, weight_decay=wd, parameters=list(model.parameters()), grad_clip=ClipGradByGlobalNorm(1.0))
    num_layers = model.backbone.get_num_layers()
    assigner = LayerDecayValueAssigner([LAYER_DECAY ** (num_layers + 1 - i) for i in range(num_layers + 2)])
    groups = get_parameter_groups(dict(weight_decay=wd), model, get_num_layer=assigner.get_layer_id,
                                  get_layer_scale=assigner.get_scale)
    grouped = AdamW(1e-3, weight_decay=wd, parameters=groups, grad_clip=ClipGradByGlobalNorm(1.0))
    plain = AdamW(1e-3, weight_decay=wd, parameters=groups)
    assert flat._tables[0] is None and flat._clip['n_sets'] == 1 and 'seg_set' in grouped._tables[0]
    p, m, v, g = arena.flat[:n], flat._m[0], flat._v[0], arena.grads
    g.copy_(torch.randn(n, generator=torch.Generator().manual_seed(1)).to(g.device) * 1e-3)
    scratch = torch.empty(n, dtype=torch.float32, device=g.device)
    hyper = torch.tensor([1e-3, 0.9, 0.999, 0.0], dtype=torch.float32, device=p.device)
    b1, b2, eps = 0.9, 0.999, 1e-8
    lib, st = L.load(), L.stream()
    plan, gplan = flat._clip, grouped._clip
    ops.grad_sumsq(g, gplan, 0, 1.0)
    ops.grad_clip_finalize(gplan, 1.0)
    ops.grad_sumsq(g, plan, 0, 1.0)
    ops.grad_clip_finalize(plan, 1.0)
    coef = flat._clip_coef[0]
    lines = ['ViT-B/16 fine-tuning arena: %d fp32 elements (%.1f MB of gradients), %d parameters; one set = %d chunks of %d, '
             '%d sets (layer_decay %.2f) = %d chunks in %d segments; %d repetitions x %d launches per window, alternating'
             % (n, n * 4 / 1e6, len(arena.param_slices), plan['total'], ops.GRAD_CLIP_CHUNK, gplan['n_sets'], LAYER_DECAY,
                gplan['total'], grouped._tables[0]['n_seg'], args.reps, args.launches),
             '%-36s %10s %10s %10s %12s' % ('launch', 'median us', 'min us', 'max us', 'GB/s (median)')]
    # 1. the read
    v1 = [('passl_hip_copy_bytes (same bytes)', lambda _i: L.check(lib.passl_hip_copy_bytes(scratch.data_ptr(), g.data_ptr(), n * 4, st))),
          ('passl_hip_grad_sumsq (1 set)', lambda _i: ops.grad_sumsq(g, plan, 0, 1.0)),
          ('passl_hip_grad_sumsq (%d sets)' % gplan['n_sets'], lambda _i: ops.grad_sumsq(g, gplan, 0, 1.0)),
          ('passl_hip_grad_clip_finalize (%d)' % gplan['n_sets'], lambda _i: ops.grad_clip_finalize(gplan, 1.0))]
    t1 = _alternate(v1, args)
    nb = {v1[0][0]: n * 8, v1[1][0]: n * 4, v1[2][0]: n * 4, v1[3][0]: gplan['total'] * 4}
    rows, med = _rows(v1, t1, nb)
    lines += rows
    copy_t, sum_t = med[v1[0][0]], med[v1[1][0]]
    ok = sum_t <= copy_t
    lines.append('sum of squares / copy = %.3f (bound set in advance: <= 1, the copy moves twice the bytes): %s'
                 % (sum_t / copy_t, 'HOLDS' if ok else 'MISSED'))
    # 2. the updates
    gt, pt = grouped._tables[0], plain._tables[0]
    v2 = [('passl_hip_adamw_dev (flat)', lambda _i: ops.adamw_dev(p, g, m, v, hyper, b1, b2, eps, wd, 1.0)),
          ('passl_hip_adamw_clip_dev', lambda _i: ops.adamw_clip_dev(p, g, m, v, hyper, coef, b1, b2, eps, wd, 1.0)),
          ('passl_hip_adamw_groups_dev', lambda _i: ops.adamw_groups_dev(p, g, m, v, pt, hyper, b1, b2, eps, 1.0)),
          ('passl_hip_adamw_groups_clip_dev', lambda _i: ops.adamw_groups_clip_dev(p, g, m, v, gt, hyper, gplan['out'], b1, b2,
                                                                                   eps, 1.0))]
    t2 = _alternate(v2, args)
    rows, med = _rows(v2, t2, {name: n * 4 * 7 for name, _f in v2})          # p, g, m, v read; p, m, v written
    lines += rows
    spread = max(t2[v2[0][0]]) - min(t2[v2[0][0]])
    for a, b in ((v2[1][0], v2[0][0]), (v2[3][0], v2[2][0])):
        d = med[a] - med[b]
        lines.append('%s - %s = %+.2f us (%+.2f %%); the flat kernel\'s max - min = %.2f us: parity %s'
                     % (a, b, d * 1e3, 100 * (med[a] / med[b] - 1), spread * 1e3, 'HOLDS' if d <= spread else 'MISSED'))
    return lines, ok


def step(args):
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm
    from passl_amd.datasets.preprocess import build_mixup
    from passl_amd.hip import config as hip_config
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    cfg = _recipe()
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    block = [dict(b) for b in cfg.dataloader.train.dataset.batch_transforms]
    ocfg = {k: val for k, val in dict(cfg.optimizer).items() if k != 'name'}
    assert cfg.optimizer.name == 'AdamW'
    runs = {}
    variants = (('optimizer as in the recipe YAML', None), ('+ grad_clip (clip_grad_norm_ 1.0)', ClipGradByGlobalNorm.like_clip_grad_norm_(1.0)),
                ('as in the YAML, a third model (control)', None))
    for name, gc in variants:
        torch.manual_seed(0)
        model = _model(cfg)
        opt = AdamW(1e-3, parameters=list(model.parameters()), grad_clip=gc, **ocfg)
        assert (opt._clip is not None) == (gc is not None) and opt._tables[0] is None
        mixup_fn = build_mixup(block)
        mixup_fn.rng = np.random.RandomState(0)

        def one(_i, model=model, opt=opt, mixup_fn=mixup_fn):
            out = model(x, y, mode='train', mixup_fn=mixup_fn)
            opt.clear_grad()
            out['loss'].backward()
            opt.step()
        runs[name] = (one, opt)
    times = {r: [] for r in runs}
    for r, (f, _o) in runs.items():
        _window(f, args.steps)
    for _ in range(args.reps):
        for r, (f, _o) in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, drop_path_rate 0.1, Mixup, batch %d, bf16, eager steps; %d repetitions x %d steps per '
             'window, alternating' % (B, args.reps, args.steps), '%-40s %10s %9s %9s' % ('', 'median ms', 'min ms', 'max ms')]
    med = []
    for r in runs:
        ts = times[r]
        med.append(statistics.median(ts))
        lines.append('%-40s %10.3f %9.3f %9.3f' % (r, med[-1], min(ts), max(ts)))
    t0 = times[list(runs)[0]]
    norm, coef = runs[variants[1][0]][1].grad_norms()[0].tolist()
    lines.append('grad_clip - YAML = %+.3f ms per step (%+.2f %%); control - YAML = %+.3f ms (%+.2f %%: what a model built '
                 'later in the process costs by itself); spread of the first model\'s windows %.2f %%; last norm %.3f, '
                 'coefficient %.4f' % (med[1] - med[0], 100 * (med[1] / med[0] - 1), med[2] - med[0],
                                       100 * (med[2] / med[0] - 1), 100 * (max(t0) - min(t0)) / med[0], norm, coef))
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
        raise SystemExit('grad_clip_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
