"""What the Adan update costs on the MI355X (DESIGN.md "Adan"): the flat launch against the flat AdamW launch on the
same buffers, and a whole supervised ViT-B step with Adan and with AdamW.

    python tools/adan_bench.py kernels [--out profiles/adan_kernels.txt]
    python tools/adan_bench.py step    [--out profiles/adan_step.txt]

kernels: six fp32 vectors of the ViT-B arena size (86.6 M elements: 2.1 GB, far more than the last-level cache holds).
passl_hip_adan_dev reads six and writes five of them (44 B per element, 3.81 GB per launch), passl_hip_adamw_dev reads
four and writes three (28 B per element, 2.42 GB).  Device events around windows of back-to-back launches, the two
kernels alternating inside every repetition; the median of the repetitions is compared in BYTES PER SECOND.  The bound
was set before the kernel was first measured: Adan's achieved bytes/s is at least 1 / 1.25 of AdamW's in the same run
(the quarter allows for eleven concurrent streams against seven).  Exit status 1 when it is missed.  The clip and the
grouped variants (a ViT-B-like table of 150 segments with 14 multipliers) are reported beside the flat one, no bound.

step: configs/v2/vit_base_adan_synthetic.yaml at batch 128, one micro-batch, bf16, through the Engine's training step,
and the same config with ``Optimizer: {name: AdamW, weight_decay: 0.02}``, both alive in one process, windows of eager
steps alternating.  No bound: the difference is stated beside the spread of the AdamW windows."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ARENA = 86_600_000                    # the ViT-B arena, rounded: a multiple of 4
BOUND = 1.25                            # Adan bytes/s >= AdamW bytes/s / BOUND — set before measuring
BETAS, EPS, WD = (0.98, 0.92, 0.99), 1e-8, 0.02


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n            # ms per call


def kernels(args):
    from passl_amd.hip import ops
    dev = torch.device('cuda')
    n = args.elements
    gen = torch.Generator().manual_seed(1)
    p = torch.randn(n, generator=gen).to(dev)
    g = (torch.randn(n, generator=gen) * 1e-3).to(dev)
    m, d, s, pre = (torch.zeros(n, device=dev) for _ in range(4))
    hyper = torch.tensor([1e-3, 0.9, 0.8, 0.95, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
    coef = torch.tensor([0.5], dtype=torch.float32, device=dev)
    # a ViT-B-like table: 150 segments, 14 multipliers, two decays
    n_seg = 150
    ends = [(n // 4 * (i + 1) // n_seg) * 4 for i in range(n_seg)]
    scales = [0.65 ** (13 - (i * 14) // n_seg) for i in range(n_seg)]
    wds = [WD if i % 2 else 0.0 for i in range(n_seg)]
    table = ops.adamw_groups_clip_table(ends, scales, wds, [i % 3 - 1 for i in range(n_seg)], n, 2, dev)
    clip = torch.tensor([[2.0, 0.5], [4.0, 0.25]], dtype=torch.float32, device=dev)
    cfg = BETAS + (EPS,)
    adan_b, adamw_b = 44 * n, 28 * n
    variants = [
        ('passl_hip_adamw_dev (flat)', adamw_b, lambda _i: ops.adamw_dev(p, g, m, s, hyper, 0.9, 0.999, EPS, WD, 1.0)),
        ('passl_hip_adan_dev (flat)', adan_b, lambda _i: ops.adan_dev(p, g, m, d, s, pre, hyper, *cfg, WD, False, 1.0)),
        ('passl_hip_adan_clip_dev', adan_b, lambda _i: ops.adan_clip_dev(p, g, m, d, s, pre, hyper, coef, *cfg, WD, False, 1.0)),
        ('passl_hip_adan_groups_dev', adan_b, lambda _i: ops.adan_groups_dev(p, g, m, d, s, pre, table, hyper, *cfg, False, 1.0)),
        ('passl_hip_adan_groups_clip_dev', adan_b,
         lambda _i: ops.adan_groups_clip_dev(p, g, m, d, s, pre, table, hyper, clip, *cfg, False, 1.0)),
    ]
    times = {name: [] for name, _b, _f in variants}
    for _name, _b, f in variants:                   # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.reps):
        for name, _b, f in variants:                # alternating: drift hits all alike
            times[name].append(_window(f, args.launches))
    lines = ['%d fp32 elements per vector; Adan moves %.2f GB per launch (6 read, 5 written), AdamW %.2f GB (4 read, 3 '
             'written); %d repetitions x %d launches per window, alternating' % (n, adan_b / 1e9, adamw_b / 1e9, args.reps, args.launches),
             '%-32s %10s %10s %10s %14s' % ('launch', 'median us', 'min us', 'max us', 'GB/s (median)')]
    rate = {}
    for name, nbytes, _f in variants:
        ts = times[name]
        med = statistics.median(ts)
        rate[name] = nbytes / (med * 1e-3) / 1e9
        lines.append('%-32s %10.2f %10.2f %10.2f %14.0f' % (name, med * 1e3, min(ts) * 1e3, max(ts) * 1e3, rate[name]))
    tw = times[variants[0][0]]
    adamw, adan = rate[variants[0][0]], rate[variants[1][0]]
    ok = adan >= adamw / BOUND
    lines.append('AdamW\'s own spread over the repetitions: max - min = %.2f us (%.2f %% of its median)'
                 % ((max(tw) - min(tw)) * 1e3, 100 * (max(tw) - min(tw)) / statistics.median(tw)))
    lines.append('flat Adan / flat AdamW in bytes per second = %.3f; bound (set before measuring) >= %.3f: %s'
                 % (adan / adamw, 1 / BOUND, 'HOLDS' if ok else 'MISSED'))
    return lines, ok


def step(args):
    from passl_amd.engine.engine import Engine
    from passl_amd.utils.config import AttrDict, get_config
    B = args.batch
    runs = {}
    for name, block in (('AdamW (weight_decay 0.02)', dict(name='AdamW', weight_decay=WD)), ('Adan (the YAML)', None),
                        ('AdamW, a third model (control)', dict(name='AdamW', weight_decay=WD))):
        cfg = get_config(os.path.join(ROOT, 'configs', 'v2', 'vit_base_adan_synthetic.yaml'),
                         ['Global.accum_steps=1', 'Global.eval_during_train=False', 'Global.output_dir=%s' % args.output_dir,
                          'DataLoader.Train.dataset.num_samples=%d' % (B * 4), 'DataLoader.Train.sampler.batch_size=%d' % B,
                          'DataLoader.Eval.dataset.num_samples=%d' % B, 'DataLoader.Eval.sampler.batch_size=%d' % B])
        if block is not None:
            cfg.Optimizer = AttrDict(block)
        torch.manual_seed(0)
        eng = Engine(cfg, mode='train')
        eng.model.train()
        assert type(eng.optimizer).__name__ == ('Adan' if block is None else 'AdamW')
        batch = next(iter(eng.train_dataloader))

        def one(_i, eng=eng, batch=batch):
            eng.train_loop.train_one_step(batch)
        runs[name] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.reps):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['ViT_base_patch16_224, drop_rate 0.1, ViTCELoss, batch %d in one micro-batch, bf16, eager steps of the Engine\'s '
             'training loop; %d repetitions x %d steps per window, alternating' % (B, args.reps, args.steps),
             '%-36s %10s %9s %9s' % ('', 'median ms', 'min ms', 'max ms')]
    med = []
    for r in runs:
        ts = times[r]
        med.append(statistics.median(ts))
        lines.append('%-36s %10.3f %9.3f %9.3f' % (r, med[-1], min(ts), max(ts)))
    t0 = times[list(runs)[0]]
    lines.append('Adan - AdamW = %+.3f ms per step (%+.2f %%); control - AdamW = %+.3f ms (%+.2f %%: what a model built later '
                 'in the process costs by itself); spread of the AdamW windows %.2f %%'
                 % (med[1] - med[0], 100 * (med[1] / med[0] - 1), med[2] - med[0], 100 * (med[2] / med[0] - 1),
                    100 * (max(t0) - min(t0)) / med[0]))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--elements', type=int, default=N_ARENA)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--output-dir', default='./output/')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.elements % 4:
        raise SystemExit('adan_bench: --elements must be a multiple of 4')
    if not torch.cuda.is_available():
        raise SystemExit('adan_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
