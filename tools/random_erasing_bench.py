"""What random erasing costs on the MI355X (DESIGN.md "Random erasing"): the stand-alone erase of
csrc/random_erasing.hip, and a whole fine-tuning step with and without the ``RandomErasing`` entry.

    python tools/random_erasing_bench.py kernels [--out profiles/random_erasing_kernels.txt]
    python tools/random_erasing_bench.py step    [--out profiles/random_erasing_step.txt]

kernels: passl_hip_random_erase, out of place, on [128, 3, 224, 224] fp32 (77 MB) in both modes, the box table drawn
with prob = 1 so that every sample carries a box, next to passl_hip_copy_bytes of the same bytes — the erase reads and
writes every byte of the batch once, the bytes of a copy, and the generator runs inside the boxes only.  Device events
around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands rotating over more
buffers than the last-level cache holds.  One bound, the project's own for the batch mix, set before anything was
measured: each mode within 1.25 x the copy of the same run.  Exit status 1 when it is missed.  The in-place form is
timed as well (no bound: it stores the box elements only).

step: configs/mae/mae_vit_b_finetune_erase_synthetic.yaml at batch 128 bf16 fed by a loader with the eraser that
build_random_erasing makes of its ``transforms`` entry, and without it (= the drop-path YAML), two models alive in one
process, windows of eager steps alternating.  No bound: the difference is what fusing the erase into the batch mix or
into passl_hip_patchify would be judged against."""
import argparse
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n            # ms per call


def _stats(ts):
    m = sum(ts) / len(ts)
    return m, min(ts), max(ts)


def kernels(args):
    from passl_amd.datasets.preprocess import RandomErasing
    from passl_amd.hip import lib as L
    lib = L.load()
    B, C, H, W = args.batch, 3, 224, 224
    nset = 4                                     # 4 x 2 x 77 MB: more than the 256 MB last-level cache
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    sets = [(torch.randn(B, C, H, W, generator=gen).to(dev), torch.empty(B, C, H, W, device=dev)) for _ in range(nset)]
    table = RandomErasing(prob=1., mode='pixel', max_count=1, rng=random.Random(0), seed=1).draw(B, H, W)
    RandomErasing.validate(table, H, W)
    boxes = torch.from_numpy(table).to(dev)
    inside = float((table[:, 2] * table[:, 3]).sum()) / (B * H * W)
    nbytes = B * C * H * W * 4
    p, st = L.ptr, L.stream()

    def copy(i):
        x, z = sets[i % nset]
        L.check(lib.passl_hip_copy_bytes(p(z), p(x), nbytes, st))

    def erase(mode, inplace=False):
        def f(i):
            x, z = sets[i % nset]
            L.check(lib.passl_hip_random_erase(p(x), p(x if inplace else z), p(boxes), B, C, H, W, mode, 1, i, st))
        return f
    box_bytes = int(inside * nbytes)
    variants = [('copy_bytes', copy, 2 * nbytes), ("random_erase mode 0 ('const')", erase(0), 2 * nbytes),
                ("random_erase mode 1 ('pixel')", erase(1), 2 * nbytes),
                ('random_erase mode 0 in place', erase(0, True), box_bytes),
                ('random_erase mode 1 in place', erase(1, True), box_bytes)]
    times = {n: [] for n, _f, _b in variants}
    for _n, f, _b in variants:                     # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.rounds):
        for n, f, _b in variants:                  # alternating: drift hits every variant alike
            times[n].append(_window(f, args.launches))
    lines = ['batch [%d, 3, 224, 224] fp32 = %.1f MB read + %.1f MB written per out-of-place launch; every sample carries '
             'a box, %.1f %% of the elements lie inside one; %d rounds x %d launches per window, %d operand sets'
             % (B, nbytes / 1e6, nbytes / 1e6, 100 * inside, args.rounds, args.launches, nset),
             '%-32s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)')]
    for n, _f, nb in variants:
        m, lo, hi = _stats(times[n])
        lines.append('%-32s %9.2f %9.2f %9.2f %10.0f' % (n, m * 1e3, lo * 1e3, hi * 1e3, nb / (m * 1e-3) / 1e9))
    cm = _stats(times['copy_bytes'])[0]
    m0 = _stats(times["random_erase mode 0 ('const')"])[0]
    m1 = _stats(times["random_erase mode 1 ('pixel')"])[0]
    ok = m0 <= 1.25 * cm and m1 <= 1.25 * cm
    lines.append('random_erase mode 0 / copy_bytes = %.3f, mode 1 / copy_bytes = %.3f (bound 1.25 each: %s)'
                 % (m0 / cm, m1 / cm, 'HOLDS' if ok else 'MISSED'))
    return lines, ok


def step(args):
    from passl_amd.datasets.preprocess import build_random_erasing
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    from passl_amd.solver.optimizer import AdamW
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_erase_synthetic.yaml'), [])
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    entry = [dict(t) for t in cfg.dataloader.train.dataset.transforms]
    runs = {}
    for name, eraser in (('without the RandomErasing entry', None),
                         ('with RandomErasing 0.25 pixel', build_random_erasing(entry))):
        torch.manual_seed(0)
        mc = dict(cfg.model)
        mc['architecture'] = dict(cfg.model.architecture)
        mc['head'] = dict(cfg.model.head)
        model = build_model(mc)
        model.train()
        opt = AdamW(1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05, parameters=list(model.parameters()))
        if eraser is not None:
            eraser.rng = random.Random(0)

        def one(_i, model=model, opt=opt, eraser=eraser):
            xb = x if eraser is None else eraser(x)          # what the loader does before it yields the batch
            out = model(xb, y, mode='train')
            opt.clear_grad()
            out['loss'].backward()
            opt.step()
        runs[name] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, drop_path_rate 0.1, batch %d, bf16, eager steps; %d rounds x %d steps per window, '
             'alternating' % (B, args.rounds, args.steps), '%-34s %9s %9s %9s' % ('', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-34s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    (m0, lo0, hi0), (m1, _lo1, _hi1) = [_stats(times[r]) for r in runs]
    lines.append('difference %.3f ms per step (%+.2f %%; spread of the windows without it %.2f %%): the host draw of %d '
                 'samples, the 2 KB table copy and one random_erase launch' % (m1 - m0, 100 * (m1 / m0 - 1),
                                                                              100 * (hi0 - lo0) / m0, B))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('random_erasing_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
