"""What Mixup / CutMix cost on the MI355X (DESIGN.md "Mixup / CutMix"): the stand-alone batch mix of csrc/mixup.hip, and
a whole fine-tuning step with and without the ``batch_transforms`` block.

    python tools/mixup_bench.py kernels [--out profiles/mixup_kernels.txt]
    python tools/mixup_bench.py step    [--out profiles/mixup_step.txt]

kernels: passl_hip_batch_mix on [128, 3, 224, 224] fp32 (77 MB), both modes, next to passl_hip_copy_bytes of the same
bytes — in its paired form the mix moves exactly the bytes of a copy, over two read and two write streams instead of
one each.  Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the
operands rotating over more buffers than the last-level cache holds.  One bound, set before anything was measured:
mode 0 within 1.25 x the copy of the same run.  Exit status 1 when it is missed.  passl_hip_mixup_target [128, 1000] is
timed as well (no bound).

step: configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml at batch 128 bf16 with the Mixup that build_dataloader makes
of its ``batch_transforms`` block, and without it (= the drop-path YAML), two models alive in one process, windows of
eager steps alternating.  No bound: the difference is what fusing the mix into passl_hip_patchify would be judged
against."""
import argparse
import os
import sys

import numpy as np
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
    from passl_amd.hip import lib as L
    lib = L.load()
    B, C, H, W = args.batch, 3, 224, 224
    nset = 4                                     # 4 x 2 x 77 MB: more than the 256 MB last-level cache
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    sets = [(torch.randn(B, C, H, W, generator=gen).to(dev), torch.empty(B, C, H, W, device=dev)) for _ in range(nset)]
    labels = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    target = torch.empty(B, 1000, device=dev)
    nbytes = B * C * H * W * 4
    p, st = L.ptr, L.stream()
    lam = 0.531506

    def copy(i):
        x, z = sets[i % nset]
        L.check(lib.passl_hip_copy_bytes(p(z), p(x), nbytes, st))

    def mix(mode, box):
        def f(i):
            x, z = sets[i % nset]
            L.check(lib.passl_hip_batch_mix(p(x), p(z), B, C, H, W, lam, 1.0 - lam, box[0], box[1], box[2], box[3], mode, st))
        return f

    def tgt(_i):
        L.check(lib.passl_hip_mixup_target(p(labels), p(target), B, 1000, lam, 0.1, st))
    variants = [('copy_bytes', copy, 2 * nbytes), ('batch_mix mode 0 (mixup)', mix(0, (0, 0, 0, 0)), 2 * nbytes),
                ('batch_mix mode 1 (cutmix)', mix(1, (30, 178, 0, 81)), 2 * nbytes),
                ('mixup_target [%d, 1000]' % B, tgt, B * 1000 * 4 + B * 8)]
    times = {n: [] for n, _f, _b in variants}
    for _n, f, _b in variants:                     # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.rounds):
        for n, f, _b in variants:                  # alternating: drift hits every variant alike
            times[n].append(_window(f, args.launches))
    lines = ['batch [%d, 3, 224, 224] fp32 = %.1f MB read + %.1f MB written per launch; %d rounds x %d launches per window, '
             '%d operand sets' % (B, nbytes / 1e6, nbytes / 1e6, args.rounds, args.launches, nset),
             '%-28s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)')]
    for n, _f, nb in variants:
        m, lo, hi = _stats(times[n])
        lines.append('%-28s %9.2f %9.2f %9.2f %10.0f' % (n, m * 1e3, lo * 1e3, hi * 1e3, nb / (m * 1e-3) / 1e9))
    cm = _stats(times['copy_bytes'])[0]
    mm = _stats(times['batch_mix mode 0 (mixup)'])[0]
    xm = _stats(times['batch_mix mode 1 (cutmix)'])[0]
    ok = mm <= 1.25 * cm
    lines.append('batch_mix mode 0 / copy_bytes = %.3f (bound 1.25: %s); mode 1 / copy_bytes = %.3f (no bound)'
                 % (mm / cm, 'HOLDS' if ok else 'MISSED', xm / cm))
    return lines, ok


def step(args):
    from passl_amd.datasets.preprocess import build_mixup
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    from passl_amd.solver.optimizer import AdamW
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml'), [])
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    block = [dict(b) for b in cfg.dataloader.train.dataset.batch_transforms]
    runs = {}
    for name, mixup_fn in (('without batch_transforms', None), ('with Mixup 0.8 / CutMix 1.0', build_mixup(block))):
        torch.manual_seed(0)
        mc = dict(cfg.model)
        mc['architecture'] = dict(cfg.model.architecture)
        mc['head'] = dict(cfg.model.head)
        model = build_model(mc)
        model.train()
        opt = AdamW(1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05, parameters=list(model.parameters()))
        if mixup_fn is not None:
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
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, drop_path_rate 0.1, batch %d, bf16, eager steps; %d rounds x %d steps per window, '
             'alternating' % (B, args.rounds, args.steps), '%-30s %9s %9s %9s' % ('', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-30s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    (m0, lo0, hi0), (m1, _lo1, _hi1) = [_stats(times[r]) for r in runs]
    lines.append('difference %.3f ms per step (%+.2f %%; spread of the unmixed windows %.2f %%): batch_mix + mixup_target + '
                 'the dense-target loss in place of the integer one' % (m1 - m0, 100 * (m1 / m0 - 1), 100 * (hi0 - lo0) / m0))
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
        raise SystemExit('mixup_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
