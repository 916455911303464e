"""What stochastic depth costs on the MI355X (DESIGN.md "Stochastic depth"): the stand-alone residual passes of
csrc/drop_path.hip, and a whole fine-tuning step with and without them.

    python tools/droppath_bench.py kernels [--out profiles/droppath_kernels.txt]
    python tools/droppath_bench.py step    [--out profiles/droppath_step.txt]

kernels: passl_hip_drop_path_add / _bwd on [128 * 197, 768] bf16 rows (ViT-B/16, batch 128) next to passl_hip_bn_apply
with a residual on the same rows — the library's streaming kernel that moves the same bytes as the add with nothing
dropped (two reads, one write).  Device events around WINDOWS of back-to-back launches, the variants alternating inside
one process, the operands rotating over more buffers than the last-level cache holds.  One bound: the add with an
all-ones table is no slower than bn_apply by more than 10 % beyond the spread of the bn_apply windows (the only extra
work is one 4-byte load per workgroup and a division per element).  Exit status 1 when it is missed.

step: configs/mae/mae_vit_b_finetune_synthetic.yaml at batch 128 bf16, drop_path_rate 0 and 0.1, two models alive in one
process, windows of eager steps alternating.  No bound: the difference is the number a fusion of the per-sample factor
into the GEMM epilogues would be judged against."""
import argparse
import os
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
    from passl_amd.hip import lib as L
    lib = L.load()
    B, T, C = args.batch, 197, 768
    M, dt, st = B * T, L.dt(torch.bfloat16), L.stream()
    nset = 6                                     # 6 x 3 x 38.7 MB: more than the 256 MB last-level cache
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    sets = [[torch.randn(M, C, generator=gen).to(dev).to(torch.bfloat16) for _ in range(2)] +
            [torch.empty(M, C, dtype=torch.bfloat16, device=dev)] for _ in range(nset)]
    ones = torch.ones(B, device=dev)
    some = torch.ones(B, device=dev)
    some[torch.randperm(B, generator=gen)[:max(1, round(0.1 * B))]] = 0.0        # 10 % of the samples dropped
    scale, shift = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    keep_prob = 0.9
    p = L.ptr

    def bn(i):
        x, r, z = sets[i % nset]
        L.check(lib.passl_hip_bn_apply(p(x), p(scale), p(shift), p(r), p(z), None, M, C, 0, dt, st))

    def add(keep):
        def f(i):
            x, r, z = sets[i % nset]
            L.check(lib.passl_hip_drop_path_add(p(x), p(r), p(keep), keep_prob, p(z), B, T, C, dt, st))
        return f

    def bwd(keep):
        def f(i):
            x, _r, z = sets[i % nset]
            L.check(lib.passl_hip_drop_path_bwd(p(x), p(keep), keep_prob, p(z), B, T, C, dt, st))
        return f
    variants = [('bn_apply + residual', bn, 3), ('drop_path_add all kept', add(ones), 3),
                ('drop_path_add 10% dropped', add(some), 2.9), ('drop_path_bwd all kept', bwd(ones), 2),
                ('drop_path_bwd 10% dropped', bwd(some), 1.9)]
    times = {n: [] for n, _f, _b in variants}
    for _n, f, _b in variants:                     # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.rounds):
        for n, f, _b in variants:                  # alternating: drift hits every variant alike
            times[n].append(_window(f, args.launches))
    elem_bytes = M * C * 2
    lines = ['rows [%d x 197, 768] bf16 = %.1f MB per operand; %d rounds x %d launches per window, %d operand sets'
             % (B, elem_bytes / 1e6, args.rounds, args.launches, nset),
             '%-28s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)')]
    for n, _f, nb in variants:
        m, lo, hi = _stats(times[n])
        lines.append('%-28s %9.2f %9.2f %9.2f %10.0f' % (n, m * 1e3, lo * 1e3, hi * 1e3, nb * elem_bytes / (m * 1e-3) / 1e9))
    bm, blo, bhi = _stats(times['bn_apply + residual'])
    am = _stats(times['drop_path_add all kept'])[0]
    spread = (bhi - blo) / bm
    limit = bm * (1.10 + spread)
    ok = am <= limit
    lines.append('bn_apply spread (max - min) / mean = %.1f %%; bound: add all kept %.2f us <= %.2f us (bn_apply x (1.10 + spread)): %s'
                 % (100 * spread, am * 1e3, limit * 1e3, 'HOLDS' if ok else 'MISSED'))
    lines.append('add all kept / bn_apply = %.3f' % (am / bm))
    return lines, ok


def step(args):
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    from passl_amd.solver.optimizer import AdamW
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_synthetic.yaml'), [])
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    runs = {}
    for rate in (0.0, 0.1):
        torch.manual_seed(0)
        mc = dict(cfg.model)
        mc['architecture'] = dict(cfg.model.architecture, drop_path_rate=rate)
        mc['head'] = dict(cfg.model.head)
        model = build_model(mc)
        model.train()
        opt = AdamW(1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05, parameters=list(model.parameters()))

        def one(_i, model=model, opt=opt):
            out = model(x, y, mode='train')
            opt.clear_grad()
            out['loss'].backward()
            opt.step()
        runs[rate] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, batch %d, bf16, eager steps; %d rounds x %d steps per window, alternating' % (
        B, args.rounds, args.steps), '%-22s %9s %9s %9s' % ('drop_path_rate', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-22s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    m0, m1 = _stats(times[0.0])[0], _stats(times[0.1])[0]
    lines.append('difference %.3f ms per step (%+.2f %%): 22 residual adds as stand-alone passes (forward add, backward '
                 'scale) + 1 draw' % (m1 - m0, 100 * (m1 / m0 - 1)))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=300)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('droppath_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
