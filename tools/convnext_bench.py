"""What the ConvNeXt block kernels (csrc/dwconv.hip) cost on the MI355X (DESIGN.md "ConvNeXt block kernels").

    python tools/convnext_bench.py kernels [--out profiles/convnext_kernels.txt] [--resources]
    python tools/convnext_bench.py step    [--out profiles/convnext_step.txt]

kernels: the depthwise 7x7 forward, data gradient and weight gradient on the four stage shapes of convnext_tiny at
batch 128 (56^2 x 96, 28^2 x 192, 14^2 x 384, 7^2 x 768), bf16 and fp32.  Each direction is reported three ways:
  * against passl_hip_copy_bytes of one operand (a copy reads n and writes n bytes: the bytes the forward and the data
    gradient move, and the two operands the weight gradient reads), in the same run;
  * against the arithmetic floor, 49 FMAs per element at the 157.3 TFLOP/s fp32 vector peak;
  * against ATen's depthwise convolution (torch.nn.functional.conv2d(groups=C), channels-last, same dtype; the forward,
    and the two gradients through autograd on a graph built once), warmed up first.  Each direction should not be slower
    than ATen's beyond the spread of ATen's own windows; the verdict is printed per row.  If ATen's kernel cannot run
    here, the row says so.
Then passl_hip_layer_scale_add_fwd next to passl_hip_drop_path_add on the same rows (they move the same bytes; bound,
set before any measurement: within 1.25 x, the margin the project gives its streaming kernels) and the backward.  Exit
status 1 when that bound is missed or a direction is slower than ATen's.

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands
rotating over more buffers than the last-level cache holds.  --resources appends tools/kernel_resources.py's table.

step: convnext_tiny and convnext_base at batch 128, bf16, eager training steps (forward, CELoss, backward, AdamW) with
drop_path_rate 0 and with the recipe's rate (0.1 / 0.5), the two models of a size alive in one process, windows of steps
alternating.  There is no parent to compare a step against: the figures are a first record, not a bound.  The share of
the step spent in the new kernels is not reported: the library's profiling classes (passl_hip_prof_*) bracket the GEMM
kernels only."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32 = 157.3e12
STAGES = ((56, 96), (28, 192), (14, 384), (7, 768))


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


def _measure(variants, launches, rounds):
    times = {n: [] for n, _f in variants}
    for _n, f in variants:                       # warm-up: code objects, clocks, library algorithm choices
        _window(f, max(3, launches // 4))
    for _ in range(rounds):
        for n, f in variants:                    # alternating: drift hits every variant alike
            times[n].append(_window(f, launches))
    return times


def conv_shape(args, HW, C, dtype, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    N, dev = args.batch, torch.device('cuda')
    elems = N * HW * HW * C
    nbytes = elems * (2 if dtype == torch.bfloat16 else 4)
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)      # x and an output per launch: past the 256 MB cache
    gen = torch.Generator().manual_seed(0)
    xs = [torch.randn(N, HW, HW, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    dys = [torch.randn(N, HW, HW, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    outs = [torch.empty(N, HW, HW, C, dtype=dtype, device=dev) for _ in range(nset)]
    w = (torch.randn(C, 1, 7, 7, generator=gen) * 0.1).to(dev)
    bias = torch.randn(C, generator=gen).to(dev)
    dw, db = torch.empty_like(w), torch.empty_like(bias)
    ws = torch.empty(ops.dwconv7_wgrad_ws_floats(N, HW, HW, C), device=dev)
    dt = L.dt(dtype)

    def copy(i):
        L.check(lib.passl_hip_copy_bytes(p(outs[i % nset]), p(xs[i % nset]), nbytes, st))

    def fwd(i):
        L.check(lib.passl_hip_dwconv7_fwd(p(xs[i % nset]), p(w), p(bias), p(outs[i % nset]), N, HW, HW, C, dt, st))

    def bwd_data(i):
        L.check(lib.passl_hip_dwconv7_bwd_data(p(dys[i % nset]), p(w), None, p(outs[i % nset]), N, HW, HW, C, dt, st))

    def bwd_weight(i):
        L.check(lib.passl_hip_dwconv7_bwd_weight(p(xs[i % nset]), p(dys[i % nset]), p(dw), p(db), p(ws), ws.numel(),
                                                 N, HW, HW, C, dt, st))
    variants = [('copy', copy), ('fwd', fwd), ('bwd_data', bwd_data), ('bwd_weight', bwd_weight)]

    aten_error = None
    try:                                        # ATen: NCHW-shaped views of the same channels-last memory
        wa, ba = w.to(dtype).requires_grad_(), bias.to(dtype).requires_grad_()
        xa = [x.permute(0, 3, 1, 2).requires_grad_() for x in xs]
        da = [d.permute(0, 3, 1, 2) for d in dys]
        F = torch.nn.functional
        ya = [F.conv2d(x, wa, ba, padding=3, groups=C) for x in xa]
        torch.cuda.synchronize()

        def a_fwd(i):
            with torch.no_grad():
                F.conv2d(xa[i % nset], wa, ba, padding=3, groups=C)

        def a_data(i):
            torch.autograd.grad(ya[i % nset], xa[i % nset], da[i % nset], retain_graph=True)

        def a_weight(i):
            torch.autograd.grad(ya[i % nset], (wa, ba), da[i % nset], retain_graph=True)
        for f in (a_fwd, a_data, a_weight):
            f(0)
        torch.cuda.synchronize()
        variants += [('aten fwd', a_fwd), ('aten bwd_data', a_data), ('aten bwd_weight', a_weight)]
    except Exception as e:                      # noqa: BLE001  (reported, not hidden)
        aten_error = '%s: %s' % (type(e).__name__, str(e).splitlines()[0][:120])

    times = _measure(variants, args.launches, args.rounds)
    name = 'fp32' if dtype == torch.float32 else 'bf16'
    floor_us = 2.0 * 49 * elems / PEAK_FP32 * 1e6
    cm = _stats(times['copy'])[0]
    lines.append('[%d, %d, %d, %d] %s: %.1f MB per operand, %d operand sets; copy_bytes %.1f us (%.0f GB/s); arithmetic '
                 'floor %.1f us' % (N, HW, HW, C, name, nbytes / 1e6, nset, cm * 1e3, 2 * nbytes / (cm * 1e-3) / 1e9,
                                    floor_us))
    lines.append('  %-12s %9s %9s %9s %8s %8s %9s %9s  %s' % ('direction', 'mean us', 'min us', 'max us', 'x copy',
                                                             'x floor', 'aten us', 'x aten', 'verdict'))
    ok = True
    for d in ('fwd', 'bwd_data', 'bwd_weight'):
        m, lo, hi = _stats(times[d])
        if 'aten ' + d in times:
            am, alo, ahi = _stats(times['aten ' + d])
            holds = m <= am * (1 + (ahi - alo) / am)
            ok = ok and holds
            aten = '%9.1f %9.2f  %s' % (am * 1e3, m / am, 'not slower than ATen' if holds else 'SLOWER than ATen')
        else:
            aten = '%9s %9s  ATen did not run' % ('-', '-')
        lines.append('  %-12s %9.1f %9.1f %9.1f %8.2f %8.2f %s' % (d, m * 1e3, lo * 1e3, hi * 1e3, m / cm,
                                                                  m * 1e3 / floor_us, aten))
    if aten_error:
        lines.append('  ATen depthwise convolution cannot run here: ' + aten_error)
    return ok


def layer_scale(args, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    B, T, C, dtype = args.batch, 56 * 56, 96, torch.bfloat16
    M, dev, dt = B * T, torch.device('cuda'), L.dt(torch.bfloat16)
    nset = 3
    gen = torch.Generator().manual_seed(0)
    sets = [[torch.randn(M, C, generator=gen).to(dev).to(dtype) for _ in range(2)] +
            [torch.empty(M, C, dtype=dtype, device=dev)] for _ in range(nset)]
    ones = torch.ones(B, device=dev)
    gamma = (torch.rand(C, generator=gen) + 0.5).to(dev)
    dgamma = torch.empty(C, device=dev)
    ws = torch.empty(ops.layer_scale_bwd_ws_floats(M, C), device=dev)
    kp = 0.9

    def dp_add(i):
        x, r, z = sets[i % nset]
        L.check(lib.passl_hip_drop_path_add(p(x), p(r), p(ones), kp, p(z), B, T, C, dt, st))

    def ls_fwd(keep):
        def f(i):
            x, r, z = sets[i % nset]
            L.check(lib.passl_hip_layer_scale_add_fwd(p(x), p(r), p(gamma), p(keep), kp, p(z), B, T, C, dt, st))
        return f

    def ls_bwd(i):
        x, r, z = sets[i % nset]
        L.check(lib.passl_hip_layer_scale_add_bwd(p(x), p(r), p(gamma), p(ones), kp, p(z), p(dgamma), p(ws), ws.numel(),
                                                  B, T, C, dt, st))
    variants = [('drop_path_add all kept', dp_add), ('layer_scale_add_fwd all kept', ls_fwd(ones)),
                ('layer_scale_add_fwd no table', ls_fwd(None)), ('layer_scale_add_bwd all kept', ls_bwd)]
    times = _measure(variants, args.launches, args.rounds)
    nbytes = M * C * 2
    lines.append('rows [%d x %d, %d] bf16 = %.1f MB per operand, %d operand sets' % (B, T, C, nbytes / 1e6, nset))
    lines.append('  %-30s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)'))
    for n, _f in variants:
        m, lo, hi = _stats(times[n])
        lines.append('  %-30s %9.1f %9.1f %9.1f %10.0f' % (n, m * 1e3, lo * 1e3, hi * 1e3, 3 * nbytes / (m * 1e-3) / 1e9))
    ratio = _stats(times['layer_scale_add_fwd all kept'])[0] / _stats(times['drop_path_add all kept'])[0]
    ok = ratio <= 1.25
    lines.append('  layer_scale_add_fwd / drop_path_add = %.3f; bound 1.25: %s' % (ratio, 'HOLDS' if ok else 'MISSED'))
    return ok


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches)]
    ok = True
    for dtype in (torch.bfloat16, torch.float32):
        for HW, C in STAGES:
            ok = conv_shape(args, HW, C, dtype, lines) and ok
            torch.cuda.empty_cache()
    ok = layer_scale(args, lines) and ok
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'dwconv.hip'],
                           capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py dwconv.hip'] + (r.stdout if r.returncode == 0 else r.stderr).splitlines()
    return lines, ok


def step(args):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    from passl_amd.loss.celoss import CELoss
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev, B = torch.device('cuda'), args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    lines = ['batch %d, 224 x 224, bf16, eager steps (forward, CELoss, backward, AdamW); %d rounds x %d steps per window, '
             'alternating' % (B, args.rounds, args.steps),
             '%-16s %-16s %9s %9s %9s' % ('model', 'drop_path_rate', 'mean ms', 'min ms', 'max ms')]
    for name, rate in (('convnext_tiny', 0.1), ('convnext_base', 0.5)):
        runs = {}
        for r in (0.0, rate):
            torch.manual_seed(0)
            model = PM.build_model(dict(name=name, drop_path_rate=r, class_num=1000)).train()
            opt = AdamW(4e-3, weight_decay=0.05, parameters=list(model.parameters()))
            celoss = CELoss()

            def one(_i, model=model, opt=opt, celoss=celoss):
                loss = celoss(model(x), y)['CELoss']
                opt.clear_grad()
                loss.backward()
                opt.step()
            runs[r] = one
        times = _measure(list(runs.items()), args.steps, args.rounds)
        stats = {r: _stats(times[r]) for r in runs}
        for r in runs:
            lines.append('%-16s %-16s %9.3f %9.3f %9.3f' % ((name, r) + stats[r]))
        m0, m1 = stats[0.0][0], stats[rate][0]
        lines.append('%-16s rate %.1f against 0: %+.3f ms per step (%+.2f %%)' % (name, rate, m1 - m0, 100 * (m1 / m0 - 1)))
        del runs
        torch.cuda.empty_cache()
    lines.append('share of the step in the new kernels: NOT MEASURED (the profiling classes bracket the GEMM kernels only)')
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('convnext_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
