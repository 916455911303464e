"""What the ConvMAE kernels (csrc/convmae.hip) and a ConvMAE pre-training step cost on the MI355X (DESIGN.md "ConvMAE").

    python tools/convmae_bench.py kernels [--out profiles/convmae_kernels.txt] [--resources]
    python tools/convmae_bench.py step    [--out profiles/convmae_step.txt]

kernels: the masked depthwise 5x5 forward, data gradient and weight gradient at batch 128, bf16, on the two maps of
convmae_convvit_base_patch16, [128, 56, 56, 256] and [128, 28, 28, 384], under a random mask of ratio 0.75 over the
14 x 14 grid.  Every expectation below is written down HERE, before any run, and each row prints HELD or MISSED:
  E1  each direction is not slower than passl_hip_dwconv7_* on the same tensor in the same run (25 of the 49 taps, a
      4-pixel halo instead of 6);
  E2  (acceptance) each direction is not slower than ATen's `x * keep` multiply plus depthwise convolution
      (torch.nn.functional.conv2d(groups=C, padding=2), channels-last, same dtype; the gradients through autograd on a
      graph built once), beyond the spread of ATen's own windows.  If ATen's kernel cannot run here, the row says so;
  E3  the stage-1 decode over the kept patches — passl_hip_patch_gather_fwd plus the GEMM over [128 * 49, 4 * 4 * 256]
      rows — takes at most K / L = 0.25 of hnn.PatchConv2D's time over the whole map plus the gather's own time.
Also printed, with no expectation: every direction against passl_hip_copy_bytes of one operand, and the same kernels
without a mask (the ConvViT path).  Exit status 1 when an expectation is MISSED.

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands
rotating over more buffers than the last-level cache holds.  --resources appends tools/kernel_resources.py's table.

step: convmae_convvit_base_patch16 (norm_pix_loss) at batch 128, bf16: eager pre-training steps (forward, backward,
AdamW) and the same step replayed from a strict step plan, windows alternating.  There is no parent to compare with:
the figures are a first record, not a bound."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAPS = ((56, 256), (28, 384))
GRID = 14
KEEP = 49


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


def _verdict(holds):
    return 'HELD' if holds else 'MISSED'


def random_mask(N, gen, dev):
    """fp32 [N, 196], 147 ones per row, and ids_keep int32 [N, 49] (ascending rank = the permutation's order)."""
    mask = torch.ones(N, GRID * GRID)
    ids = torch.empty(N, KEEP, dtype=torch.int32)
    for n in range(N):
        perm = torch.randperm(GRID * GRID, generator=gen)[:KEEP]
        mask[n, perm] = 0.0
        ids[n] = perm.to(torch.int32)
    return mask.to(dev), ids.to(dev)


def conv_shape(args, HW, C, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    N, dev, dtype = args.batch, torch.device('cuda'), torch.bfloat16
    elems = N * HW * HW * C
    nbytes = elems * 2
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)      # x and an output per launch: past the 256 MB cache
    gen = torch.Generator().manual_seed(0)
    xs = [torch.randn(N, HW, HW, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    dys = [torch.randn(N, HW, HW, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    outs = [torch.empty(N, HW, HW, C, dtype=dtype, device=dev) for _ in range(nset)]
    w5 = (torch.randn(C, 1, 5, 5, generator=gen) * 0.1).to(dev)
    w7 = (torch.randn(C, 1, 7, 7, generator=gen) * 0.1).to(dev)
    bias = torch.randn(C, generator=gen).to(dev)
    dw5, dw7, db = torch.empty_like(w5), torch.empty_like(w7), torch.empty_like(bias)
    ws5 = torch.empty(ops.dwconv5_wgrad_ws_floats(N, HW, HW, C), device=dev)
    ws7 = torch.empty(ops.dwconv7_wgrad_ws_floats(N, HW, HW, C), device=dev)
    mask, _ids = random_mask(N, gen, dev)
    dt = L.dt(dtype)

    def copy(i):
        L.check(lib.passl_hip_copy_bytes(p(outs[i % nset]), p(xs[i % nset]), nbytes, st))

    def d5(m):
        def fwd(i):
            L.check(lib.passl_hip_dwconv5_masked_fwd(p(xs[i % nset]), p(w5), p(bias), p(m), p(outs[i % nset]), N, HW, HW,
                                                     C, GRID, GRID, dt, st))

        def bwd_data(i):
            L.check(lib.passl_hip_dwconv5_masked_bwd_data(p(dys[i % nset]), p(w5), p(m), p(outs[i % nset]), N, HW, HW, C,
                                                          GRID, GRID, dt, st))

        def bwd_weight(i):
            L.check(lib.passl_hip_dwconv5_masked_bwd_weight(p(xs[i % nset]), p(dys[i % nset]), p(m), p(dw5), p(db),
                                                            p(ws5), ws5.numel(), N, HW, HW, C, GRID, GRID, dt, st))
        return fwd, bwd_data, bwd_weight

    def f7(i):
        L.check(lib.passl_hip_dwconv7_fwd(p(xs[i % nset]), p(w7), p(bias), p(outs[i % nset]), N, HW, HW, C, dt, st))

    def d7(i):
        L.check(lib.passl_hip_dwconv7_bwd_data(p(dys[i % nset]), p(w7), None, p(outs[i % nset]), N, HW, HW, C, dt, st))

    def w7g(i):
        L.check(lib.passl_hip_dwconv7_bwd_weight(p(xs[i % nset]), p(dys[i % nset]), p(dw7), p(db), p(ws7), ws7.numel(),
                                                 N, HW, HW, C, dt, st))
    dirs = ('fwd', 'bwd_data', 'bwd_weight')
    variants = [('copy', copy)]
    variants += [('masked ' + d, f) for d, f in zip(dirs, d5(mask))]
    variants += [('nomask ' + d, f) for d, f in zip(dirs, d5(None))]
    variants += [('dwconv7 ' + d, f) for d, f in zip(dirs, (f7, d7, w7g))]

    aten_error = None
    try:                                        # ATen: NCHW-shaped views of the same channels-last memory
        F = torch.nn.functional
        g = HW // GRID
        keep = (1 - mask).view(N, GRID, GRID).repeat_interleave(g, 1).repeat_interleave(g, 2).to(dtype).view(N, 1, HW, HW)
        wa, ba = w5.to(dtype).requires_grad_(), bias.to(dtype).requires_grad_()
        xa = [x.permute(0, 3, 1, 2).requires_grad_() for x in xs]
        da = [d.permute(0, 3, 1, 2) for d in dys]
        ya = [F.conv2d(x * keep, wa, ba, padding=2, groups=C) for x in xa]
        torch.cuda.synchronize()

        def a_fwd(i):
            with torch.no_grad():
                F.conv2d(xa[i % nset] * keep, wa, ba, padding=2, groups=C)

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
    cm = _stats(times['copy'])[0]
    lines.append('[%d, %d, %d, %d] bf16, mask ratio 0.75 over 14 x 14: %.1f MB per operand, %d operand sets; copy_bytes '
                 '%.1f us (%.0f GB/s)' % (N, HW, HW, C, nbytes / 1e6, nset, cm * 1e3, 2 * nbytes / (cm * 1e-3) / 1e9))
    lines.append('  %-12s %9s %9s %9s %8s %10s %10s %8s  %-6s %9s %8s  %s'
                 % ('direction', 'mean us', 'min us', 'max us', 'x copy', 'nomask us', 'dwconv7 us', 'x dw7', 'E1',
                    'aten us', 'x aten', 'E2'))
    ok = True
    for d in dirs:
        m, lo, hi = _stats(times['masked ' + d])
        nm = _stats(times['nomask ' + d])[0]
        sm, slo, shi = _stats(times['dwconv7 ' + d])
        e1 = m <= sm * (1 + (shi - slo) / sm)
        ok = ok and e1
        if 'aten ' + d in times:
            am, alo, ahi = _stats(times['aten ' + d])
            e2 = m <= am * (1 + (ahi - alo) / am)
            ok = ok and e2
            aten = '%9.1f %8.2f  %s' % (am * 1e3, m / am, _verdict(e2))
        else:
            aten = '%9s %8s  ATen did not run' % ('-', '-')
        lines.append('  %-12s %9.1f %9.1f %9.1f %8.2f %10.1f %10.1f %8.2f  %-6s %s'
                     % (d, m * 1e3, lo * 1e3, hi * 1e3, m / cm, nm * 1e3, sm * 1e3, m / sm, _verdict(e1), aten))
    if aten_error:
        lines.append('  ATen mask multiply + depthwise convolution cannot run here: ' + aten_error)
    return ok


def decode(args, lines):
    """E3: the stage-1 decode (Conv2D 256 -> 768, 4x4 stride 4) over the kept patches against the whole map."""
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import nn as hnn
    from passl_amd.hip import ops
    from passl_amd.models.convmae.conv_vit import PatchRowsConv2D
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    N, dev, dtype = args.batch, torch.device('cuda'), torch.bfloat16
    HW, C, D, pp = 56, 256, 768, 4
    gen = torch.Generator().manual_seed(1)
    nbytes = N * HW * HW * C * 2
    nset = max(2, -(-(300 << 20) // nbytes) + 1)
    xs = [torch.randn(N, HW, HW, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    _mask, ids = random_mask(N, gen, dev)

    class Both(hnn.Layer):
        def __init__(self):
            super().__init__()
            self.rows = PatchRowsConv2D(C, D, pp)
            self.full = hnn.PatchConv2D(C, D, pp, pp)
    both = Both()
    with torch.no_grad():
        for m in (both.rows, both.full):
            m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * 0.02)
    arena = hnn.EncoderArena(both, trainable=True)
    arena.refresh()

    def gather(i):
        ops.patch_gather_fwd(xs[i % nset], ids, (GRID, GRID), pp)

    def gather_gemm(i):
        with torch.no_grad():
            both.rows(ops.patch_gather_fwd(xs[i % nset], ids, (GRID, GRID), pp))

    def full(i):
        with torch.no_grad():
            both.full(xs[i % nset])
    variants = [('gather', gather), ('gather + GEMM (kept patches)', gather_gemm), ('PatchConv2D (whole map)', full)]
    times = _measure(variants, args.launches, args.rounds)
    lines.append('stage-1 decode, Conv2D(256, 768, 4, stride 4) on [%d, 56, 56, 256] bf16, %d of %d patches kept'
                 % (N, KEEP, GRID * GRID))
    lines.append('  %-32s %9s %9s %9s' % ('launches', 'mean us', 'min us', 'max us'))
    for n, _f in variants:
        lines.append('  %-32s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in _stats(times[n]))))
    g, gg, f = (_stats(times[n])[0] for n, _f in variants)
    limit = 0.25 * f + g
    holds = gg <= limit
    lines.append('  E3: gather + GEMM %.1f us against 0.25 x %.1f + %.1f = %.1f us: %s (GEMM part %.1f us = %.2f of the '
                 'whole map)' % (gg * 1e3, f * 1e3, g * 1e3, limit * 1e3, _verdict(holds), (gg - g) * 1e3, (gg - g) / f))
    return holds


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches),
             'E1: not slower than dwconv7 on the same tensor; E2: not slower than ATen mask multiply + depthwise 5x5 '
             '(both beyond the spread of the other side\'s windows); E3: stage-1 decode through the gather <= 0.25 x the '
             'whole map + the gather']
    ok = True
    for HW, C in MAPS:
        ok = conv_shape(args, HW, C, lines) and ok
        torch.cuda.empty_cache()
    ok = decode(args, lines) and ok
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'convmae.hip'],
                           capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py convmae.hip'] + (r.stdout if r.returncode == 0 else r.stderr).splitlines()
    return lines, ok


def step(args):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    from passl_amd.hip import ops
    from passl_amd.hip.replay import StepPlan
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev, B = torch.device('cuda'), args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    lines = ['convmae_convvit_base_patch16, norm_pix_loss, mask ratio 0.75, batch %d, 224 x 224, bf16; pre-training steps '
             '(forward, backward, AdamW beta2 0.95 wd 0.05); %d rounds x %d steps per window, alternating'
             % (B, args.rounds, args.steps),
             '%-28s %9s %9s %9s' % ('step', 'mean ms', 'min ms', 'max ms')]
    runs, plans = {}, []
    for mode in ('eager', 'planned'):
        torch.manual_seed(0)
        model = PM.convmae_convvit_base_patch16(norm_pix_loss=True).train()
        opt = AdamW(1.5e-4 * B / 256, beta1=0.9, beta2=0.95, weight_decay=0.05, parameters=list(model.parameters()))

        def full_step(x, model=model, opt=opt):
            loss, _pred, _mask = model(x, 0.75)
            opt.clear_grad()
            loss.backward(ops.ones_like_cached(loss))
            opt.step()
            return dict(loss=loss)
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode == 'planned'), strict=True)
        plans.append(sp)
        runs[mode] = lambda _i, sp=sp: sp.run(x)
    times = _measure(list(runs.items()), args.steps, args.rounds)
    for mode in runs:
        lines.append('%-28s %9.3f %9.3f %9.3f' % ((mode,) + _stats(times[mode])))
    sp = plans[1]
    lines.append('planned: captured %s, replays %d, failed %r, foreign %r; %s'
                 % (sp.captured, sp.replays, sp.failed, sp.foreign, sp.info))
    e, p = _stats(times['eager'])[0], _stats(times['planned'])[0]
    lines.append('planned against eager: %+.3f ms per step (%+.2f %%); %.0f images/s planned'
                 % (p - e, 100 * (p / e - 1), B / (p * 1e-3)))
    lines.append('no parent to compare with: a first record')
    return lines, sp.failed is None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('convmae_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
