"""What element-wise dropout costs on the MI355X: the launches of csrc/dropout.hip next to the launches
they extend or replace, and a whole supervised ViT-B step with drop_rate 0.1 and 0.

    python tools/dropout_bench.py kernels [--out profiles/dropout_kernels.txt]
    python tools/dropout_bench.py step    [--out profiles/dropout_step.txt]

kernels: on [128 * 197, 768] bf16 rows (ViT-B/16, batch 128) passl_hip_dropout_add next to passl_hip_drop_path_add with
every sample kept (the same two reads and one write, no Philox) and passl_hip_copy_bytes (one read, one write), and
passl_hip_dropout (the backward of every site); on [128 * 197, 3072] rows passl_hip_gelu_dropout_fwd / _bwd next to
passl_hip_gelu_fwd / _bwd, which move the same bytes.  Device events around WINDOWS of back-to-back launches, the
variants alternating inside one process, the operands rotating over more buffers than the last-level cache holds.
No pass/fail time was set in advance: one Philox4x32-10 call per 8 elements is ~40 32-bit multiplies, and whether the
launches stay HBM-bound is what this measures.  The ratio dropout_add / drop_path_add is printed against the 1.25 the
earlier tools use as a margin; beyond it the known alternative is a stored 1-bit mask for the backward.

step: the v2 ViT_base_patch16_224 at batch 128 bf16 with ViTCELoss and AdamW, drop_rate 0 and 0.1, two models alive in
one process, windows of eager steps alternating.  No bound."""
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
    from passl_amd.hip import ops
    lib = L.load()
    B, T = args.batch, 197
    M, dt, st = B * T, L.dt(torch.bfloat16), L.stream()
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    thr, factor = ops.dropout_params(0.1)
    seed = (7 << 32) + 99
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    ones = torch.ones(B, device=dev)
    p = L.ptr

    def operand_sets(C, nset):
        return [[torch.randn(M, C, generator=gen).to(dev).to(torch.bfloat16) for _ in range(2)] +
                [torch.empty(M, C, dtype=torch.bfloat16, device=dev)] for _ in range(nset)]

    def variants_of(C, nset):
        sets = operand_sets(C, nset)
        n = M * C

        def pick(i):
            return sets[i % nset]

        def copy(i):
            x, _r, z = pick(i)
            L.check(lib.passl_hip_copy_bytes(p(z), p(x), n * 2, st))

        def dp_add(i):
            x, r, z = pick(i)
            L.check(lib.passl_hip_drop_path_add(p(x), p(r), p(ones), 1.0, p(z), B, T, C, dt, st))

        def do_add(i):
            x, r, z = pick(i)
            L.check(lib.passl_hip_dropout_add(p(x), p(r), p(z), n, thr, factor, seed, p(step), 1, dt, st))

        def do(i):
            x, _r, z = pick(i)
            L.check(lib.passl_hip_dropout(p(x), p(z), n, thr, factor, seed, p(step), 1, dt, st))

        def gelu_f(i):
            x, _r, z = pick(i)
            L.check(lib.passl_hip_gelu_fwd(p(x), p(z), n, dt, st))

        def gelu_do_f(i):
            x, _r, z = pick(i)
            L.check(lib.passl_hip_gelu_dropout_fwd(p(x), p(z), n, thr, factor, seed, p(step), 2, dt, st))

        def gelu_b(i):
            x, r, z = pick(i)
            L.check(lib.passl_hip_gelu_bwd(p(r), p(x), p(z), n, dt, st))

        def gelu_do_b(i):
            x, r, z = pick(i)
            L.check(lib.passl_hip_gelu_dropout_bwd(p(r), p(x), p(z), n, thr, factor, seed, p(step), 2, dt, st))
        if C == 768:
            return n, [('copy_bytes', copy, 2), ('drop_path_add all kept', dp_add, 3), ('dropout_add p=0.1', do_add, 3),
                       ('dropout p=0.1', do, 2)]
        return n, [('gelu_fwd', gelu_f, 2), ('gelu_dropout_fwd p=0.1', gelu_do_f, 2), ('gelu_bwd', gelu_b, 3),
                   ('gelu_dropout_bwd p=0.1', gelu_do_b, 3)]

    lines, means = [], {}
    # 6 x 3 x 38.7 MB and 3 x 3 x 154.9 MB: more than the 256 MB last-level cache either way
    for C, nset in ((768, 6), (3072, 3)):
        n, variants = variants_of(C, nset)
        times = {name: [] for name, _f, _b in variants}
        for _name, f, _b in variants:                  # warm-up: code objects, clocks
            _window(f, args.launches)
        for _ in range(args.rounds):
            for name, f, _b in variants:               # alternating: drift hits every variant alike
                times[name].append(_window(f, args.launches))
        lines.append('rows [%d x 197, %d] bf16 = %.1f MB per operand; %d rounds x %d launches per window, %d operand sets'
                     % (B, C, n * 2 / 1e6, args.rounds, args.launches, nset))
        lines.append('%-28s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)'))
        for name, _f, nb in variants:
            m, lo, hi = _stats(times[name])
            means[name] = m
            lines.append('%-28s %9.2f %9.2f %9.2f %10.0f' % (name, m * 1e3, lo * 1e3, hi * 1e3, nb * n * 2 / (m * 1e-3) / 1e9))
        del variants
        torch.cuda.empty_cache()
    r = means['dropout_add p=0.1'] / means['drop_path_add all kept']
    lines.append('dropout_add / drop_path_add all kept = %.3f (margin of the earlier tools: 1.25 — %s)'
                 % (r, 'within' if r <= 1.25 else 'EXCEEDED: a stored 1-bit mask for the backward is the known alternative'))
    lines.append('dropout_add / copy_bytes = %.3f (bytes 3 : 2)' % (means['dropout_add p=0.1'] / means['copy_bytes']))
    lines.append('gelu_dropout_fwd / gelu_fwd = %.3f   gelu_dropout_bwd / gelu_bwd = %.3f'
                 % (means['gelu_dropout_fwd p=0.1'] / means['gelu_fwd'], means['gelu_dropout_bwd p=0.1'] / means['gelu_bwd']))
    return lines, True


def step(args):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    from passl_amd.loss import ViTCELoss
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    loss_fn = ViTCELoss(epsilon=1e-4)
    runs = {}
    for rate in (0.0, 0.1):
        torch.manual_seed(0)
        model = PM.ViT_base_patch16_224(class_num=1000, drop_rate=rate)
        model.train()
        opt = AdamW(1e-3, beta1=0.9, beta2=0.999, weight_decay=0.3, parameters=list(model.parameters()))

        def one(_i, model=model, opt=opt):
            loss = loss_fn(model(x), y)['ViTCELoss']
            opt.clear_grad()
            loss.backward()
            opt.step()
        runs[rate] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['ViT_base_patch16_224 + ViTCELoss + AdamW, batch %d, bf16, eager steps; %d rounds x %d steps per window, '
             'alternating' % (B, args.rounds, args.steps), '%-22s %9s %9s %9s' % ('drop_rate', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-22s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    m0, m1 = _stats(times[0.0])[0], _stats(times[0.1])[0]
    lines.append('difference %.3f ms per step (%+.2f %%): 1 advance, pos_drop, and per block 2 residual adds as stand-alone '
                 'passes (forward add, backward mask) + the mask inside the GELU launches' % (m1 - m0, 100 * (m1 / m0 - 1)))
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
        raise SystemExit('dropout_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
