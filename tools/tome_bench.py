"""What token merging (csrc/tome.hip, passl_amd/models/utils/tome.py) costs and saves on the MI355X (DESIGN.md "ToMe").

    python tools/tome_bench.py kernels [--out profiles/tome_kernels.txt]
    python tools/tome_bench.py step    [--out profiles/tome_step.txt] [--dtypes bf16,fp32]

kernels: ViT-B/16 shapes (12 heads of 64, C = 768), batch 128, the token count of every layer of r = 16 (197, 181, ...,
37 with r = 16, then 21 with the clamped r = 10): tome_match, tome_merge_fwd, tome_merge_bwd, and at the same T
passl_hip_attention_fwd against passl_hip_attention_fwd_keybias.  Expectations, set before any measurement:
  * the three ToMe launches together cost less than the attention forward launch of the same layer;
  * key-bias attention is within a few percent (5 %) of the plain kernel: the bias is one add per score.
step: ViT_base_patch16_224 at batch 128, per dtype the evaluation forward (no_grad) and the full training step (forward,
CELoss, backward, AdamW) of the unpatched model, the patched model with r = 0, r = 16 and r = (16, -1).  Expectations:
  * patched r = 0 is within run-to-run noise of unpatched (inside the spread of the unpatched windows);
  * patched r = 16 is faster than unpatched, in evaluation and in training.
Every expectation is printed as met or MISSED with its ratio; a miss is reported, it is not an error (exit status 0).

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process; the kernel operands
rotate over more buffers than the last-level cache holds (tools/convnext_bench.py has the windows)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from convnext_bench import _measure, _stats          # noqa: E402  (the same windows)

H, DH, C = 12, 64, 768


def layer_shapes():
    from passl_amd.models.utils import tome
    r_i, t_in, _ = tome.token_schedule(197, tome.parse_r(12, 16))
    return list(zip(t_in, r_i))


def _met(lines, what, ratio, ok):
    lines.append('  %s: %s (%.3f)' % (what, 'met' if ok else 'MISSED', ratio))


def kernels(args):
    from passl_amd.hip import lib as L
    lib, st, p = L.load(), L.stream(), L.ptr
    B, dev, dtype = args.batch, torch.device('cuda'), torch.bfloat16
    dt = L.dt(dtype)
    lines = ['batch %d, %d heads of %d, C = %d, bf16; %d rounds x %d launches per window, variants alternating; times are '
             'device-event windows / launches' % (B, H, DH, C, args.rounds, args.launches),
             '%5s %3s %9s %9s %9s %9s %9s %9s %8s %8s' % ('T', 'r', 'match', 'merge', 'merge_bwd', 'sum of 3', 'attn fwd',
                                                          'keybias', 'sum/attn', 'kb/attn')]
    worst_sum, worst_kb = 0.0, 0.0
    for T, r in layer_shapes():
        nbytes = B * T * 3 * H * DH * 2
        nset = max(2, -(-(300 << 20) // nbytes) + 1)
        gen = torch.Generator().manual_seed(T)
        qkvs = [torch.randn(B * T, 3 * H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
        xs = [torch.randn(B * T, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
        dys = [torch.randn(B * (T - r), C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
        outs = [torch.empty(B * T, H * DH, dtype=dtype, device=dev) for _ in range(2)]
        ys = [torch.empty(B * (T - r), C, dtype=dtype, device=dev) for _ in range(2)]
        dxs = [torch.empty(B * T, C, dtype=dtype, device=dev) for _ in range(2)]
        dest = torch.empty(B, T, dtype=torch.int32, device=dev)
        size = torch.randint(1, 4, (B, T), generator=gen).float().to(dev)
        size_out = torch.empty(B, T - r, device=dev)
        bias = torch.log(size)
        lse = torch.empty(B, H, T, device=dev)

        def match(i):
            L.check(lib.passl_hip_tome_match(p(qkvs[i % nset]), p(dest), None, None, B, T, H, DH, r, dt, st))

        def merge(i):
            L.check(lib.passl_hip_tome_merge_fwd(p(xs[i % nset]), p(size), p(dest), p(ys[i % 2]), p(size_out), None, B, T, r,
                                                 C, dt, st))

        def merge_bwd(i):
            L.check(lib.passl_hip_tome_merge_bwd(p(dys[i % nset]), p(size), p(size_out), p(dest), p(dxs[i % 2]), B, T, r, C,
                                                 dt, st))

        def attn(i):
            L.check(lib.passl_hip_attention_fwd(p(qkvs[i % nset]), p(outs[i % 2]), p(lse), B, T, H, DH, 0.125, 0, dt, st))

        def keybias(i):
            L.check(lib.passl_hip_attention_fwd_keybias(p(qkvs[i % nset]), p(bias), p(outs[i % 2]), p(lse), B, T, H, DH,
                                                        0.125, dt, st))
        variants = [('match', match), ('merge', merge), ('merge_bwd', merge_bwd), ('attn', attn), ('keybias', keybias)]
        for _n, f in variants:
            f(0)
        torch.cuda.synchronize()
        times = _measure(variants, args.launches, args.rounds)
        m = {n: _stats(ts)[0] * 1e3 for n, ts in times.items()}
        three = m['match'] + m['merge'] + m['merge_bwd']
        lines.append('%5d %3d %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %8.3f %8.3f' % (
            T, r, m['match'], m['merge'], m['merge_bwd'], three, m['attn'], m['keybias'], three / m['attn'],
            m['keybias'] / m['attn']))
        worst_sum, worst_kb = max(worst_sum, three / m['attn']), max(worst_kb, m['keybias'] / m['attn'])
        del qkvs, xs, dys
        torch.cuda.empty_cache()
    lines.append('times in us.  Expectations (worst layer):')
    _met(lines, 'match + merge + merge_bwd cost less than the attention forward of the layer', worst_sum, worst_sum < 1.0)
    _met(lines, 'key-bias attention within 5 % of the plain kernel', worst_kb, worst_kb <= 1.05)
    return lines


def step(args):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    from passl_amd.loss.celoss import CELoss
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    dev, B = torch.device('cuda'), args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    lines = ['ViT_base_patch16_224, batch %d, 224 x 224, eager; %d rounds x %d passes per window, variants alternating'
             % (B, args.rounds, args.steps)]
    cases = [('unpatched', None), ('patched r=0', 0), ('patched r=16', 16), ('patched r=(16,-1)', [16, -1.0])]
    for dname in args.dtypes.split(','):
        dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[dname]
        hip_config.set_compute_dtype(dtype)
        evals, trains = [], []
        for name, r in cases:
            torch.manual_seed(0)
            cfg = dict(name='ViT_base_patch16_224', class_num=1000)
            if r is not None:
                cfg['tome'] = dict(r=r)
            model = PM.build_model(cfg)
            opt = AdamW(1e-4, weight_decay=0.05, parameters=[q for _n, q in model.named_parameters()])
            celoss = CELoss()

            def ev(_i, model=model):
                model.eval()
                with torch.no_grad():
                    model(x)

            def tr(_i, model=model, opt=opt, celoss=celoss):
                model.train()
                loss = celoss(model(x), y)['CELoss']
                opt.clear_grad()
                loss.backward()
                opt.step()
            ev(0)
            tr(0)
            evals.append((name, ev))
            trains.append((name, tr))
        torch.cuda.synchronize()
        for what, variants in (('evaluation forward', evals), ('training step', trains)):
            times = _measure(variants, args.steps, args.rounds)
            stats = {n: _stats(times[n]) for n, _f in variants}
            lines.append('%s, %s' % (dname, what))
            lines.append('  %-20s %9s %9s %9s %8s' % ('model', 'mean ms', 'min ms', 'max ms', '/ unpat.'))
            base = stats['unpatched']
            for n, _f in variants:
                lines.append('  %-20s %9.3f %9.3f %9.3f %8.3f' % ((n,) + stats[n] + (stats[n][0] / base[0],)))
            r0 = stats['patched r=0'][0]
            _met(lines, 'r = 0 within the spread of the unpatched windows (%.3f .. %.3f ms)' % (base[1], base[2]),
                 r0 / base[0], base[1] - (base[2] - base[1]) <= r0 <= base[2] + (base[2] - base[1]))
            r16 = stats['patched r=16'][0]
            _met(lines, 'r = 16 faster than unpatched', r16 / base[0], r16 < base[0])
            lines.append('  r = (16, -1) / unpatched = %.3f (no expectation set)' % (stats['patched r=(16,-1)'][0] / base[0]))
        del evals, trains
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--dtypes', default='bf16,fp32')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tome_bench: needs an MI355X (a CPU run says nothing about time)')
    lines = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
