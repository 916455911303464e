"""What the key-tiled attention kernels (csrc/attention_tiled.hip) and the DeiT steps cost on the MI355X (DESIGN.md "DeiT").

    python tools/deit_bench.py kernels [--out profiles/deit_kernels.txt] [--resources]
    python tools/deit_bench.py step    [--out profiles/deit_step.txt]

kernels: batch 64, 12 heads x 64, bf16 and fp32, the shapes of DeiT-B at 384 pixels (T = 577) and at 224 (T = 197).
Set before any measurement:
  * ACCEPTANCE: the tiled forward + backward at T = 577 is not slower than ATen's scaled_dot_product_attention forward +
    backward (through autograd) in the same run, warmed up first; "not slower" = inside the spread of ATen's own windows;
  * EXPECTATION, reported as HELD or MISSED and no gate: the tiled pair at T = 577 is within 1.25 x of the dense pair
    (passl_hip_attention_fwd / _bwd) at T = 197 scaled by (577 / 197)^2 — the same work per score, staged differently,
    and 1.25 is the project's usual margin for that;
  * informative only: the tiled pair at T = 197 against the dense pair on the same buffers (are the dense kernels still
    worth keeping below 208 tokens?).
Exit status 1 when the acceptance fails.

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands
rotating over at least two buffer sets that together exceed the last-level cache.  --resources appends
tools/kernel_resources.py's table.

step: eager bf16 training steps (forward, CELoss, backward, AdamW with the config's no-decay groups, no clipping) of
DeiT_base_patch16_384 at batch 64 and of DeiT_base_patch16_224 at batch 128 with drop_path_rate 0 and the recipe's 0.1.
There is no parent to compare a step against: the figures are a first record, not a bound."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from convnext_bench import _measure, _stats          # noqa: E402  (the same windows)

H, DH = 12, 64
T_LONG, T_SHORT = 577, 197
MARGIN = 1.25
NO_DECAY = ['cls_token', 'pos_embed', 'norm', 'bias']


def _buffers(B, T, dtype, gen, dev):
    nbytes = B * T * 3 * H * DH * torch.empty(0, dtype=dtype).element_size()
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)
    qkv = [torch.randn(B * T, 3 * H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    dout = [torch.randn(B * T, H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    out = [torch.empty(B * T, H * DH, dtype=dtype, device=dev) for _ in range(nset)]
    dqkv = [torch.empty_like(q) for q in qkv]
    return nset, nbytes, qkv, dout, out, dqkv


def attention(args, dtype, lines):
    from passl_amd.hip import lib as L
    lib, st, p = L.load(), L.stream(), L.ptr
    B, dev, dt, scale = args.batch, torch.device('cuda'), L.dt(dtype), DH ** -0.5
    gen = torch.Generator().manual_seed(0)
    name = {torch.bfloat16: 'bf16', torch.float32: 'fp32'}[dtype]
    mean = {}
    for T in (T_LONG, T_SHORT):
        nset, nbytes, qkv, dout, out, dqkv = _buffers(B, T, dtype, gen, dev)
        lse = torch.empty(B, H, T, device=dev)

        def t_fwd(i):
            j = i % nset
            L.check(lib.passl_hip_attention_tiled_fwd(p(qkv[j]), p(out[j]), p(lse), B, T, H, DH, scale, dt, st))

        def t_bwd(i):
            j = i % nset
            L.check(lib.passl_hip_attention_tiled_bwd(p(qkv[j]), p(out[j]), p(dout[j]), p(lse), p(dqkv[j]), B, T, H, DH,
                                                      scale, dt, st))

        def d_fwd(i):
            j = i % nset
            L.check(lib.passl_hip_attention_fwd(p(qkv[j]), p(out[j]), p(lse), B, T, H, DH, scale, 0, dt, st))

        def d_bwd(i):
            j = i % nset
            L.check(lib.passl_hip_attention_bwd(p(qkv[j]), p(out[j]), p(dout[j]), p(lse), p(dqkv[j]), B, T, H, DH, scale, 0,
                                                dt, st))
        t_fwd(0)                                          # lse and out of the backward's operands are real ones
        variants = [('tiled fwd', t_fwd), ('tiled bwd', t_bwd)]
        if T == T_SHORT:
            variants += [('dense fwd', d_fwd), ('dense bwd', d_bwd)]
        else:
            leaf = [q.clone().requires_grad_() for q in qkv]

            def sdpa(x):
                q, k, v = x.view(B, T, 3, H, DH).permute(2, 0, 3, 1, 4).unbind(0)
                o = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
                return o.transpose(1, 2).reshape(B * T, H * DH)

            def e_fwd(i):
                with torch.no_grad():
                    sdpa(qkv[i % nset])

            def e_fwd_bwd(i):
                j = i % nset
                leaf[j].grad = None
                sdpa(leaf[j]).backward(dout[j])
            e_fwd(0)
            e_fwd_bwd(0)
            variants += [('aten sdpa fwd', e_fwd), ('aten sdpa fwd+bwd', e_fwd_bwd)]
        torch.cuda.synchronize()
        times = _measure(variants, args.launches, args.rounds)
        mean[T] = {n: _stats(ts) for n, ts in times.items()}
        lines.append('%s [%d, %d] %d heads x %d: qkv %.1f MB, %d operand sets' % (name, B, T, H, DH, nbytes / 1e6, nset))
        lines.append('  %-18s %9s %9s %9s' % ('launch', 'mean us', 'min us', 'max us'))
        for n, _f in variants:
            lines.append('  %-18s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in mean[T][n])))
        del qkv, dout, out, dqkv, variants
        torch.cuda.empty_cache()
    lo, sh = mean[T_LONG], mean[T_SHORT]
    pair = lo['tiled fwd'][0] + lo['tiled bwd'][0]
    am, alo, ahi = lo['aten sdpa fwd+bwd']
    ok = pair <= am * (1 + (ahi - alo) / am)
    lines.append('  %s tiled fwd+bwd at T = %d: %.1f us against ATen sdpa %.1f us = %.2f x: %s' % (
        name, T_LONG, pair * 1e3, am * 1e3, pair / am, 'not slower than ATen' if ok else 'SLOWER than ATen'))
    lines.append('  %s tiled fwd at T = %d: %.1f us against ATen sdpa fwd %.1f us = %.2f x (no bound)' % (
        name, T_LONG, lo['tiled fwd'][0] * 1e3, lo['aten sdpa fwd'][0] * 1e3, lo['tiled fwd'][0] / lo['aten sdpa fwd'][0]))
    grow = (T_LONG / T_SHORT) ** 2
    for d in ('fwd', 'bwd'):
        want = sh['dense ' + d][0] * grow
        r = lo['tiled ' + d][0] / want
        lines.append('  %s tiled %s at T = %d: %.1f us against dense %s at T = %d x %.2f = %.1f us: %.2f x, expectation %.2f x %s'
                     % (name, d, T_LONG, lo['tiled ' + d][0] * 1e3, d, T_SHORT, grow, want * 1e3, r, MARGIN,
                        'HELD' if r <= MARGIN else 'MISSED'))
        lines.append('  %s tiled %s / dense %s at T = %d = %.2f (informative)' % (
            name, d, d, T_SHORT, sh['tiled ' + d][0] / sh['dense ' + d][0]))
    return ok


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches)]
    ok = True
    for dtype in (torch.bfloat16, torch.float32):
        ok = attention(args, dtype, lines) and ok
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'attention_tiled.hip',
                            'deit_tokens.hip'], capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py attention_tiled.hip deit_tokens.hip'] + \
            (r.stdout if r.returncode == 0 else r.stderr).splitlines()
    return lines, ok


def step(args):
    import passl.models as PM
    from passl_amd.hip import config as hip_config
    from passl_amd.loss.celoss import CELoss
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(0)
    lines = ['bf16, eager steps (forward, CELoss, backward, AdamW with no-decay groups); %d rounds x %d steps per window, '
             'alternating' % (args.rounds, args.steps),
             '%-26s %5s %-16s %9s %9s %9s' % ('model', 'batch', 'drop_path_rate', 'mean ms', 'min ms', 'max ms')]
    for name, size, B, rates in (('DeiT_base_patch16_384', 384, 64, (0.1,)), ('DeiT_base_patch16_224', 224, 128, (0.0, 0.1))):
        x = torch.randn(B, 3, size, size, generator=gen).to(dev)
        y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
        runs = {}
        for r in rates:
            torch.manual_seed(0)
            model = PM.build_model(dict(name=name, drop_path_rate=r, class_num=1000)).train()
            named = list(model.named_parameters())
            skip = {n for n, _ in named if any(nd in n for nd in NO_DECAY)}
            groups = [{'params': [q for n, q in named if n not in skip]},
                      {'params': [q for n, q in named if n in skip], 'weight_decay': 0.0}]
            opt = AdamW(1e-3, weight_decay=0.05, parameters=groups)
            celoss = CELoss()

            def one(_i, model=model, opt=opt, celoss=celoss, x=x, y=y):
                loss = celoss(model(x), y)['CELoss']
                opt.clear_grad()
                loss.backward()
                opt.step()
            runs[r] = one
        times = _measure(list(runs.items()), args.steps, args.rounds)
        stats = {r: _stats(times[r]) for r in runs}
        for r in runs:
            lines.append('%-26s %5d %-16s %9.3f %9.3f %9.3f' % ((name, B, r) + stats[r]))
        if len(rates) > 1:
            m0, m1 = stats[rates[0]][0], stats[rates[1]][0]
            lines.append('%-26s rate %.1f against 0: %+.3f ms per step (%+.2f %%)' % (name, rates[1], m1 - m0,
                                                                                     100 * (m1 / m0 - 1)))
        del runs, x, y
        torch.cuda.empty_cache()
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=64, help='kernels: images per launch')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('deit_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
