"""What the CaiT kernels (csrc/cait_attention.hip) cost on the MI355X (DESIGN.md "CaiT").

    python tools/cait_bench.py kernels [--out profiles/cait_kernels.txt] [--resources]
    python tools/cait_bench.py step    [--out profiles/cait_step.txt]

kernels: bf16, batch 128, the recipe's shapes: cait_s24_224 (H = 8) and cait_xxs24_224 (H = 4), head dimension 48,
talking heads at T = 196 and class attention at T = 197.  Bounds, set before any measurement:
  * ACCEPTANCE: forward, and forward + backward, of each new attention is not slower than ATen's composition in the same
    run (matmul, the two Linears over the head axis, softmax, matmul; for class attention matmul, softmax, matmul),
    through autograd for the backward, warmed up first; "not slower" = inside the spread of ATen's own windows;
  * reported WITHOUT a bound: the ratio to passl_hip_attention_fwd / _bwd at the same B, T, H with head dimension 64.
    No figure can be derived for a kernel that couples the H heads of a row block and does 2 H extra multiply-adds per
    score in each direction.
Exit status 1 when a direction is slower than ATen's.

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands
rotating over more buffers than the last-level cache holds.  --resources appends tools/kernel_resources.py's table.

step: cait_xxs24_224 and cait_s24_224 at batch 128, bf16, eager training steps (forward, CELoss, backward, AdamW with the
config's no-decay groups, no clipping) with drop_path_rate 0 and with the recipe's 0.1.  There is no parent to compare a
step against: the figures are a first record, not a bound."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from convnext_bench import _measure, _stats          # noqa: E402  (the same windows)

DH = 48
SHAPES = (('cait_s24_224', 8), ('cait_xxs24_224', 4))
NO_DECAY = ['cls_token', 'pos_embed', 'norm', 'bias']


def _verdict(lines, what, ours, aten_stats, label):
    am, alo, ahi = aten_stats
    holds = ours <= am * (1 + (ahi - alo) / am)
    lines.append('  %s %s %.1f us against ATen %.1f us = %.2f x: %s' % (
        what, label, ours * 1e3, am * 1e3, ours / am, 'not slower than ATen' if holds else 'SLOWER than ATen'))
    return holds


def talking_heads(args, name, H, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    B, T, dev, dtype = args.batch, 196, torch.device('cuda'), torch.bfloat16
    nbytes = B * T * 3 * H * DH * 2
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)
    gen = torch.Generator().manual_seed(0)
    qkvs = [torch.randn(B * T, 3 * H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    douts = [torch.randn(B * T, H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    outs = [torch.empty(B * T, H * DH, dtype=dtype, device=dev) for _ in range(nset)]
    dqkvs = [torch.empty_like(q) for q in qkvs]
    q64 = [torch.randn(B * T, 3 * H * 64, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    d64 = [torch.randn(B * T, H * 64, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    o64 = [torch.empty(B * T, H * 64, dtype=dtype, device=dev) for _ in range(nset)]
    dq64 = [torch.empty_like(q) for q in q64]
    wl, ww = [(torch.eye(H) + 0.5 * torch.randn(H, H, generator=gen) / H ** 0.5).to(dev) for _ in range(2)]
    bl, bw = [(0.1 * torch.randn(H, generator=gen)).to(dev) for _ in range(2)]
    small = [torch.empty_like(t) for t in (wl, bl, ww, bw)]
    lse = torch.empty(B, H, T, device=dev)
    wsb = torch.empty(ops.talking_heads_attention_ws_floats(B, T, H), device=dev)
    scale, dt = DH ** -0.5, L.dt(dtype)

    def t_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_talking_heads_attention_fwd(p(qkvs[j]), p(wl), p(bl), p(ww), p(bw), p(outs[j]), p(lse), B, T, H,
                                                          DH, scale, dt, st))

    def t_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_talking_heads_attention_bwd(p(qkvs[j]), p(wl), p(bl), p(ww), p(bw), p(douts[j]), p(lse),
                                                          p(dqkvs[j]), *[p(t) for t in small], p(wsb), wsb.numel(), B, T, H,
                                                          DH, scale, dt, st))

    def a_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_attention_fwd(p(q64[j]), p(o64[j]), p(lse), B, T, H, 64, 0.125, 0, dt, st))

    def a_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_attention_bwd(p(q64[j]), p(o64[j]), p(d64[j]), p(lse), p(dq64[j]), B, T, H, 64, 0.125, 0, dt, st))
    variants = [('attention64 fwd', a_fwd), ('talking fwd', t_fwd), ('attention64 bwd', a_bwd), ('talking bwd', t_bwd)]
    t_fwd(0)
    a_fwd(0)
    wlb, wwb, blb, bwb = wl.to(dtype), ww.to(dtype), bl.to(dtype), bw.to(dtype)

    def aten(qkv):
        q, k, v = qkv.view(B, T, 3, H, DH).permute(2, 0, 3, 1, 4).unbind(0)
        a = (q * scale) @ k.transpose(-1, -2)
        a = (a.permute(0, 2, 3, 1) @ wlb + blb).permute(0, 3, 1, 2)
        a = torch.softmax(a, dim=-1)
        a = (a.permute(0, 2, 3, 1) @ wwb + bwb).permute(0, 3, 1, 2)
        return (a @ v).transpose(1, 2).reshape(B * T, H * DH)
    leaf = [q.clone().requires_grad_() for q in qkvs]

    def e_fwd(i):
        with torch.no_grad():
            aten(qkvs[i % nset])

    def e_fwd_bwd(i):
        j = i % nset
        leaf[j].grad = None
        aten(leaf[j]).backward(douts[j])
    e_fwd(0)
    e_fwd_bwd(0)
    torch.cuda.synchronize()
    variants += [('aten fwd', e_fwd), ('aten fwd+bwd', e_fwd_bwd)]
    times = _measure(variants, args.launches, args.rounds)
    mean = {n: _stats(ts) for n, ts in times.items()}
    lines.append('%s talking heads [%d, %d] %d heads x %d, bf16: qkv %.1f MB, %d operand sets' % (name, B, T, H, DH, nbytes / 1e6,
                                                                                              nset))
    lines.append('  %-16s %9s %9s %9s' % ('launch', 'mean us', 'min us', 'max us'))
    for n, _f in variants:
        lines.append('  %-16s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in mean[n])))
    for d in ('fwd', 'bwd'):
        lines.append('  talking %s / attention64 %s = %.3f (no bound)' % (d, d, mean['talking ' + d][0] / mean['attention64 ' + d][0]))
    ok = _verdict(lines, 'talking heads', mean['talking fwd'][0], mean['aten fwd'], 'fwd')
    return _verdict(lines, 'talking heads', mean['talking fwd'][0] + mean['talking bwd'][0], mean['aten fwd+bwd'], 'fwd+bwd') and ok


def class_attention(args, name, H, lines):
    from passl_amd.hip import lib as L
    lib, st, p = L.load(), L.stream(), L.ptr
    B, T, dev, dtype = args.batch, 197, torch.device('cuda'), torch.bfloat16
    nbytes = 2 * B * T * H * DH * 2
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)
    gen = torch.Generator().manual_seed(1)
    ks, vs = [[torch.randn(B * T, H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)] for _ in range(2)]
    qs, dos = [[torch.randn(B, H * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)] for _ in range(2)]
    out, dq = torch.empty_like(qs[0]), torch.empty_like(qs[0])
    dk, dv = torch.empty_like(ks[0]), torch.empty_like(ks[0])
    lse = torch.empty(B, H, device=dev)
    scale, dt = DH ** -0.5, L.dt(dtype)

    def c_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_class_attention_fwd(p(qs[j]), p(ks[j]), p(vs[j]), p(out), p(lse), B, T, H, DH, scale, dt, st))

    def c_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_class_attention_bwd(p(qs[j]), p(ks[j]), p(vs[j]), p(dos[j]), p(lse), p(dq), p(dk), p(dv), B, T,
                                                  H, DH, scale, dt, st))
    c_fwd(0)

    def aten(q, k, v):
        a = torch.softmax((q.view(B, H, 1, DH) * scale) @ k.view(B, T, H, DH).permute(0, 2, 3, 1), dim=-1)
        return (a @ v.view(B, T, H, DH).transpose(1, 2)).reshape(B, H * DH)
    leaves = [[t.clone().requires_grad_() for t in (qs[j], ks[j], vs[j])] for j in range(nset)]

    def e_fwd(i):
        j = i % nset
        with torch.no_grad():
            aten(qs[j], ks[j], vs[j])

    def e_fwd_bwd(i):
        j = i % nset
        for t in leaves[j]:
            t.grad = None
        aten(*leaves[j]).backward(dos[j])
    e_fwd(0)
    e_fwd_bwd(0)
    torch.cuda.synchronize()
    variants = [('class fwd', c_fwd), ('class bwd', c_bwd), ('aten fwd', e_fwd), ('aten fwd+bwd', e_fwd_bwd)]
    times = _measure(variants, args.launches, args.rounds)
    mean = {n: _stats(ts) for n, ts in times.items()}
    lines.append('%s class attention [%d, %d] %d heads x %d, bf16: k + v %.1f MB, %d operand sets' % (name, B, T, H, DH,
                                                                                                  nbytes / 1e6, nset))
    for n, _f in variants:
        lines.append('  %-16s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in mean[n])))
    lines.append('  class fwd reads k, v at %.0f GB/s; class bwd moves 2 x that at %.0f GB/s' % (
        nbytes / (mean['class fwd'][0] * 1e-3) / 1e9, 2 * nbytes / (mean['class bwd'][0] * 1e-3) / 1e9))
    ok = _verdict(lines, 'class attention', mean['class fwd'][0], mean['aten fwd'], 'fwd')
    return _verdict(lines, 'class attention', mean['class fwd'][0] + mean['class bwd'][0], mean['aten fwd+bwd'], 'fwd+bwd') and ok


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches)]
    ok = True
    for name, H in SHAPES:
        ok = talking_heads(args, name, H, lines) and ok
        torch.cuda.empty_cache()
        ok = class_attention(args, name, H, lines) and ok
        torch.cuda.empty_cache()
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'cait_attention.hip'],
                           capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py cait_attention.hip'] + \
            (r.stdout if r.returncode == 0 else r.stderr).splitlines()
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
    lines = ['batch %d, 224 x 224, bf16, eager steps (forward, CELoss, backward, AdamW with no-decay groups); %d rounds x %d '
             'steps per window, alternating' % (B, args.rounds, args.steps),
             '%-18s %-16s %9s %9s %9s' % ('model', 'drop_path_rate', 'mean ms', 'min ms', 'max ms')]
    for name in ('cait_xxs24_224', 'cait_s24_224'):
        runs, rate = {}, 0.1
        for r in (0.0, rate):
            torch.manual_seed(0)
            model = PM.build_model(dict(name=name, drop_path_rate=r, num_classes=1000)).train()
            named = list(model.named_parameters())
            skip = {n for n, _ in named if any(nd in n for nd in NO_DECAY)}
            groups = [{'params': [q for n, q in named if n not in skip]},
                      {'params': [q for n, q in named if n in skip], 'weight_decay': 0.0}]
            opt = AdamW(1e-3, weight_decay=0.05, parameters=groups)
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
            lines.append('%-18s %-16s %9.3f %9.3f %9.3f' % ((name, r) + stats[r]))
        m0, m1 = stats[0.0][0], stats[rate][0]
        lines.append('%-18s rate %.1f against 0: %+.3f ms per step (%+.2f %%)' % (name, rate, m1 - m0, 100 * (m1 / m0 - 1)))
        del runs
        torch.cuda.empty_cache()
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cait_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
