"""What the Swin kernels (csrc/window_attention.hip) cost on the MI355X (DESIGN.md "Swin Transformer").

    python tools/swin_bench.py kernels [--out profiles/swin_kernels.txt] [--resources]
    python tools/swin_bench.py step    [--out profiles/swin_step.txt]

kernels: window attention on the four stage shapes of swin_tiny at batch 128 (56^2 x 3 heads with shift 0 and 3,
28^2 x 6, 14^2 x 12 shifted, 7^2 x 24), window 7, head dimension 32, bf16.  Each direction is reported
  * against passl_hip_attention_fwd / _bwd on the same number of (sequence, head) pairs laid out contiguously
    ([B * nW, 49, 3, nH, 32]) in the same run: the same arithmetic and the same 64-byte head rows.  Bound, set before any
    measurement: within 1.25 x, the margin the project gives "same bytes" comparisons.  The backward is timed as the
    whole entry point, its two table-gradient reduction launches included (the C ABI does not launch them apart), so a
    backward inside the bound is inside it without them too; the reduction alone is not separated here;
  * against ATen: roll + window_partition + scaled_dot_product_attention with the additive bias-and-mask tensor +
    window_reverse + roll, forward and forward + backward through autograd, warmed up first.  Acceptance: not slower
    beyond the spread of ATen's own windows.
Then passl_hip_patch_merge / _bwd next to passl_hip_copy_bytes of the bytes they move (bound 1.25 x).  Exit status 1 when
a bound is missed or a direction is slower than ATen's.

Device events around WINDOWS of back-to-back launches, the variants alternating inside one process, the operands
rotating over more buffers than the last-level cache holds.  --resources appends tools/kernel_resources.py's table.

step: swin_tiny and swin_base (patch 4, window 7, 224) at batch 128, bf16, eager training steps (forward, CELoss,
backward, AdamW with the config's no-decay groups and clipping) with drop_path_rate 0 and with the recipe's rate
(0.2 / 0.5).  There is no parent to compare a step against: the figures are a first record, not a bound."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from convnext_bench import _measure, _stats          # noqa: E402  (the same windows)

WS, DH = 7, 32
STAGES = ((56, 3, 0), (56, 3, 3), (28, 6, 3), (14, 12, 3), (7, 24, 0))      # (map side, heads, shift)
NO_DECAY = ['absolute_pos_embed', 'relative_position_bias_table', 'norm', 'bias']


def _aten_bias_mask(table, Hp, Wp, shift, nH):
    """[nW, nH, T, T] additive tensor of the reference: bias gather + -100 mask."""
    from passl_amd.models.swin_transformer import get_relative_position_index, shifted_window_mask
    T = WS * WS
    idx = get_relative_position_index(WS, WS).to(table.device)
    bias = table[idx.reshape(-1)].reshape(T, T, nH).permute(2, 0, 1)
    nW = (Hp // WS) * (Wp // WS)
    add = bias.unsqueeze(0).expand(nW, nH, T, T).clone()
    if shift:
        add += shifted_window_mask(Hp, Wp, WS, shift).to(table.device).unsqueeze(1)
    return add


def attention_shape(args, HW, nH, shift, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    B, dev, dtype = args.batch, torch.device('cuda'), torch.bfloat16
    Ln, T, nW = HW * HW, WS * WS, (HW // WS) ** 2
    seqs = B * nW
    nbytes = B * Ln * 3 * nH * DH * 2
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)
    gen = torch.Generator().manual_seed(0)
    qkvs = [torch.randn(B * Ln, 3 * nH * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    douts = [torch.randn(B * Ln, nH * DH, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    outs = [torch.empty(B * Ln, nH * DH, dtype=dtype, device=dev) for _ in range(nset)]
    dqkvs = [torch.empty_like(q) for q in qkvs]
    table = (torch.randn((2 * WS - 1) ** 2, nH, generator=gen) * 0.5).to(dev)
    dtable = torch.empty_like(table)
    lse = torch.empty(seqs, nH, T, device=dev)
    wsb = torch.empty(ops.window_attention_ws_floats(seqs, nH, WS), device=dev)
    scale, dt = DH ** -0.5, L.dt(dtype)

    def w_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_window_attention_fwd(p(qkvs[j]), p(table), p(outs[j]), p(lse), B, HW, HW, WS, shift, nH, DH,
                                                   scale, dt, st))

    def w_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_window_attention_bwd(p(qkvs[j]), p(table), p(outs[j]), p(douts[j]), p(lse), p(dqkvs[j]),
                                                   p(dtable), p(wsb), wsb.numel(), B, HW, HW, WS, shift, nH, DH, scale,
                                                   dt, st))

    def a_fwd(i):                                   # the same tensors read as [seqs, 49, 3, nH, DH]: contiguous sequences
        j = i % nset
        L.check(lib.passl_hip_attention_fwd(p(qkvs[j]), p(outs[j]), p(lse), seqs, T, nH, DH, scale, 0, dt, st))

    def a_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_attention_bwd(p(qkvs[j]), p(outs[j]), p(douts[j]), p(lse), p(dqkvs[j]), seqs, T, nH, DH,
                                            scale, 0, dt, st))
    variants = [('attention fwd', a_fwd), ('window fwd', w_fwd), ('attention bwd', a_bwd), ('window bwd', w_bwd)]
    w_fwd(0)
    aten_error = None
    try:
        F = torch.nn.functional
        add = _aten_bias_mask(table, HW, HW, shift, nH).to(dtype)

        def aten(qkv):
            x = qkv.view(B, HW, HW, 3 * nH * DH)
            if shift:
                x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
            x = x.view(B, HW // WS, WS, HW // WS, WS, 3, nH, DH).permute(5, 0, 1, 3, 6, 2, 4, 7)
            q, k, v = x.reshape(3, B, nW, nH, T, DH).unbind(0)
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=add.unsqueeze(0), scale=scale)
            o = o.view(B, HW // WS, HW // WS, nH, WS, WS, DH).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, HW, HW, nH * DH)
            if shift:
                o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
            return o.reshape(B * Ln, nH * DH)
        leaf = [q.clone().requires_grad_() for q in qkvs]

        def t_fwd(i):
            with torch.no_grad():
                aten(qkvs[i % nset])

        def t_fwd_bwd(i):
            j = i % nset
            leaf[j].grad = None
            aten(leaf[j]).backward(douts[j])
        t_fwd(0)
        t_fwd_bwd(0)
        torch.cuda.synchronize()
        variants += [('aten fwd', t_fwd), ('aten fwd+bwd', t_fwd_bwd)]
    except Exception as e:                      # noqa: BLE001  (reported, not hidden)
        aten_error = '%s: %s' % (type(e).__name__, str(e).splitlines()[0][:120])
    times = _measure(variants, args.launches, args.rounds)
    mean = {n: _stats(ts) for n, ts in times.items()}
    lines.append('[%d, %d, %d] window %d shift %d, %d heads x %d, bf16: %d sequences of %d tokens, qkv %.1f MB, %d operand '
                 'sets' % (B, HW, HW, WS, shift, nH, DH, seqs, T, nbytes / 1e6, nset))
    lines.append('  %-14s %9s %9s %9s' % ('launch', 'mean us', 'min us', 'max us'))
    for n, _f in variants:
        lines.append('  %-14s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in mean[n])))
    ok = True
    for d in ('fwd', 'bwd'):
        ratio = mean['window ' + d][0] / mean['attention ' + d][0]
        holds = ratio <= 1.25
        ok = ok and holds
        lines.append('  window %s / attention %s = %.3f; bound 1.25: %s' % (d, d, ratio, 'HOLDS' if holds else 'MISSED'))
    if aten_error:
        lines.append('  ATen cannot run here: ' + aten_error)
    else:
        for ours, theirs in (((mean['window fwd'][0]), 'aten fwd'),
                             ((mean['window fwd'][0] + mean['window bwd'][0]), 'aten fwd+bwd')):
            am, alo, ahi = mean[theirs]
            holds = ours <= am * (1 + (ahi - alo) / am)
            ok = ok and holds
            lines.append('  window %s %.1f us against %s %.1f us = %.2f x: %s' % (
                theirs[5:], ours * 1e3, theirs, am * 1e3, ours / am, 'not slower than ATen' if holds else 'SLOWER than ATen'))
    return ok


def patch_merge(args, lines):
    from passl_amd.hip import lib as L
    lib, st, p = L.load(), L.stream(), L.ptr
    B, H, C, dtype, dev = args.batch, 56, 96, torch.bfloat16, torch.device('cuda')
    n = B * H * H * C
    nbytes = n * 2
    nset = max(2, -(-(300 << 20) // (2 * nbytes)) + 1)
    xs = [torch.randn(n, device=dev).to(dtype) for _ in range(nset)]
    ys = [torch.empty(n, dtype=dtype, device=dev) for _ in range(nset)]
    dt = L.dt(dtype)

    def copy(i):
        L.check(lib.passl_hip_copy_bytes(p(ys[i % nset]), p(xs[i % nset]), nbytes, st))

    def fwd(i):
        L.check(lib.passl_hip_patch_merge(p(xs[i % nset]), p(ys[i % nset]), B, H, H, C, dt, st))

    def bwd(i):
        L.check(lib.passl_hip_patch_merge_bwd(p(xs[i % nset]), p(ys[i % nset]), B, H, H, C, dt, st))
    variants = [('copy_bytes', copy), ('patch_merge', fwd), ('patch_merge_bwd', bwd)]
    times = _measure(variants, args.launches, args.rounds)
    cm = _stats(times['copy_bytes'])[0]
    lines.append('patch merge [%d, %d, %d, %d] bf16 = %.1f MB, %d operand sets' % (B, H, H, C, nbytes / 1e6, nset))
    ok = True
    for name, _f in variants:
        m, lo, hi = _stats(times[name])
        lines.append('  %-16s %9.1f %9.1f %9.1f us  %6.0f GB/s  %.2f x copy' % (name, m * 1e3, lo * 1e3, hi * 1e3,
                                                                                2 * nbytes / (m * 1e-3) / 1e9, m / cm))
        if name != 'copy_bytes':
            holds = m <= 1.25 * cm
            ok = ok and holds
            lines.append('  %s / copy_bytes = %.3f; bound 1.25: %s' % (name, m / cm, 'HOLDS' if holds else 'MISSED'))
    return ok


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches)]
    ok = True
    for HW, nH, shift in STAGES:
        ok = attention_shape(args, HW, nH, shift, lines) and ok
        torch.cuda.empty_cache()
    ok = patch_merge(args, lines) and ok
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'window_attention.hip'],
                           capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py window_attention.hip'] + \
            (r.stdout if r.returncode == 0 else r.stderr).splitlines()
    return lines, ok


def step(args):
    import passl.models as PM
    from passl_amd.core.grad_clip import ClipGradByGlobalNorm
    from passl_amd.hip import config as hip_config
    from passl_amd.loss.celoss import CELoss
    from passl_amd.solver.optimizer import AdamW
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev, B = torch.device('cuda'), args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    y = torch.randint(0, 1000, (B,), generator=gen).to(dev)
    lines = ['batch %d, 224 x 224, bf16, eager steps (forward, CELoss, backward, AdamW with no-decay groups and clipping '
             'at 5); %d rounds x %d steps per window, alternating' % (B, args.rounds, args.steps),
             '%-30s %-16s %9s %9s %9s' % ('model', 'drop_path_rate', 'mean ms', 'min ms', 'max ms')]
    for name, rate in (('swin_tiny_patch4_window7_224', 0.2), ('swin_base_patch4_window7_224', 0.5)):
        runs = {}
        for r in (0.0, rate):
            torch.manual_seed(0)
            model = PM.build_model(dict(name=name, drop_path_rate=r, num_classes=1000)).train()
            named = list(model.named_parameters())
            skip = {n for n, _ in named if any(nd in n for nd in NO_DECAY)}
            groups = [{'params': [q for n, q in named if n not in skip]},
                      {'params': [q for n, q in named if n in skip], 'weight_decay': 0.0}]
            opt = AdamW(1e-3, weight_decay=0.05, parameters=groups, grad_clip=ClipGradByGlobalNorm(clip_norm=5.0))
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
            lines.append('%-30s %-16s %9.3f %9.3f %9.3f' % ((name, r) + stats[r]))
        m0, m1 = stats[0.0][0], stats[rate][0]
        lines.append('%-30s rate %.1f against 0: %+.3f ms per step (%+.2f %%)' % (name, rate, m1 - m0, 100 * (m1 / m0 - 1)))
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
        raise SystemExit('swin_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
