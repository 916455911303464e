"""What the CAE kernels (csrc/cross_attention.hip, csrc/cae.hip) and the CAE pre-training step cost on the MI355X
(DESIGN.md "CAE").

    python tools/cae_bench.py kernels [--out profiles/cae_kernels.txt] [--resources]
    python tools/cae_bench.py step    [--out profiles/cae_step.txt]

kernels: batch 128, 12 heads x 64, Tq = 75 queries against Tk = 196 keys, bf16 and fp32.  Set before any measurement:
  * ACCEPTANCE: cross-attention forward + backward is not slower than ATen's scaled_dot_product_attention forward +
    backward (through autograd) on the same tensors in the same run; "not slower" = inside the spread of ATen's windows;
  * EXPECTATION, reported as HELD or MISSED and no gate: forward and backward each within 1.25 x of
    passl_hip_attention_tiled_fwd / _bwd at T = 196 in the same run scaled by 75 / 196 (the ratio of score work); the
    margin covers the partly filled last query block;
  * EXPECTATION: cae_tokens_assemble and its backward each within 1.25 x of passl_hip_copy_bytes of the bytes they move;
  * mse forward and backward: reported only.
Exit status 1 when the acceptance fails.

step: the bf16 batch-128 step of cae_base_patch16_224_8k_vocab with pretrain.sh's values (forward, the two losses,
backward, clipped AdamW in the two groups), eager and replayed from a strict step plan.  A first record: there is no
parent to compare with.  The share of the step spent in the new kernels is the kernels' own time (measured here, in the
same process, on the step's shapes) times their launches per step over the replayed step; it is NOT MEASURED inside
the step."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from convnext_bench import _measure, _stats          # noqa: E402  (the same windows)

H, DH, TQ, TK, C = 12, 64, 75, 196, 768
MARGIN = 1.25


def _sets(nbytes):
    return max(2, -(-(300 << 20) // (2 * nbytes)) + 1)          # past the 256 MB last-level cache


def _rows(lines, variants, stats):
    lines.append('  %-26s %9s %9s %9s' % ('launch', 'mean us', 'min us', 'max us'))
    for n, _f in variants:
        lines.append('  %-26s %9.1f %9.1f %9.1f' % ((n,) + tuple(v * 1e3 for v in stats[n])))


def attention(args, dtype, lines):
    from passl_amd.hip import lib as L
    lib, st, p = L.load(), L.stream(), L.ptr
    B, dev, dt, scale = args.batch, torch.device('cuda'), L.dt(dtype), DH ** -0.5
    gen = torch.Generator().manual_seed(0)
    name = {torch.bfloat16: 'bf16', torch.float32: 'fp32'}[dtype]
    es = torch.empty(0, dtype=dtype).element_size()
    nset = _sets(B * (2 * TQ + 2 * TK) * H * DH * es)

    def rand(T, cols=H * DH):
        return [torch.randn(B * T, cols, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    q, k, v, dout = rand(TQ), rand(TK), rand(TK), rand(TQ)
    out = [torch.empty_like(t) for t in q]
    dq, dk, dv = [torch.empty_like(t) for t in q], [torch.empty_like(t) for t in k], [torch.empty_like(t) for t in v]
    lse = torch.empty(B, H, TQ, device=dev)
    qkv, dout_t = rand(TK, 3 * H * DH), rand(TK)
    out_t, dqkv = [torch.empty_like(t) for t in dout_t], [torch.empty_like(t) for t in qkv]
    lse_t = torch.empty(B, H, TK, device=dev)

    def x_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_cross_attention_fwd(p(q[j]), p(k[j]), p(v[j]), p(out[j]), p(lse), B, TQ, TK, H, DH, scale,
                                                  dt, st))

    def x_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_cross_attention_bwd(p(q[j]), p(k[j]), p(v[j]), p(out[j]), p(dout[j]), p(lse), p(dq[j]),
                                                  p(dk[j]), p(dv[j]), B, TQ, TK, H, DH, scale, dt, st))

    def t_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_attention_tiled_fwd(p(qkv[j]), p(out_t[j]), p(lse_t), B, TK, H, DH, scale, dt, st))

    def t_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_attention_tiled_bwd(p(qkv[j]), p(out_t[j]), p(dout_t[j]), p(lse_t), p(dqkv[j]), B, TK, H, DH,
                                                  scale, dt, st))
    leaves = [[t.clone().requires_grad_() for t in ts] for ts in (q, k, v)]

    def sdpa(a, b, c):
        a, b, c = [t.view(B, -1, H, DH).transpose(1, 2) for t in (a, b, c)]
        o = torch.nn.functional.scaled_dot_product_attention(a, b, c, scale=scale)
        return o.transpose(1, 2).reshape(B * TQ, H * DH)

    def e_fwd(i):
        j = i % nset
        with torch.no_grad():
            sdpa(q[j], k[j], v[j])

    def e_fwd_bwd(i):
        j = i % nset
        for ls in leaves:
            ls[j].grad = None
        sdpa(leaves[0][j], leaves[1][j], leaves[2][j]).backward(dout[j])
    for f in (x_fwd, t_fwd, e_fwd, e_fwd_bwd):
        f(0)
    variants = [('cross fwd', x_fwd), ('cross bwd', x_bwd), ('tiled fwd T=196', t_fwd), ('tiled bwd T=196', t_bwd),
                ('aten sdpa fwd', e_fwd), ('aten sdpa fwd+bwd', e_fwd_bwd)]
    torch.cuda.synchronize()
    times = _measure(variants, args.launches, args.rounds)
    s = {n: _stats(ts) for n, ts in times.items()}
    lines.append('%s [%d] %d heads x %d, Tq = %d, Tk = %d: %d operand sets' % (name, B, H, DH, TQ, TK, nset))
    _rows(lines, variants, s)
    pair = s['cross fwd'][0] + s['cross bwd'][0]
    am, alo, ahi = s['aten sdpa fwd+bwd']
    ok = pair <= am * (1 + (ahi - alo) / am)
    lines.append('  %s cross fwd+bwd %.1f us against ATen sdpa fwd+bwd %.1f us = %.2f x: %s' % (
        name, pair * 1e3, am * 1e3, pair / am, 'not slower than ATen' if ok else 'SLOWER than ATen'))
    for d in ('fwd', 'bwd'):
        want = s['tiled %s T=196' % d][0] * TQ / TK
        r = s['cross ' + d][0] / want
        lines.append('  %s cross %s %.1f us against tiled %s at T = 196 x 75 / 196 = %.1f us: %.2f x, expectation %.2f x %s'
                     % (name, d, s['cross ' + d][0] * 1e3, d, want * 1e3, r, MARGIN, 'HELD' if r <= MARGIN else 'MISSED'))
    return ok, {'cross fwd': s['cross fwd'][0], 'cross bwd': s['cross bwd'][0]}


def streaming(args, dtype, lines):
    from passl_amd.hip import lib as L
    from passl_amd.hip import ops
    lib, st, p = L.load(), L.stream(), L.ptr
    B, dev, dt = args.batch, torch.device('cuda'), L.dt(dtype)
    Nu, Nm, Ln = TK - TQ, TQ, TK
    gen = torch.Generator().manual_seed(1)
    name = {torch.bfloat16: 'bf16', torch.float32: 'fp32'}[dtype]
    es = torch.empty(0, dtype=dtype).element_size()
    row = C * es
    fwd_bytes = B * ((1 + Nu) + Nm + Nm + 2 * (Nu + Nm)) * row          # xu (class row skipped), xm | q_in, k_in, v_in
    bwd_bytes = B * (Nm + 2 * (Nu + Nm) + (1 + Nu) + Nm) * row
    nset = _sets(fwd_bytes)

    def rand(T):
        return [torch.randn(B * T, C, generator=gen).to(dev).to(dtype) for _ in range(nset)]
    xu, xm, dq, dk, dv = rand(1 + Nu), rand(Nm), rand(Nm), rand(Nu + Nm), rand(Nu + Nm)
    q_in, k_in, v_in = [torch.empty_like(t) for t in dq], [torch.empty_like(t) for t in dk], [torch.empty_like(t) for t in dv]
    dxu, dxm = [torch.empty_like(t) for t in xu], [torch.empty_like(t) for t in xm]
    pos = torch.randn(1 + Ln, C, generator=gen).to(dev)
    mask = torch.zeros(B, Ln)
    for b in range(B):
        mask[b, torch.randperm(Ln, generator=gen)[:Nm]] = 1.0
    ids_vis, ids_msk, _rank = ops.cae_mask_ids(mask.to(dev), Nu)
    big = max(fwd_bytes, bwd_bytes) // 2
    ca = [torch.empty(big, dtype=torch.uint8, device=dev) for _ in range(nset)]
    cb = [torch.empty(big, dtype=torch.uint8, device=dev) for _ in range(nset)]
    loss, ws = torch.empty(1, device=dev), torch.empty(B * Nm, device=dev)
    tgt = rand(1 + Nm)

    def a_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_cae_tokens_assemble(p(xu[j]), p(xm[j]), p(pos), p(ids_vis), p(ids_msk), p(q_in[j]),
                                                  p(k_in[j]), p(v_in[j]), B, 1, Nu, Nm, Ln, C, dt, st))

    def a_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_cae_tokens_assemble_bwd(p(dq[j]), p(dk[j]), p(dv[j]), p(dxu[j]), p(dxm[j]), B, 1, Nu, Nm, C,
                                                      dt, st))

    def copy(nbytes):
        return lambda i: L.check(lib.passl_hip_copy_bytes(p(cb[i % nset]), p(ca[i % nset]), nbytes // 2, st))

    def m_fwd(i):
        j = i % nset
        L.check(lib.passl_hip_mse_fwd(p(xm[j]), p(tgt[j]), p(loss), B, Nm, 1, C, dt, p(ws), B * Nm, st))

    def m_bwd(i):
        j = i % nset
        L.check(lib.passl_hip_mse_bwd(p(xm[j]), p(tgt[j]), None, p(dxm[j]), B, Nm, 1, C, dt, st))

    def ids(i):
        ops.cae_mask_ids(mask_dev, Nu)
    mask_dev = mask.to(dev)
    variants = [('assemble fwd', a_fwd), ('copy_bytes (fwd bytes)', copy(fwd_bytes)), ('assemble bwd', a_bwd),
                ('copy_bytes (bwd bytes)', copy(bwd_bytes)), ('mse fwd', m_fwd), ('mse bwd', m_bwd), ('mask_ids', ids)]
    torch.cuda.synchronize()
    times = _measure(variants, args.launches, args.rounds)
    s = {n: _stats(ts) for n, ts in times.items()}
    lines.append('%s [%d] Nu = %d, Nm = %d, C = %d: assemble moves %.1f MB forward, %.1f MB backward; %d operand sets' % (
        name, B, Nu, Nm, C, fwd_bytes / 1e6, bwd_bytes / 1e6, nset))
    _rows(lines, variants, s)
    for d in ('fwd', 'bwd'):
        r = s['assemble ' + d][0] / s['copy_bytes (%s bytes)' % d][0]
        lines.append('  %s assemble %s / copy_bytes of its bytes = %.2f, expectation %.2f x %s' % (
            name, d, r, MARGIN, 'HELD' if r <= MARGIN else 'MISSED'))
    lines.append('  %s mse fwd %.1f us, bwd %.1f us for %.1f MB read (reported only)' % (
        name, s['mse fwd'][0] * 1e3, s['mse bwd'][0] * 1e3, 2 * B * Nm * row / 1e6))
    return {n: s[n][0] for n in ('assemble fwd', 'assemble bwd', 'mse fwd', 'mse bwd', 'mask_ids')}


def kernels(args):
    lines = ['%d rounds x %d launches per window, variants alternating; times are device-event windows / launches'
             % (args.rounds, args.launches)]
    ok, own = True, {}
    for dtype in (torch.bfloat16, torch.float32):
        good, t = attention(args, dtype, lines)
        ok = good and ok
        t.update(streaming(args, dtype, lines))
        own[dtype] = t
    if args.resources:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), 'cross_attention.hip',
                            'cae.hip'], capture_output=True, text=True)
        lines += ['', 'tools/kernel_resources.py cross_attention.hip cae.hip'] + \
            (r.stdout if r.returncode == 0 else r.stderr).splitlines()
    return lines, ok, own


def step(args):
    import passl.models as PM
    from passl_amd.engine.loops.cae_pretrain_loop import build_optimizer, forward_backward
    from passl_amd.hip import config as hip_config
    from passl_amd.hip.replay import StepPlan
    from passl_amd.models.cae import cae_pretrain_args
    from passl_amd.datasets.synthetic import SyntheticMaskedTokens
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    a = cae_pretrain_args()
    ds = SyntheticMaskedTokens(num_samples=B, seed=0)
    x, mask, labels = ds.per_iteration(tuple(t.to(dev) for t in ds.make_batch(torch.Generator().manual_seed(0), B)))
    lines = ['bf16, batch %d, cae_base_patch16_224_8k_vocab with pretrain.sh\'s values: forward, CE + %g x MSE, backward, '
             'AdamW in two groups with clip %g; %d rounds x %d steps per window, alternating'
             % (B, a.dual_loss_weight, a.clip_grad, args.rounds, args.steps),
             '%-34s %9s %9s %9s' % ('step', 'mean ms', 'min ms', 'max ms')]
    runs = {}
    for mode in ('eager', 'replayed from a strict plan'):
        torch.manual_seed(0)
        model = PM.build_model(dict(name='cae_base_patch16_224_8k_vocab', args=a)).train()
        opt, sched = build_optimizer(model, a, 1000)
        sched.step(5000)                                   # a rate inside the warm-up: every update moves something

        def full_step(x, mask, labels, model=model, opt=opt):
            opt.clear_grad()
            lm, mse = forward_backward(model, x, mask, labels, ds.num_masked, a.dual_loss_weight)
            opt.step()
            return dict(loss_main=lm, mse=mse)
        sp = StepPlan(full_step, optimizers=[opt], warmup=1, enabled=(mode != 'eager'), strict=True)
        runs[mode] = (lambda _i, sp=sp: sp.run(x, mask, labels), sp)
    times = _measure([(m, f) for m, (f, _sp) in runs.items()], args.steps, args.rounds)
    stats = {m: _stats(times[m]) for m in runs}
    for m in runs:
        lines.append('%-34s %9.3f %9.3f %9.3f' % ((m,) + stats[m]))
    sp = runs['replayed from a strict plan'][1]
    lines.append('plan: %s; failed %s, foreign %s' % (sp.info, sp.failed, sp.foreign))
    del runs
    torch.cuda.empty_cache()
    _l, _ok, own = kernels(argparse.Namespace(batch=B, rounds=3, launches=args.launches, resources=False))
    t = own[torch.bfloat16]
    n_reg, per = a.regressor_depth, stats['replayed from a strict plan'][0]
    new = n_reg * (t['cross fwd'] + t['cross bwd'] + t['assemble fwd'] + t['assemble bwd']) + t['assemble fwd'] + \
        t['mse fwd'] + t['mse bwd'] + t['mask_ids']
    lines.append('new kernels, their own time on the step\'s shapes x launches per step (%d cross-attention and assemble '
                 'pairs, the decoder\'s position add, mse pair, mask ids): %.3f ms = %.1f %% of the replayed step; inside '
                 'the step: NOT MEASURED' % (n_reg, new, 100 * new / per))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--resources', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cae_bench: needs an MI355X (a CPU run says nothing about time)')
    if args.mode == 'kernels':
        lines, ok, _own = kernels(args)
    else:
        lines, ok = step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
