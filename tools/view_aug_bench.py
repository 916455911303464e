"""What the two-view colour pipeline costs on the MI355X (DESIGN.md "Colour jitter, grayscale, blur, solarise"): every
launch of a view stand-alone, and a whole MoCo-v3 step with and without the pipelines in front of it.

    python tools/view_aug_bench.py kernels [--out profiles/view_aug_kernels.txt]
    python tools/view_aug_bench.py step    [--out profiles/view_aug_step.txt]

kernels: batch 128, uint8 256 x 256 -> 224 x 224, the tables drawn by view 1 of
configs/v2/mocov3_vit_base_pt_views_synthetic.yaml (ColorJitter 0.8, RandomGrayscale 0.2, SimCLRGaussianBlur 1.0).  Each
launch — crop_resize_u8, view_gray_sum, view_pointwise to uint8 (part 1), gaussian_blur_u8, view_pointwise to fp32 (part 2
behind the blur, and part 0 = the whole list, as a view without a blur runs it) — alternates, window by window in one
process, with passl_hip_copy_bytes moving the bytes that launch reads plus writes (half of them read, half written).
Device events around WINDOWS of back-to-back launches, operands rotating over four sets.  Bound set before measuring,
as for mixup and random erasing: the two streaming pointwise launches within 1.25 x their copy.  No bound for the crop,
the gray sum and the blur: the ratio is printed, nothing is judged.

step: mocov3_vit_base_pretrain at batch 128 bf16, eager steps, on a resident fp32 two-view batch (what the parent
commit trains on) and on a resident uint8 256 x 256 batch through the TwoViewsTransform of the YAML (host draws, two
table copies, the launches of both views), two models alive in one process, windows of steps alternating.  The spread of
the windows WITHOUT the pipeline is printed next to the difference."""
import argparse
import ctypes as C
import os
import random
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YAML = os.path.join(ROOT, 'configs', 'v2', 'mocov3_vit_base_pt_views_synthetic.yaml')
BOUND = 1.25


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


def _two_views(seed=0):
    from passl_amd.datasets.preprocess import build_two_views
    with open(YAML) as f:
        block = yaml.safe_load(f)['DataLoader']['Train']['dataset']
    two = build_two_views(block['transform'])
    rng, nrng = random.Random(seed), np.random.RandomState(seed)
    for v in (two.base_transform1, two.base_transform2):
        v.crop.rng, v.crop.np_rng, v.flip.np_rng = rng, nrng, nrng
        for t in v.ops:
            if hasattr(t, 'rng'):
                t.rng = rng
            if hasattr(t, 'np_rng'):
                t.np_rng = nrng
    return two


def _source(B, dev, seed=0):
    from passl_amd.datasets.synthetic import SyntheticRawTwoView
    ds = SyntheticRawTwoView(num_samples=B, source_h=256, source_w=256, image_size=224)
    return ds.make_batch(torch.Generator().manual_seed(seed), B)[0].to(dev)


def kernels(args):
    from passl_amd.hip import lib as L
    lib = L.load()
    B, Hs, Ws, S = args.batch, 256, 256, 224
    nset = 4
    dev = torch.device('cuda')
    view = _two_views().base_transform1
    samples = [view.draw_sample(Hs, Ws) for _ in range(B)]
    crop_t, table = view.encode(samples)
    view.validate(table)
    r_max = int(table[:, 2].max())
    tc, tt = torch.from_numpy(crop_t).to(dev), torch.from_numpy(table).to(dev)
    n = view.normalize
    kp = C.cast((C.c_float * 7)(*n.mean, *n.std, n.scale), C.c_void_p)
    srcs = [_source(B, dev, i) for i in range(nset)]
    u8a = [torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev) for _ in range(nset)]
    u8b = [torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev) for _ in range(nset)]
    f32 = [torch.empty(B, 3, S, S, device=dev) for _ in range(nset)]
    sums = torch.empty(B, dtype=torch.int64, device=dev)
    big = max(B * Hs * Ws * 3 + B * S * S * 3, B * S * S * 3 * 5)
    ca = [torch.empty(big // 2 + 16, dtype=torch.uint8, device=dev) for _ in range(nset)]
    cb = [torch.empty(big // 2 + 16, dtype=torch.uint8, device=dev) for _ in range(nset)]
    p, st = L.ptr, L.stream()
    for i in range(nset):                         # real images in every buffer a launch reads
        L.check(lib.passl_hip_crop_resize_u8(p(srcs[i]), p(u8a[i]), p(tc), B, Hs, Ws, S, st))
        L.check(lib.passl_hip_crop_resize_u8(p(srcs[i]), p(u8b[i]), p(tc), B, Hs, Ws, S, st))
    L.check(lib.passl_hip_view_gray_sum(p(u8a[0]), p(tt), p(sums), B, S, S, st))
    src_b, u8_b, f32_b = B * Hs * Ws * 3, B * S * S * 3, B * S * S * 3 * 4

    def copy_of(nbytes):
        half = (nbytes // 2 + 15) & ~15
        return lambda i: L.check(lib.passl_hip_copy_bytes(p(cb[i % nset]), p(ca[i % nset]), half, st))
    launches = [
        ('crop_resize_u8', src_b + u8_b, None,
         lambda i: L.check(lib.passl_hip_crop_resize_u8(p(srcs[i % nset]), p(u8a[i % nset]), p(tc), B, Hs, Ws, S, st))),
        ('view_gray_sum', u8_b, None,
         lambda i: L.check(lib.passl_hip_view_gray_sum(p(u8a[i % nset]), p(tt), p(sums), B, S, S, st))),
        ('view_pointwise part 1 -> uint8', 2 * u8_b, BOUND,
         lambda i: L.check(lib.passl_hip_view_pointwise(p(u8a[i % nset]), p(tt), p(sums), p(u8b[i % nset]), None, B, S, S, 1,
                                                        None, st))),
        ('gaussian_blur_u8', 2 * u8_b, None,
         lambda i: L.check(lib.passl_hip_gaussian_blur_u8(p(u8b[i % nset]), p(u8a[i % nset]), p(tt), B, S, S, r_max, st))),
        ('view_pointwise part 2 -> fp32', u8_b + f32_b, BOUND,
         lambda i: L.check(lib.passl_hip_view_pointwise(p(u8a[i % nset]), p(tt), None, None, p(f32[i % nset]), B, S, S, 2, kp,
                                                        st))),
        ('view_pointwise part 0 -> fp32', u8_b + f32_b, BOUND,
         lambda i: L.check(lib.passl_hip_view_pointwise(p(u8b[i % nset]), p(tt), p(sums), None, p(f32[i % nset]), B, S, S, 0,
                                                        kp, st))),
    ]
    n_ops = table[:, 0]
    lines = ['batch %d, uint8 %d x %d -> %d x %d; view 1 of the recipe: %.2f operations per sample on average (%d samples '
             'with none), %d with a contrast entry, %d gray, box radius 0 / 1 for %d / %d samples, %d flipped; %d rounds x %d '
             'launches per window, %d operand sets'
             % (B, Hs, Ws, S, S, float(n_ops.mean()), int((n_ops == 0).sum()), int((table[:, 6] >= 0).sum()),
                int((table[:, 8:16] == 5).any(axis=1).sum()), int((table[:, 2] == 0).sum()), int((table[:, 2] == 1).sum()),
                int(table[:, 1].sum()), args.rounds, args.launches, nset),
             '%-32s %8s %9s %9s %9s %9s %8s %7s' % ('launch', 'MB moved', 'mean us', 'min us', 'max us', 'copy us', 'ratio',
                                                   'bound')]
    ok = True
    for name, nbytes, bound, fn in launches:
        cp = copy_of(nbytes)
        _window(fn, args.launches)
        _window(cp, args.launches)
        tk, tcp = [], []
        for _ in range(args.rounds):              # alternating: drift hits both alike
            tk.append(_window(fn, args.launches))
            tcp.append(_window(cp, args.launches))
        m, lo, hi = _stats(tk)
        c = _stats(tcp)[0]
        verdict = '' if bound is None else ('%.2f %s' % (bound, 'ok' if m / c <= bound else 'MISSED'))
        ok = ok and (bound is None or m / c <= bound)
        lines.append('%-32s %8.1f %9.2f %9.2f %9.2f %9.2f %8.3f %7s' % (name, nbytes / 1e6, m * 1e3, lo * 1e3, hi * 1e3,
                                                                      c * 1e3, m / c, verdict))
    return lines, ok


def step(args):
    from passl_amd.hip import config as hip_config
    from passl_amd.models.mocov3 import mocov3_vit_base_pretrain
    from passl_amd.solver.optimizer import AdamW
    from passl_amd.utils.infohub import runtime_info_hub
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    runtime_info_hub.max_steps = 100000
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    xq = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    xk = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    src = _source(B, dev)
    runs = {}
    for name, two in (('resident fp32 two-view batch', None), ('uint8 256 x 256 through both views', _two_views())):
        torch.manual_seed(0)
        model = mocov3_vit_base_pretrain()
        model.train()
        opt = AdamW(1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, parameters=list(model.parameters()))

        def one(_i, model=model, opt=opt, two=two):
            views = (xq, xk) if two is None else two(src)     # what the loader does before it yields the batch
            loss = model(list(views))
            opt.clear_grad()
            loss.backward()
            opt.step()
        runs[name] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['mocov3_vit_base_pretrain (ViT-B/16), batch %d, bf16, eager steps; %d rounds x %d steps per window, alternating'
             % (B, args.rounds, args.steps), '%-38s %9s %9s %9s' % ('', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-38s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    (m0, lo0, hi0), (m1, _lo1, _hi1) = [_stats(times[r]) for r in runs]
    lines.append('difference %.3f ms per step (%+.2f %%; spread of the windows without it %.2f %%): the host draws of 2 x %d '
                 'samples, two table copies and the launches of both views' % (m1 - m0, 100 * (m1 / m0 - 1),
                                                                              100 * (hi0 - lo0) / m0, B))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('view_aug_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
