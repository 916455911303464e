"""What the device-side crop pipeline costs on the MI355X (DESIGN.md "Random resized crop"): the stand-alone launch of
csrc/crop_resize.hip, and a whole fine-tuning step with and without the pipeline in front of it.

    python tools/crop_resize_bench.py kernels [--out profiles/crop_resize_kernels.txt]
    python tools/crop_resize_bench.py step    [--out profiles/crop_resize_step.txt]

kernels: passl_hip_crop_resize_norm on uint8 [128, 256, 256, 3] -> fp32 [128, 3, 224, 224] (25 MB read, 77 MB written),
the table drawn by MAERandCropImage(224) + RandomHorizontalFlip as the recipe draws it, next to passl_hip_copy_bytes of
the 77 MB the launch writes.  Device events around WINDOWS of back-to-back launches, the variants alternating inside one
process, the operands rotating over more buffers than the last-level cache holds.  No bound was set before measuring:
the ratio is printed, nothing is judged.

step: the model of configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml at batch 128 bf16 on a resident fp32 batch (what
every commit before this one trains on), and on a resident uint8 256 x 256 batch through the pipeline (host draws, the
4 KB table copy, one launch), two models alive in one process, windows of eager steps alternating.  The spread of the
windows WITHOUT the pipeline is printed next to the difference."""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRANSFORMS = [dict(name='MAERandCropImage', size=224, interpolation='bicubic', backend='pil'),
              dict(name='RandomHorizontalFlip'),
              dict(name='NormalizeImage', scale='1.0/255.0', mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225],
                   order='hwc'),
              dict(name='ToCHWImage')]


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


def _pipeline(seed=0):
    from passl_amd.datasets.preprocess import build_crop_pipeline
    fn = build_crop_pipeline([dict(t) for t in TRANSFORMS])
    fn.crop.rng, fn.crop.np_rng = random.Random(seed), np.random.RandomState(seed)
    fn.flip.np_rng = fn.crop.np_rng
    return fn


def _sources(B, n, dev):
    from passl_amd.datasets.synthetic import SyntheticRawLabeled
    ds = SyntheticRawLabeled(num_samples=B, source_h=256, source_w=256, image_size=224)
    gen = torch.Generator().manual_seed(0)
    return [tuple(t.to(dev) for t in ds.make_batch(gen, B)) for _ in range(n)]


def kernels(args):
    import ctypes as C
    from passl_amd.hip import lib as L
    lib = L.load()
    B, Hs, Ws, S = args.batch, 256, 256, 224
    nset = 4                                     # 4 x (25 + 77 MB), and 4 x 2 x 77 MB for the copy: past the 256 MB cache
    dev = torch.device('cuda')
    srcs = [s for s, _y in _sources(B, nset, dev)]
    outs = [torch.empty(B, 3, S, S, device=dev) for _ in range(nset)]
    twins = [torch.randn(B, 3, S, S, device=dev) for _ in range(nset)]
    fn = _pipeline()
    table = fn.draw(B, Hs, Ws)
    fn.validate(table, Hs, Ws)
    tdev = torch.from_numpy(table).to(dev)
    n = fn.normalize
    consts = (C.c_float * 7)(*n.mean, *n.std, n.scale)
    kp = C.cast(consts, C.c_void_p)
    out_bytes, src_bytes = B * 3 * S * S * 4, B * Hs * Ws * 3
    p, st = L.ptr, L.stream()

    def copy(i):
        L.check(lib.passl_hip_copy_bytes(p(outs[i % nset]), p(twins[i % nset]), out_bytes, st))

    def crop(i):
        L.check(lib.passl_hip_crop_resize_norm(p(srcs[i % nset]), p(outs[i % nset]), p(tdev), B, Hs, Ws, S, kp, st))
    variants = [('copy_bytes (77 MB)', copy, 2 * out_bytes), ('crop_resize_norm', crop, src_bytes + out_bytes)]
    times = {v[0]: [] for v in variants}
    for _n, f, _b in variants:                     # warm-up: code objects, clocks
        _window(f, args.launches)
    for _ in range(args.rounds):
        for name, f, _b in variants:               # alternating: drift hits every variant alike
            times[name].append(_window(f, args.launches))
    area = float((table[:, 2].astype(np.int64) * table[:, 3]).mean()) / (Hs * Ws)
    lines = ['uint8 [%d, %d, %d, 3] -> fp32 [%d, 3, %d, %d]: %.1f MB source, %.1f MB written; mean crop %.1f %% of the source, '
             '%d of %d flipped; %d rounds x %d launches per window, %d operand sets'
             % (B, Hs, Ws, B, S, S, src_bytes / 1e6, out_bytes / 1e6, 100 * area, int(table[:, 4].sum()), B, args.rounds,
                args.launches, nset),
             '%-24s %9s %9s %9s %10s' % ('launch', 'mean us', 'min us', 'max us', 'GB/s (mean)')]
    for name, _f, nb in variants:
        m, lo, hi = _stats(times[name])
        lines.append('%-24s %9.2f %9.2f %9.2f %10.0f' % (name, m * 1e3, lo * 1e3, hi * 1e3, nb / (m * 1e-3) / 1e9))
    cm, km = _stats(times['copy_bytes (77 MB)'])[0], _stats(times['crop_resize_norm'])[0]
    lines.append('crop_resize_norm / copy_bytes = %.3f (no bound was set)' % (km / cm))
    return lines, True


def step(args):
    from passl_amd.hip import config as hip_config
    from passl_amd.modeling import build_model
    from passl_amd.solver.optimizer import AdamW
    from passl_amd.utils.config import get_config
    cfg = get_config(os.path.join(ROOT, 'configs/mae/mae_vit_b_finetune_recipe_synthetic.yaml'), [])
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(torch.bfloat16)
    dev = torch.device('cuda')
    B = args.batch
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, 224, 224, generator=gen).to(dev)
    (src, y), = _sources(B, 1, dev)
    runs = {}
    for name, pipe in (('resident fp32 batch, no pipeline', None), ('uint8 256 x 256 through the pipeline', _pipeline())):
        torch.manual_seed(0)
        mc = dict(cfg.model)
        mc['architecture'] = dict(cfg.model.architecture)
        mc['head'] = dict(cfg.model.head)
        model = build_model(mc)
        model.train()
        opt = AdamW(1e-3, beta1=0.9, beta2=0.999, weight_decay=0.05, parameters=list(model.parameters()))

        def one(_i, model=model, opt=opt, pipe=pipe):
            xb = x if pipe is None else pipe(src)            # what the loader does before it yields the batch
            out = model(xb, y, mode='train')
            opt.clear_grad()
            out['loss'].backward()
            opt.step()
        runs[name] = one
    times = {r: [] for r in runs}
    for r, f in runs.items():
        _window(f, args.steps)
    for _ in range(args.rounds):
        for r, f in runs.items():
            times[r].append(_window(f, args.steps))
    lines = ['MAE_FINETUNE ViT-B/16, drop_path_rate 0.1, batch %d, bf16, eager steps; %d rounds x %d steps per window, '
             'alternating' % (B, args.rounds, args.steps), '%-38s %9s %9s %9s' % ('', 'mean ms', 'min ms', 'max ms')]
    for r in runs:
        m, lo, hi = _stats(times[r])
        lines.append('%-38s %9.3f %9.3f %9.3f' % (r, m, lo, hi))
    (m0, lo0, hi0), (m1, _lo1, _hi1) = [_stats(times[r]) for r in runs]
    lines.append('difference %.3f ms per step (%+.2f %%; spread of the windows without it %.2f %%): the host draws of %d '
                 'samples, the 4 KB table copy and one crop_resize_norm launch' % (m1 - m0, 100 * (m1 / m0 - 1),
                                                                                  100 * (hi0 - lo0) / m0, B))
    return lines, True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('crop_resize_bench: needs an MI355X (a CPU run says nothing about time)')
    lines, ok = kernels(args) if args.mode == 'kernels' else step(args)
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
