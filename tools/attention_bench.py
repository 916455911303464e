"""A/B of two builds of the fused attention kernels (csrc/attention_core.h and its two policies) on the MI355X: are the
results the same bits, and is either build slower?  A library is loaded from the path given, one library per process.

    python tools/attention_bench.py --bits --lib LIB.so --out A.pt      every case x path -> raw bits of out, lse, dqkv
    python tools/attention_bench.py --compare A.pt B.pt                 lists each case / path / tensor that differs
    python tools/attention_bench.py --time --lib LIB.so                 one JSON line: us per launch, every workload shape
    python tools/attention_bench.py --ab PARENT.so NEW.so [--reps 5] [--out profiles/x.txt]

--bits: every case of tests/attention_util.CASES through the C ABI, forward then backward, on the paths of
tests/test_attention_numerics_gpu.py: fp32 | bf16 default | bf16 attn_waves=4 | attn_waves=8 | attn_f32mfma=1 | bf16
default options with every operand 2 bytes off 16-byte alignment.  Outputs are NaN before the call.

--time: forward and backward (both sweeps) of the five workload shapes of profiles/r03_attn.txt in bf16 and fp32, default
options.  Device events around one window of back-to-back launches per figure; the window is sized from a warm-up window
to last about --window seconds.

--ab: the driver of one GPU visit.  It opens no GPU itself; it starts one child at a time, each under its own time limit:
--bits of either library and the comparison, then --time alternating PARENT, NEW, PARENT, ... --reps times each.  A child
that fails or runs out of time ends the run (nothing more is started).  The table gives, per shape, dtype and direction,
the median of either build and the parent's own spread, (max - min) / median over its repetitions; exit status 1 if a
tensor differs or a median of NEW exceeds the parent's by more than that spread.  attn_waves = 4 / 8 A/Bs of one build:
PASSL_OPTIONS does not reach a library loaded by path, use --waves."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# name, B, T, H, DH, causal (profiles/r03_attn.txt)
SHAPES = (('clip16 vision', 256, 197, 12, 64, False), ('clip text', 256, 77, 8, 64, True),
          ('mae encoder', 256, 50, 12, 64, False), ('mae decoder', 256, 197, 16, 32, False),
          ('clip32 vision', 128, 50, 12, 64, False))
# name, dtype, options, elements off alignment
PATHS = (('fp32', 'float32', {}, 0), ('bf16', 'bfloat16', {}, 0), ('bf16-waves4', 'bfloat16', {'attn_waves': 4}, 0),
         ('bf16-waves8', 'bfloat16', {'attn_waves': 8}, 0), ('bf16-f32mfma', 'bfloat16', {'attn_f32mfma': 1}, 0),
         ('bf16-unaligned', 'bfloat16', {}, 1))
BITS_LIMIT, TIME_LIMIT = 600, 300        # seconds per child


class Lib:
    """One library by path; options go to that library's own table."""

    def __init__(self, path):
        from passl_amd.hip import lib as L
        self.L, self.lib = L, L.load(os.path.abspath(path))

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError('%s failed: %s (status %d)' % (what, self.lib.passl_hip_strerror(rc).decode(), rc))

    def options(self, **opts):
        for name in ('attn_waves', 'attn_f32mfma'):
            self.check(self.lib.passl_hip_set_option(name.encode(), int(opts.get(name, 0))), 'set_option ' + name)

    def fwd(self, qkv, out, lse, B, T, H, DH, causal):
        L = self.L
        self.check(self.lib.passl_hip_attention_fwd(L.ptr(qkv), L.ptr(out), L.ptr(lse), B, T, H, DH, DH ** -0.5,
                                                    int(causal), L.dt(qkv), L.stream()), 'attention_fwd')

    def bwd(self, qkv, out, dout, lse, dqkv, B, T, H, DH, causal):
        L = self.L
        self.check(self.lib.passl_hip_attention_bwd(L.ptr(qkv), L.ptr(out), L.ptr(dout), L.ptr(lse), L.ptr(dqkv), B, T, H,
                                                    DH, DH ** -0.5, int(causal), L.dt(qkv), L.stream()), 'attention_bwd')


def _skewed(numel, dtype, skew, fill=None):
    """`numel` elements `skew` elements past a 16-byte boundary: NaN, or a copy of `fill`."""
    import torch
    buf = torch.empty(numel + 8, dtype=dtype, device='cuda')
    v = buf[skew:skew + numel]
    if fill is None:
        v.fill_(float('nan'))
    else:
        v.copy_(fill.flatten().to('cuda').to(dtype))
    return v


def bits(args):
    import torch
    import attention_util as A
    lib = Lib(args.lib)
    res = {}
    for case in A.CASES:
        DH, T, causal, _ = case
        d = A.case_data(case)
        for path, dtype, opts, skew in PATHS:
            dtype = getattr(torch, dtype)
            lib.options(**opts)
            qkv = _skewed(A.B * T * 3 * A.H * DH, dtype, skew, d['qkv'])
            dout = _skewed(A.B * T * A.H * DH, dtype, skew, d['dout'])
            out, lse = _skewed(A.B * T * A.H * DH, dtype, skew), _skewed(A.B * A.H * T, torch.float32, skew)
            dqkv = _skewed(A.B * T * 3 * A.H * DH, dtype, skew)
            lib.fwd(qkv, out, lse, A.B, T, A.H, DH, causal)
            lib.bwd(qkv, out, dout, lse, dqkv, A.B, T, A.H, DH, causal)
            torch.cuda.synchronize()
            for name, t in (('out', out), ('lse', lse), ('dqkv', dqkv)):
                res['%s %s %s' % (A.case_id(case), path, name)] = t.view(
                    torch.int16 if t.element_size() == 2 else torch.int32).cpu().clone()
    lib.options()
    torch.save(res, args.out)
    print('%d tensors (%d cases x %d paths x out, lse, dqkv) -> %s' % (len(res), len(A.CASES), len(PATHS), args.out))
    return 0


def compare(args):
    import torch
    a, b = torch.load(args.compare[0]), torch.load(args.compare[1])
    bad = [k for k in a if k not in b or not torch.equal(a[k], b[k])] + [k for k in b if k not in a]
    for k in bad:
        n = int((a[k] != b[k]).sum()) if k in a and k in b and a[k].shape == b[k].shape else -1
        print('DIFFERENT %s (%d of %d elements)' % (k, n, a[k].numel() if k in a else 0))
    print('%d tensors compared (case, path, tensor): %s' % (len(a), 'all bit-equal' if not bad else '%d differ' % len(bad)))
    return 1 if bad else 0


def _window(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n * 1e3            # us per call


def time_one(args):
    import torch
    lib = Lib(args.lib)
    lib.options(attn_waves=args.waves)
    res = {}
    for name, B, T, H, DH, causal in SHAPES:
        for dname in ('bfloat16', 'float32'):
            dtype = getattr(torch, dname)
            gen = torch.Generator(device='cuda').manual_seed(T * H + DH)
            qkv = torch.randn(B * T, 3 * H * DH, device='cuda', generator=gen).to(dtype)
            dout = torch.randn(B * T, H * DH, device='cuda', generator=gen).to(dtype)
            out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
            lse = torch.empty(B * H * T, device='cuda')
            runs = (('fwd', lambda: lib.fwd(qkv, out, lse, B, T, H, DH, causal)),
                    ('bwd', lambda: lib.bwd(qkv, out, dout, lse, dqkv, B, T, H, DH, causal)))
            for direction, fn in runs:           # the forward first: the backward reads its out and lse
                est = _window(fn, 20)            # warm-up: code object, clocks
                n = max(20, int(args.window * 1e6 / est))
                res['%s|%s|%s' % (name, dname, direction)] = _window(fn, n)
    print(json.dumps(res))
    return 0


def _child(argv, limit):
    """One process on the GPU, under its own time limit; a failure or a time-out ends the whole run."""
    print('attention_bench: %s' % ' '.join(argv), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stdout.write(r.stdout + r.stderr)
        raise SystemExit('attention_bench: `%s` ended with status %d; nothing more is started' % (' '.join(argv), r.returncode))
    return r.stdout


def ab(args):
    parent, new = args.ab
    lines = ['parent %s, new %s' % (parent, new), '']
    tmp = args.tmp or tempfile.mkdtemp(prefix='attention_bench_')
    os.makedirs(tmp, exist_ok=True)
    fa, fb = os.path.join(tmp, 'bits_parent.pt'), os.path.join(tmp, 'bits_new.pt')
    lines.append('bits, parent: ' + _child(['--bits', '--lib', parent, '--out', fa], BITS_LIMIT).split(' -> ')[0])
    lines.append('bits, new:    ' + _child(['--bits', '--lib', new, '--out', fb], BITS_LIMIT).split(' -> ')[0])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--compare', fa, fb], capture_output=True, text=True)
    lines += r.stdout.strip().split('\n')
    ok = r.returncode == 0
    times = {parent: [], new: []}
    for _ in range(args.reps):
        for lib in (parent, new):                # alternating: drift hits both alike
            out = _child(['--time', '--lib', lib, '--window', str(args.window)], TIME_LIMIT)
            times[lib].append(json.loads(out.strip().split('\n')[-1]))
    lines += ['', 'us per launch (bwd = dQ sweep + dK / dV sweep), %d repetitions each, one process per repetition, alternating; '
              'windows of about %.2f s' % (args.reps, args.window),
              '%-14s %-19s %-8s %-4s %11s %11s %8s %9s  %s' % ('shape', 'B, T, H, d', 'dtype', 'dir', 'parent med', 'new med',
                                                              'new/par', 'par spread', '')]
    for name, B, T, H, DH, causal in SHAPES:
        for dname in ('bfloat16', 'float32'):
            for direction in ('fwd', 'bwd'):
                k = '%s|%s|%s' % (name, dname, direction)
                tp, tn = [t[k] for t in times[parent]], [t[k] for t in times[new]]
                mp, mn = statistics.median(tp), statistics.median(tn)
                spread = (max(tp) - min(tp)) / mp
                good = mn <= mp * (1 + spread)
                ok = ok and good
                lines.append('%-14s %-19s %-8s %-4s %11.2f %11.2f %8.4f %8.2f %%  %s' % (
                    name, '%d, %d, %d, %d%s' % (B, T, H, DH, ' causal' if causal else ''), dname, direction, mp, mn, mn / mp,
                    100 * spread, 'ok' if good else 'SLOWER'))
    lines.append('every tensor bit-equal and no median of the new build beyond the parent\'s spread: %s' % ('yes' if ok else 'NO'))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--bits', action='store_true')
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--compare', nargs=2, metavar='FILE')
    ap.add_argument('--ab', nargs=2, metavar='LIB')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.4)
    ap.add_argument('--waves', type=int, default=0, choices=(0, 4, 8))
    ap.add_argument('--tmp', default=None, help='where --ab keeps the two --bits files (default: a temporary directory)')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args))
    if args.ab:
        sys.exit(ab(args))
    if not (args.bits or args.time) or not args.lib or (args.bits and not args.out):
        ap.error('one of --bits --lib L --out F | --compare A B | --time --lib L | --ab PARENT NEW')
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('attention_bench: needs an MI355X (a CPU run says nothing about bits or time)')
    sys.exit(bits(args) if args.bits else time_one(args))


if __name__ == '__main__':
    main()
