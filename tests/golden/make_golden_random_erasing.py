"""Generate tests/golden/random_erasing_boxes.npz by EXECUTING THE REFERENCE's own file under the paddle shim
(oracle/ref_runner.py): class RandomErasing, passl_v110/datasets/preprocess/random_erasing.py.

    python tests/golden/make_golden_random_erasing.py

For every case of tests/random_erasing_util.py:CASES — random.seed, (B, H, W), the class's arguments — the reference's
RandomErasing(mode='const', **arguments) is called sample by sample on arrays of ones [3, H, W]; stored is the bounding
box (top, left, h, w) of the zeroed region per sample, all zeros when nothing was erased, plus the number of erased
samples and of rejected attempts (counted through random.uniform / random.randint).  For seed 3 a second consecutive
call is recorded too: the stream continues.  Nothing is written when a case erases fewer than 8 samples, when the
(24, 40) case has no box with h != w (an axis swap would hide), or when the counts differ from the table in CASES."""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import random_erasing_util as RU                   # noqa: E402
from oracle import ref_runner                      # noqa: E402


def _load_file(name, *rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_runner.REF_ROOT, *rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Counter:
    """Counts the calls of random.uniform and random.randint while it is installed."""

    def __enter__(self):
        self.uniform = self.randint = 0
        self._u, self._r = random.uniform, random.randint

        def uniform(*a):
            self.uniform += 1
            return self._u(*a)

        def randint(*a):
            self.randint += 1
            return self._r(*a)
        random.uniform, random.randint = uniform, randint
        return self

    def __exit__(self, *exc):
        random.uniform, random.randint = self._u, self._r


def run_batch(fn, B, H, W):
    y = np.ones((B, 3, H, W), dtype=np.float32)
    for b in range(B):
        fn(y[b])                                    # a 3-D input: _erase writes into it
    return RU.bounding_boxes(y)


def main():
    ref_runner.load()
    mod = _load_file('_ref_random_erasing', 'passl_v110', 'datasets', 'preprocess', 'random_erasing.py')
    out = {}
    for seed, (B, H, W), kw, want_erased, want_rejected in RU.CASES:
        random.seed(seed)
        fn = mod.RandomErasing(mode='const', **kw)
        with Counter() as c:
            t = run_batch(fn, B, H, W)
        erased = int((t[:, 2] > 0).sum())
        draws_count = 0 if fn.min_count == fn.max_count else B       # (prob 1 in the only such case)
        placed = (c.randint - draws_count) // 2
        rejected = c.uniform // 2 - placed
        print('seed %d  %s  %s: erased %d, rejected attempts %d' % (seed, (B, H, W), kw, erased, rejected))
        assert erased >= 8, 'fewer than 8 erased samples'
        assert placed == erased
        assert (erased, rejected) == (want_erased, want_rejected), (erased, rejected)
        if (H, W) == (24, 40):
            assert (t[:, 2] != t[:, 3]).any(), 'no box with h != w'
        out['boxes_%d' % seed] = t
        out['counts_%d' % seed] = np.array([erased, rejected], dtype=np.int64)
        if seed == RU.SECOND_CALL_SEED:
            t2 = run_batch(fn, B, H, W)
            assert (t2[:, 2] > 0).sum() >= 8 and not np.array_equal(t, t2)
            out['boxes_%d_second' % seed] = t2
            print('         second call: erased %d' % int((t2[:, 2] > 0).sum()))
    path = os.path.join(HERE, 'random_erasing_boxes.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 64 * 1024
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    assert ref_runner.available(), 'needs the reference tree'
    main()
