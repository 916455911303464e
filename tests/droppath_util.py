"""A numpy restatement of the stochastic-depth draw (include/passl_hip.h: passl_hip_drop_path_draw), shared by
tests/test_droppath_host.py (known-answer vectors, no GPU) and tests/test_droppath_gpu.py (the kernel, bit for bit)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl constants: the key schedule
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 -> the 4 output words as uint64 arrays holding 32 bits."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)           # 32 x 32 -> 64 bits: exact in uint64
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def keep_table(keep_prob, B, seed, step):
    """[slots, B] float32 of 0 / 1: counter (b, slot, step_lo, step_hi), key (seed_lo, seed_hi),
    u = float(x0 >> 8) * 2^-24, keep = keep_prob[slot] + u >= 1 with the sum rounded to float32."""
    keep_prob = np.asarray(keep_prob, dtype=np.float32)
    slots = keep_prob.shape[0]
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    b, slot = np.meshgrid(np.arange(B), np.arange(slots))
    x0 = philox4x32_10((b, slot, np.full_like(b, step & MASK), np.full_like(b, step >> 32)),
                       (seed & MASK, seed >> 32))[0]
    u = (x0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    s = (keep_prob[:, None] + u).astype(np.float32)
    return (s >= np.float32(1.0)).astype(np.float32)


# the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def check_known_answers():
    for counter, key, want in KAT:
        got = tuple(int(v) for v in philox4x32_10(counter, key))
        assert got == want, ('Philox4x32-10', [hex(v) for v in got], [hex(v) for v in want])
