"""Device buffers between guard regions, shared by the tests that call kernels through the C ABI.

A kernel that stores past the end of a fresh torch tensor corrupts whatever the caching allocator placed next to it,
silently.  A `Guarded` payload lies inside a larger buffer whose margins hold a fixed bit pattern: `intact()` says
whether both margins survived, and the payload starts out as NaN (floating types) or 0xA5 bytes (`prefill='a5'`,
always for integer types), so that an element a kernel never wrote can be told from one it did.
"""
import torch

DEV = 'cuda'
GUARD_BYTES = 4096
PATTERN = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
PREFILL = {1: 0xA5 - 256, 2: 0xA5A5 - (1 << 16), 4: 0xA5A5A5A5 - (1 << 32), 8: 0xA5A5A5A5A5A5A5A5 - (1 << 64)}
_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Guarded:
    """`numel` elements inside a larger device buffer, `skew` elements past a 16-byte boundary, with at least
    GUARD_BYTES of a fixed bit pattern on either side.  dtype: bfloat16, float32, float64, uint8, int32 or
    int64 (labels, indices).  The payload holds `fill` when given, else NaN, else (integer types, or prefill='a5')
    bytes of 0xA5."""

    def __init__(self, numel, dtype, skew=0, fill=None, prefill=None):
        size = torch.empty(0, dtype=dtype).element_size()
        g = GUARD_BYTES // size
        self.lo, self.hi, self.pattern = g + skew, g + skew + numel, PATTERN[size]
        self.buf = torch.empty(self.hi + g, dtype=dtype, device=DEV)
        self.bits = self.buf.view(_BITS[size])
        self.bits.fill_(self.pattern)
        self.view = self.buf[self.lo:self.hi]
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (skew * size) % 16
        self.a5 = PREFILL[size] if (prefill == 'a5' or not dtype.is_floating_point) else None
        self.fill = None if fill is None else fill.flatten().to(DEV).to(dtype)
        self.reset()

    def reset(self):
        """The payload as it was before any launch."""
        if self.fill is not None:
            self.view.copy_(self.fill)
        elif self.a5 is not None:
            self.bits[self.lo:self.hi].fill_(self.a5)
        else:
            self.view.fill_(float('nan'))

    def intact(self):
        return bool((self.bits[:self.lo] == self.pattern).all()) and bool((self.bits[self.hi:] == self.pattern).all())

    def raw(self):
        return self.bits[self.lo:self.hi].clone()

    def unwritten(self, numel=None):
        """Number of payload elements (of the first `numel`) that still hold the prefill (NaN or 0xA5 bytes)."""
        hi = self.hi if numel is None else self.lo + numel
        if self.a5 is not None:
            return int((self.bits[self.lo:hi] == self.a5).sum())
        return int((~torch.isfinite(self.buf[self.lo:hi])).sum())
