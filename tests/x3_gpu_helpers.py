"""Shared pieces of the f16x3 operator tests on the GPU (tests/test_x3_ops_gpu.py, tests/test_train_x3_ops_gpu.py):
sentinel-guarded plane allocations, plane upload, pointers and the path report's rendering."""
import ctypes as C
import zlib

import torch

SENTINEL = 0x7DC1          # an fp16 signalling-NaN pattern: marks halfs a kernel must not write / has not written
WS, R512, T448 = 1, 2, 3
ERR_INVALID_ARG, ERR_HIP = 1, 4


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) % 100003


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    """host float32 tensor -> pointer (the tensor must stay alive for the call)"""
    return C.c_void_p(a.data_ptr()) if a is not None else None


# ---- planes with guards -------------------------------------------------------------------------------------------

class Planes:
    """hi / lo planes (n,h,w,ld) inside one sentinel-filled allocation: [guard | hi | guard | lo | guard], the guard at
    least one image row"""

    def __init__(self, n, h, w, ld):
        self.shape = (n, h, w, ld)
        self.elems = n * h * w * ld
        self.guard = (max(w * ld, 64) + 63) // 64 * 64
        self.buf = torch.full((3 * self.guard + 2 * self.elems,), SENTINEL, dtype=torch.int16, device="cuda")
        self.lo_off = self.elems + self.guard

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 2 * self.guard)

    def _plane(self, k):
        o = self.guard + k * self.lo_off
        return self.buf[o:o + self.elems].view(self.shape)

    def bits(self, c0=0, c1=None):
        """(hi, lo) int16 views of channels [c0, c1)"""
        return self._plane(0)[..., c0:c1], self._plane(1)[..., c0:c1]

    def halves(self, c0=0, c1=None):
        hi, lo = self.bits(c0, c1)
        return hi.contiguous().view(torch.float16).cpu(), lo.contiguous().view(torch.float16).cpu()

    def assert_written_only(self, c0, c1, label):
        """every half of channels [c0, c1) written, every other half of the allocation still the sentinel"""
        hi, lo = self.bits(c0, c1)
        assert not (hi == SENTINEL).any() and not (lo == SENTINEL).any(), f"{label}: output elements not written"
        g, e = self.guard, self.elems
        for name, a, b in (("before hi", 0, g), ("between the planes", g + e, 2 * g + e), ("after lo", 2 * g + 2 * e, 3 * g + 2 * e)):
            assert (self.buf[a:b] == SENTINEL).all(), f"{label}: guard {name} overwritten"
        for k in (0, 1):
            pl = self._plane(k)
            assert (pl[..., :c0] == SENTINEL).all() and (pl[..., c1:] == SENTINEL).all(), \
                f"{label}: channels outside [{c0}, {c1}) overwritten"


def to_dev(hi, lo):
    """fp16 planes (CPU) -> one device tensor [hi | lo], its pointer and the lo offset in elements"""
    x = torch.stack([hi, lo]).contiguous().cuda()
    return x, x[0].numel()


def path_str(p):
    names = {0: "none", WS: "ws", R512: "r512", T448: "t448"}
    return (f"{names.get(p[0], p[0])} tw{p[1]} epi{p[2]}{' flat' if p[3] else ''} kSplit{p[4]} waves{p[5]}"
            f"{' +pool pass' if p[6] else ''}")


class GuardedF32:
    """an fp32 tensor of `shape` inside one allocation filled with a NaN pattern no kernel produces: a guard of at least
    one image row before and behind it"""
    PATTERN = 0x7FC12345

    def __init__(self, *shape):
        self.shape = tuple(shape)
        self.elems = 1
        for d in shape:
            self.elems *= d
        row = self.elems // (shape[0] * shape[1]) if len(shape) > 2 else 64
        self.guard = (max(row, 64) + 63) // 64 * 64
        self.buf = torch.full((2 * self.guard + self.elems,), self.PATTERN, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.guard)

    def bits(self):
        return self.buf[self.guard:self.guard + self.elems].view(self.shape)

    def values(self):
        return self.bits().view(torch.float32)

    def assert_written_only(self, label, c0=0, c1=None):
        """every element of the last dimension's range [c0, c1) written, everything else still the pattern"""
        b = self.bits()
        assert not (b[..., c0:c1] == self.PATTERN).any(), f"{label}: output elements not written"
        g, e = self.guard, self.elems
        assert (self.buf[:g] == self.PATTERN).all() and (self.buf[g + e:] == self.PATTERN).all(), f"{label}: guard overwritten"
        if c0 or (c1 is not None and c1 < self.shape[-1]):
            assert (b[..., :c0] == self.PATTERN).all() and (b[..., c1:] == self.PATTERN).all(), \
                f"{label}: elements outside [{c0}, {c1}) overwritten"

    def assert_untouched(self, label):
        assert (self.buf == self.PATTERN).all(), f"{label}: buffer written"
