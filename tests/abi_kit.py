"""Raw C-ABI plumbing shared by the tests: pointers and streams as ctypes arguments, bit equality, guarded buffers, MacxOpts.
Depends on ctypes, torch and numpy only -- it imports neither the product nor the oracle, so a test of macx._lib never checks the
library with the library's own helper.  tests/test_abi_kit_host.py pins what these definitions promise."""
import contextlib
import ctypes as C

import numpy as np
import torch

SENT = -7.03125e11            # what guard zones are filled with: far from any result of these tests (held as its fp32 rounding)
GUARD = 1024                  # elements in front of / behind a guarded buffer (a multiple of 4: keeps 16-byte alignment)

_INT = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}


def ptr(t):
    """device or host address of a tensor as a ctypes argument; None -> NULL"""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream(where):
    """torch's current stream on a device (or on a tensor's device) as a ctypes argument"""
    return C.c_void_p(torch.cuda.current_stream(where.device if isinstance(where, torch.Tensor) else where).cuda_stream)


def _int_view(t):
    return t.detach().contiguous().view(_INT[t.element_size()])


def bits(t):
    """detached, CPU, contiguous integer view of the same width"""
    return _int_view(t).cpu()


def bits_equal(a, b):
    """same shape, same dtype, same bits (torch.equal would take -0.0 for +0.0 and refuse equal NaNs); two tensors or two arrays"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype
                and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes())
    if a.device != b.device:
        a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_int_view(a), _int_view(b))


class Guarded:
    """n elements (.view) in the middle of a larger buffer (.buf) filled with `fill`"""

    def __init__(self, n, dev, dtype=torch.float32, fill=SENT, before=GUARD, after=GUARD):
        self.n, self.before = int(n), before
        self.buf = torch.full((before + self.n + after,), fill, dtype=dtype, device=dev)
        self.view = self.buf[before:before + self.n]
        assert self.view.data_ptr() % 16 == 0
        self._fill = int(bits(torch.full((1,), fill, dtype=dtype)))

    def _holds_fill(self, t):
        return bool((_int_view(t) == self._fill).all())

    def intact(self):
        """both bands hold `fill` bit for bit"""
        return self._holds_fill(self.buf[:self.before]) and self._holds_fill(self.buf[self.before + self.n:])

    def untouched(self):
        """the whole buffer holds `fill` bit for bit"""
        return self._holds_fill(self.buf)

    def np(self, *shape):
        return self.view.cpu().numpy().reshape(shape)


# ---- guard bands around whole torch.empty allocations (sized for that: `saved`, `ws`) ----------------------------------------
ALLOC_GUARD = 2048            # floats per side (multiple of 4: the inner view stays 16-byte aligned)
ALLOC_SENTINEL = -7.25e11


@contextlib.contextmanager
def guarded_allocations():
    real_empty = torch.empty
    seen = []

    def empty(*size, **kw):
        one_d = len(size) == 1 and isinstance(size[0], int)
        if one_d and kw.get("dtype") is torch.float32 and str(kw.get("device", "cpu")).startswith("cuda") and size[0] >= 16:
            n = (size[0] + 3) & ~3
            full = real_empty(n + 2 * ALLOC_GUARD, **kw)
            full.fill_(ALLOC_SENTINEL)
            seen.append((full, n))
            return full[ALLOC_GUARD: ALLOC_GUARD + size[0]]
        return real_empty(*size, **kw)

    torch.empty = empty
    try:
        yield seen
    finally:
        torch.empty = real_empty


def assert_guards_intact(seen, what):
    assert seen, what
    for full, n in seen:
        lo, hi = full[:ALLOC_GUARD], full[ALLOC_GUARD + n:]
        assert bool((lo == ALLOC_SENTINEL).all()) and bool((hi == ALLOC_SENTINEL).all()), \
            (what, "buffer of %d floats: %d guard floats overwritten below, %d above"
             % (n, int((lo != ALLOC_SENTINEL).sum()), int((hi != ALLOC_SENTINEL).sum())))


def opts(macx, **tune):
    """MacxOpts with abi_version set and the tune keys applied"""
    o = macx._lib.MacxOpts()
    o.abi_version = macx._lib.ABI_VERSION
    for k, v in tune.items():
        macx._lib.set_tune(o, k, v)
    return o
