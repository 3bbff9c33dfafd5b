"""Caller-held outputs for tests that go through the C ABI: a sentinel-filled buffer with a guard band on both sides of
the output, the checks that every output element was written and nothing else was, and that a refused call wrote
nothing.  Shared by tests/test_gpu_frontend_edges.py and tests/test_gpu_conv2d_edges.py."""
import ctypes

import numpy as np
import torch

SENTINEL = -3.0e33
GUARD = 32              # elements in front of and behind a held output (fp32: 128 bytes, bf16: 64 bytes)


def p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)


def held(shape, device, dtype=torch.float32, offset=0):
    """(buffer, view): a sentinel-filled buffer and a contiguous view of `shape` GUARD + offset elements into it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=dtype, device=device)
    v = buf[GUARD + offset:GUARD + offset + n].view(shape)
    assert v.data_ptr() % 16 == (offset * buf.element_size()) % 16
    return buf, v


def sentinel_of(x):
    return torch.tensor(SENTINEL, dtype=x.dtype)


def assert_written_inside_only(buf, v, what):
    b = buf.cpu()
    n, lo = v.numel(), v.storage_offset()
    s = sentinel_of(b)
    assert bool((b[:lo] == s).all()) and bool((b[lo + n:] == s).all()), f"{what}: wrote outside the output"
    never = int((b[lo:lo + n] == s).sum())
    assert never == 0, f"{what}: {never} of {n} outputs never written"


def assert_untouched(buf, what):
    assert bool((buf.cpu() == sentinel_of(buf)).all()), f"{what}: a refused call wrote to the output"


def refused(tspn, rc, code, what):
    assert rc == code, f"{what}: returned {rc}, expected {code}"
