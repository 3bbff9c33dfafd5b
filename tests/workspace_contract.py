"""Caller-held scratch for tests that hold an entry to its workspace contract (include/tspn_mi355x.h, Conventions): a
view of EXACTLY the bytes the entry's `*_workspace_bytes` helper asks for, 256-byte aligned, with a guard band on both
sides, in a chosen state -- zeros, 0xFF in every byte, or whatever an earlier launch of the same entry left there -- and
a replacement for `ops._ws` that hands such views to the Python wrappers and records them.  The counterpart of
tests/sentinel_buffers.py for the scratch side of a call.  Used by tests/test_gpu_workspace_contract.py."""
import contextlib

import torch

GUARD_BYTES = 64 * 1024     # in front of and behind the view
GUARD_FILL = 0xA5
ALIGN = 256
FILLS = ("zero", "ones", "stale")
# every byte 0xFF: a NaN in fp32, bf16 and fp16, -1 in every integer width
_FILL_BYTE = {"zero": 0x00, "ones": 0xFF, "stale": 0xFF}


def guarded_ws(nbytes, device, fill):
    """(buffer, view): `view` is a uint8 view of exactly `nbytes` bytes (256 for a need of 0, like ops._ws), 256-byte
    aligned, GUARD_BYTES of GUARD_FILL on either side of it inside `buffer`.  fill "zero" / "ones" sets every byte of
    the view to 0x00 / 0xFF; "stale" starts as "ones" and is meant to be run in once, on other inputs, before the launch
    under test (guarded_ops_ws(..., reuse=...) hands the same views out again, untouched)."""
    assert fill in FILLS, fill
    n = int(nbytes) if int(nbytes) > 0 else 256
    buf = torch.full((n + 2 * GUARD_BYTES + ALIGN,), GUARD_FILL, dtype=torch.uint8, device=device)
    lo = GUARD_BYTES + (-(buf.data_ptr() + GUARD_BYTES)) % ALIGN
    view = buf[lo:lo + n]
    assert view.data_ptr() % ALIGN == 0 and view.numel() == n and _view_bounds(buf) == (lo, n)
    view.fill_(_FILL_BYTE[fill])
    return buf, view


def _view_bounds(buffer):
    """(offset, bytes) of the view inside a guarded_ws buffer."""
    n = buffer.numel() - 2 * GUARD_BYTES - ALIGN
    return GUARD_BYTES + (-(buffer.data_ptr() + GUARD_BYTES)) % ALIGN, n


def assert_guards_intact(buffer, what):
    """Nothing in front of or behind the view of a guarded_ws `buffer` was written."""
    lo, n = _view_bounds(buffer)
    front, back = buffer[:lo], buffer[lo + n:]
    bad = int((front != GUARD_FILL).sum()), int((back != GUARD_FILL).sum())
    assert bad == (0, 0), f"{what}: {bad[0]} bytes written in front of and {bad[1]} behind a workspace of {n} bytes"


def assert_all_ones(view, what):
    """A "ones" view that a refused call must not have touched."""
    changed = int((view != 0xFF).sum())
    assert changed == 0, f"{what}: a refused call wrote {changed} bytes of its workspace"


class _Recorder:
    """The replacement of ops._ws: a guarded view per request, in the order of the requests."""

    def __init__(self, fill, reuse, short):
        self.fill, self.reuse, self.short = fill, reuse, int(short)
        self.records = []            # (buffer, view, bytes asked for)

    def __call__(self, nbytes, device):
        k = len(self.records)
        if self.reuse is not None:   # the k-th view of an earlier run of the same entry at the same shape
            assert k < len(self.reuse.records), "the stale run asks for more workspaces than the run before it"
            buf, view, asked = self.reuse.records[k]
            assert asked == int(nbytes), f"workspace {k}: {nbytes} bytes now, {asked} in the run before"
        else:
            buf, view = guarded_ws(nbytes, device, self.fill)
        self.records.append((buf, view, int(nbytes)))
        if self.short:
            assert int(nbytes) >= self.short, f"cannot shorten a workspace of {nbytes} bytes by {self.short}"
            return view[:int(nbytes) - self.short]
        return view

    @property
    def calls(self):
        return len(self.records)

    def assert_guards_intact(self, what):
        for k, (buf, view, _) in enumerate(self.records):
            assert_guards_intact(buf, f"{what} (workspace {k})")

    def assert_untouched(self, what):
        for k, (buf, view, _) in enumerate(self.records):
            assert_all_ones(view, f"{what} (workspace {k})")


@contextlib.contextmanager
def guarded_ops_ws(ops, fill="ones", reuse=None, short=0):
    """Replaces `ops._ws` inside the block by a function that hands out guarded views (guarded_ws) of exactly the bytes
    asked for and records them; yields the recorder.  `reuse` = the recorder of an earlier block: its views are handed out
    again as they were left ("stale").  `short` = n: the view handed to the wrapper is n bytes shorter than asked for
    (the memory behind it is still the full view: an entry that fails to refuse it runs on valid memory).  On leaving
    the block without an exception the guard bands are checked, and the wrapper must have asked for a workspace at all
    -- one that stops going through `_ws` cannot make a test vacuous."""
    rec = _Recorder(fill, reuse, short)
    orig = ops._ws
    ops._ws = rec
    try:
        yield rec
    finally:
        ops._ws = orig
    assert rec.calls > 0, "the wrapper never asked ops._ws for a workspace"
    torch.cuda.synchronize()
    rec.assert_guards_intact(f"fill={fill!r}")


def same_bits(a, b):
    """Bit equality of two tensors of one dtype and shape, NaN payloads and signed zeros included."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(ints), b.contiguous().view(ints))
