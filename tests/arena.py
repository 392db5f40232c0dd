"""Guarded, exact-size, minimally aligned buffers for kernel tests (no test functions here; tests/test_arena_host.py proves the checker,
tests/test_hip_arena.py uses it on the device).

Every tensor an Arena hands out lives in its own uint8 allocation laid out as [guard | payload | guard]:

  * the payload starts at an address with ptr % 256 == 16 — the 16 bytes the ABI asks for and nothing better;
  * both guards hold byte 0xFF, which reads as float32 NaN, float64 NaN and int32 -1: a load that strays into a guard and is then
    "masked" by a multiplication with zero gives NaN, a stray store changes a byte that check() finds;
  * the guard on each side is max(64 KiB, 2 x 128 x (last dimension x itemsize)) rounded up to 256: two full 128-row tiles of the
    tensor's own rows (the largest legitimate off-by-one of a tile kernel is one tile), 64 KiB for vectors and scratch.  This is a
    condition, not a measurement.

The guards belong to the test's own allocation, so a kernel that oversteps writes into test memory and is reported; nothing faults that
could not fault before.  Works on CPU tensors as well as on the device.
"""
import math

import torch

FILL = 0xFF
MIN_GUARD = 64 * 1024
ALIGN = 256
OFFSET = 16                 # payload address modulo ALIGN


def guard_bytes(last_dim, itemsize):
    """Guard size per side for a tensor whose rows are `last_dim` elements of `itemsize` bytes."""
    g = max(MIN_GUARD, 2 * 128 * int(last_dim) * int(itemsize))
    return (g + ALIGN - 1) // ALIGN * ALIGN


def guard_for(shape, itemsize):
    """Guard size per side of a tensor of this shape: its rows are its last dimension; a vector (one dimension) has no rows."""
    return guard_bytes(shape[-1] if len(shape) >= 2 else 1, itemsize)


def arena_bytes(shape, dtype=torch.float32):
    """Bytes of the allocation behind one arena tensor of this shape (payload, both guards and the alignment slack)."""
    itemsize = torch.empty(0, dtype=dtype).element_size()
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    return math.prod(shape) * itemsize + 2 * guard_for(shape, itemsize) + ALIGN


def scratch_bytes(nbytes):
    """Bytes of the allocation behind one exact scratch request."""
    return int(nbytes) + 2 * guard_bytes(1, 1) + ALIGN


class _NonNullEmpty(torch.Tensor):
    """A zero-length uint8 view that still reports where it sits: torch gives data_ptr() == 0 for every tensor without elements, and a
    wrapper that passes its scratch pointer on must not turn "0 bytes at p" into a null pointer."""

    def data_ptr(self):
        return self._arena_ptr


class _Block:
    def __init__(self, name, kind, raw, start, nbytes, tensor):
        self.name, self.kind, self.raw, self.start, self.nbytes, self.tensor = name, kind, raw, start, nbytes, tensor

    @property
    def payload(self):
        return self.raw[self.start:self.start + self.nbytes]

    def changed(self):
        """Does the payload hold anything but the fill byte?  (scratch / output: was it written?)"""
        return bool((self.payload != FILL).any().item()) if self.nbytes else False


class Arena:
    """Hands out guarded tensors on `device` and checks them.  kinds: input (read only: guards checked), output (payload filled with
    0xFF: guards, unwritten and non-finite elements checked), inout (copy of a tensor, written in place: guards and non-finite elements
    checked), scratch (raw bytes, 0xFF: guards checked)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.blocks = []

    # ---- allocation ------------------------------------------------------------------------------------------------------------
    def _new(self, name, kind, shape, dtype):
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty(0, dtype=dtype).element_size()
        nbytes = math.prod(shape) * itemsize
        guard = guard_for(shape, itemsize)
        raw = torch.full((nbytes + 2 * guard + ALIGN,), FILL, dtype=torch.uint8, device=self.device)
        start = guard + (OFFSET - (raw.data_ptr() + guard)) % ALIGN
        assert (raw.data_ptr() + start) % ALIGN == OFFSET and start + nbytes + guard <= raw.numel()
        t = raw[start:start + nbytes].view(dtype).view(shape)
        blk = _Block(name or f"{kind}{len(self.blocks)}", kind, raw, start, nbytes, t)
        self.blocks.append(blk)
        return blk

    def input(self, t, name=None):
        """A guarded copy of `t` (any device) that the call under test only reads."""
        blk = self._new(name, "input", t.shape, t.dtype)
        blk.tensor.copy_(t)
        return blk.tensor

    def output(self, shape, dtype=torch.float32, name=None):
        """A guarded tensor whose every byte is 0xFF: an element the kernel never stores is still NaN (or -1) afterwards."""
        if isinstance(shape, int):
            shape = (shape,)
        return self._new(name, "output", shape, dtype).tensor

    def inout(self, t, name=None):
        """A guarded copy of `t` that the call under test updates in place (accumulate forms, running statistics, dgamma / dbeta)."""
        blk = self._new(name, "inout", t.shape, t.dtype)
        blk.tensor.copy_(t)
        return blk.tensor

    def scratch(self, nbytes, name=None):
        """Exactly `nbytes` of 0xFF as a uint8 tensor; 0 bytes gives a zero-length view whose data_ptr() is still inside the arena."""
        blk = self._new(name, "scratch", (int(nbytes),), torch.uint8)
        if blk.nbytes == 0:
            t = torch.Tensor._make_subclass(_NonNullEmpty, blk.tensor)
            t._arena_ptr = blk.raw.data_ptr() + blk.start
            blk.tensor = t
        return blk.tensor

    def block_of(self, t):
        for blk in self.blocks:
            if blk.tensor is t:
                return blk
        raise KeyError("not an arena tensor")

    # ---- the check -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _span(mask):
        idx = mask.nonzero().flatten()
        return int(idx[0].item()), int(idx[-1].item()), int(idx.numel())

    def problems(self):
        """Every finding as one line of text (empty: clean)."""
        out = []
        for b in self.blocks:
            front, back = b.raw[:b.start], b.raw[b.start + b.nbytes:]
            fbad, bbad = front != FILL, back != FILL
            if bool(fbad.any().item()):
                lo, hi, n = self._span(fbad)
                out.append(f"{b.name} ({b.kind}): guard BEFORE the payload overwritten: {n} bytes changed, first at payload offset "
                           f"{lo - b.start}, last at {hi - b.start}")
            if bool(bbad.any().item()):
                lo, hi, n = self._span(bbad)
                out.append(f"{b.name} ({b.kind}): guard AFTER the payload overwritten: {n} bytes changed, first at payload offset "
                           f"{b.nbytes + lo}, last at {b.nbytes + hi} (payload is {b.nbytes} bytes)")
            if b.kind == "output" and b.nbytes:
                item = b.tensor.element_size()
                unwritten = (b.payload.view(-1, item) == FILL).all(dim=1)
                if bool(unwritten.any().item()):
                    lo, hi, n = self._span(unwritten)
                    out.append(f"{b.name} (output): {n} of {unwritten.numel()} elements hold the fill pattern (never written, or a NaN that "
                               f"came out of a guard), first at flat index {lo}, last at {hi}")
                    continue                                   # (the fill pattern is NaN: do not report the same elements twice)
            if b.kind in ("output", "inout") and b.nbytes and b.tensor.is_floating_point():
                bad = ~torch.isfinite(b.tensor).flatten()
                if bool(bad.any().item()):
                    lo, hi, n = self._span(bad)
                    out.append(f"{b.name} ({b.kind}): {n} of {bad.numel()} elements are not finite, first at flat index {lo}, last "
                               f"at {hi}")
        return out

    def check(self):
        """Assert that no guard byte changed, that every output element was written and that every output / inout element is finite."""
        found = self.problems()
        assert not found, "arena check failed:\n  " + "\n  ".join(found)


class ScratchRequest:
    """One call of ops._scratch under exact_scratch."""

    def __init__(self, kind, nbytes, block):
        self.kind, self.nbytes, self._block = kind, nbytes, block

    @property
    def changed(self):
        """Did anything store into the payload?  (read it after the synchronize)"""
        return self._block.changed()

    def __repr__(self):
        return f"ScratchRequest(kind={self.kind}, nbytes={self.nbytes})"


def exact_scratch(monkeypatch, arena):
    """Replace pcgan_amd.ops._scratch (ops.workspace / workspace2 reach it through the module global) until the test ends: every
    request gets a fresh arena payload of exactly `nbytes`, all 0xFF, registered for arena.check().  Returns the list of requests
    (ScratchRequest: kind, nbytes, changed), which grows with every call."""
    from pcgan_amd import ops
    log = []

    def _scratch(kind, nbytes, device):
        nbytes = int(nbytes)
        t = arena.scratch(nbytes, name=f"scratch request {len(log)} (kind {kind}, {nbytes} bytes)")
        log.append(ScratchRequest(kind, nbytes, arena.blocks[-1]))
        return t

    monkeypatch.setattr(ops, "_scratch", _scratch)
    return log
