"""What the graphed steppers share on the host side: the one way a training step is captured in a HIP graph, and the
batch walk of the two classifier fits.  No kernel is launched from here.

A step is captured once per batch size and replayed with one host call.  Capture needs real warm-up executions first, so building a
stepper goes: clone what a warm-up advances (Held) -> warm up on THE side stream (warmup_stream) and join -> put the state back ->
collector off -> capture -> collector back on -> put the state back again (capture_steps).  nn.GraphedStep, which cuts its step
into segments, walks the same sequence by hand over Held and the backend."""
import gc

import torch

from ._lib import PcgError

_warmup_streams = {}


def warmup_stream(dev):
    """ONE side stream per device for the warm-up execution of every capture.  A stream's first convolution hands it 64 MiB of stream-K
    scratch for the life of the process (ops._conv_scratch), so a fresh stream per capture -- one per batch size per stepper -- pinned
    that much per graph."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _warmup_streams:
        _warmup_streams[key] = torch.cuda.Stream(dev)
    return _warmup_streams[key]


class HipGraphCapture:
    """The capture backend: HIP graphs (torch.cuda.CUDAGraph).  segmented=True (nn.GraphedStep): every segment of the step in ONE
    memory pool, and capture_error_mode="thread_local"; False (capture_steps: one graph holds a whole step): torch's defaults."""

    def __init__(self, device, tick=True, segmented=True):
        self._device, self._segmented, self._pool = torch.device(device), segmented, None
        self._tick = torch.zeros(1, device=device) if tick else None     # tick=False: one segment holding the whole step, never empty

    def warmup(self, run, n, dp):
        # segmented (nn.GraphedStep) keeps a side stream of its own per capture, as it always had: on the shared stream the third
        # graph built in one process (the CounteRGAN step behind the DCGAN and WGAN steps) replayed 0.2 % slower, 26.57 against
        # 26.50 ms, five alternating runs each; which allocation moved is not known
        side = torch.cuda.Stream(self._device) if self._segmented else warmup_stream(self._device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(n):
                run()
            if dp is not None:
                dp.wait_all()
        torch.cuda.current_stream().wait_stream(side)

    def begin(self, collect=True):
        """Python's cyclic collector must not run while a stream captures: freeing a graph, an event or a cached block from a finalizer
        is a HIP call the capture forbids, and an error raised inside a finalizer aborts the process.  collect=True: collect now, then
        hold it off.  False: only hold it off -- what is garbage now stays so until the collector is back on, and a collection costs
        60 ms, more than two epochs of a classifier fit."""
        if collect:
            gc.collect()
        self._gc_was_on = gc.isenabled()
        gc.disable()
        try:
            self._g = torch.cuda.CUDAGraph()
            # thread_local: calls made by other threads (the RCCL watchdog polling events) must not invalidate the capture
            mode = dict(pool=self._pool, capture_error_mode="thread_local") if self._segmented else {}
            self._ctx = torch.cuda.graph(self._g, **mode)
            self._ctx.__enter__()
        except BaseException:
            self._gc_restore()         # the capture never began: end() will not run, the collector must not stay off
            raise
        if self._tick is not None:
            self._tick.add_(1.0)   # no segment is ever empty (an empty capture cannot be instantiated)

    def _gc_restore(self):
        if getattr(self, "_gc_was_on", False):
            gc.enable()
        self._gc_was_on = False

    def end(self):
        try:
            self._ctx.__exit__(None, None, None)
        finally:
            self._gc_restore()
        if self._segmented and self._pool is None:
            self._pool = self._g.pool()
        return self._g             # .replay()

    abort = end


class Held:
    """Clones of everything a warm-up execution advances: each module's flat parameters and buffers, each optimizer's snapshot(), each
    plain tensor (a device RNG counter, a tally, an accumulator; None entries are skipped).  restore() puts all of it back in place, so
    building a stepper does not advance training.  Parameters AND buffers are always held: a stepper whose graph has no Adam, or whose
    nets have no BatchNorm, pays a few copies at construction and nobody has to argue why a subset is enough."""

    def __init__(self, modules=(), optimizers=(), tensors=()):
        self._modules = [(m, m.flat_params.clone(), [b.clone() for b in m.buffers()]) for m in modules]
        self._optimizers = [(o, o.snapshot()) for o in optimizers]
        self._tensors = [(t, t.clone()) for t in tensors if t is not None]

    def restore_tensors(self):
        for t, t0 in self._tensors:
            t.copy_(t0)

    def restore(self):
        for m, fp, bufs in self._modules:
            m.flat_params.copy_(fp)
            for b, b0 in zip(m.buffers(), bufs):
                b.copy_(b0)
        for o, snap in self._optimizers:
            o.restore(snap)
        self.restore_tensors()


def capture_steps(runs, held, dev, *, collect=False, backend=None):
    """Capture every fn of runs = [(fn, n_warmup)] in a graph of its own; returns [(graph, what fn returned while capturing)].
    Each fn is first executed n_warmup times on the warm-up stream; the plain tensors of `held` go back after each run's warm-up (a
    cursor that the runs share never walks past its data), all of `held` before the first capture (the graphs see Adam at the step
    the caller is at; capture executes nothing, so this costs a few copies) and again after the last.  The cyclic collector is off
    from the first capture to the last and handed back on every path (HipGraphCapture.begin says why, and what `collect` buys)."""
    if backend is None:
        backend = HipGraphCapture(dev, tick=False, segmented=False)
    for fn, n in runs:
        backend.warmup(fn, n, None)
        held.restore_tensors()
    held.restore()
    if collect:
        gc.collect()
    gc_on = gc.isenabled()
    gc.disable()
    got = []
    try:
        for fn, _ in runs:
            backend.begin(collect=False)
            try:
                out = fn()
            except BaseException:
                backend.abort()
                raise
            got.append((backend.end(), out))
    finally:
        if gc_on:
            gc.enable()
        held.restore()
    return got


class BatchWalkFit:
    """The walk of a classifier fit over one epoch's batches, one graph replay per step: the training set, the epoch's permutation and
    the tally pair (sum of loss * rows, correct rows, rows; training and validation) live on the device, a device counter holds the
    Philox offset and the cursor into the permutation, and there is one buffer set and one graph per batch size met -- the full batch
    and the tail N % batch_size.  graph=False: the same launches called eagerly with by-value draws (what the replays must equal).

    A subclass sets `rng` and `optimizer`, and gives `_buffers(R)` (the buffer set of R rows: a dict with "x", "y", "m" (the Dropout
    masks) and "loss"), `_launches(b, cursor=None)` (one step over the set b; cursor None: offsets and rows from the device counter,
    the captured form), `_forward_backward(b)`, `_span(R)` (the Philox offsets one step consumes) and, if something follows every
    step outside the graph, `_after_step()`."""

    def __init__(self, N, B):
        self.N, self.B = int(N), int(B)
        self.tail = self.N % self.B if self.B > 0 else 0
        self._cur = 0

    def _start(self, module, dev, graph=True, backend=None):
        """The device state of the walk, the buffer sets, and (graph=True) their graphs."""
        self._tallies = torch.zeros(6, dtype=torch.float64, device=dev)
        self.tally, self.val_tally = self._tallies[:3], self._tallies[3:]
        self.perm = torch.arange(self.N, dtype=torch.int64, device=dev)               # identity until new_epoch()
        self._ctr = self.rng.device_counter(dev, cursor=True)
        self._bufs = {R: self._buffers(R) for R in sorted({self.B if self.N >= self.B else 0, self.tail} - {0})}
        self._graphs = self._capture(module, dev, backend) if graph else None

    def _capture(self, module, dev, backend=None):
        held = Held([module], [self.optimizer], [self._ctr, self._tallies])
        got = capture_steps([(lambda b=b: self._launches(b), 1) for b in self._bufs.values()], held, dev, backend=backend)
        return {R: g for R, (g, _) in zip(self._bufs, got)}

    def _after_step(self):
        pass

    def new_epoch(self, perm):
        """Upload this epoch's row order (N entries) and rewind the cursor: one small copy per EPOCH."""
        if perm.numel() != self.N:
            raise PcgError(f"{type(self).__name__}.new_epoch: permutation of {perm.numel()} entries, {self.N} needed")
        self.perm.copy_(perm.to(torch.int64))
        self._ctr[2:3].zero_()
        self._cur = 0

    @property
    def steps_per_epoch(self):
        return self.N // self.B + (1 if self.tail else 0)

    def step(self, record=None):
        """The next batch of the epoch: one replay, then _after_step().  record (a dict): receives clones of the batch's rows ("x",
        "y"), its masks ("masks") and its loss ("loss", a [1] device tensor)."""
        left = self.N - self._cur
        if left <= 0:
            raise PcgError(f"{type(self).__name__}.step: the epoch is used up; call new_epoch(perm)")
        R = self.B if left >= self.B else left
        b = self._bufs[R]
        if self._graphs is not None:
            self._graphs[R].replay()
            self.rng.offset += self._span(R)                  # the host-side mirror of the device counter
        else:
            self._launches(b, cursor=self._cur)
        self._after_step()
        self._cur += R
        if record is not None:
            record.update(x=b["x"].clone(), y=b["y"].clone(), masks=[m.clone() for m in b["m"]], loss=b["loss"].clone())
        return R

    def run_batch(self, x, y, masks):
        """Forward, loss and backward of one GIVEN batch with GIVEN Dropout masks (runs that must reproduce recorded draws), called
        eagerly: the gradients land in the flat gradient buffer, the tally counts the batch; no optimizer step.  Returns the loss
        ([1], device)."""
        R = int(x.shape[0])
        if R not in self._bufs:
            raise PcgError(f"{type(self).__name__}.run_batch: {R} rows; this fit holds buffers for {sorted(self._bufs)}")
        b = self._bufs[R]
        b["x"].copy_(x.reshape(R, -1)); b["y"].copy_(y)
        for dst, src in zip(b["m"], masks):
            dst.copy_(src.reshape(dst.shape))
        self._forward_backward(b)
        return b["loss"]

    def epoch(self, perm):
        """All steps of one epoch in the order perm, with no host read."""
        self.new_epoch(perm)
        for _ in range(self.steps_per_epoch):
            self.step()

    def read_tally(self):
        """(sum of loss * rows, correct rows, rows) of the training steps since the last read; clears it.  One host read."""
        t = self.tally.cpu().tolist()
        self.tally.zero_()
        return tuple(t)

    def read_tallies(self):
        """The training tally and val_tally (same layout; train_classifier's validation adds to it) in ONE host read; clears both."""
        t = self._tallies.cpu().tolist()
        self._tallies.zero_()
        return tuple(t)
