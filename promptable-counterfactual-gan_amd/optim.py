"""torch.optim.Adam / AdamW drop-ins on the fused HIP kernel (mnist_dcgan.py:126-127; mnist/trainer.py:77-78;
mnist_wgan_conditional.py:118-119).

Parameters of a `FlatModule` are views of one flat buffer, so the whole net is updated by ONE launch; parameters
that are adjacent in memory are coalesced into segments generically (any dense fp32 parameter works).  The step
counter lives on the device and the bias corrections are computed there, so `step()` can be captured in a HIP graph.

`state_dict()` / `load_state_dict()` speak torch's format in both directions: per parameter index
{"step", "exp_avg", "exp_avg_sq"}, the moments in the parameter's logical shape, so a checkpoint written here loads into
torch.optim.Adam / AdamW and one written there resumes here.
"""
import torch

from . import ops
from ._lib import PcgError


class _PendingState:
    """What Adam.snapshot() returns while a loaded state waits for the segments: the state itself (its tensors are only ever read)."""

    def __init__(self, state):
        self.state = state


class Adam(torch.optim.Optimizer):
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
        if amsgrad:
            raise PcgError("amsgrad is not implemented (the reference never enables it)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._segments = None  # per group: list of dicts(param_flat, grad_flat, exp_avg, exp_avg_sq, step, hyper)
        self._pending = None   # a loaded state {param: {"step", "exp_avg", "exp_avg_sq"}} that waits for the segments (_build)

    # -- segments: maximal runs of parameters that are adjacent in memory (with identical grad layout) -----
    @staticmethod
    def _dense_span(t):
        """(ptr, numel) if the tensor's elements occupy one dense span of memory (any permutation), else None."""
        if t.numel() == 0:
            return None
        dims = sorted(((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1), key=lambda d: d[0])
        expect = 1
        for st, sz in dims:
            if st != expect:
                return None
            expect *= sz
        return t.data_ptr(), t.numel()

    def _plan(self, on_gpu=True):
        """Per group, the runs of parameters that are adjacent in memory (pointer arithmetic only: nothing is allocated).  on_gpu
        False leaves out the float32-on-the-GPU refusal: a loaded state is checked against the runs wherever the parameters are."""
        plan = []
        for group in self.param_groups:
            items = []
            for p in group["params"]:
                if not p.requires_grad and p.grad is None:
                    continue
                if p.grad is None:
                    raise PcgError("Adam.step(): a parameter has no gradient yet (FlatModule attaches .grad views at its "
                                   "first forward/zero_grad; call step() after backward)")
                sp, sg = self._dense_span(p.data), self._dense_span(p.grad)
                if sp is None or sg is None or p.grad.stride() != p.data.stride():
                    raise PcgError("Adam: parameter/gradient memory must be dense with identical layout")
                if on_gpu and (p.dtype != torch.float32 or not p.is_cuda):
                    raise PcgError("Adam: parameters must be float32 tensors on the GPU")
                items.append((sp[0], sg[0], sp[1], p))
            items.sort(key=lambda it: it[0])
            segs = []
            for pptr, gptr, n, p in items:
                if segs:
                    s = segs[-1]
                    gap = (pptr - s["pend"]) // 4
                    # FlatModule pads every parameter to a multiple of 4 floats; the padding is zero in both buffers
                    if 0 <= gap < 4 and (pptr - s["pend"]) % 4 == 0 and gptr - s["gptr"] == pptr - s["pptr"] and p.device == s["dev"]:
                        s["pend"] = pptr + 4 * n
                        s["params"].append(p)
                        continue
                segs.append({"pptr": pptr, "gptr": gptr, "pend": pptr + 4 * n, "params": [p], "dev": p.device})
            plan.append(segs)
        return plan

    def _build(self):
        self._segments = []
        for segs in self._plan():
            built = []
            for s in segs:
                n = (s["pend"] - s["pptr"]) // 4
                p0 = s["params"][0]
                # typed views over the raw spans (no copy): storage-level views of the first parameter / gradient
                pflat = torch.as_strided(p0.data, (n,), (1,), storage_offset=p0.data.storage_offset())
                gflat = torch.as_strided(p0.grad, (n,), (1,), storage_offset=p0.grad.storage_offset())
                assert pflat.data_ptr() == s["pptr"] and gflat.data_ptr() == s["gptr"]
                dev = s["dev"]
                st = {
                    "param": pflat, "grad": gflat, "n": n, "params": s["params"],
                    "offsets": [(self._dense_span(p.data)[0] - s["pptr"]) // 4 for p in s["params"]],   # first element of each parameter
                    "exp_avg": ops.fill(torch.empty(n, dtype=torch.float32, device=dev), 0.0),
                    "exp_avg_sq": ops.fill(torch.empty(n, dtype=torch.float32, device=dev), 0.0),
                    "step": torch.zeros(1, dtype=torch.int64, device=dev),
                    "hyper": torch.zeros(12, dtype=torch.float32, device=dev),       # 48 bytes of kernel-side scratch (ticket + cached corrections)
                }
                built.append(st)
            self._segments.append(built)
        if self._pending is not None:
            try:
                self._write_state(self._pending)
            except PcgError:
                self._segments = None    # the refused state stays pending: every later step() refuses it again
                raise
            self._pending = None

    def _stale(self):
        if self._segments is None:
            return True
        for built in self._segments:
            for st in built:
                p0 = st["params"][0]
                if p0.grad is None or p0.data_ptr() != st["param"].data_ptr() or p0.grad.data_ptr() != st["grad"].data_ptr():
                    return True
        return False

    def _ensure_built(self, what="Adam"):
        """The segments exist and lie over the parameters' current storage (built now if they were not yet); moments that have
        been stepped cannot follow a storage that moved."""
        if self._stale():
            if self._segments is not None and any(int(st["step"].item()) for b in self._segments for st in b):
                raise PcgError(f"{what}: parameter storage changed after optimisation started (module moved or re-flattened)")
            self._build()

    def flat_segment(self, net, what="Adam"):
        """The one state segment (param, grad, exp_avg, exp_avg_sq, step, n) over FlatModule `net`'s flat buffer: what a fused
        trainer hands to its kernel.  Refused unless this optimizer holds exactly the module's parameters."""
        net._ensure_flat()
        self._ensure_built(what)
        segs = [st for b in self._segments for st in b]
        if len(segs) != 1 or segs[0]["param"].data_ptr() != net.flat_params.data_ptr():
            raise PcgError(f"{what}: the optimizer must hold exactly the module's parameters (one flat segment)")
        return segs[0]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ensure_built()
        for group, built in zip(self.param_groups, self._segments):
            b1, b2 = group["betas"]
            for st in built:
                ops.adam_step_capturable(st["param"], st["grad"], st["exp_avg"], st["exp_avg_sq"], float(group["lr"]), float(b1),
                                         float(b2), float(group["eps"]), float(group["weight_decay"]), self._decoupled,
                                         st["step"], st["hyper"])
        return loss

    def zero_grad(self, set_to_none=False):
        """Zero gradients in place (one launch per segment); `.grad` views are kept."""
        if self._stale():
            have = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
            if not have:
                return
            if self._segments is None or not any(int(st["step"].item()) for b in self._segments for st in b):
                self._build()
        for built in self._segments:
            for st in built:
                ops.fill(st["grad"], 0.0)

    # -- state snapshot (used around HIP-graph warm-up, which has to execute real steps before capture) ---------------
    def snapshot(self):
        """Copies of (exp_avg, exp_avg_sq, step) per segment; a loaded state that still waits for the segments (_PendingState: the
        warm-up's first step builds them and consumes it); or None if there is neither."""
        if self._pending is not None:
            return _PendingState(self._pending)
        if self._segments is None:
            return None
        return [[(st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()) for st in built] for built in self._segments]

    def restore(self, snap):
        """Put the state back (snap=None: back to 'never stepped' — zero moments, step 0 — keeping the buffers, so a
        captured graph that references them stays valid).  A _PendingState goes back into the segments the warm-up built, in place,
        or stays pending if nothing built them."""
        if isinstance(snap, _PendingState):
            if self._segments is None:
                self._pending = snap.state
            else:
                self._write_state(snap.state)
            return
        if self._segments is None:
            return
        for gi, built in enumerate(self._segments):
            for si, st in enumerate(built):
                if snap is None:
                    ops.fill(st["exp_avg"], 0.0); ops.fill(st["exp_avg_sq"], 0.0); st["step"].zero_()
                else:
                    ea, es, stp = snap[gi][si]
                    st["exp_avg"].copy_(ea); st["exp_avg_sq"].copy_(es); st["step"].copy_(stp)

    # -- torch-format state ---------------------------------------------------------------------------------------
    _torch_class = torch.optim.Adam

    @staticmethod
    def _under(flat, st, i):
        """The part of a segment-long tensor that lies under the segment's i-th parameter, seen through that parameter's own layout:
        a conv weight is a permuted view of the flat buffer (FlatModule._views: physical [o, kh, kw, i]), so element [o, i, kh, kw]
        of the result belongs to element [o, i, kh, kw] of the weight.  The pad4 gaps between parameters lie under no parameter."""
        p = st["params"][i]
        return torch.as_strided(flat, p.shape, p.stride(), st["offsets"][i])

    def _live_state(self):
        """{param: {"step", "exp_avg", "exp_avg_sq"}} of every segment that has been stepped, as torch writes it: contiguous clones in
        the parameter's logical shape on its device, `step` a 0-dim float32 tensor holding the segment's device counter (exact up to
        2^24 steps, as in torch).  One host read per segment."""
        state = {}
        for built in self._segments or []:
            for st in built:
                t = int(st["step"].item())
                if t == 0:
                    continue                              # never stepped: no entry, as in torch
                for i, p in enumerate(st["params"]):
                    state[p] = {"step": torch.tensor(float(t), dtype=torch.float32),
                                "exp_avg": self._under(st["exp_avg"], st, i).clone(memory_format=torch.contiguous_format),
                                "exp_avg_sq": self._under(st["exp_avg_sq"], st, i).clone(memory_format=torch.contiguous_format)}
        return state

    @staticmethod
    def _check_segments(state, runs):
        """The two refusals that need the segments: one device counter serves a whole segment, so its parameters come with one
        `step` value, all of them or none.  runs: lists of parameters, one per segment."""
        for params in runs:
            have = [p for p in params if p in state]
            if not have:
                continue
            if len(have) != len(params):
                raise PcgError(f"Adam.load_state_dict: the state covers {len(have)} of the {len(params)} parameters of one segment (parameters "
                               "that are adjacent in memory share one step counter): a state for some but not all parameters of a segment "
                               "cannot be loaded")
            steps = sorted({float(state[p]["step"]) for p in have})
            if len(steps) != 1:
                raise PcgError(f"Adam.load_state_dict: differing step values {steps} inside one segment (parameters that are adjacent in "
                               "memory share one device step counter)")

    def _write_state(self, state):
        """A torch-format state into the EXISTING exp_avg / exp_avg_sq / step tensors, in place: their addresses do not change, so a
        captured graph that references them stays valid.  A segment the state does not cover goes back to 'never stepped'.  Checked
        as a whole before anything is written.
        The AdamCache scratch (st["hyper"]: the ticket and the cached bias corrections of the next step) needs no handling: its tag
        names the step it was computed for, misses after a restored counter, and the kernel recomputes the corrections
        (csrc/pointwise.hip, struct AdamCache)."""
        segs = [st for built in self._segments for st in built]
        self._check_segments(state, [st["params"] for st in segs])
        with torch.no_grad():
            for st in segs:
                if st["params"][0] not in state:
                    ops.fill(st["exp_avg"], 0.0); ops.fill(st["exp_avg_sq"], 0.0); st["step"].zero_()
                    continue
                for i, p in enumerate(st["params"]):
                    self._under(st["exp_avg"], st, i).copy_(state[p]["exp_avg"])
                    self._under(st["exp_avg_sq"], st, i).copy_(state[p]["exp_avg_sq"])
                st["step"].fill_(int(float(state[st["params"][0]]["step"])))

    def state_dict(self):
        """torch.optim.Adam / AdamW's state_dict: loads into the torch optimizer over the same parameters, whose next step then runs.
        The param_groups carry the keys of the installed torch's defaults (amsgrad: False, maximize: False, ...), read from a
        throw-away torch optimizer.  A state that was loaded and still waits for the segments is returned as it was loaded."""
        state = self._pending if self._pending is not None else self._live_state()
        self.state.update(state)                          # torch's own packing (parameter indices, hooks) over a momentarily filled self.state
        try:
            sd = super().state_dict()
        finally:
            self.state.clear()
        if self._pending is not None:
            sd["state"] = {k: {n: v.clone() for n, v in s.items()} for k, s in sd["state"].items()}
        defaults = self._torch_class([torch.zeros(1)]).defaults
        for g in sd["param_groups"]:
            for k, v in defaults.items():
                g.setdefault(k, v)
        return sd

    def load_state_dict(self, state_dict):
        """A torch.optim.Adam / AdamW state_dict (or one of this class).  Segments that exist are written in place; before the first
        backward (no gradients, so no segments yet) the state is kept pending, applied when step() builds them, and state_dict()
        returns it meanwhile.  Refused: amsgrad / maximize, a shape mismatch, differing `step` values inside one segment, a state for
        some but not all parameters of a segment (the last two as soon as the segments are known: here, or at the first step)."""
        for g in state_dict["param_groups"]:
            for flag in ("amsgrad", "maximize"):
                if g.get(flag):
                    raise PcgError(f"Adam.load_state_dict: the state was written with {flag}=True, which is not implemented")
        by_index = {i: p for g, mine in zip(state_dict["param_groups"], self.param_groups) for i, p in zip(g["params"], mine["params"])}
        for i, s in state_dict["state"].items():
            missing = [k for k in ("step", "exp_avg", "exp_avg_sq") if k not in s]
            if missing:
                raise PcgError(f"Adam.load_state_dict: the state of parameter {i} lacks {missing}")
            for k in ("exp_avg", "exp_avg_sq"):
                if i in by_index and tuple(s[k].shape) != tuple(by_index[i].shape):
                    raise PcgError(f"Adam.load_state_dict: shape mismatch: {k} of parameter {i} is {tuple(s[k].shape)}, the parameter "
                                   f"{tuple(by_index[i].shape)}")
        super().load_state_dict(state_dict)               # torch's checks and casts; fills self.state and the param_groups
        state = {p: dict(s) for p, s in self.state.items()}
        self.state.clear()                                # the moments live in the segments, never in self.state
        for p, s in state.items():
            state[p] ={"step": torch.as_tensor(s["step"], dtype=torch.float32).detach().reshape(()).cpu().clone(),
                        "exp_avg": s["exp_avg"].detach().clone(), "exp_avg_sq": s["exp_avg_sq"].detach().clone()}
        if self._segments is not None and not self._stale():
            self._write_state(state)
            self._pending = None
            return
        if all(p.grad is not None or not p.requires_grad for g in self.param_groups for p in g["params"]):
            self._check_segments(state, [s["params"] for segs in self._plan(on_gpu=False) for s in segs])
        self._segments, self._pending = None, state       # segments over a storage that moved are dropped with their state

    # number of kernel launches a step() issues (for tests / DESIGN.md)
    def num_segments(self):
        if self._stale():
            self._build()
        return sum(len(b) for b in self._segments)


class AdamW(Adam):
    _decoupled = True
    _torch_class = torch.optim.AdamW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
