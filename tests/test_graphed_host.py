"""Host logic of pcgan_amd._graphed with no GPU: capture_steps over a recording backend (the one of tests/test_parallel_gloo.py:
"kernels" are thunks that are recorded, not executed, while a capture is open and run on replay -- the contract of stream capture),
and BatchWalkFit's walk over a stub subclass."""
import gc

import pytest
import torch

import pcgan_amd  # noqa: F401
from pcgan_amd import _graphed as GR
from pcgan_amd._lib import PcgError


class _Recorder:
    def __init__(self, fail_begin=False):
        self.open, self.log, self.fail_begin = None, [], fail_begin

    def launch(self, fn):
        if self.open is not None:
            self.open.append(fn)
        else:
            fn()

    def warmup(self, run, n, dp):
        assert dp is None
        for _ in range(n):
            run()

    def begin(self, collect=True):
        assert self.open is None and not collect and not gc.isenabled()   # capture_steps owns the collector
        self.log.append("begin")
        if self.fail_begin:
            raise RuntimeError("capture refused")
        self.open = []

    def end(self):
        seg, self.open = self.open, None
        self.log.append("end")

        class _Seg:
            def replay(_self):
                for fn in seg:
                    fn()
        return _Seg()

    def abort(self):
        self.open = None
        self.log.append("abort")


class _ToyNet:
    def __init__(self):
        self.flat_params = torch.arange(6.0)
        self.running = torch.tensor([0.5, -2.0])

    def buffers(self):
        return [self.running]


class _ToyOpt:
    def __init__(self):
        self.steps = torch.tensor([7.0])

    def snapshot(self):
        return self.steps.clone()

    def restore(self, s):
        self.steps.copy_(s)


class _Rig:
    """Two runs over one net, one optimizer and one counter; every execution is logged with the state it saw."""

    def __init__(self, fail_begin=False, raise_in_capture=False):
        self.rec, self.net, self.opt, self.ctr = _Recorder(fail_begin), _ToyNet(), _ToyOpt(), torch.tensor([3, 0, 0, 0])
        self.before = self.state()
        self.held = GR.Held([self.net], [self.opt], [self.ctr, None])
        self.calls, self.raise_in_capture = [], raise_in_capture

    def state(self):
        return [self.net.flat_params.clone(), self.net.running.clone(), self.opt.steps.clone(), self.ctr.clone()]

    def unchanged(self):
        return all(torch.equal(a, b) for a, b in zip(self.state(), self.before))

    def run(self, name):
        def fn():
            capturing = self.rec.open is not None
            self.calls.append((name, capturing, self.unchanged()))
            if capturing and self.raise_in_capture:
                raise ValueError("a launch failed")

            def k():
                self.net.flat_params.add_(1.0); self.net.running.mul_(2.0); self.opt.steps.add_(1.0); self.ctr.add_(5)
            self.rec.launch(k)
            return name + "-out"
        return fn

    def capture(self, **kw):
        return GR.capture_steps([(self.run("a"), 3), (self.run("b"), 1)], self.held, torch.device("cpu"), backend=self.rec, **kw)


def test_capture_steps_order_restores_and_return_values():
    rig = _Rig()
    got = rig.capture()
    assert [(n, c) for n, c, _ in rig.calls] == [("a", False)] * 3 + [("b", False), ("a", True), ("b", True)]
    # the plain tensors go back after each run's warm-up, everything before the first capture
    assert [u for _, _, u in rig.calls] == [True, False, False, False, True, True]
    assert rig.rec.log == ["begin", "end", "begin", "end"] and [out for _, out in got] == ["a-out", "b-out"]
    assert rig.unchanged() and gc.isenabled()
    got[0][0].replay()                                        # a graph holds its own run's launches
    assert torch.equal(rig.net.flat_params, rig.before[0] + 1) and int(rig.ctr[0]) == 8


def test_warmup_of_the_second_run_starts_from_the_held_tensors():
    rig, seen = _Rig(), []
    GR.capture_steps([(lambda: (seen.append(int(rig.ctr[0])), rig.ctr.add_(5))[0], 2), (lambda: seen.append(int(rig.ctr[0])), 1)],
                     rig.held, torch.device("cpu"), backend=_Recorder())
    assert seen[:3] == [3, 8, 3]                              # a cursor that the runs share never walks on from run to run


def test_collector_is_handed_back_when_begin_raises():
    rig = _Rig(fail_begin=True)
    with pytest.raises(RuntimeError, match="capture refused"):
        rig.capture()
    assert gc.isenabled() and rig.unchanged() and rig.rec.log == ["begin"]


def test_collector_is_handed_back_and_capture_aborted_when_a_run_raises():
    rig = _Rig(raise_in_capture=True)
    with pytest.raises(ValueError, match="a launch failed"):
        rig.capture()
    assert gc.isenabled() and rig.unchanged() and rig.rec.log == ["begin", "abort"]


def test_a_collector_that_was_off_stays_off():
    gc.disable()
    try:
        _Rig().capture()
        assert not gc.isenabled()
    finally:
        gc.enable()


@pytest.mark.parametrize("collect", [False, True])
def test_collection_is_forced_only_when_asked(monkeypatch, collect):
    forced = []
    monkeypatch.setattr(gc, "collect", lambda *a: forced.append(gc.isenabled()) or 0)
    _Rig().capture(collect=collect)
    assert forced == ([True] if collect else [])               # once, before the collector goes off


# ---- BatchWalkFit ----------------------------------------------------------------------------------------------------------------------
class _ToyRNG:
    offset = 0

    def device_counter(self, dev, cursor=False):
        return torch.zeros(4, dtype=torch.int64)


class ClassifierFit(GR.BatchWalkFit):
    def __init__(self, N, B):
        super().__init__(N, B)
        self.rng, self.optimizer, self.seen, self.after = _ToyRNG(), _ToyOpt(), [], 0
        self._start(_ToyNet(), torch.device("cpu"), graph=False)

    def _buffers(self, R):
        return {"x": torch.zeros(R, 2), "y": torch.zeros(R, dtype=torch.int64), "m": [torch.zeros(R, 2)], "loss": torch.zeros(1)}

    def _launches(self, b, cursor=None):
        self.seen.append((b["x"].shape[0], cursor))

    def _forward_backward(self, b):
        self.seen.append(("fb", b["x"].shape[0]))

    def _after_step(self):
        self.after += 1


@pytest.mark.parametrize("N,B,keys", [(5, 3, [2, 3]), (6, 3, [3]), (2, 3, [2]), (4, 4, [4])])
def test_buffer_set_keys(N, B, keys):
    fit = ClassifierFit(N, B)
    assert list(fit._bufs) == keys and fit.tail == N % B and fit.steps_per_epoch == -(-N // B)


def test_walk_refusals_and_tallies():
    fit = ClassifierFit(8, 3)
    fit.new_epoch(torch.arange(8).flip(0))
    assert [fit.step() for _ in range(3)] == [3, 3, 2] and fit.seen == [(3, 0), (3, 3), (2, 6)] and fit.after == 3
    with pytest.raises(PcgError, match=r"ClassifierFit\.step: the epoch is used up; call new_epoch\(perm\)"):
        fit.step()
    with pytest.raises(PcgError, match=r"ClassifierFit\.new_epoch: permutation of 7 entries, 8 needed"):
        fit.new_epoch(torch.arange(7))
    fit._ctr[2] = 8
    fit.new_epoch(torch.arange(8))
    assert fit._cur == 0 and int(fit._ctr[2]) == 0 and torch.equal(fit.perm, torch.arange(8))
    rec = {}
    assert fit.step(record=rec) == 3 and rec["x"].shape == (3, 2) and len(rec["masks"]) == 1
    with pytest.raises(PcgError, match=r"ClassifierFit\.run_batch: 4 rows; this fit holds buffers for \[2, 3\]"):
        fit.run_batch(torch.zeros(4, 2), torch.zeros(4), [torch.zeros(4, 2)])
    assert fit.run_batch(torch.ones(2, 1, 2), torch.ones(2), [torch.ones(2, 1, 2)]) is fit._bufs[2]["loss"]   # the reshaping form
    assert torch.equal(fit._bufs[2]["x"], torch.ones(2, 2)) and fit.seen[-1] == ("fb", 2)
    fit._tallies.copy_(torch.arange(1.0, 7.0, dtype=torch.float64))
    assert fit.read_tally() == (1.0, 2.0, 3.0) and fit._tallies.tolist() == [0.0, 0.0, 0.0, 4.0, 5.0, 6.0]
    fit.tally.fill_(9.0)
    assert fit.read_tallies() == (9.0, 9.0, 9.0, 4.0, 5.0, 6.0) and not fit._tallies.any()


def test_the_fit_captures_one_graph_per_buffer_set_through_capture_steps():
    fit, rec = ClassifierFit(5, 3), _Recorder()
    fit._ctr[0] = 11
    graphs = fit._capture(_ToyNet(), torch.device("cpu"), backend=rec)
    assert list(graphs) == [2, 3] and rec.log == ["begin", "end"] * 2 and int(fit._ctr[0]) == 11
    assert fit.seen == [(2, None), (3, None)] * 2               # warm-up, then capture, in the order of the buffer sets
