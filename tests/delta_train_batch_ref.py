"""Live references for the two MNIST CounteRGAN ports at the batch they train at, 128 (gan_train.params, countergan2.params), where the
recorded runs of tests/golden/ stop at 4: the float64 and float32 restatements (tests/delta_gan_restate.py, tests/countergan2_restate.py,
both with the interface used here) on batches(128)[0], and DESIGN.md §3.18's routing precondition computed from the two of them as
tests/golden/make_golden_delta_gan.py computes it for the recorded batches, and the same treatment of the nets' own ReLU / LeakyReLU
masks (`_Act`, `mask_report`).  Shared by tests/test_hip_delta_steps_train_batch.py (GPU)
and tests/test_delta_train_batch_host.py (the preconditions alone, no GPU).

CPU work only, on at most 16 threads."""
import contextlib
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pool_clf_restate as PR  # noqa: E402

B_TRAIN, B_TAIL = 128, 96                            # params["batch_size"]; MNIST's real tail, 60000 % 128
NEAR_CAP = 0.002                                     # §3.18: at most 0.2 % of a layer's live windows under the gap bound
NEAR_CAP_AFTER_ADAM = 0.01                           # D's masks in the G step: see mask_report
MAX_THREADS = 16
FORWARD = ("delta", "x_cf", "d_real", "d_fake", "d_fake_g", "cls_logits")


@contextlib.contextmanager
def cpu_threads():
    """At most MAX_THREADS torch threads while the restatements run; the earlier setting afterwards."""
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, MAX_THREADS))
    try:
        yield
    finally:
        torch.set_num_threads(before)


def batch(RS, B=B_TRAIN):
    x, y = RS.batches(B)[0]
    return x, y, torch.full_like(y, RS.TARGET_CLASS)


def rule_a(got, want64, what):
    """Rule (a) of tests/test_hip_delta_gan.py: rtol 1e-4, atol 2e-5 * max|reference|.  -> the largest error over that atol."""
    want64 = np.asarray(want64, np.float64)
    atol = 2e-5 * float(np.abs(want64).max())
    np.testing.assert_allclose(np.asarray(got, np.float64), want64, rtol=1e-4, atol=atol, err_msg=what)
    return float(np.abs(np.asarray(got, np.float64) - want64).max()) / atol if atol > 0 else 0.0


def routing(clf32, clf64):
    """§3.18's precondition from two pool_clf_restate.forward results on the same rows, float32 and float64: per pool layer the bound
    max(1e-5, 100 * max|z32 - z64|), the float64 run's live windows (p > 0), those of them whose top-two gap is under the bound
    (`near`), and the float64 run's window positions."""
    out = {}
    for layer in (1, 2):
        z32, z64 = clf32[f"z{layer}"], clf64[f"z{layer}"]
        bound = max(1e-5, 100.0 * float((z32.double() - z64).abs().max()))
        live = clf64[f"p{layer}"] > 0
        near = live & (PR.top2_gap(z64) < bound)
        out[layer] = {"bound": bound, "live": live.numpy(), "near": near.numpy(), "idx": clf64[f"idx{layer}"].numpy()}
    return out


# ---- the nets' own ReLU / LeakyReLU masks ------------------------------------------------------------------------------------------------------
# A ReLU's derivative jumps at zero as max-pooling's routing jumps at a tie: where a float64 pre-activation is within fp32 rounding of
# zero (at batch 128 a layer has 3 to 13 million units; a handful lie within 1e-7), an fp32 run may take the other branch -- a
# discontinuity of the derivative, not an error of either run, and one flipped unit of G's last ReLU moves every gradient below it by
# up to 4e-4 of its maximum.  So, as pool_clf_restate.pinned_forward does for the classifier, the float64 iteration takes the masks
# (activation > 0) of the run under test from outside, and the masks themselves are checked where they decide: wherever |z64| is at
# least the bound max(1e-5, 100 * max|z32 - z64|) the mask must be z64 > 0, and at most NEAR_CAP of a layer's units may lie under it.
class _Act(nn.Module):
    """Stands in for one ReLU / LeakyReLU(slope) of a restatement net.  Without masks: the activation itself.  With masks (one per
    call, the last repeated; bool, the input's shape): z * (mask ? 1 : slope).  keep: every call's pre-activation is kept in `seen`;
    z32 (the pre-activations of the float32 run, call by call): one mask_report per call in `reports`."""

    def __init__(self, slope, masks=None, z32=None, keep=False):
        super().__init__()
        self.slope, self.masks, self.z32, self.keep, self.calls, self.seen, self.reports = float(slope), masks, z32, keep, 0, [], []

    def forward(self, z):
        k, self.calls = self.calls, self.calls + 1
        if self.keep:
            self.seen.append(z.detach())
        if self.masks is None:
            return F.leaky_relu(z, self.slope) if self.slope else torch.relu(z)
        m = self.masks[min(k, len(self.masks) - 1)]
        if self.z32 is not None:
            self.reports.append(mask_report(z.detach(), self.z32[k], m))
        return z * torch.where(m, torch.ones((), dtype=z.dtype), torch.full((), self.slope, dtype=z.dtype))


def mask_report(z64, z32, mask):
    """One layer, one call: the bound, the units under it (`near`), the units where `mask` is not z64 > 0 (`flips`) and those of them
    at or over the bound (`wrong`: must be none)."""
    bound = max(1e-5, 100.0 * float((z32.double() - z64).abs().max()))
    near = z64.abs() < bound
    differ = mask != (z64 > 0)
    return {"units": z64.numel(), "bound": bound, "near": int(near.sum()), "flips": int(differ.sum()), "wrong": int((differ & ~near).sum())}


def install_acts(net, masks=None, z32=None, keep=False):
    """Replace the ReLU / LeakyReLU modules of net.net (they hold no parameters: state_dict keys and the optimizers are untouched) by
    _Act; masks / z32: one list per activation, in order.  -> the _Act modules."""
    acts = []
    for i, m in enumerate(net.net):
        if isinstance(m, (nn.ReLU, nn.LeakyReLU)):
            j = len(acts)
            net.net[i] = _Act(getattr(m, "negative_slope", 0.0), masks[j] if masks is not None else None, z32[j] if z32 is not None else None, keep)
            acts.append(net.net[i])
    return acts


def g_and_classifier_forward(RS, dtype, B=B_TRAIN):
    """G's and the frozen classifier's forward of step 1 in `dtype`, unpinned: delta, x_cf, cls_logits, loss_cls, loss_reg, the
    classifier's intermediates under "clf" and the pre-activations of G's ReLUs under "z"."""
    x, _, target = batch(RS, B)
    G, _ = RS.seeded_nets(dtype)
    acts = install_acts(G, keep=True)
    with torch.no_grad():
        x_cf, delta = G(x.to(dtype), target)
        clf = PR.forward(RS.classifier_state(dtype), x_cf)
        return {"delta": delta, "x_cf": x_cf, "cls_logits": clf["logits"], "loss_cls": float(F.cross_entropy(clf["logits"], target)),
                "loss_reg": float(delta.abs().mean()), "clf": clf, "z": [a.seen[0] for a in acts]}


def iteration(RS, dtype, pins=None, masks=None, z32=None, keep=False, B=B_TRAIN):
    """RS.iteration of step 1 in `dtype` from the seeded state, with its Adam steps (d_fake_g runs on the updated D).  masks / z32:
    {"G": [per ReLU: [mask]], "D": [per LeakyReLU: [real rows, fake rows, the G step's rows]]}, NCHW, as _Act takes them.  The result
    carries the _Act modules under "acts"."""
    x, y, target = batch(RS, B)
    G, D = RS.seeded_nets(dtype)
    acts = {n: install_acts(net, masks[n] if masks else None, z32[n] if z32 else None, keep) for n, net in (("G", G), ("D", D))}
    res = RS.iteration(G, D, RS.classifier_state(dtype), *RS.make_optimizers(G, D), x.to(dtype), y, target, pins=pins)
    res["acts"] = acts
    return res


def reference(RS, pins, masks, B=B_TRAIN):
    """What the GPU tests at batch B compare with: "f64" the float64 iteration with the classifier routing pinned to `pins` and the
    nets' activation masks to `masks` (the run under test's); "f32" the float32 iteration, the yardstick (.dist = |f32 - f64|), its
    classifier unpinned and its activation masks the same `masks`, so that the distance is fp32 arithmetic's and not a flipped unit's;
    "routing" from the unpinned classifier forwards of the two on their own x_cf; "masks" {net: [per layer: [a mask_report per
    call]]}; and "seconds", the wall time of all of it."""
    t0 = time.perf_counter()
    with cpu_threads():
        f32 = iteration(RS, torch.float32, None, masks, None, True, B)
        z32 = {n: [a.seen for a in acts] for n, acts in f32.pop("acts").items()}
        f64 = iteration(RS, torch.float64, pins, masks, z32, False, B)
        reports = {n: [a.reports for a in acts] for n, acts in f64.pop("acts").items()}
        del z32
        with torch.no_grad():
            clf64 = PR.forward(RS.classifier_state(torch.float64), f64["x_cf"])
            clf32 = PR.forward(RS.classifier_state(torch.float32), f32["x_cf"])
        route = routing(clf32, clf64)
    return {"f64": f64, "f32": f32, "routing": route, "masks": reports, "cls_logits_unpinned": clf64["logits"],
            "seconds": time.perf_counter() - t0}


def dist(ref, name, net=None):
    """|float32 restatement - float64 restatement| of a loss, a forward tensor or (net "G" / "D") a parameter gradient."""
    a, b = (ref["f32"][name], ref["f64"][name]) if net is None else (ref["f32"][f"grad_{net}"][name], ref["f64"][f"grad_{net}"][name])
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
