"""GPU: step 1 of both MNIST CounteRGAN ports (pcgan_amd.gan_train; pcgan_amd.countergan2, §3.21) at the batch they
train and are timed at, 128, through the op chain, the fused entries run eagerly, and one graph replay -- where tests/test_hip_delta_gan.py
and tests/test_hip_countergan2.py stop at 4.  At 128 the convolutions take other plans, the head backward runs 16 rows per wave
(D pass, R = 256) and 8 (G pass), pcg_prob_head_fwd takes its default slab counts, and the classifier guidance, the embedding-table
gradients and the workspaces run at sizes nothing else compares with anything.

The reference is live (tests/delta_train_batch_ref.py), once per port: the float64 restatement's iteration on batches(128)[0] with the
classifier routing pinned to the GPU's, the float32 restatement's, its classifier unpinned, as the yardstick, and the unpinned float64
classifier forward for the routing check.  The rule is tests/test_hip_delta_gan.py's `_rule` -- (a) rtol 1e-4, atol 2e-5 *
max|float64|, or (b) 3x the distance of the float32 restatement from the float64 one, here taken from the two live runs.  A tail
batch of 96 rows (60000 % 128; R = 192 and 96 for the heads) follows a full one through the graphed stepper, replay against eager
entries.

Both restatements are pinned to the GPU's ReLU / LeakyReLU masks as well.  At this batch a layer has 1 to 6 million units and a few
float64 pre-activations lie within fp32 rounding of zero; the derivative jumps there as the max-pool's routing jumps at a tie.  Without
the pins the gradients miss the rule for that reason alone: the GPU is on the other side of zero than float64 on 2 units of gan_train's
last ReLU of G (z64 = 4.6e-8 and -5.9e-8), which moves G's gradients below it by 1.2e-4 ... 4.5e-4 * max|g|, and on 1 unit of
countergan2's second LeakyReLU of D (3.1e-5 * max|g| on net.2.weight); the CPU's own float32 run happens to flip none.  The masks are
checked where they decide (test_gpu_activation_masks_...), as the routing is.

Helpers (`_nets`, `_params`, `_step1`, `_rule`) are the two files' own, imported.

Measured (MI355X, these seeds): every loss uses at most 0.003 of rule (a)'s atol, every forward tensor at most 0.08 (gan_train's
d_fake), every parameter gradient at most 0.59 through the op chain (gan_train D net.7.bias; 0.05 for countergan2) and 0.03 / 0.01
through the fused step; rule (b) decided nowhere.  Under the routing bound: gan_train 74 of 713727 live windows (pool 1) and 135 of
249143 (pool 2), countergan2 81 of 711228 and 124 of 250160.  Under the activation bound: at most 0.03 % of a layer's units before
Adam(D), at most 0.33 % in D's pass of the G step.  The op chain's masks equal the fused step's, so one reference serves a port: 1.5 s
(gan_train) and 2.8 s (countergan2) for the float32 and float64 iterations on 16 threads; the 22 cases take 9 s."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countergan2_restate as CR  # noqa: E402
import delta_gan_restate as RS  # noqa: E402
import delta_train_batch_ref as TB  # noqa: E402
import pool_clf_restate as PR  # noqa: E402
import test_hip_countergan2 as TC  # noqa: E402
import test_hip_delta_gan as TD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = TB.B_TRAIN
PATHS = TD.PATHS
PORTS = {"gan_train": (TD, RS), "countergan2": (TC, CR)}
PORT = pytest.mark.parametrize("port", sorted(PORTS))


def _module(port):
    import pcgan_amd  # noqa: F401
    from pcgan_amd import countergan2, gan_train
    return {"gan_train": gan_train, "countergan2": countergan2}[port]


def _params(port, **kw):
    return TD._params(**kw) if port == "gan_train" else TC._params(_module(port), **kw)


def _step1(port, path):
    return PORTS[port][0]._step1(_module(port), B, path)


def _masks(port, path):
    """The activation masks of the GPU's own forwards in step 1 (post-activation > 0, what its backward kernels branch on), NCHW on the
    CPU, as delta_train_batch_ref.iteration takes them.  The kernels are deterministic and pick their plan from the geometry alone, so
    these forwards repeat the step's bit for bit: G from the seeded state; D from the seeded state on the real and the fake rows -- two
    passes of B rows in the op chain, one of 2B in the fused step -- and D after the step (Adam(D) done) on x_cf, as the G step ran it."""
    mod, rs = PORTS[port]
    r = _step1(port, path)
    G0, D0, _ = mod._nets(_module(port))
    D1 = r["nets"][1]
    for net in (G0, D0, D1):
        net._ensure_flat()                                                      # as their forward() does before it walks the layers
    x, y, t = (v.to(DEV) for v in TB.batch(rs))
    x_cf = r["fwd"]["x_cf"].to(DEV)
    on = lambda a: PR.nchw(a > 0).cpu()                                          # noqa: E731
    with torch.no_grad():
        layers = G0._run_forward(x, t)[2][0]
        g = [[on(layers[i + 1][1])] for i in range(len(layers) - 1)]
        if path == "chain":
            real, fake = (D0._run_forward(a, c)[1][0] for a, c in ((x, y), (x_cf, t)))
            d = [[on(lr[2]), on(lf[2])] for lr, lf in zip(real, fake)]
        else:
            both = D0._run_forward(torch.cat([x, x_cf]), torch.cat([y, t]))[1][0]
            d = [[on(l[2][:B]), on(l[2][B:])] for l in both]
        for calls, l in zip(d, D1._run_forward(x_cf, t)[1][0]):
            calls.append(on(l[2]))
    torch.cuda.synchronize()
    return {"G": g, "D": d}


def _same(a, b):
    return all(torch.equal(u, v) for n in a for la, lb in zip(a[n], b[n]) for u, v in zip(la, lb))


_refs = {}


@pytest.fixture(scope="module")
def ref():
    """(port, path) -> the live reference, pinned to the classifier routing and the activation masks of the GPU's run on that path;
    computed once per port and set of masks (eager and graph share theirs; the op chain's are the same unless a unit under the bound
    falls differently in D's pass of B rows)."""
    def get(port, path):
        key = (port, "chain" if path == "chain" else "fused")
        if key not in _refs:
            masks = _masks(port, path)
            other = _refs.get((port, "fused" if key[1] == "chain" else "chain"))
            if other is not None and _same(masks, other["gpu_masks"]):
                _refs[key] = other
            else:
                _refs[key] = TB.reference(PORTS[port][1], _step1(port, "eager")["pins"], masks)
                _refs[key]["gpu_masks"] = masks
                print(f"{port} {key[1]}: float64 and float32 iterations at batch {B} took {_refs[key]['seconds']:.1f} s on the CPU")
        return _refs[key]
    return get


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@PORT
def test_step_one_losses_and_forward_tensors(ref, port, path):
    """The five losses and delta, x_cf, d_real, d_fake, cls_logits of the untouched state, and for the fused paths the stepper's own
    buffers, d_fake_g (after Adam(D)) among them, by the rule."""
    mod, r, want = PORTS[port][0], _step1(port, path), ref(port, path)
    assert all(torch.equal(a, b) for a, b in zip(r["pins"], _step1(port, "eager")["pins"])), "the classifier's routing differs between two runs"
    for name in RS.LOSSES:
        mod._rule(r["losses"][name], want["f64"][name], TB.dist(want, name), f"{port} {path} {name}")
    for name in ("delta", "x_cf", "d_real", "d_fake", "cls_logits"):
        mod._rule(r["fwd"][name].numpy(), want["f64"][name].numpy(), TB.dist(want, name), f"{port} {path} {name}")
    # as the recorded batches have it: against the float64 run's own routing as well (it differs on the windows under the bound only)
    mod._rule(r["fwd"]["cls_logits"].numpy(), want["cls_logits_unpinned"].numpy(), TB.dist(want, "cls_logits"), f"{port} {path} cls_logits, unpinned")
    if path != "chain":
        for name in TB.FORWARD:
            mod._rule(r["fwd"]["step." + name].numpy(), want["f64"][name].numpy(), TB.dist(want, name), f"{port} {path} step {name}")
        assert torch.equal(r["fwd"]["step.x_cf"], r["fwd"]["x_cf"]) and torch.equal(r["fwd"]["step.delta"], r["fwd"]["delta"])


@PORT
def test_gpu_routing_is_the_float64_runs_where_it_decides(ref, port):
    """Where §3.18's gap bound max(1e-5, 100 * max|z32 - z64|) decides, the GPU's max-pool positions are the unpinned float64 run's; the
    share of live windows under the bound is at most 0.2 % (a condition on the batch, asserted without a GPU by
    tests/test_delta_train_batch_host.py)."""
    idx1, live1, idx2, live2, _ = _step1(port, "eager")["pins"]
    route = ref(port, "eager")["routing"]
    for layer, idx, livep in ((1, idx1, live1), (2, idx2, live2)):
        r = route[layer]
        print(f"{port} B {B} pool {layer}: {int(r['near'].sum())} of {int(r['live'].sum())} live windows under the bound {r['bound']:.1e}")
        assert r["near"].sum() / r["live"].sum() <= TB.NEAR_CAP
        pinned = r["live"] & ~r["near"]
        np.testing.assert_array_equal(idx.numpy()[pinned], r["idx"][pinned])
        assert livep.numpy()[pinned].all()


@pytest.mark.parametrize("path", ["chain", "eager"])
@PORT
def test_gpu_activation_masks_are_the_float64_runs_where_they_decide(ref, port, path):
    """The ReLU masks of G and the LeakyReLU masks of D that the float64 iteration is pinned to (delta_train_batch_ref): wherever
    |z64| is at least max(1e-5, 100 * max|z32 - z64|) the GPU's mask is z64 > 0, and at most 0.2 % of a layer's units lie under that
    bound -- 1 % for D in the G step, where Adam(D)'s sign noise on near-zero gradients separates the float32 and float64 runs."""
    for net, layers in ref(port, path)["masks"].items():
        for i, calls in enumerate(layers):
            for k, rep in enumerate(calls[:1] if net == "G" else calls):
                print(f"{port} {path} {net} activation {i} call {k}: {rep['flips']} of {rep['units']} units on the other side of zero than float64, "
                      f"{rep['near']} under the bound {rep['bound']:.1e}, {rep['wrong']} at or over it")
                assert rep["wrong"] == 0
                assert rep["near"] / rep["units"] <= (TB.NEAR_CAP_AFTER_ADAM if net == "D" and k == 2 else TB.NEAR_CAP)


@pytest.mark.parametrize("path", PATHS)
@PORT
def test_step_one_parameter_gradients_against_the_pinned_float64_restatement(ref, port, path):
    mod, rs, r, want = PORTS[port][0], PORTS[port][1], _step1(port, path), ref(port, path)
    for net, keys in (("G", rs.G_KEYS), ("D", rs.D_KEYS)):
        for k in keys:
            w64 = want["f64"][f"grad_{net}"][k].numpy()
            assert np.abs(w64).max() > 0 and np.abs(r[f"grad_{net}"][k].numpy()).max() > 0, (net, k)
            mod._rule(r[f"grad_{net}"][k].numpy(), w64, TB.dist(want, k, net), f"{port} {path} grad {net} {k}")


@PORT
def test_fused_and_graph_are_identical_and_the_op_chain_agrees(port):
    rs = PORTS[port][1]
    chain, fused, graph = (_step1(port, p) for p in PATHS)
    for net, keys in (("G", rs.G_KEYS), ("D", rs.D_KEYS)):
        for k in keys:
            a, b = chain[f"grad_{net}"][k].numpy(), fused[f"grad_{net}"][k].numpy()
            np.testing.assert_allclose(b, a, rtol=1e-4, atol=2e-5 * float(np.abs(a).max()), err_msg=f"{port} {net} {k}")
            assert torch.equal(fused[f"grad_{net}"][k], graph[f"grad_{net}"][k]), f"replay differs from the eager entries: {port} {net} {k}"
    assert fused["losses"] == graph["losses"]


# ---- the tail batch -----------------------------------------------------------------------------------------------------------------------------
def _run_loader(port, graph):
    T, mod = _module(port), PORTS[port][0]
    gen = torch.Generator().manual_seed(3)
    n = B + TB.B_TAIL
    x = (2 * torch.rand(n, 1, 28, 28, generator=gen) - 1).to(DEV)
    y = torch.randint(0, 10, (n,), generator=gen).to(DEV)
    G, D, C = mod._nets(T)
    stepper = T.GraphedTrainStep(G, D, C, B, _params(port), graph=graph)
    rec = []
    for i in (0, B):                                                             # one full batch, then the tail of 96
        out = stepper.step(x[i:i + B], y[i:i + B], torch.full_like(y[i:i + B], RS.TARGET_CLASS))
        rec.append(torch.cat([out[k] for k in RS.LOSSES]).clone())
    torch.cuda.synchronize()
    return G.flat_params.clone(), D.flat_params.clone(), torch.stack(rec).cpu(), stepper


@PORT
def test_replays_equal_the_eager_entries_bit_for_bit_with_the_tail_of_96(port):
    """128 rows, then 96: R = 192 (12 rows per wave of the head backward) and R = 96 (two slabs of pcg_prob_head_fwd).  No float64."""
    g1, d1, l1, s1 = _run_loader(port, True)
    g0, d0, l0, _ = _run_loader(port, False)
    assert sorted(s1._graphs) == [TB.B_TAIL, B], "one graph per batch size met: the full batch and the tail"
    assert torch.equal(l1, l0), (l1, l0)
    assert torch.equal(g1, g0) and torch.equal(d1, d0)
    assert bool(torch.isfinite(l1).all()) and l1.shape == (2, 5)
