"""GPU parity of the fused moons GAN / conditional GAN path (csrc/moons_gan.hip; pcgan_amd.moons.TrainSteps / train_gan,
pcgan_amd.moons_cgan): whole iterations in one launch against the reference's recorded runs and the float64 restatement
(tests/moons_gan_restate.py, pinned to the reference by tests/test_moons_gan_host.py, which also asserts the kink precondition
for every case used here).

Tolerances are the project's own for the same comparisons: against the reference's fp32 recordings tests/test_hip_moons.py's
(losses rtol 2e-5, weights rtol 1e-4 + atol 2e-5); against float64 DESIGN.md §3.8's (scalars 1e-5, state 1e-4 + 1e-6)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moons_gan_restate as RS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = RS.G_KEYS


def build(params, L):
    """Our modules with the given parameters on the GPU, and their optimizers."""
    from pcgan_amd import moons as M, moons_cgan as C
    H, gi = params["G"]["0.weight"].shape
    if L:
        G, D, pre = C.Generator(gi - L, L, H), C.Discriminator(L, H), "net."
    else:
        G, D, pre = M.build_generator(gi, H), M.build_discriminator(H), ""
    for net, tag in ((G, "G"), (D, "D")):
        net.load_state_dict({pre + k: torch.tensor(np.asarray(params[tag][k]), dtype=torch.float32) for k in KEYS})
        net.to(DEV)
    optG, optD = M.make_optimizers(G, D)
    return G, D, optG, optD, pre


def state(net, pre):
    sd = net.state_dict()
    return {k: sd[pre + k].detach().cpu().numpy() for k in KEYS}


def moments(runner, net, which, pre):
    """The optimizer's flat exp_avg / exp_avg_sq cut into the net's tensors."""
    seg = runner.sg if net is runner.G else runner.sd
    flat = seg[which].cpu().numpy()
    names = [n for n, _ in net.named_parameters()]
    return {n[len(pre):]: flat[off:off + cnt].reshape(tuple(p.shape)) for n, (p, off, cnt) in zip(names, net._seg)}


def close(a, b, rtol, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    print(f"{what}: max abs {err.max():.3e}, max |ref| {np.abs(b).max():.3e}, worst err/(atol+rtol|ref|) {(err / (atol + rtol * np.abs(b))).max():.3f}")
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def test_moons_ref_two_steps_one_launch(golden_dir):
    """The reference's own epoch of make_moons_gan.py (moons_ref.npz: 2 iterations of 50 rows) in ONE launch."""
    from pcgan_amd import moons as M
    gold = dict(np.load(os.path.join(golden_dir, "moons_ref.npz")))
    G, D, optG, optD, pre = build({t: {k: gold[f"init.{t}.{k}"] for k in KEYS} for t in "GD"}, 0)
    runner = M.TrainSteps(G, D, optG, optD, gold["X_shuffled"], batch_size=50)
    logs = runner.run(torch.arange(100).view(2, 50), torch.from_numpy(gold["z"]).view(2, 2, 50, 32)).cpu().numpy()
    assert runner.launches == 1
    close(sum(float(v) for v in logs[:, 0]), float(gold["loss_D_total"]), 2e-5, 0, "loss_D_total")
    close(sum(float(v) for v in logs[:, 1]), float(gold["loss_G_total"]), 2e-5, 0, "loss_G_total")
    for tag, net in (("G", G), ("D", D)):
        for k, v in state(net, pre).items():
            close(v, gold[f"final.{tag}.{k}"], 1e-4, 2e-5, f"{tag}.{k}")


def test_moons_cgan_ref_four_steps_one_launch(golden_dir):
    """The reference's own four iterations of make_moons_cgan.py (moons_cgan_ref.npz) in ONE launch: per-iteration losses, final
    weights, Adam moments and step counters."""
    from pcgan_amd import moons as M
    gold = dict(np.load(os.path.join(golden_dir, "moons_cgan_ref.npz")))
    G, D, optG, optD, pre = build({t: {k: gold[f"init.{t}.net.{k}"] for k in KEYS} for t in "GD"}, 2)
    runner = M.TrainSteps(G, D, optG, optD, gold["X"], gold["Y"], batch_size=RS.BATCH)
    n = RS.ITERS
    z = torch.from_numpy(np.stack([np.stack([gold[f"it{i}.z_d"], gold[f"it{i}.z_g"]]) for i in range(n)]))
    labels = torch.from_numpy(np.stack([np.stack([gold[f"it{i}.labels_d"], gold[f"it{i}.labels_g"]]) for i in range(n)]))
    logs = runner.run(torch.arange(n * RS.BATCH).view(n, RS.BATCH), z, labels).cpu().numpy()
    assert runner.launches == 1
    for i in range(n):
        close(logs[i, 0], gold[f"it{i}.loss_D"], 2e-5, 0, f"it{i}.loss_D")
        close(logs[i, 1], gold[f"it{i}.loss_G"], 2e-5, 0, f"it{i}.loss_G")
    for tag, net in (("G", G), ("D", D)):
        st, ea, es = state(net, pre), moments(runner, net, "exp_avg", pre), moments(runner, net, "exp_avg_sq", pre)
        for k in KEYS:
            close(st[k], gold[f"final.{tag}.net.{k}"], 1e-4, 2e-5, f"{tag}.{k}")
            close(ea[k], gold[f"it{n-1}.{tag}.exp_avg.net.{k}"], 1e-4, 1e-6, f"{tag}.exp_avg.{k}")
            close(es[k], gold[f"it{n-1}.{tag}.exp_avg_sq.net.{k}"], 1e-4, 1e-6, f"{tag}.exp_avg_sq.{k}")
    assert int(runner.sg["step"].item()) == n == int(gold[f"it{n-1}.G.step"]) and int(runner.sd["step"].item()) == n


@pytest.mark.parametrize("B,H,Z,L,seed", RS.STEP_CASES)
def test_single_step_vs_float64(B, H, Z, L, seed):
    """One iteration from a recorded state against the float64 oracle: both losses, every updated parameter, both Adam moments."""
    from pcgan_amd import moons as M
    case = RS.random_case(B, H, Z, L, seed)
    ref, outs = RS.run_case(case)
    G, D, optG, optD, pre = build(case["params"], L)
    runner = M.TrainSteps(G, D, optG, optD, case["X"], case["Y"] if L else None, batch_size=B)
    print(f"activation scratch: {runner.scratch_bytes} bytes")
    logs = runner.run(torch.from_numpy(case["rows"]), torch.from_numpy(case["z"]), torch.from_numpy(case["labels"]) if L else None).cpu().numpy()
    close(logs[0, 0], outs[0]["loss_D"], 1e-5, 0, "loss_D")
    close(logs[0, 1], outs[0]["loss_G"], 1e-5, 0, "loss_G")
    for tag, net in (("G", G), ("D", D)):
        st, ea, es = state(net, pre), moments(runner, net, "exp_avg", pre), moments(runner, net, "exp_avg_sq", pre)
        for k in KEYS:
            close(st[k], ref.p[tag][k].detach().numpy(), 1e-4, 1e-6, f"{tag}.{k}")
            close(ea[k], ref.m[tag][k].numpy(), 1e-4, 1e-6, f"{tag}.exp_avg.{k}")
            close(es[k], ref.v[tag][k].numpy(), 1e-4, 1e-6, f"{tag}.exp_avg_sq.{k}")


def _snapshot(runner):
    return [t.clone() for t in (runner.G.flat_params, runner.D.flat_params, runner.sg["exp_avg"], runner.sg["exp_avg_sq"], runner.sg["step"],
                                runner.sd["exp_avg"], runner.sd["exp_avg_sq"], runner.sd["step"])]


@pytest.mark.parametrize("B,H,Z,L,seed,n", RS.MULTI_CASES)
def test_n_steps_bit_identical_to_n_launches(B, H, Z, L, seed, n):
    from pcgan_amd import moons as M
    case = RS.random_case(B, H, Z, L, seed, iters=n)
    rows, z = torch.from_numpy(case["rows"]), torch.from_numpy(case["z"])
    labels = torch.from_numpy(case["labels"]) if L else None
    results = []
    for mode in ("one", "one", "each"):
        G, D, optG, optD, _ = build(case["params"], L)
        runner = M.TrainSteps(G, D, optG, optD, case["X"], case["Y"] if L else None, batch_size=B)
        if mode == "one":
            logs = runner.run(rows, z, labels)
        else:
            logs = torch.cat([runner.run(rows[i:i + 1], z[i:i + 1], labels[i:i + 1] if L else None) for i in range(n)])
            assert runner.launches == n
        results.append([logs.clone()] + _snapshot(runner))
    for other, what in ((results[1], "two identical runs"), (results[2], "n launches of one step")):
        for a, b in zip(results[0], other):
            assert torch.equal(a, b), what
    assert torch.isfinite(results[0][0]).all()


def test_eager_adam_continues_after_a_launch():
    """The kernel advances the optimizers' device step counters: an eager opt.step() with supplied gradients afterwards equals
    torch's Adam continued from the same state.  Both sides run one elementwise fp32 update per step: a few ulp apart (rtol 1e-5,
    and atol 1e-7 for parameters near 0, one fp32 ulp of the 1e-3 step)."""
    from pcgan_amd import moons as M
    B, H, Z, L, seed, n = RS.MULTI_CASES[0]
    case = RS.random_case(B, H, Z, L, seed, iters=n)
    G, D, optG, optD, pre = build(case["params"], L)
    runner = M.TrainSteps(G, D, optG, optD, case["X"], case["Y"], batch_size=B)
    runner.run(torch.from_numpy(case["rows"]), torch.from_numpy(case["z"]), torch.from_numpy(case["labels"]))
    g = torch.Generator().manual_seed(3)
    for net, opt, seg in ((G, optG, runner.sg), (D, optD, runner.sd)):
        ref_p = [p.detach().cpu().clone().requires_grad_(True) for p in net.parameters()]
        ref = torch.optim.Adam(ref_p, lr=1e-3)
        ea, es = seg["exp_avg"].cpu(), seg["exp_avg_sq"].cpu()
        for q, (p, off, cnt) in zip(ref_p, net._seg):
            ref.state[q] = {"step": torch.tensor(float(n)), "exp_avg": ea[off:off + cnt].view(p.shape).clone(),
                            "exp_avg_sq": es[off:off + cnt].view(p.shape).clone()}
        for _ in range(2):
            for q, p in zip(ref_p, net.parameters()):
                gr = torch.randn(p.shape, generator=g) * 0.01
                q.grad = gr.clone()
                p.grad.copy_(gr.to(DEV))
            opt.step(); ref.step()
        assert int(seg["step"].item()) == n + 2
        for q, (name, p) in zip(ref_p, net.named_parameters()):
            close(p.detach().cpu().numpy(), q.detach().numpy(), 1e-5, 1e-7, name)


@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("R", [1, 50, 2000, 20000])
def test_forward_vs_float64(R, L):
    from pcgan_amd import moons as M, moons_cgan as C
    H, Z = 128, 32
    params = RS.init_params(Z, L, H, 77)
    G, D, _, _, _ = build(params, L)
    ref = RS.Model(params)
    rs = np.random.RandomState(R + L)
    z, x = rs.normal(size=(R, Z)).astype(np.float32), rs.normal(size=(R, 2)).astype(np.float32)
    lab = rs.randint(0, max(L, 1), R)
    with torch.no_grad():
        if L:
            oh = C.one_hot_encode(torch.from_numpy(lab).to(DEV), L)
            assert torch.equal(oh.cpu(), torch.nn.functional.one_hot(torch.from_numpy(lab), L).float())
            g_out, d_out = G(torch.from_numpy(z).to(DEV), oh), D(torch.from_numpy(x).to(DEV), oh)
        else:
            g_out, d_out = M.gan_forward(G, 0, torch.from_numpy(z).to(DEV)), M.gan_forward(D, 1, torch.from_numpy(x).to(DEV))
            assert torch.equal(M.sample(G, R, z=torch.from_numpy(z).to(DEV)), g_out)
        want_g = ref.G(torch.from_numpy(z).double(), ref.onehot(lab) if L else None)
        want_d = ref.D(torch.from_numpy(x).double(), ref.onehot(lab) if L else None)
    assert g_out.shape == (R, 2) and d_out.shape == (R, 1)
    close(g_out.cpu().numpy(), want_g.numpy(), 1e-5, 1e-6, "G forward")
    close(d_out.cpu().numpy(), want_d.numpy(), 1e-5, 1e-6, "D forward")


def test_module_forward_refuses_autograd():
    from pcgan_amd import PcgError, moons_cgan as C
    G, D = C.Generator(32, 2, 128).to(DEV), C.Discriminator(2, 128).to(DEV)
    z, x = torch.randn(4, 32, device=DEV), torch.randn(4, 2, device=DEV)
    oh = C.one_hot_encode(torch.tensor([0, 1, 1, 0], device=DEV), 2)
    with pytest.raises(PcgError, match="no autograd"):
        G(z, oh)
    with pytest.raises(PcgError, match="no autograd"):
        D(x, oh)
    with torch.no_grad():
        s, lab = C.sample(G, 10)
        assert s.shape == (10, 2) and lab.shape == (10,) and torch.isfinite(s).all()
        assert torch.isfinite(D(s, C.one_hot_encode(lab, 2))).all()


def _hooked(L):
    """train_gan / moons_cgan.train with the draws and perm hooks against the oracle loop run with the same draws and row order."""
    from pcgan_amd import moons as M, moons_cgan as C
    case = RS.loop_case(L)
    ref, lD, lG, _ = RS.run_loop(case)
    G, D, optG, optD, pre = build(case["params"], L)
    cfg = {"n_samples": RS.LOOP_ROWS, "z_dim": RS.Z_DIM, "hidden_dim": RS.HIDDEN, "label_dim": L, "batch_size": RS.LOOP_BATCH, "lr": RS.LR,
           "epochs": RS.LOOP_EPOCHS}
    perm = lambda e: case["perms"][e]
    if L:
        draws = lambda e, b: (case["z"][e, b, 0], case["labels"][e, b, 0], case["z"][e, b, 1], case["labels"][e, b, 1])
        got = C.train(torch.from_numpy(case["X"]), torch.from_numpy(case["Y"]), G, D, cfg, draws=draws, perm=perm, verbose=False)
    else:
        X = case["X"].astype(np.float64)
        got = M.train_gan(X, G, D, cfg, draws=lambda e, b: (case["z"][e, b, 0], case["z"][e, b, 1]), perm=perm)
        want_X = case["X"].astype(np.float64)
        for p in case["perms"]:
            want_X = want_X[p]
        assert np.array_equal(X, want_X), "train_gan leaves the caller's X shuffled as the reference does (:56)"
    close(got[0], lD, 1e-5, 0, "loss_D_values")
    close(got[1], lG, 1e-5, 0, "loss_G_values")
    for tag, net in (("G", G), ("D", D)):
        for k, v in state(net, pre).items():
            close(v, ref.p[tag][k].detach().numpy(), 1e-4, 1e-6, f"{tag}.{k}")


def test_train_gan_hooked_vs_oracle_loop():
    _hooked(0)


def test_cgan_train_hooked_vs_oracle_loop():
    _hooked(2)


@pytest.mark.parametrize("L", [0, 2])
def test_train_device_draws(L, monkeypatch):
    """Device draws: finite, reproducible for a seed, different for another seed, one step launch (and one randn launch) per epoch."""
    from pcgan_amd import _lib, moons as M, moons_cgan as C
    case = RS.loop_case(L)
    cfg = {"n_samples": RS.LOOP_ROWS, "z_dim": RS.Z_DIM, "hidden_dim": RS.HIDDEN, "label_dim": L, "batch_size": RS.LOOP_BATCH, "lr": RS.LR,
           "epochs": RS.LOOP_EPOCHS}
    calls = []
    real_check = M.ops.check
    monkeypatch.setattr(M.ops, "check", lambda rc, what="": (calls.append(what), real_check(rc, what))[1])

    def run(seed):
        G, D, _, _, pre = build(case["params"], L)
        del calls[:]
        np.random.seed(0)
        if L:
            out = C.train(torch.from_numpy(case["X"]), torch.from_numpy(case["Y"]), G, D, cfg, seed=seed, verbose=False)
        else:
            out = M.train_gan(case["X"].astype(np.float64), G, D, cfg, seed=seed)
        return out, state(G, pre), list(calls)
    a, ga, ca = run(5)
    b, gb, _ = run(5)
    c, gc, _ = run(6)
    assert len(a[0]) == len(a[1]) == RS.LOOP_EPOCHS and np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert a == b and all(np.array_equal(ga[k], gb[k]) for k in KEYS), "same seed, same run"
    assert a != c and any(not np.array_equal(ga[k], gc[k]) for k in KEYS), "another seed, other draws"
    assert ca.count("pcg_moons_gan_train_steps") == RS.LOOP_EPOCHS and ca.count("pcg_randn") == RS.LOOP_EPOCHS
    assert ca.count("pcg_randint") == (RS.LOOP_EPOCHS if L else 0)


def test_out_of_range_rows_and_labels_refused_before_launch():
    from pcgan_amd import PcgError, moons as M
    case = RS.random_case(50, 128, 32, 2, 1)
    G, D, optG, optD, _ = build(case["params"], 2)
    runner = M.TrainSteps(G, D, optG, optD, case["X"], case["Y"], batch_size=50)
    before = _snapshot(runner)
    rows, z, labels = torch.from_numpy(case["rows"]), torch.from_numpy(case["z"]), torch.from_numpy(case["labels"])
    for bad_rows, bad_labels in ((rows.clone().index_fill_(1, torch.tensor([3]), case["X"].shape[0]), labels),
                                 (rows.clone().index_fill_(1, torch.tensor([0]), -1), labels),
                                 (rows, labels.clone().index_fill_(2, torch.tensor([7]), 2)),
                                 (rows, labels.clone().index_fill_(2, torch.tensor([7]), -1))):
        with pytest.raises(PcgError, match="must lie in"):
            runner.run(bad_rows, z, bad_labels)
    assert runner.launches == 0
    torch.cuda.synchronize()
    for a, b in zip(before, _snapshot(runner)):
        assert torch.equal(a, b)
    with pytest.raises(PcgError, match="values in"):
        M.TrainSteps(G, D, optG, optD, case["X"], np.full(case["X"].shape[0], 2), batch_size=50)
