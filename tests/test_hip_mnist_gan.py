"""GPU: the MNIST MLP GAN port (pcgan_amd.mnist_gan on csrc/dense_rows.hip) against the float64 restatement of the reference's loop
body (tests/mnist_gan_restate.py, torch.float64 on the CPU) and against the run recorded from the reference's own code
(tests/golden/mnist_gan_ref.npz): six iterations, five batches of 64 rows and the 32-row tail.

Bounds.  The yardstick of every quantity is the distance between the reference's fp32 CPU computation and the float64 restatement of
the same quantity, measured in the test run itself; the HIP result has to stay within max(FLOOR, 3 x yardstick) of float64 (3: another
summation order may land anywhere in the same noise).  Against the recorded run the yardstick is added once more (triangle
inequality).  The bound never looks at the HIP result.
  FLOOR = 4e-6 relative L2, the floor of tests/test_hip_dense_rows.py: the fp32 matrix instruction is a k-ordered fmaf chain with an
    error of about 1.5e-7 * sum|a b|, up to 3.1e-6 of a zero-mean column at K = 1024, where the CPU's blocked GEMM carries less.
  LeakyReLU kinks get no floor: the float64 reference is told which side the run under test took, for near-zero pre-activations
    only.  A pre-activation within fp32 rounding of zero lands on either side of the kink depending on the summation order; both are
    correct fp32 results, the unit's derivative is 1 on one side and 0.2 on the other, and everything below it inherits the
    difference (about 0.8 / sqrt(rows x width) of the layer's gradient: 1e-2 here, where a floor that wide would hide a wrong
    kernel).  `train_step(record=...)` hands out the hidden activations of its three passes; mnist_gan_restate.KinkLeaky takes
    their signs and follows them where |x| < 4e-6 x rms(x) (the FLOOR argument: that is the rounding error a column can carry) and
    nowhere else.  The float64 run and the fp32 yardstick run are both told; a third float64 run is left alone, and the exactly
    known distance between the two float64 runs is added to the bound of the comparison with the recorded run, which took its own
    sides.  In a run of six iterations 5 to 10 of 1.3 M pre-activations are that near, and this fixture has two where runs differ:
      * iteration 0, D's second layer inside the G step, |x| = 1.0e-9 in float64: the op chain lands on the other side than
        float64, torch fp32 and the fused kernels.  Without the kink-aware reference its G model.0.weight gradient stood 1.706e-2
        from float64 (grad-input at that layer 9.4e-3, forward activations of the two paths within 8e-7); with it, 1.2e-6 at most.
      * iteration 5 (the 32-row tail), one unit of G's first layer: the GPU (both paths) and torch fp32 on several threads land on
        one side, float64 and the recorded single-thread run on the other (6.94e-3 on G model.0.weight's gradient).
    The yardstick of the recorded comparison is the larger of the recorded run's distance from float64 (taken on a digest for the
    large tensors, which can miss a row) and the full-tensor fp32 distance.
  Losses: max(2 ulp of fp32 at the loss's magnitude = 1.2e-7, 3 x yardstick).
  D model.4.bias has ONE element, a cancelling sum over the 2n rows: its floor is sqrt(2n) u sum|dz_r| / |g| (see the loop).
  Maximum-norm figures of the gradients are bounded relative to the tensor's largest entry with the same rule.  For the post-Adam
    weights the maximum norm is printed and NOT asserted; only their relative L2 is.  The first version of this test asserted it with
    the GEMM floor and that was a mistake of the test: Adam's first step is lr g / (|g| + 1e-8), so an element whose gradient is within
    a few 1e-8 of zero turns a rounding difference of 1e-12 in g into 5e-9 in the weight, 2.5e-5 of lr.  The GEMM floor says nothing
    about that quotient.  Measured on the first GPU run, G model.3.bias (initialised to 0, every entry +-lr after one step): rel-max
    5.5e-6 on the GPU, 1.0e-6 for the reference's own fp32 run, relative L2 3.9e-7 and 1.7e-7.
  The six gradient-free tensors (asserted by name below): G model.2/5/8.bias have an exactly zero gradient (BatchNorm subtracts the
    mean), so fp32 leaves rounding noise that Adam normalises into steps of up to 3.2 lr each (tests/test_hip_moons_cf.py); the
    running means of model.3/6/9 contain those biases.  After n steps they are compared with n * 3.2 * lr absolute.  Their gradients
    must stay below 1e-6 of the same layer's weight-gradient norm (column sums of dz, whose rounding noise is u R |dz|).

Measured distances on this fixture (GPU runs, printed by -s), relative L2 unless noted, all six iterations:
  | quantity                                          | fp32 CPU vs float64 | fused vs float64  | op chain vs float64 |
  | gradients (all but D model.4.bias)                | 6.5e-8 .. 8.1e-7    | 8.5e-8 .. 1.0e-6  | 3.0e-8 .. 1.2e-6    |
  | D model.4.bias gradient (one element)             | 7.8e-8 .. 1.2e-5    | 3.9e-9 .. 5.3e-5  | 6.1e-7 .. 1.0e-4    |
  | post-Adam weights                                 | 3.8e-9 .. 3.8e-6    | 3.8e-9 .. 7.3e-6  | 3.8e-9 .. 6.4e-6    |
  | BatchNorm running_var                             | 3.2e-8 .. 1.8e-7    | 3.2e-8 .. 1.8e-7  | 3.2e-8 .. 1.8e-7    |
  | losses (absolute)                                 | 9e-9 .. 8.4e-8      | 9e-9 .. 7.7e-8    | <= 7.7e-8           |
  | gradient-free biases after 6 iterations (max abs) | 5.2e-7 .. 5.6e-6    | 8.7e-7 .. 1.1e-5  | 5.1e-7 .. 3.7e-6    |
  | running means that contain them (max abs)         |                     | 1.5e-7 .. 2.6e-6  | 1.1e-7 .. 1.1e-6    |
  | gradient of a gradient-free bias (max abs)        | 1.3e-10 (f64 6e-19) | 3.2e-10           | 1.2e-10             |
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mnist_gan_restate as RS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 4e-6
LOSS_FLOOR = 1.2e-7
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mnist_gan_ref.npz")
LOOSE = {"model.2.bias", "model.5.bias", "model.8.bias", "model.3.running_mean", "model.6.running_mean", "model.9.running_mean"}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def M():
    import pcgan_amd
    from pcgan_amd import mnist_gan
    pcgan_amd.load()
    return mnist_gan


def _hip_nets(M, src_G, src_D, fused=True):
    G, D = M.Generator(), M.Discriminator()
    G.load_state_dict({k: v.float() for k, v in src_G.state_dict().items()})
    D.load_state_dict({k: v.float() for k, v in src_D.state_dict().items()})
    G.to(DEV); D.to(DEV)
    G.use_fused = D.use_fused = fused
    return G, D


def _cmp(what, hip, t64, t32, gold_entry=None, FLOOR=FLOOR, assert_max=True, t_nat=None):
    """relative L2 and relative max-norm of hip against float64, bounded by the fp32-CPU yardstick; then against the recorded run."""
    h, a, b = RS.np64(hip), RS.np64(t64), RS.np64(t32)
    den2, deni = max(np.linalg.norm(a), 1e-300), max(np.abs(a).max(), 1e-300)
    l2, y2 = np.linalg.norm(h - a) / den2, np.linalg.norm(b - a) / den2
    mx, ym = np.abs(h - a).max() / deni, np.abs(b - a).max() / deni
    print(f"{what}: rel-L2 hip {l2:.2e} fp32 {y2:.2e} | rel-max hip {mx:.2e} fp32 {ym:.2e}")
    assert np.isfinite(l2) and l2 <= max(FLOOR, 3 * y2), f"{what}: rel-L2 {l2:.3e} > max({FLOOR}, 3 x {y2:.3e})"
    if assert_max:
        assert mx <= max(FLOOR, 3 * ym), f"{what}: rel-max {mx:.3e} > max({FLOOR}, 3 x {ym:.3e})"
    if gold_entry is not None:
        g, dig = gold_entry
        hh, aa = (RS.digest(h)[1:], RS.digest(a)[1:]) if dig else (h.ravel(), a.ravel())
        # the yardstick of the recorded comparison is the larger of the recorded run's own distance from float64 and this run's
        # full-tensor fp32-vs-float64 distance y2: a digest (norm + 64 samples) cannot measure the distance of a whole tensor
        yg = max(RS.rel_l2(g.ravel() if not dig else g[1:], aa), y2)
        dg = RS.rel_l2(hh, g.ravel() if not dig else g[1:])
        # the recorded run took its own sides at the kinks: where the run under test took others, the float64 reference that follows
        # it (t64) has moved away from the natural float64 run (t_nat) by a distance known exactly, and the recorded run stays there
        moved = RS.rel_l2(a, RS.np64(t_nat)) if t_nat is not None else 0.0
        assert dg <= max(FLOOR, 3 * yg) + yg + moved, f"{what} against the recorded run: {dg:.3e} (yardstick {yg:.3e}, kinks {moved:.3e})"


def _gold_entry(gold, key):
    if key in gold:
        return gold[key].astype(np.float64), False
    return gold[key + "#digest"], True


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op-chain"])
def test_train_step_against_float64_and_the_recorded_run(M, gold, fused):
    """Six iterations from the recorded initialisation: batch 64 five times, then the 32-row tail.  fused and use_fused=False both
    stay within the same bounds of float64, which is the sense in which they are equivalent.  The HIP step runs first: the
    restatements are then told its near-kink LeakyReLU decisions (module docstring)."""
    G64, D64 = RS.build(torch.float64); og64, od64 = RS.optimizers(G64, D64)      # float64, told the run's near-kink decisions
    G32, D32 = RS.build(torch.float32); og32, od32 = RS.optimizers(G32, D32)      # fp32 CPU, told the same: the yardstick
    GN, DN = RS.build(torch.float64); ogN, odN = RS.optimizers(GN, DN)            # float64 left alone: where the recorded run stays
    for tag, net in (("G", G32), ("D", D32)):
        for k, v in net.state_dict().items():
            assert np.array_equal(RS.digest(v), gold[f"init.{tag}.{k}#digest"]), f"initialisation of {tag}.{k} differs from the recorded run's"
    G, D = _hip_nets(M, G32, D32, fused)
    og, od = M.make_optimizers(G, D)
    loose_seen = set()
    for it, n in enumerate(RS.SIZES):
        real, z = RS.normalize_u8(gold[f"real_u8.{it}"]), gold[f"z.{it}"]
        rec = {}
        gl, dl = M.train_step(G, D, og, od, torch.from_numpy(real).to(DEV).view(n, 1, 28, 28), torch.from_numpy(z).to(DEV), record=rec)
        pos = lambda ts, rows=slice(None): [(t[rows] > 0).cpu() for t in ts]
        sides = {"g": pos(rec["g_acts"]), "d_fake_g": pos(rec["d_acts_g_step"]), "d_real": pos(rec["d_acts_d_step"], slice(0, n)),
                 "d_fake": pos(rec["d_acts_d_step"], slice(n, 2 * n))}
        o64 = RS.step(G64, D64, og64, od64, torch.from_numpy(real).double(), torch.from_numpy(z).double(), keep_grads=True, sides=sides)
        o32 = RS.step(G32, D32, og32, od32, torch.from_numpy(real), torch.from_numpy(z), keep_grads=True, sides=sides)
        oN = RS.step(GN, DN, ogN, odN, torch.from_numpy(real).double(), torch.from_numpy(z).double(), keep_grads=True)
        kinks = {t: (sum(m.near for m in RS.leakies(a) + RS.leakies(b)), sum(m.changed for m in RS.leakies(a) + RS.leakies(b)))
                 for t, a, b in (("f64", G64, D64), ("fp32", G32, D32))}
        print(f"it{it} near-kink pre-activations so far (near, moved to the run's side): {kinks}")
        for name, got in (("g_loss", gl.item()), ("d_loss", dl.item())):
            yard = abs(o32[name] - o64[name])
            print(f"it{it} {name}: hip {got:.9f} f64 {o64[name]:.9f} fp32 {o32[name]:.9f} recorded {float(gold[f'it{it}.{name}']):.9f}")
            assert abs(got - o64[name]) <= max(LOSS_FLOOR, 3 * yard), f"it{it} {name}"
            assert abs(got - float(gold[f"it{it}.{name}"])) <= max(LOSS_FLOOR, 3 * yard) + abs(float(gold[f"it{it}.{name}"]) - oN[name]) + abs(o64[name] - oN[name])
        for tag, net, n64, n32, nN, gk in (("G", G, G64, G32, GN, "g_grads"), ("D", D, D64, D32, DN, "d_grads")):
            p64, p32, pN = dict(n64.named_parameters()), dict(n32.named_parameters()), dict(nN.named_parameters())
            for k, p in net.named_parameters():
                if tag == "G" and k in RS.GRADIENT_FREE:
                    loose_seen.add(k)
                    wk = k.replace("bias", "weight")
                    gb = float(p.grad.abs().max().item())
                    lim = 1e-6 * float(np.linalg.norm(RS.np64(o64[gk][wk])))
                    print(f"it{it} G grad {k}: max |g| hip {gb:.2e} (fp32 {float(o32[gk][k].abs().max()):.2e}, f64 {float(o64[gk][k].abs().max()):.2e}) limit {lim:.2e}")
                    assert gb <= lim, f"it{it} gradient-free {k}: {gb:.3e}"
                    d = float(np.abs(RS.np64(p) - RS.np64(p64[k])).max())
                    print(f"it{it} G {k}: max |hip - f64| {d:.2e}, fp32 {float(np.abs(RS.np64(p32[k]) - RS.np64(p64[k])).max()):.2e}, bound {(it + 1) * 3.2 * RS.LR:.2e}")
                    assert d <= (it + 1) * 3.2 * RS.LR
                    continue
                floor = FLOOR
                if tag == "D" and k == "model.4.bias":
                    # ONE element: the sum over 2n rows of dz_r = (p_r - t_r) / 2n, real rows negative, generated rows positive.  Its
                    # rounding error is relative to S = sum |dz_r|, not to the cancelled sum g, and a one-element tensor has no
                    # averaging over elements, so "3 x one fp32 draw" is no yardstick: floor sqrt(2n) u S / |g| (u = 2^-24; the rigorous
                    # bound of a recursive sum is (2n - 1) u S, sqrt(2n) is its random-walk size).
                    S = float(((1.0 - o64["d_real"]).abs().sum() + o64["d_fake"].abs().sum()) / (2 * n))
                    floor = max(FLOOR, (2 * n) ** 0.5 * 2.0 ** -24 * S / abs(float(o64[gk][k])))
                _cmp(f"it{it} {tag} grad {k}", p.grad, o64[gk][k], o32[gk][k], _gold_entry(gold, f"it{it}.{tag}.grad.{k}"), FLOOR=floor,
                     t_nat=oN[gk][k])
                _cmp(f"it{it} {tag} weight {k}", p, p64[k], p32[k], _gold_entry(gold, f"it{it}.{tag}.{k}"), assert_max=False, t_nat=pN[k])
            b64, b32, bN = dict(n64.named_buffers()), dict(n32.named_buffers()), dict(nN.named_buffers())
            for k, b in net.named_buffers():
                if k.endswith("num_batches_tracked"):
                    assert int(b.item()) == it + 1 == int(gold[f"it{it}.{tag}.{k}"])
                elif k in RS.INHERITS_GRADIENT_FREE:
                    loose_seen.add(k)
                    d = float(np.abs(RS.np64(b) - RS.np64(b64[k])).max())
                    print(f"it{it} G {k}: max |hip - f64| {d:.2e}, bound {(it + 1) * 3.2 * RS.LR:.2e}")
                    assert d <= (it + 1) * 3.2 * RS.LR
                else:
                    _cmp(f"it{it} {tag} buffer {k}", b, b64[k], b32[k], _gold_entry(gold, f"it{it}.{tag}.{k}"), t_nat=bN[k])
    assert loose_seen == LOOSE, "exactly these six tensors are compared with the Adam-step bound"
    # D's outputs and the generated batch of the last iteration (forward of the state after five steps)
    ws = G._step_ws[next(iter(k for k in G._step_ws if k[0] == RS.SIZES[-1]))]
    R = RS.SIZES[-1]
    _cmp("last generated batch", ws.X[R:], o64["fake"], o32["fake"], (gold["last.fake"].astype(np.float64), False), t_nat=oN["fake"])
    if fused:
        _cmp("last D(real)", ws.d_acts[-1][:R], o64["d_real"], o32["d_real"], (gold[f"it{len(RS.SIZES) - 1}.d_real"].astype(np.float64), False),
             t_nat=oN["d_real"])
        _cmp("last D(fake), computed in the G step", ws.d_acts[-1][R:], o64["d_fake_g"], o32["d_fake_g"],
             (gold[f"it{len(RS.SIZES) - 1}.d_fake_g"].astype(np.float64), False), t_nat=oN["d_fake_g"])
        assert np.array_equal(gold[f"it{len(RS.SIZES) - 1}.d_fake_g"], gold[f"it{len(RS.SIZES) - 1}.d_fake"]), \
            "the reference's two D(fake) passes are bit-identical: the skipped recomputation loses nothing"


def test_graph_replay_equals_eager_launches_bitwise(M):
    from pcgan_amd.nn import GraphedStep
    data = RS.inputs()[:3]
    outs = []
    for graphed in (False, True):
        G32, D32 = RS.build(torch.float32)
        G, D = _hip_nets(M, G32, D32)
        og, od = M.make_optimizers(G, D)
        real0, z0 = torch.from_numpy(data[0][0]).to(DEV), torch.from_numpy(data[0][1]).to(DEV)
        losses = []
        if graphed:
            sr, sz = real0.clone(), z0.clone()
            gs = GraphedStep(lambda: M.train_step(G, D, og, od, sr, sz), {"real": sr, "z": sz}, [G, D], [og, od])
        for real, z in data:
            real, z = torch.from_numpy(real).to(DEV), torch.from_numpy(z).to(DEV)
            if graphed:
                gs.load(real=real, z=z)
                gl, dl = gs.replay()
            else:
                gl, dl = M.train_step(G, D, og, od, real, z)
            losses.append((gl.clone(), dl.clone()))
        torch.cuda.synchronize()
        outs.append((G.flat_params.clone(), D.flat_params.clone(), [b.clone() for b in G.buffers()], losses))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(outs[0][3], outs[1][3]))


def test_train_step_is_bitwise_repeatable(M):
    data = RS.inputs()[:2]
    outs = []
    for _ in range(2):
        G32, D32 = RS.build(torch.float32)
        G, D = _hip_nets(M, G32, D32)
        og, od = M.make_optimizers(G, D)
        for real, z in data:
            M.train_step(G, D, og, od, torch.from_numpy(real).to(DEV), torch.from_numpy(z).to(DEV))
        outs.append((G.flat_params.clone(), D.flat_params.clone(), G.flat_grads.clone(), D.flat_grads.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_evaluation_mode_sampling_from_a_loaded_checkpoint(M):
    """A checkpoint with non-trivial running statistics (three float64 training iterations), loaded into the HIP generator."""
    G64, D64 = RS.build(torch.float64); og, od = RS.optimizers(G64, D64)
    for real, z in RS.inputs()[:3]:
        RS.step(G64, D64, og, od, torch.from_numpy(real).double(), torch.from_numpy(z).double())
    G32, _ = RS.build(torch.float32)
    G32.load_state_dict({k: v.float() for k, v in G64.state_dict().items()})
    G, _ = _hip_nets(M, G32, RS.build(torch.float32)[1])
    z = torch.from_numpy(np.random.RandomState(5).normal(0, 1, (25, RS.LATENT)).astype(np.float32))
    G64r, _ = RS.build(torch.float64)
    G64r.load_state_dict({k: v.double() for k, v in G32.state_dict().items()})      # float64 arithmetic on the fp32 checkpoint
    G64r.eval(); G32.eval()
    before = {k: v.clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        want64, want32 = G64r(z.double()), G32(z)
    got = M.sample(G, z.to(DEV))
    assert got.shape == (25, 1, 28, 28) and G.training
    _cmp("evaluation-mode samples", got.view(25, -1), want64, want32)
    for k, v in G.state_dict().items():
        assert torch.equal(v, before[k]), f"sampling changed {k}"


def test_short_train_run_with_the_draws_hook_visits_a_tail_batch(M):
    from pcgan_amd.data import DeviceLoader
    rs = np.random.RandomState(3)
    n, seed = 64 * 2 + 32, 11
    images = RS.normalize_u8(rs.randint(0, 256, (n, RS.IMG)).astype(np.uint8))
    zs = {(e, i): rs.normal(0, 1, (r, RS.LATENT)) for e in (1, 2) for i, r in enumerate((64, 64, 32))}
    seen = []

    def draws(epoch, i, rows):
        seen.append((epoch, i, rows))
        return zs[(epoch, i)]                      # float64 host array, as np.random.normal returns it (:122)

    G32, D32 = RS.build(torch.float32)
    G64, D64 = RS.build(torch.float64); og64, od64 = RS.optimizers(G64, D64)
    og32, od32 = RS.optimizers(G32, D32)
    G, D = _hip_nets(M, G32, D32)
    x = torch.from_numpy(images).to(DEV).view(n, 1, 28, 28)
    loader = DeviceLoader(x, torch.zeros(n, device=DEV), 64, shuffle=True, seed=seed)
    losses = M.train(G, D, loader, epochs=2, draws=draws)
    assert seen == [(e, i, r) for e in (1, 2) for i, r in enumerate((64, 64, 32))] and len(losses) == 2
    gen = torch.Generator(device="cpu"); gen.manual_seed(seed)      # DeviceLoader's permutation stream
    for e in (1, 2):
        order = torch.randperm(n, generator=gen).numpy()
        for i, lo in enumerate(range(0, n, 64)):
            real = images[order[lo:lo + 64]]
            z32 = zs[(e, i)].astype(np.float32)
            o64 = RS.step(G64, D64, og64, od64, torch.from_numpy(real).double(), torch.from_numpy(z32).double())
            o32 = RS.step(G32, D32, og32, od32, torch.from_numpy(real), torch.from_numpy(z32))
        for j, name in enumerate(("g_loss", "d_loss")):
            print(f"epoch {e} {name}: hip {losses[e - 1][j]:.9f} f64 {o64[name]:.9f} fp32 {o32[name]:.9f}")
            assert abs(losses[e - 1][j] - o64[name]) <= max(LOSS_FLOOR, 3 * abs(o32[name] - o64[name]))
    for (k, p), (_, q), (_, r) in zip(D.named_parameters(), D64.named_parameters(), D32.named_parameters()):
        _cmp(f"after 6 iterations of train(): D {k}", p, q, r)
    with pytest.raises(Exception, match="2 <= batch <= 64"):
        M.train_step(G, D, None, None, torch.zeros(65, 784, device=DEV), torch.zeros(65, 100, device=DEV))


def test_memory_is_flat_over_an_epoch_of_iterations(M):
    """938 iterations (60000 / 64, rounded up) of the eager-launch step, the last one the tail batch's size: the allocator's
    footprint after a warm-up does not grow."""
    G32, D32 = RS.build(torch.float32)
    G, D = _hip_nets(M, G32, D32)
    og, od = M.make_optimizers(G, D)
    real = torch.rand(64, 784, device=DEV) * 2 - 1
    z = torch.randn(64, 100, device=DEV)
    for r in (64, 32):
        for _ in range(5):
            M.train_step(G, D, og, od, real[:r], z[:r])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i in range(938):
        r = 32 if i == 937 else 64
        M.train_step(G, D, og, od, real[:r], z[:r])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    assert bool(torch.isfinite(G.flat_params).all()) and bool(torch.isfinite(D.flat_params).all())
