"""GPU parity, CounteRGAN/mnist (conditional_counteRGAN/mnist): the drop-ins in pcgan_amd.countergan against
  (a) vectors produced by the reference's own modules and train_countergan (tests/golden/countergan_ref_b4.npz), and
  (b) the oracle restatement (oracle/countergan_ref.py) evaluated live in float64 (truth) and float32 (noise floor).
Embedding lookups / concatenation must be bit-exact; floating point within the tolerances stated in each assert."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import countergan_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import countergan  # noqa: F401
    return pcgan_amd


def _digest(t, nsamples=64):
    a = np.asarray(t.detach().cpu().numpy(), dtype=np.float64).ravel()
    idx = np.linspace(0, a.size - 1, num=min(nsamples, a.size)).astype(np.int64)
    return np.concatenate([[a.sum(), np.abs(a).sum(), (a * a).sum()], a[idx]])


def _build(pcg, seed=0):
    K = pcg.countergan
    refG, refD, refC = CR.build(seed=seed)
    G, D, C = K.ResidualGenerator(), K.Discriminator(), K.CNNClassifier()
    assert list(G.state_dict()) == list(refG.state_dict()) and list(D.state_dict()) == list(refD.state_dict())
    assert list(C.state_dict()) == list(refC.state_dict())
    G.load_state_dict(refG.state_dict()); D.load_state_dict(refD.state_dict()); C.load_state_dict(refC.state_dict())
    C.eval()
    for p in C.parameters():
        p.requires_grad = False
    return (G.to(DEV), D.to(DEV), C.to(DEV)), (refG, refD, refC)


def test_embedding_concat_is_bit_exact(pcg):
    ops = pcg.ops
    g = torch.Generator().manual_seed(0)
    B, HW, K = 37, 784, 10
    x = torch.randn(B, HW, generator=g); m = (torch.rand(B, HW, generator=g) > 0.5).float()
    table = torch.randn(K, HW, generator=g); idx = torch.randint(0, K, (B,), generator=g)
    out = ops.embed_concat_fwd(x.to(DEV), idx.to(DEV), table.to(DEV), m.to(DEV)).cpu()
    ref = torch.stack([x, table[idx], m], dim=-1)
    assert torch.equal(out, ref)
    out2 = ops.embed_concat_fwd(x.to(DEV), idx.to(DEV), table.to(DEV), None).cpu()
    assert torch.equal(out2, ref[..., :2].contiguous())
    # backward: scatter-add by index (fixed order) and channel-0 pass-through
    d = torch.randn(B, HW, 3, generator=g)
    dt = torch.ones(K, HW, device=DEV)
    dx = ops.embed_concat_bwd(d.to(DEV), idx.to(DEV), 3, K, dtable=dt, accumulate=True, need_dx=True)
    ref_t = torch.ones(K, HW).index_add_(0, idx, d[..., 1])
    np.testing.assert_allclose(dt.cpu().numpy(), ref_t.numpy(), rtol=1e-6, atol=1e-6)
    assert torch.equal(dx.cpu(), d[..., 0].contiguous())


def test_small_ops(pcg):
    ops = pcg.ops
    g = torch.Generator().manual_seed(1)
    n = 5000
    x = torch.rand(n, generator=g) * 2 - 1; r = torch.randn(n, generator=g) * 0.5; m = (torch.rand(n, generator=g) > 0.4).float()
    xd, rd, md = x.to(DEV), r.to(DEV), m.to(DEV)
    assert torch.equal(ops.clamp_add_fwd(xd, rd, -1.0, 1.0).cpu(), torch.clamp(x + r, -1.0, 1.0))
    dy = torch.randn(n, generator=g)
    inside = ((x + r) >= -1) & ((x + r) <= 1)
    assert torch.equal(ops.clamp_add_bwd(dy.to(DEV), xd, rd, -1.0, 1.0).cpu(), dy * inside)
    np.testing.assert_allclose(ops.abs_mean_fwd(rd, md, True).item(), (r * (1 - m)).abs().mean().item(), rtol=2e-6)
    np.testing.assert_allclose(ops.abs_mean_fwd(rd).item(), r.abs().mean().item(), rtol=2e-6)
    go = torch.tensor([0.7], device=DEV)
    da = ops.abs_mean_bwd(rd, md, True, go).cpu()
    np.testing.assert_allclose(da.numpy(), (0.7 * torch.sign(r * (1 - m)) * (1 - m) / n).numpy(), rtol=1e-6, atol=1e-12)
    raw, masked = ops.scale_mask_fwd(rd, md, 0.1)
    assert torch.equal(raw.cpu(), 0.1 * r) and torch.equal(masked.cpu(), 0.1 * r * m)
    a = torch.randn(6, 4, 256, generator=g)
    np.testing.assert_allclose(ops.avgpool_fwd(a.to(DEV), 6, 4, 256).cpu().numpy(), a.mean(1).numpy(), rtol=1e-6, atol=1e-7)
    z = torch.randn(33, 10, generator=g) * 3; t = torch.randint(0, 10, (33,), generator=g)
    zr = z.clone().requires_grad_(True)
    lr = torch.nn.functional.cross_entropy(zr, t); lr.backward()
    l, dz = ops.cross_entropy_fwd_bwd(z.to(DEV), t.to(DEV))
    np.testing.assert_allclose(l.item(), lr.item(), rtol=2e-6)
    np.testing.assert_allclose(dz.cpu().numpy(), zr.grad.numpy(), rtol=2e-5, atol=1e-8)


def test_golden_reference_forward_and_step(pcg, golden_dir):
    K = pcg.countergan
    gold = dict(np.load(os.path.join(golden_dir, "countergan_ref_b4.npz")))
    (G, D, C), _ = _build(pcg, seed=int(gold["meta.seed"]))
    x, y = torch.from_numpy(gold["in.x"]).to(DEV), torch.from_numpy(gold["in.y"]).to(DEV)
    t, m = torch.from_numpy(gold["in.target_y"]).to(DEV), torch.from_numpy(gold["in.mask"]).to(DEV)
    sdG, sdD = copy.deepcopy(G.state_dict()), copy.deepcopy(D.state_dict())
    with torch.no_grad():
        raw, masked = G(x, t, m)
        np.testing.assert_allclose(raw.cpu().numpy(), gold["fwd.raw"], rtol=1e-5, atol=2e-7)
        np.testing.assert_allclose(masked.cpu().numpy(), gold["fwd.masked"], rtol=1e-5, atol=2e-7)
        assert torch.equal(masked == 0, (raw == 0) | (m == 0))
        np.testing.assert_allclose(D(x, y).cpu().numpy(), gold["fwd.d_logits"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(C(x).cpu().numpy(), gold["fwd.c_logits"], rtol=1e-5, atol=2e-6)
    G.load_state_dict(sdG); D.load_state_dict(sdD)   # undo the BatchNorm running-stat update of the forward above

    opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
    ts, ms = torch.from_numpy(gold["step.target_y"]).to(DEV), torch.from_numpy(gold["step.mask"]).to(DEV)
    out = K.train_step(G, D, C, opt_g, opt_d, bce, ce, x, y, ts, ms, skip_dead_d_wgrad=False)
    log = str(gold["step.log"])
    # the reference prints its scalars with 3-6 decimals (trainer.py:135-137,145-147): compare to half a printed unit
    import re
    def logged(pat):
        return float(re.search(pat, log).group(1))
    d_real_p = torch.sigmoid(out["d_real_logits"]).mean().item(); d_fake_p = torch.sigmoid(out["d_fake_logits"]).mean().item()
    assert abs(d_real_p - logged(r"D\(real\)=([0-9.]+)")) <= 6e-4 and abs(d_fake_p - logged(r"D\(fake\)=([0-9.]+)")) <= 6e-4, log
    assert abs(out["g_adv"].item() - logged(r"g_adv=([0-9.]+)")) <= 6e-5 + 2e-5, log
    assert abs(out["g_cls"].item() - logged(r"g_cls=([0-9.]+)")) <= 6e-5 + 5e-5, log
    assert abs(out["reg_l1"].item() - logged(r"reg=([0-9.]+)")) <= 6e-7 + 1e-6, log
    assert abs(out["g_loss"].item() - logged(r"\| G: ([0-9.]+)")) <= 6e-5 + 1e-4, log
    assert abs(out["d_loss"].item() - logged(r", D: ([0-9.]+)")) <= 6e-5 + 5e-5, log
    for tag, net in (("G", G), ("D", D)):
        for n, p in net.named_parameters():
            # digest = 3 sums + 64 samples; sums of a gradient tensor cancel, so judge them against the abs-sum
            got, ref = _digest(p.grad), gold[f"grad.{tag}.{n}"]
            scale = max(ref[1] / max(p.numel(), 1), 1e-12)
            if ref[1] < 1e-6 * p.numel():
                # a conv bias in front of a BatchNorm has an exactly-zero gradient (BN removes the mean); what the
                # reference stores there is fp32 rounding noise (~1e-9): only require ours to be noise too
                assert got[1] < 1e-6 * p.numel(), f"grad {tag}.{n}: expected ~0, got abs-sum {got[1]:.2e}"
                continue
            np.testing.assert_allclose(got[1:3], ref[1:3], rtol=2e-4, err_msg=f"grad {tag}.{n} (abs-sum, sum-sq)")
            assert abs(got[0] - ref[0]) <= 2e-4 * ref[1] + 1e-9, f"grad {tag}.{n} sum"
            np.testing.assert_allclose(got[3:], ref[3:], rtol=2e-3, atol=20 * scale * 2e-4 + 1e-9, err_msg=f"grad {tag}.{n} samples")
        for k, v in net.state_dict().items():
            got, ref = _digest(v.float()), gold[f"final.{tag}.{k}"]
            np.testing.assert_allclose(got[3:], ref[3:], rtol=1e-4, atol=1.2e-4, err_msg=f"final {tag}.{k}")  # Adam: <= 2*lr


@pytest.mark.parametrize("batch", [16, 1024])
def test_step_vs_oracle_float64(pcg, batch):
    """One train_step (trainer.py:96-123) against the float64 and float32 oracle: every loss, every G and D gradient.  batch 1024 is
    BASELINE config 4's per-GPU shard (r04: the whole step at the bench size against the oracle, ~25 s of CPU work — the CPU
    baseline of scripts/bench_countergan.py shows one fp32 step takes ~7 s there): the three-per-CU 128x64 kernels, the 64x192
    weight gradient, the skip-add epilogues and the fused column sums composed end to end."""
    K = pcg.countergan
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    (G, D, C), (refG, refD, refC) = _build(pcg, seed=3)
    r64 = [copy.deepcopy(n).double() for n in (refG, refD, refC)]
    x, y, t, m = CR.synthetic_batch(batch, seed=5)
    o32 = CR.make_optimizers(refG, refD); o64 = CR.make_optimizers(r64[0], r64[1])
    ref = CR.countergan_step(refG, refD, refC, *o32, x, y, t, m)
    tru = CR.countergan_step(*r64, *o64, x.double(), y, t, m.double())
    opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
    # skip_dead_d_wgrad=False: D's .grad then holds what the oracle's autograd leaves there (D step + the G step's critic weight
    # gradients, trainer.py:111-122)
    out = K.train_step(G, D, C, opt_g, opt_d, bce, ce, x.to(DEV), y.to(DEV), t.to(DEV), m.to(DEV), skip_dead_d_wgrad=False)
    for name in ("d_loss", "g_adv", "g_cls", "reg_l1", "mask_pen", "g_loss"):
        tol = max(2e-5 * abs(tru[name]) + 1e-6, 3 * abs(ref[name] - tru[name]))
        assert abs(out[name].item() - tru[name]) <= tol, f"{name}: {out[name].item()} vs {tru[name]} (tol {tol:.1e})"
    for (n, p), (_, q), (_, w) in zip(G.named_parameters(), refG.named_parameters(), r64[0].named_parameters()):
        got, t64, r32 = (a.detach().cpu().double().numpy() for a in (p.grad, w.grad, q.grad))
        den = max(np.linalg.norm(t64), 1e-30)
        l2, l2r = np.linalg.norm(got - t64) / den, np.linalg.norm(r32 - t64) / den
        assert l2 <= max(1e-4, 3 * l2r), f"G grad {n}: rel-L2 {l2:.2e} (reference fp32 noise {l2r:.2e})"
    for (n, p), (_, q), (_, w) in zip(D.named_parameters(), refD.named_parameters(), r64[1].named_parameters()):
        got, t64, r32 = (a.detach().cpu().double().numpy() for a in (p.grad, w.grad, q.grad))
        den = max(np.linalg.norm(t64), 1e-30)
        l2, l2r = np.linalg.norm(got - t64) / den, np.linalg.norm(r32 - t64) / den
        # D's LeakyReLU(0.2) kinks: at batch 1024 some of the 6.4 M pre-activations per layer lie within rounding of zero, and two fp32
        # convolutions that sum in different orders disagree about one's sign — that element's gradient changes by 80 %, which is
        # ~0.8 / sqrt(pixels) / sqrt(channels) ~ 1-3e-4 of the layer's weight gradient (DESIGN.md §3.2 "the ReLU-kink noise floor";
        # measured r04: 1.2e-4 on main.4.weight with the oracle's own fp32 run at 8e-7, i.e. no flip there).  Floor: two flips.
        flip_floor = 5e-4 if batch >= 256 else 0.0
        assert l2 <= max(1e-4, 3 * l2r, flip_floor), f"D grad {n}: rel-L2 {l2:.2e} (reference fp32 noise {l2r:.2e})"


def test_device_batch_synthesis(pcg):
    """build_mask / randint / randn on the device: exact structure, uniform marginals, determinism."""
    ops = pcg.ops
    rng = ops.DeviceRNG(seed=1234)
    B = 4096
    m = rng.patch_mask(B, 28, 28, 7, 10, DEV).cpu()
    assert m.shape == (B, 1, 28, 28) and set(m.unique().tolist()) == {0.0, 1.0}
    patches = m.view(B, 4, 7, 4, 7)
    assert torch.equal(patches, patches[:, :, :1, :, :1].expand_as(patches))          # constant inside every 7x7 patch
    sel = patches[:, :, 0, :, 0].reshape(B, 16)
    assert torch.equal(sel.sum(1), torch.full((B,), 10.0))                              # exactly 10 of 16 per sample (trainer.py:63-65)
    freq = sel.mean(0)                                                                   # each patch chosen w.p. 10/16
    assert float((freq - 10 / 16).abs().max()) < 4 * (10 / 16 * 6 / 16 / B) ** 0.5 + 1e-3, freq
    assert len({tuple(r.tolist()) for r in sel[:256]}) > 200                            # samples differ from each other
    rng2 = ops.DeviceRNG(seed=1234)
    assert torch.equal(rng2.patch_mask(B, 28, 28, 7, 10, DEV).cpu(), m)                 # deterministic in (seed, offset)
    assert not torch.equal(rng2.patch_mask(B, 28, 28, 7, 10, DEV).cpu(), m)             # the stream advances
    t = rng.randint(0, 10, 100000, DEV).cpu()
    assert t.min() == 0 and t.max() == 9
    assert float((torch.bincount(t, minlength=10).float() / 1e5 - 0.1).abs().max()) < 5e-3
    src = torch.randint(0, 4, (50000,), device=DEV)
    t2 = rng.randint(0, 4, 50000, DEV, exclude=src)
    assert not bool((t2 == src).any()) and t2.min() == 0 and t2.max() == 3              # house_sales trainer.py:248-249
    # the reference's rule conditioned on the source class y: randint over all K, a collision goes to (y + 1) % K — so
    # P(y+1 | y) = 2/K and 1/K for the two remaining classes (NOT uniform over the K-1 others)
    for y in range(4):
        sel_y = (src == y)
        n_y = int(sel_y.sum())
        p = torch.bincount(t2[sel_y], minlength=4).float().cpu() / n_y
        want = torch.full((4,), 0.25); want[y] = 0.0; want[(y + 1) % 4] = 0.5
        assert float((p - want).abs().max()) < 5 * (0.25 / n_y) ** 0.5, (y, p.tolist())
    z = rng.randn((512, 100, 1, 1), DEV).cpu()
    assert abs(z.mean().item()) < 0.02 and abs(z.std().item() - 1.0) < 0.02
    assert abs((z ** 3).mean().item()) < 0.05 and abs((z ** 4).mean().item() - 3.0) < 0.15


def test_grad_norm_diagnostic(pcg):
    """trainer.py:41-42,142-143: sqrt(sum ||p.grad||^2), from the flat gradient buffer."""
    K = pcg.countergan
    (G, D, C), _ = _build(pcg, seed=1)
    x, y, t, m = (a.to(DEV) for a in CR.synthetic_batch(8, seed=2))
    opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
    K.train_step(G, D, C, opt_g, opt_d, bce, ce, x, y, t, m)
    ref = float(torch.sqrt(sum((p.grad.norm() ** 2) for p in G.parameters())).item())
    np.testing.assert_allclose(K.grad_norm(G), ref, rtol=1e-5)


def test_train_countergan_tail_matches_reference_trainer(pcg, golden_dir, tmp_path, capsys):
    """countergan.train_countergan(generator, discriminator, classifier, train_loader, cfg, device) against a run of the reference's
    own function (tests/golden/countergan_loop_b4.npz: 2 epochs x 3 batches): per-epoch means, G_grad / D_grad (D's = its D-step
    gradients + the generator step's critic weight gradients: the epoch's last iteration keeps them), residual_mean in the batch
    log line, every log line's format, the saved generator checkpoint."""
    import re
    K = pcg.countergan
    g = dict(np.load(os.path.join(golden_dir, "countergan_loop_b4.npz")))
    (G, D, C), _ = _build(pcg, seed=int(g["meta.seed"]))
    for tag, net in (("G", G), ("D", D), ("C", C)):
        for k, v in net.state_dict().items():
            np.testing.assert_array_equal(_digest(v.float()), g[f"init.{tag}.{k}"], err_msg=f"{tag}.{k}")
    E, S = int(g["meta.epochs"]), int(g["meta.nbatches"])

    class Cfg(K.Config):
        num_epochs_gan = E
        generator_path = str(tmp_path / "ckpt" / "generator.pt")
    loader = ((torch.from_numpy(g["data.x"][i]), torch.from_numpy(g["data.y"][i])) for i in range(S))      # a bare generator: no len()

    class Loader:                      # "any iterable of (x, y)": re-iterable, no __len__
        def __iter__(self):
            return iter([(torch.from_numpy(g["data.x"][i]), torch.from_numpy(g["data.y"][i])) for i in range(S)])
    del loader
    hist = K.train_countergan(G, D, C, Loader(), Cfg, DEV,
                              draws=lambda e, i, x: (torch.from_numpy(g["it.target_y"][e, i]), torch.from_numpy(g["it.mask"][e, i])))
    np.testing.assert_allclose(hist["G_grad"], g["epoch.G_grad"], rtol=2e-3)
    np.testing.assert_allclose(hist["D_grad"], g["epoch.D_grad"], rtol=2e-3)
    ours = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[")]
    ref = [l for l in str(g["log"]).splitlines() if l.startswith("[")]
    skel = lambda s: re.sub(r"-?[0-9]+\.[0-9]+", "#", s)
    assert [skel(l) for l in ours] == [skel(l) for l in ref]
    for lo, lr_ in zip(ours, ref):
        a, b = [float(v) for v in re.findall(r"-?[0-9]+\.[0-9]+", lo)], [float(v) for v in re.findall(r"-?[0-9]+\.[0-9]+", lr_)]
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=6e-4, err_msg=lo)
    saved = torch.load(Cfg.generator_path, map_location="cpu", weights_only=True)
    assert list(saved) == [str(k) for k in g["saved.keys"]]
    for k, v in saved.items():
        if re.fullmatch(r"resblocks\.\d+\.conv[12]\.bias", k):      # zero-gradient biases: Adam sign noise, bound the move
            assert np.abs(_digest(v.float())[3:] - g[f"saved.G.{k}"][3:]).max() <= E * S * 2.2 * Cfg.g_lr, k
            continue
        np.testing.assert_allclose(_digest(v.float())[3:], g[f"saved.G.{k}"][3:], rtol=2e-4, atol=E * S * 2.2 * Cfg.g_lr * 0.2, err_msg=k)
        assert torch.equal(v, G.state_dict()[k].cpu())


def test_trained_checkpoint_eval_forward(pcg, golden_dir):
    """The generator checkpoint the reference ships (results/generator.pt) loads into the drop-in class unchanged and, in
    eval mode (BatchNorm running statistics, the inference path of eval_utils.py / the Gradio app), reproduces the
    reference module's counterfactual residuals."""
    K = pcg.countergan
    gold = dict(np.load(os.path.join(golden_dir, "countergan_trained_eval.npz")))
    G = K.ResidualGenerator()
    G.load_state_dict(torch.load(os.path.join(golden_dir, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    G.to(DEV).eval()
    x, t, m = (torch.from_numpy(gold[k]).to(DEV) for k in ("x", "target", "mask"))
    with torch.no_grad():
        raw, masked = G(x, t, m)
        x_cf = K.clamp_add(x, masked, -1.0, 1.0)
    scale = float(np.abs(gold["raw"]).max())
    np.testing.assert_allclose(raw.cpu().numpy(), gold["raw"], rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(masked.cpu().numpy(), gold["masked"], rtol=1e-4, atol=2e-5 * scale)
    np.testing.assert_allclose(x_cf.cpu().numpy(), gold["x_cf"], rtol=1e-4, atol=2e-5 * scale)


def test_evaluate_counterfactuals_matches_reference(pcg, golden_dir):
    """eval_utils.py:46-79 lifted from the reference (tests/golden/make_golden.py: make_countergan_eval): shipped generator
    checkpoint, seeded classifier; flip rate, prediction gain, actionability and the de-normalised counterfactual images."""
    K = pcg.countergan
    gold = dict(np.load(os.path.join(golden_dir, "countergan_eval.npz")))
    G, C = K.ResidualGenerator(), None
    G.load_state_dict(torch.load(os.path.join(golden_dir, "countergan_generator_trained.pt"), map_location="cpu", weights_only=True))
    torch.manual_seed(3)
    C = K.CNNClassifier()
    for k, v in C.state_dict().items():
        np.testing.assert_array_equal(_digest(v), gold[f"C.{k}"], err_msg=k)
    G, C = G.to(DEV), C.to(DEV)
    m, (x_vis, x_cf_vis) = K.evaluate_counterfactuals(G, C, torch.from_numpy(gold["x"]), torch.from_numpy(gold["y_true"]),
                                                      torch.from_numpy(gold["y_target"]), torch.device(DEV))
    np.testing.assert_allclose([m["class_flip_rate"], m["prediction_gain"], m["actionability"]], gold["metrics"], rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(x_cf_vis.numpy(), gold["x_cf_vis"], rtol=1e-4, atol=2e-5)


def test_classifier_pretraining_matches_reference(pcg, golden_dir):
    """mnist/trainer.py:train_classifier as run by the reference on two seeded batches (+ one validation batch): CNNClassifier
    in training mode with the reference's Dropout2d / Dropout draws, Adam(1e-3), CrossEntropyLoss.  (a) per step, from the
    float64 oracle's current parameters: loss and every gradient (1e-4 of scale or 3x the float32 oracle's own distance);
    (b) the free-running result against the reference's final state, every entry within the total possible Adam move, and
    the validation accuracy it printed."""
    import re
    import torch.nn.functional as F
    K = pcg.countergan
    gold = dict(np.load(os.path.join(golden_dir, "classifier_pretrain_mnist.npz")))
    torch.manual_seed(5)
    o64 = CR.CNNClassifier()
    init = {k: v.clone() for k, v in o64.state_dict().items()}
    for k, v in init.items():
        np.testing.assert_array_equal(_digest(v), gold[f"init.{k}"], err_msg=k)
    o32 = CR.CNNClassifier(); o32.load_state_dict(init)
    o64 = o64.double()
    opt64 = torch.optim.Adam(o64.parameters(), lr=1e-3)
    mine = K.CNNClassifier(); mine.load_state_dict(init)
    mine = mine.to(DEV).train()
    ce = K.CrossEntropyLoss()
    for i in range(2):
        x, y = torch.from_numpy(gold[f"x{i}"]), torch.from_numpy(gold[f"y{i}"])
        masks = (torch.from_numpy(gold[f"mask{2 * i}"]), torch.from_numpy(gold[f"mask{2 * i + 1}"]))
        sd = {k: v.float() for k, v in o64.state_dict().items()}
        o32.load_state_dict(sd); mine.load_state_dict(sd)
        o32.train(); o32.zero_grad()
        l32 = F.cross_entropy(CR.classifier_forward_train(o32, x, masks), y); l32.backward()
        l64 = CR.classifier_train_step(o64, opt64, x.double(), y, masks)
        mine.dropout_masks = [m.to(DEV) for m in masks]
        mine.zero_grad()
        lm = ce(mine(x.to(DEV)), y.to(DEV)); lm.backward()
        assert abs(lm.item() - l64) <= max(2e-5, 3 * abs(l32.item() - l64)), (i, lm.item(), l64)
        for (n, p), (_, q32), (_, q64) in zip(mine.named_parameters(), o32.named_parameters(), o64.named_parameters()):
            truth = q64.grad
            tol = max(1e-4 * float(truth.abs().max()), 3 * float((q32.grad.double() - truth).abs().max()), 1e-8)
            err = float((p.grad.cpu().double() - truth).abs().max())
            assert err <= tol, (f"step {i} grad {n}", err, tol)
    mine.load_state_dict(init)
    opt = pcg.optim.Adam(mine.parameters(), lr=1e-3)
    for i in range(2):
        mine.dropout_masks = [torch.from_numpy(gold[f"mask{2 * i}"]).to(DEV), torch.from_numpy(gold[f"mask{2 * i + 1}"]).to(DEV)]
        opt.zero_grad()
        ce(mine(torch.from_numpy(gold[f"x{i}"]).to(DEV)), torch.from_numpy(gold[f"y{i}"]).to(DEV)).backward()
        opt.step()
    for k in ("fc.4.weight", "conv.0.weight"):
        assert float(np.abs(mine.state_dict()[k].cpu().numpy() - gold[f"final.{k}.full"]).max()) <= 2.2 * 1e-3 * 2 + 1e-5, k
    for k, v in mine.state_dict().items():
        np.testing.assert_allclose(_digest(v)[3:], gold[f"final.{k}"][3:], rtol=0, atol=2.2 * 1e-3 * 2 + 1e-5, err_msg=k)
    mine.dropout_masks = None
    mine.eval()
    with torch.no_grad():
        acc = pcg.ops.cf_metrics(mine(torch.from_numpy(gold["x2"]).to(DEV)).contiguous(), torch.from_numpy(gold["y2"]).to(DEV),
                                 other=torch.from_numpy(gold["y2"]).to(DEV))[0].item()
    assert abs(acc - float(re.search(r"Val Acc: ([0-9.]+)", str(gold["log"])).group(1))) < 0.13   # 8 samples: at most one flips


def test_fused_backward_epilogues_equal_separate_passes(pcg):
    """countergan.FUSE_BACKWARD_EPILOGUE: the LeakyReLU / ReLU derivative of the layer below, BatchNorm-backward's column sums
    (bn1 of every residual block) and the skip-connection add are taken in the grad-input kernels' epilogue.  Against the separate
    passes: the add is bit-identical by construction, masks use the same expression, only the order of the BatchNorm sums differs —
    all G and D gradients of one training step agree to 2e-5 rel-L2 (entries that are pure summation noise excepted: a conv bias
    in front of a BatchNorm has an exactly-zero gradient)."""
    K = pcg.countergan
    x, y, t, m = (a.to(DEV) for a in CR.synthetic_batch(32, seed=7))
    grads = {}
    try:
        for fuse in (True, False):
            K.FUSE_BACKWARD_EPILOGUE = fuse
            (G, D, C), _ = _build(pcg, seed=4)
            opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
            K.train_step(G, D, C, opt_g, opt_d, bce, ce, x, y, t, m)
            grads[fuse] = {**{f"G.{n}": p.grad.clone() for n, p in G.named_parameters()},
                           **{f"D.{n}": p.grad.clone() for n, p in D.named_parameters()}}
    finally:
        K.FUSE_BACKWARD_EPILOGUE = True
    checked = 0
    for k, ref in grads[False].items():
        got = grads[True][k]
        assert torch.isfinite(got).all(), k
        if k.startswith("G.resblocks") and k.endswith((".conv1.bias", ".conv2.bias")):
            continue   # zero in exact arithmetic (bias in front of BatchNorm): fp32 summation noise in every implementation
        r, g_ = ref.double().cpu().numpy(), got.double().cpu().numpy()
        l2 = np.linalg.norm(g_ - r) / max(np.linalg.norm(r), 1e-30)
        assert l2 <= 2e-5, f"{k}: rel-L2 {l2:.2e}"
        checked += 1
    assert checked >= 45


def test_fused_bias_colsum_equals_separate_pass(pcg):
    """countergan.FUSE_BIAS_COLSUM: the gradients of the conv biases in front of BatchNorm layers come out of the BatchNorm
    backward's apply pass instead of a pcg_colsum pass over dz.  Everything else of the step is bit-identical; the bias gradients
    themselves are rounding residue of an analytically zero sum (both forms accumulate in fp64: equal to ~1e-6 of |dz| sums)."""
    K = pcg.countergan
    x, y, t, m = (a.to(DEV) for a in CR.synthetic_batch(16, seed=5))
    res = {}
    try:
        for fuse in (True, False):
            K.FUSE_BIAS_COLSUM = fuse
            (G, D, C), _ = _build(pcg, seed=2)
            opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
            out = K.train_step(G, D, C, opt_g, opt_d, bce, ce, x, y, t, m)
            res[fuse] = (out["g_loss"].item(), out["d_loss"].item(),
                         {n: p.grad.clone() for n, p in G.named_parameters()}, {n: p.grad.clone() for n, p in D.named_parameters()})
    finally:
        K.FUSE_BIAS_COLSUM = True
    assert res[True][:2] == res[False][:2]
    for n, gref in res[False][2].items():
        got = res[True][2][n]
        if n.endswith("bias") and ".conv" in n and "resblocks" in n:
            scale = max(float(res[False][2][n.replace("bias", "weight")].abs().max()), 1e-12)
            assert float((got - gref).abs().max()) <= 1e-4 * scale + 1e-9, n     # residue of a zero sum: tiny next to the weight gradient
        else:
            assert torch.equal(got, gref), n
    for n, gref in res[False][3].items():
        assert torch.equal(res[True][3][n], gref), n


def test_skip_add_bnsum_equals_separate_reduction(pcg):
    """countergan.FUSE_SKIP_BNSUM: bn2's backward column sums (sum 0.1*dh, sum 0.1*dh*xhat) come out of the previous block's
    skip-add grad-input epilogue (PCG_CONV_EPI_ADD_BNSUM) instead of a reduction pass over (dh, z2).  Same values summed in
    fp64 in another order: every gradient of the step agrees to fp32 rounding of the two means (1e-6 of the tensor's scale)."""
    K = pcg.countergan
    x, y, t, m = (a.to(DEV) for a in CR.synthetic_batch(16, seed=7))
    res = {}
    try:
        for fuse in (True, False):
            K.FUSE_SKIP_BNSUM = fuse
            (G, D, C), _ = _build(pcg, seed=3)
            opt_g, opt_d, bce, ce = K.make_optimizers(G, D)
            out = K.train_step(G, D, C, opt_g, opt_d, bce, ce, x, y, t, m)
            res[fuse] = (out["g_loss"].item(), out["d_loss"].item(), {n: p.grad.clone() for n, p in G.named_parameters()})
    finally:
        K.FUSE_SKIP_BNSUM = True
    assert res[True][:2] == res[False][:2]
    for n, gref in res[False][2].items():
        got = res[True][2][n]
        if n.endswith("bias") and ".conv" in n and "resblocks" in n:
            continue                                   # rounding residue of an analytically zero sum
        scale = float(gref.abs().max())
        assert float((got - gref).abs().max()) <= 2e-5 * scale + 1e-12, (n, float((got - gref).abs().max()), scale)


def test_train_countergan_memory_stays_flat_over_an_epoch(pcg):
    """the per-iteration scalars the trainer keeps until the epoch's end must not keep the iteration's autograd
    graph — and with it every custom node's saved activations (0.67 GB per iteration at the reference batch) — alive.  The loader
    below reads torch.cuda.memory_allocated() before every batch: flat after the first iterations."""
    K = pcg.countergan
    (G, D, C), _ = _build(pcg, seed=2)

    class Cfg(K.Config):
        num_epochs_gan = 1
        generator_path = None
    g = torch.Generator().manual_seed(0)
    B = 32
    x = (torch.rand(B, 1, 28, 28, generator=g) * 2 - 1).to(DEV)
    y = torch.randint(0, 10, (B,), generator=g).to(DEV)
    mem = []

    def loader():
        for _ in range(20):
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated())
            yield x, y
    hist = K.train_countergan(G, D, C, loader(), Cfg, torch.device(DEV), verbose=False, save=False)
    assert len(hist["g_losses"]) == 1 and np.isfinite(hist["g_losses"][0])
    assert len(mem) == 20
    grown = max(mem[5:]) - mem[5]
    assert grown <= 4 << 20, f"memory grows over the epoch: {[m >> 20 for m in mem]} MiB"


def test_label_channel_grad_input_equals_the_three_channel_form(pcg):
    """conv_in's grad-input computed for the label-map channel only (the image and mask channels' gradients have no consumer) against
    the three-channel grad-input + pcg_embed_concat_bwd: the embedding table's gradient to summation-order accuracy, every other
    gradient bit-identical."""
    K = pcg.countergan
    x, y, t, m = (v.to(DEV) for v in CR.synthetic_batch(16, seed=9))
    grads = {}
    for flag in (True, False):
        K.GRAD_INPUT_LABEL_CHANNEL_ONLY = flag
        try:
            (G, D, C), _ = _build(pcg, seed=6)
            raw, masked = G(x, t, m)
            (raw.square().mean() + masked.abs().mean()).backward()
            grads[flag] = {n: p.grad.clone() for n, p in G.named_parameters()}
        finally:
            K.GRAD_INPUT_LABEL_CHANNEL_ONLY = True
    for n in grads[True]:
        if n == "embed.weight":
            a, b = grads[True][n], grads[False][n]
            assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-12, n
            assert float(b.abs().max()) > 0
        else:
            assert torch.equal(grads[True][n], grads[False][n]), n
