"""GPU: the moons CounteRGAN step kernel (csrc/moons_cf.hip through pcgan_amd.moons_countergan) against a float64 oracle written
here — the three nets in torch.float64 on the CPU (nn.utils.spectral_norm, BatchNorm1d) and the loop body of trainer.py:58-99 as the
reference writes it — and against the reference's own recorded epoch (tests/golden/moons_cf_ref.npz)."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = {"seed": 42, "epochs": 1, "batch_size": 64, "lr_G": 1e-3, "lr_D": 1e-3, "lambda_cls": 2.0, "lambda_reg_l1": 5.0, "lambda_reg_l2": 5.0,
       "lambda_mask": 3.0, "input_dim": 2, "hidden_dim": 32, "out_dir": "results", "clf_model_path": "", "generator_path": "", "cuda": DEV}
PRE_BN_BIAS = ("net.0.bias", "net.3.bias", "net.6.bias")     # gradient exactly 0 in exact arithmetic: fp32 noise, Adam-amplified
# One Adam step moves such a parameter by at most lr (1 - beta1) / sqrt(1 - beta2) = 3.16 lr once its moments hold a noise history
# that differs from the fresh gradient's (the first step: at most lr).  Both sides move by such steps in unrelated directions.
BIAS_STEP = 3.2e-3
# A gradient element is a sum over the batch of terms as large as the tensor's largest entries: near-zero elements carry fp32
# cancellation error of that scale, so the absolute floor of a state comparison is also relative to the tensor's magnitude.
SCALE = 1e-5


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "moons_cf_ref.npz")))


@pytest.fixture(scope="module")
def M():
    import pcgan_amd
    from pcgan_amd import moons_countergan
    pcgan_amd.load()
    return moons_countergan


# ---- float64 oracle --------------------------------------------------------------------------------------------------------------
def o_nets(H):
    G = nn.Sequential(nn.Linear(7, H), nn.BatchNorm1d(H), nn.ReLU(), nn.Linear(H, H), nn.BatchNorm1d(H), nn.ReLU(),
                      nn.Linear(H, H // 2), nn.BatchNorm1d(H // 2), nn.ReLU(), nn.Linear(H // 2, 2))
    sn = nn.utils.spectral_norm
    D = nn.Sequential(sn(nn.Linear(5, H)), nn.LeakyReLU(0.2), sn(nn.Linear(H, H // 2)), nn.LeakyReLU(0.2), sn(nn.Linear(H // 2, H // 2)),
                      nn.LeakyReLU(0.2), sn(nn.Linear(H // 2, 1)))
    C = nn.Sequential(nn.Linear(2, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 3))
    return Net(G).double(), Net(D).double(), Net(C).double()


class Net(nn.Module):
    """`self.net = nn.Sequential(...)`, as the reference's modules hold it: state_dict keys net.<i>.<name>."""

    def __init__(self, seq):
        super().__init__()
        self.net = seq

    def forward(self, x):
        return self.net(x)


def o_step(G, D, C, optG, optD, x, y, t, m, cfg=CFG):
    """trainer.py:64-99 with the draws given; returns the nine logged scalars."""
    G.train(); D.train(); C.eval()
    onehot = F.one_hot(t, 3).double()
    raw = G(torch.cat([x, onehot, m], 1))
    masked = raw * m
    mask_pen = torch.mean(torch.abs(raw * (1.0 - m)))
    x_cf = x + masked
    D_real = D(torch.cat([x, F.one_hot(y, 3).double()], 1))
    D_fake = D(torch.cat([x_cf.detach(), onehot], 1))
    D_loss = -D_real.mean() + D_fake.mean()
    optD.zero_grad(); D_loss.backward(); optD.step()
    D_fg = D(torch.cat([x_cf, onehot], 1))
    g_adv = -D_fg.mean()
    g_cls = F.cross_entropy(C(x_cf), t)
    l1 = torch.mean(torch.norm(masked, p=1, dim=1))
    l2 = torch.mean(torch.norm(masked, p=2, dim=1))
    G_loss = g_adv + cfg["lambda_cls"] * g_cls + cfg["lambda_reg_l1"] * l1 + cfg["lambda_reg_l2"] * l2 + cfg["lambda_mask"] * mask_pen
    optG.zero_grad(); G_loss.backward(); optG.step()
    for p in G.parameters():
        assert torch.isfinite(p.grad).all()
    return np.array([D_loss.item(), G_loss.item(), torch.sigmoid(D_real).mean().item(), torch.sigmoid(D_fake).mean().item(), g_adv.item(),
                     g_cls.item(), l1.item(), l2.item(), mask_pen.item()])


def prefixed(gold, pre):
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre)}


def param_names(net):
    return [n for n, _ in net.named_parameters()]


# ---- state transfer --------------------------------------------------------------------------------------------------------------
class Rig:
    """HIP modules + Adams + TrainSteps, and the float64 oracle, loadable from one state."""

    def __init__(self, M, H=32, B=64, X=None, Y=None, clf_state=None, lr=1e-3):
        self.M, self.H, self.B = M, H, B
        self.G, self.D, self.C = M.ResidualGenerator(2, H, 3).to(DEV), M.Discriminator(2, H, 3).to(DEV), M.NNClassifier(2).to(DEV)
        if clf_state is not None:
            self.C.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in clf_state.items()})
        self.optG, self.optD = M.Adam(self.G.parameters(), lr=lr), M.Adam(self.D.parameters(), lr=lr)
        self.cfg = dict(CFG, batch_size=B, hidden_dim=H, lr_G=lr, lr_D=lr)
        self.X, self.Y = X, Y
        self.run = M.TrainSteps(self.G, self.D, self.C, self.optG, self.optD, X, Y, self.cfg)
        self.oG, self.oD, self.oC = o_nets(H)
        self.oC.load_state_dict({k: v.double() for k, v in self.C.state_dict().items()} if clf_state is None else
                                {k: torch.from_numpy(np.array(v)).double() for k, v in clf_state.items()})
        self.ooptG = torch.optim.Adam(self.oG.parameters(), lr=lr)
        self.ooptD = torch.optim.Adam(self.oD.parameters(), lr=lr)

    def state(self):
        """(G state_dict, D state_dict, G adam, D adam) of the HIP side as numpy (adam: {name: (m, v)}, step)."""
        out = []
        for net in (self.G, self.D):
            out.append({k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()})
        for opt, net in ((self.optG, self.G), (self.optD, self.D)):
            seg = opt._segments[0][0]
            m, v = seg["exp_avg"].cpu().numpy(), seg["exp_avg_sq"].cpu().numpy()
            names = dict((id(p), n) for n, p in net.named_parameters())
            out.append(({names[id(p)]: (m[off:off + n].reshape(p.shape), v[off:off + n].reshape(p.shape)) for p, off, n in net._seg},
                        int(seg["step"].item())))
        return out

    def load(self, Gs, Ds, adamG=None, adamD=None):
        """Both sides to this state; adam*: ({name: (exp_avg, exp_avg_sq)}, step) or None (fresh)."""
        t = lambda v: torch.from_numpy(np.array(v))
        self.G.load_state_dict({k: t(v) for k, v in Gs.items()}); self.D.load_state_dict({k: t(v) for k, v in Ds.items()})
        self.oG.load_state_dict({k: t(v).double() if t(v).is_floating_point() else t(v) for k, v in Gs.items()})
        self.oD.load_state_dict({k: t(v).double() for k, v in Ds.items()})
        for opt, oopt, net, onet, st in ((self.optG, self.ooptG, self.G, self.oG, adamG), (self.optD, self.ooptD, self.D, self.oD, adamD)):
            seg = opt._segments[0][0]
            seg["exp_avg"].zero_(); seg["exp_avg_sq"].zero_(); seg["step"].zero_()
            oopt.state.clear()
            if st is None:
                continue
            mom, step = st
            seg["step"].fill_(step)
            names = dict((id(p), n) for n, p in net.named_parameters())
            for p, off, n in net._seg:
                seg["exp_avg"][off:off + n] = t(mom[names[id(p)]][0]).reshape(-1).to(DEV)
                seg["exp_avg_sq"][off:off + n] = t(mom[names[id(p)]][1]).reshape(-1).to(DEV)
            for name, q in onet.named_parameters():
                oopt.state[q] = {"step": torch.tensor(float(step), dtype=torch.float64), "exp_avg": t(mom[name][0]).double().clone(),
                                 "exp_avg_sq": t(mom[name][1]).double().clone()}

    def step_both(self, rows, ty, mk):
        """One iteration on each side; returns (hip logs [9], oracle logs [9])."""
        logs = self.run.run(torch.as_tensor(rows).view(1, -1), torch.as_tensor(ty).view(1, -1), torch.as_tensor(mk).view(1, -1, 2))
        x = torch.from_numpy(np.asarray(self.X)[np.asarray(rows)]).double()
        y = torch.as_tensor(np.asarray(self.Y)[np.asarray(rows)], dtype=torch.long)
        ol = o_step(self.oG, self.oD, self.oC, self.ooptG, self.ooptD, x, y, torch.as_tensor(ty, dtype=torch.long),
                    torch.as_tensor(mk).double())
        return logs.cpu().numpy()[0].astype(np.float64), ol

    def compare(self, rtol=1e-4, atol=1e-6, bias_atol=2 * BIAS_STEP, what="", skip_g=()):
        Gs, Ds, (aG, sG), (aD, sD) = self.state()
        for tag, ours, onet in (("G", Gs, self.oG), ("D", Ds, self.oD)):
            for k, v in onet.state_dict().items():
                if tag == "G" and k in skip_g:
                    continue
                ref = v.numpy().astype(np.float64) if v.is_floating_point() else v.numpy()
                if tag == "G" and k in PRE_BN_BIAS:
                    np.testing.assert_allclose(ours[k], ref, rtol=0, atol=bias_atol, err_msg=f"{what} {tag}.{k}")
                elif v.is_floating_point():
                    np.testing.assert_allclose(ours[k], ref, rtol=rtol, atol=atol + SCALE * np.abs(ref).max(), err_msg=f"{what} {tag}.{k}")
                else:
                    assert np.array_equal(ours[k], ref), f"{what} {tag}.{k}"
        for tag, (mom, step), oopt, onet in (("G", (aG, sG), self.ooptG, self.oG), ("D", (aD, sD), self.ooptD, self.oD)):
            for name, q in onet.named_parameters():
                st = oopt.state[q]
                assert step == int(st["step"]), f"{what} opt{tag} step"
                if tag == "G" and (name in PRE_BN_BIAS or name in skip_g):
                    continue
                for j, key in ((0, "exp_avg"), (1, "exp_avg_sq")):
                    ref = st[key].numpy()
                    np.testing.assert_allclose(mom[name][j], ref, rtol=rtol, atol=atol + SCALE * np.abs(ref).max(),
                                               err_msg=f"{what} opt{tag}.{name}.{key}")


def gold_state(gold, i):
    """(G, D, adamG, adamD) before golden iteration i."""
    if i == 0:
        return prefixed(gold, "init.G."), prefixed(gold, "init.D."), None, None
    pre = f"it{i - 1}."
    out = [prefixed(gold, pre + "G."), prefixed(gold, pre + "D.")]
    for tag in ("G", "D"):
        ad = prefixed(gold, f"{pre}opt{tag}.")
        step = int(ad.pop("step"))
        names = sorted({k.rsplit(".", 1)[0] for k in ad})
        out.append(({n: (ad[n + ".exp_avg"], ad[n + ".exp_avg_sq"]) for n in names}, step))
    return tuple(out)


def make_rig(M, gold, **kw):
    return Rig(M, X=gold["data.X_train"], Y=gold["data.y_train"], clf_state=prefixed(gold, "init.C."), **kw)


# ---- 1. teacher-forced single iterations ---------------------------------------------------------------------------------------
def test_teacher_forced_iterations_vs_float64(M, gold):
    rig = make_rig(M, gold)
    for i in range(gold["rows"].shape[0]):
        rig.load(*gold_state(gold, i))
        ours, ref = rig.step_both(gold["rows"][i], gold["target_y"][i], gold["mask"][i])
        np.testing.assert_allclose(ours, ref, rtol=1e-5, atol=1e-7, err_msg=f"logs, iteration {i}")
        np.testing.assert_allclose(ref, gold["logs"][i], rtol=1e-5, atol=1e-7, err_msg=f"oracle vs reference logs, iteration {i}")
        rig.compare(what=f"iteration {i}", bias_atol=2 * BIAS_STEP)


def test_pre_batchnorm_biases_do_not_change_outputs(M, gold):
    G = M.ResidualGenerator(2, 32, 3).to(DEV)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.G.").items()})
    x = torch.from_numpy(gold["data.X_train"][:64]).float().to(DEV)
    oh = F.one_hot(torch.from_numpy(gold["target_y"][0]), 3).float().to(DEV)
    mk = torch.from_numpy(gold["mask"][0]).to(DEV)
    with torch.no_grad():
        raw0, _ = G(x, oh, mk)
        for k in PRE_BN_BIAS:
            dict(G.named_parameters())[k].add_(0.37)
        raw1, _ = G(x, oh, mk)
    np.testing.assert_allclose(raw1.cpu().numpy(), raw0.cpu().numpy(), rtol=0, atol=2e-5)


# ---- 2. one launch equals many ---------------------------------------------------------------------------------------------------
def test_one_launch_equals_many_bitwise(M, gold):
    rig = make_rig(M, gold)
    rows, ty, mk = (torch.from_numpy(gold[k]) for k in ("rows", "target_y", "mask"))
    results = []
    for split in ((15,), (1,) * 15, (5, 5, 5)):
        rig.load(*gold_state(gold, 0))
        logs, i = [], 0
        for n in split:
            logs.append(rig.run.run(rows[i:i + n], ty[i:i + n], mk[i:i + n]).cpu())
            i += n
        Gs, Ds, (aG, sG), (aD, sD) = rig.state()
        results.append((torch.cat(logs).numpy(), Gs, Ds, aG, aD, sG, sD))
    a = results[0]
    for b in results[1:]:
        assert np.array_equal(a[0], b[0])
        for d1, d2 in ((a[1], b[1]), (a[2], b[2])):
            for k in d1:
                assert np.array_equal(d1[k], d2[k]), k
        for d1, d2 in ((a[3], b[3]), (a[4], b[4])):
            for k in d1:
                assert np.array_equal(d1[k][0], d2[k][0]) and np.array_equal(d1[k][1], d2[k][1]), k
        assert a[5:] == b[5:] == (15, 15)


# ---- 3. the reference's own trajectory -------------------------------------------------------------------------------------------
def _gold_draws(gold):
    def draws(epoch, batch_idx, y):
        assert np.array_equal(y.numpy(), gold["data.y_train"][gold["rows"][batch_idx]])
        return torch.from_numpy(gold["target_y"][batch_idx % 15]), torch.from_numpy(gold["mask"][batch_idx % 15])
    return draws


def test_epoch_through_train_countergan_follows_reference(M, gold, tmp_path):
    G = M.ResidualGenerator(2, 32, 3)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.G.").items()})
    C = M.NNClassifier(2)
    C.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.C.").items()})
    cfg = dict(CFG, out_dir=str(tmp_path), generator_path=str(tmp_path / "g.pt"))
    res = M.train_countergan(G, cfg, gold["data.X_train"], gold["data.y_train"], C, draws=_gold_draws(gold))
    np.testing.assert_allclose(res["d_losses"][0], np.mean(gold["logs"][:, 0]), rtol=1e-4)
    np.testing.assert_allclose(res["g_losses"][0], np.mean(gold["logs"][:, 1]), rtol=1e-4)
    np.testing.assert_allclose(res["logs"].cpu().numpy(), gold["logs"], rtol=1e-4, atol=1e-6)
    for tag, net in (("G", G), ("D", res["discriminator"])):
        ref = prefixed(gold, f"it14.{tag}.")
        for k, v in net.state_dict().items():
            v = v.cpu().numpy()
            # the pre-BatchNorm biases, and the running means that average them in (net.{1,4,7}.running_mean: an EMA of the batch
            # mean of Wx + b): a free walk of fp32 noise on both sides
            if tag == "G" and (k in PRE_BN_BIAS or k.endswith("running_mean")):
                np.testing.assert_allclose(v, ref[k], rtol=0, atol=15 * 1e-3, err_msg=k)
            elif v.dtype.kind == "f":
                np.testing.assert_allclose(v, ref[k], rtol=1e-3, atol=1e-5, err_msg=f"{tag}.{k}")
            else:
                assert np.array_equal(v, ref[k]), f"{tag}.{k}"
    saved = torch.load(cfg["generator_path"])
    assert list(saved) == list(G.state_dict())


def test_printed_lines_have_reference_format(M, gold, tmp_path):
    G = M.ResidualGenerator(2, 32, 3)
    G.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.G.").items()})
    C = M.NNClassifier(2)
    C.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.C.").items()})
    cfg = dict(CFG, epochs=10, out_dir=str(tmp_path), generator_path=str(tmp_path / "g.pt"))
    buf = io.StringIO()
    draws = _gold_draws(gold)
    with contextlib.redirect_stdout(buf):
        M.train_countergan(G, cfg, gold["data.X_train"], gold["data.y_train"], C, draws=lambda e, b, y: draws(0, b, y) if e == 0 else
                           (torch.remainder(y + 1, 3), torch.ones(y.shape[0], 2)))
    lines = buf.getvalue().splitlines()
    pat = (r"^\[Epoch (\d+)/10\] batch (\d+) :: D\(real\)=-?\d+\.\d{3}, D\(fake\)=-?\d+\.\d{3}, g_adv=-?\d+\.\d{4}, g_cls=-?\d+\.\d{4}, "
           r"reg_l1=-?\d+\.\d{5}, reg_l2= -?\d+\.\d{5}, mask_pen=-?\d+\.\d{5}$")
    batch_lines = [l for l in lines if l.startswith("[Epoch")]
    assert len(batch_lines) == 10 * 3 and all(re.match(pat, l) for l in batch_lines), batch_lines[:3]
    assert [int(re.match(pat, l).group(2)) for l in batch_lines[:3]] == [0, 5, 10]
    first = re.findall(r"=\s?(-?\d+\.\d+)", batch_lines[0])
    np.testing.assert_allclose([float(v) for v in first], gold["logs"][0, 2:], atol=2e-3)
    summary = [l for l in lines if re.match(r"^\[\d+/10\] D: -?\d+\.\d{4}, G: -?\d+\.\d{4}$", l)]
    assert len(summary) == 5
    assert lines[-1] == f"Generator saved to {cfg['generator_path']}"


# ---- 4. hard corners -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", ["zero_mask", "full_mask", "dead_relu"])
def test_hard_corners_vs_float64(M, gold, corner):
    rig = make_rig(M, gold)
    Gs, Ds, aG, aD = gold_state(gold, 3)
    mk = gold["mask"][3].copy()
    if corner == "zero_mask":
        mk[:] = 0.0
    elif corner == "full_mask":
        mk[:] = 1.0
    else:
        Gs = dict(Gs)
        Gs["net.4.weight"] = Gs["net.4.weight"].copy(); Gs["net.4.bias"] = Gs["net.4.bias"].copy()
        Gs["net.4.weight"][5] = 0.0; Gs["net.4.bias"][5] = -1.0          # BN 1, unit 5: gamma 0, beta -1 -> ReLU dead on every row
    rig.load(Gs, Ds, aG, aD)
    ours, ref = rig.step_both(gold["rows"][3], gold["target_y"][3], mk)
    assert np.isfinite(ours).all()
    np.testing.assert_allclose(ours, ref, rtol=1e-5, atol=1e-7, err_msg=corner)
    rig.compare(what=corner)
    for net in (rig.G, rig.D):
        assert torch.isfinite(net.flat_params).all()


# ---- 5. forwards -----------------------------------------------------------------------------------------------------------------
def test_shipped_checkpoints_eval_forward(M, gold):
    G = M.ResidualGenerator(2, 32, 3)
    G.load_state_dict(torch.load(os.path.join(GOLD, "moons_cf_generator_trained.pt"), map_location="cpu"))
    C = M.NNClassifier(2)
    C.load_state_dict(torch.load(os.path.join(GOLD, "moons_cf_classifier_trained.pt"), map_location="cpu"))
    G.to(DEV).eval(); C.to(DEV).eval()
    for p in list(G.parameters()) + list(C.parameters()):
        p.requires_grad = False
    g = lambda k: torch.from_numpy(gold[f"eval.{k}"]).to(DEV)
    raw, masked = G(g("x"), g("onehot"), g("mask"))
    np.testing.assert_allclose(raw.cpu().numpy(), gold["eval.raw"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(masked.cpu().numpy(), gold["eval.masked"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(C(g("x")).cpu().numpy(), gold["eval.logits"], rtol=1e-5, atol=1e-6)
    with pytest.raises(M.PcgError):
        G.requires_grad_(True)
        G(g("x"), g("onehot"), g("mask"))


def test_train_mode_forwards_update_buffers_like_torch(M, gold):
    _, oD, _ = o_nets(32)
    oG = o_nets(32)[0]
    Ds, Gs = prefixed(gold, "init.D."), prefixed(gold, "init.G.")
    D = M.Discriminator(2, 32, 3).to(DEV); D.load_state_dict({k: torch.from_numpy(v) for k, v in Ds.items()})
    G = M.ResidualGenerator(2, 32, 3).to(DEV); G.load_state_dict({k: torch.from_numpy(v) for k, v in Gs.items()})
    oD.load_state_dict({k: torch.from_numpy(v).double() for k, v in Ds.items()})
    oG.load_state_dict({k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in Gs.items()})
    x = torch.from_numpy(gold["data.X_train"][:100])
    oh = F.one_hot(torch.from_numpy(gold["data.y_train"][:100]), 3).double()
    mk = torch.from_numpy(gold["mask"][0][:36]).double().repeat(3, 1)[:100]
    with torch.no_grad():
        for _ in range(2):                              # two power iterations: u / v advance as torch's do
            out = D(x.float().to(DEV), oh.float().to(DEV))
            ref = oD(torch.cat([x, oh], 1))
            np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6)
            raw, masked = G(x.float().to(DEV), oh.float().to(DEV), mk.float().to(DEV))
            oraw = oG(torch.cat([x, oh, mk], 1))
            np.testing.assert_allclose(raw.cpu().numpy(), oraw.numpy(), rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(masked.cpu().numpy(), (oraw * mk).numpy(), rtol=1e-4, atol=1e-5)
    for (k, v), (_, w) in zip(D.state_dict().items(), oD.state_dict().items()):
        np.testing.assert_allclose(v.cpu().numpy(), w.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    for (k, v), (_, w) in zip(G.state_dict().items(), oG.state_dict().items()):
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), w.numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
        elif "num_batches" in k:
            assert int(v) == int(w) == 2
    D.eval()
    u0 = D.net[0].weight_u.clone()
    oD.eval()
    with torch.no_grad():
        np.testing.assert_allclose(D(x.float().to(DEV), oh.float().to(DEV)).cpu().numpy(), oD(torch.cat([x, oh], 1)).numpy(), rtol=1e-5, atol=1e-6)
    assert torch.equal(u0, D.net[0].weight_u)


# ---- 6. batch sizes and widths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(32, 2), (32, 64), (32, 300), (32, 512), (64, 64), (64, 300)])
def test_batch_sizes_and_widths_vs_float64(M, gold, H, B):
    torch.manual_seed(100 + B + H)
    rig = make_rig(M, gold, H=H, B=B)
    Gs = {k: v.detach().cpu().numpy() for k, v in M.ResidualGenerator(2, H, 3).state_dict().items()}
    Ds = {k: v.detach().cpu().numpy() for k, v in M.Discriminator(2, H, 3).state_dict().items()}
    # a warm optimizer state (step 10, second moments 1e-4): Adam's FIRST step, lr g / (|g| + eps), is ill-conditioned for
    # gradient elements near zero and would compare fp32 rounding, not the step
    warm = lambda sd: ({n: (np.zeros_like(v), np.full_like(v, 1e-4)) for n, v in sd.items() if n.split(".")[-1] in
                        ("weight", "bias", "weight_orig")}, 10)
    rig.load(Gs, Ds, warm(Gs), warm(Ds))
    g = torch.Generator().manual_seed(B)
    N = gold["data.X_train"].shape[0]
    rows = torch.randint(0, N, (B,), generator=g)
    y = torch.from_numpy(gold["data.y_train"])[rows]
    ty = torch.remainder(y + torch.randint(1, 3, (B,), generator=g), 3)
    mk = torch.randint(0, 2, (B, 2), generator=g).float()
    ours, ref = rig.step_both(rows.numpy(), ty.numpy(), mk.numpy())
    np.testing.assert_allclose(ours, ref, rtol=1e-5, atol=1e-7, err_msg=f"H {H} B {B}")
    if B == 2:
        # two rows: x-hat = +-1 and every BatchNorm1d's input gradient is identically zero; G below its last BatchNorm sees only
        # fp32 noise (Adam steps of at most BIAS_STEP), everything else is compared as usual
        below = {f"net.{i}.{k}" for i in (0, 3, 6) for k in ("weight", "bias")} | {f"net.{i}.{k}" for i in (1, 4) for k in ("weight", "bias")}
        Gs_ours = rig.state()[0]
        for k in below:
            np.testing.assert_allclose(Gs_ours[k], rig.oG.state_dict()[k].numpy(), rtol=0, atol=2 * BIAS_STEP, err_msg=k)
        rig.compare(what=f"H {H} B {B}", skip_g=below)
    else:
        rig.compare(what=f"H {H} B {B}")


# ---- 7. optimizer interop --------------------------------------------------------------------------------------------------------
def test_eager_adam_step_continues_after_fused_launch(M, gold):
    rig = make_rig(M, gold)
    rig.load(*gold_state(gold, 0))
    rig.step_both(gold["rows"][0], gold["target_y"][0], gold["mask"][0])
    g = torch.Generator().manual_seed(3)
    for (name, p), (_, q) in zip(rig.G.named_parameters(), rig.oG.named_parameters()):
        grad = torch.randn(p.shape, generator=g, dtype=torch.float64) * 1e-2
        p.grad.copy_(grad.float().to(DEV))
        q.grad = grad.clone()
    rig.optG.step()
    rig.ooptG.step()
    for (k, v), (_, w) in zip(rig.G.state_dict().items(), rig.oG.state_dict().items()):
        if k in PRE_BN_BIAS or not w.is_floating_point():
            continue
        np.testing.assert_allclose(v.cpu().numpy(), w.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
    assert int(rig.optG._segments[0][0]["step"].item()) == 2


# ---- 8. device draws -------------------------------------------------------------------------------------------------------------
def test_device_draws_deterministic_and_valid(M, gold, tmp_path):
    finals = []
    for _ in range(2):
        G = M.ResidualGenerator(2, 32, 3)
        G.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.G.").items()})
        C = M.NNClassifier(2)
        C.load_state_dict({k: torch.from_numpy(v) for k, v in prefixed(gold, "init.C.").items()})
        cfg = dict(CFG, epochs=3, generator_path=str(tmp_path / "g.pt"), out_dir=str(tmp_path))
        res = M.train_countergan(G, cfg, gold["data.X_train"], gold["data.y_train"], C, verbose=False, save=False)
        assert all(np.isfinite(res["d_losses"])) and all(np.isfinite(res["g_losses"]))
        finals.append(({k: v.cpu().clone() for k, v in G.state_dict().items()}, res["d_losses"], res["g_losses"]))
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], finals[1][0][k]), k
    assert finals[0][1] == finals[1][1] and finals[0][2] == finals[1][2]
    # the draws train_countergan makes per epoch: targets never equal y, masks 0 / 1 with mean near 1/2
    from pcgan_amd import ops
    rng = ops.DeviceRNG(seed=42)
    y = torch.from_numpy(gold["data.y_train"]).to(DEV)
    t = rng.randint(0, 3, y.numel(), DEV, exclude=y)
    m = rng.feature_mask(y.numel(), 2, DEV)
    assert not torch.any(t == y).item() and int(t.min()) >= 0 and int(t.max()) <= 2
    assert torch.all((m == 0) | (m == 1)).item()
    assert abs(m.mean().item() - 0.5) < 0.05
