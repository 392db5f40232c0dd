"""GPU: the image sheets (csrc/image_sheet.hip, pcgan_amd.sheets) against the torch-CPU restatement of make_grid /
save_image (tests/sheet_restate.py), BIT FOR BIT (torch.equal: the sign of a zero does not count): the float grid, the uint8 image and
the device range, over odd sizes, a misaligned first element, partly empty rows, one image, the trainers' own shapes and a batch large
enough for many workgroups in the range pass; value sets that order negative numbers, a constant tensor, an extremum in the last
unaligned element and a tensor on which a reciprocal product differs from the division; the reference's recorded original.png; a
captured range + sheet pair replayed on new contents; and the call each trainer makes."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sheet_restate as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [((7, 3, 9, 5), 8), ((5, 1, 28, 28), 4), ((3, 1, 28, 28), 8), ((1, 1, 28, 28), 8), ((25, 1, 28, 28), 5), ((64, 1, 64, 64), 8)]
NORMS = [dict(normalize=False), dict(normalize=True), dict(normalize=True, value_range=(-0.5, 0.5))]
PRES = [(1.0, 0.0), (0.5, 0.5)]


@pytest.fixture(scope="module")
def S():
    import pcgan_amd
    pcgan_amd.load()
    return pcgan_amd.sheets


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "sheets_ref.npz")))


def _misaligned(t):
    """The same values on the device, contiguous, with the first element 4 bytes past a 16-byte boundary."""
    base = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _check(S, x_cpu, x_dev, **kw):
    want = SR.make_grid(x_cpu, **kw)
    want_u8 = SR.to_u8(want)
    grid = S.make_grid(x_dev, **kw)
    u8, grid2, rng = S.sheet_u8(x_dev, with_grid=True, with_range=True, **kw)
    assert grid.shape == want.shape and grid.dtype == torch.float32 and u8.shape == want_u8.shape and u8.dtype == torch.uint8
    assert torch.equal(grid.cpu(), want), kw
    assert torch.equal(grid2.cpu(), want), kw
    assert torch.equal(u8.cpu(), want_u8), kw
    assert torch.equal(S.sheet_u8(x_dev, **kw).cpu(), want_u8), kw                       # the uint8 image alone
    if kw.get("normalize") and kw.get("value_range") is None:
        assert torch.equal(rng.cpu(), SR.image_range(x_cpu, kw.get("pre", (1.0, 0.0)))), kw
    else:
        assert rng is None
    return want


@pytest.mark.parametrize("shape,nrow", SHAPES, ids=[str(s) for s, _ in SHAPES])
def test_sheets_equal_the_restatement(S, shape, nrow):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    x_dev = _misaligned(x) if shape[1] == 3 else x.to(DEV)
    for padding, pad_value, norm, pre in itertools.product((0, 2, 5), (0.0, 0.5), NORMS, PRES):
        want = _check(S, x, x_dev, nrow=nrow, padding=padding, pad_value=pad_value, pre=pre, **norm)
        assert tuple(want.shape[1:]) == S.grid_shape(shape[0], shape[2], shape[3], nrow, padding)
    if shape[1] == 1:                                                                    # the gray image: one byte per pixel
        gray = S.sheet_u8(x_dev, nrow=nrow, normalize=True, gray=True)
        assert torch.equal(gray.cpu(), SR.sheet_u8(x, nrow=nrow, normalize=True)[:, :, 0])
    assert torch.equal(S.image_range(x_dev).cpu(), SR.image_range(x))
    assert torch.equal(S.image_range(x_dev, pre=(0.5, 0.5)).cpu(), SR.image_range(x, (0.5, 0.5)))


def _value_sets(shape):
    g = torch.Generator().manual_seed(11 + shape[0])
    x = torch.randn(shape, generator=g)
    sets = {"negative": -x.abs() - 0.125, "positive": x.abs() + 0.125, "mixed": x, "constant": torch.full(shape, 0.3)}
    hi_last, lo_last = x.clone(), x.clone()
    hi_last.view(-1)[-1], lo_last.view(-1)[-1] = 9.5, -9.5
    sets["max in the last element"], sets["min in the last element"] = hi_last, lo_last
    lo_first = x.clone()
    lo_first.view(-1)[0] = -9.5
    sets["min in the first element"] = lo_first
    return sets


@pytest.mark.parametrize("shape,nrow", [((7, 3, 9, 5), 8), ((64, 1, 64, 64), 8)], ids=["tails", "many blocks"])
def test_range_pass_orders_every_value_set(S, shape, nrow):
    for name, x in _value_sets(shape).items():
        x_dev = _misaligned(x)                                                           # 3 head elements, and a scalar tail
        rng = S.image_range(x_dev).cpu()
        assert torch.equal(rng, torch.stack([x.min(), x.max()])), name
        want = _check(S, x, x_dev, nrow=nrow, normalize=True)
        _check(S, x, x_dev, nrow=nrow, normalize=True, pre=(0.5, 0.5))
        if name == "constant":
            assert not want[:, 2:2 + shape[2], 2:2 + shape[3]].any() and float(rng[0]) == float(rng[1])
        if name == "negative":
            assert float(rng[1]) < 0.0
        if name == "positive":
            assert float(rng[0]) > 0.0


def test_the_kernel_divides(S):
    """On this tensor x * (1 / d) and x / d differ on the CPU (asserted first): a kernel that multiplied by a reciprocal would not
    reproduce the restatement."""
    found = None
    for seed in range(20):
        x = torch.randn((16, 1, 28, 28), generator=torch.Generator().manual_seed(seed))
        lo, hi = x.min(), x.max()
        d = torch.tensor(max(float(hi) - float(lo), 1e-5), dtype=torch.float64).to(torch.float32)
        num = x - lo
        if not torch.equal(num / torch.full_like(num, float(d)), num * (torch.tensor(1.0) / d)):
            found = x
            break
    assert found is not None, "no tensor among 20 seeds tells the reciprocal form from the division"
    _check(S, found, found.to(DEV), nrow=4, normalize=True)


def test_reference_pin_on_the_device(S, gold):
    rec = gold["countergan.original"]
    cells = SR.cells(rec, 16, 4, 28, 28)
    x = torch.from_numpy((cells.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).view(16, 1, 28, 28)
    u8 = S.sheet_u8(x.to(DEV), nrow=4, normalize=True)
    assert u8.shape == (122, 122, 3) and np.array_equal(u8.cpu().numpy(), rec)


def test_graph_replay_on_new_contents(S):
    from pcgan_amd._graphed import Held, capture_steps
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(3)
    buf = torch.randn((25, 1, 28, 28), generator=g).to(DEV)
    (graph, (u8, grid, rng)), = capture_steps([(lambda: S.sheet_u8(buf, nrow=5, normalize=True, with_grid=True, with_range=True), 1)], Held(), dev)
    for scale, shift in ((3.0, -1.0), (0.25, 4.0)):                                      # the range moves with every refill
        fresh = torch.randn((25, 1, 28, 28), generator=g) * scale + shift
        buf.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        e_u8, e_grid, e_rng = S.sheet_u8(buf, nrow=5, normalize=True, with_grid=True, with_range=True)
        assert torch.equal(u8, e_u8) and torch.equal(grid, e_grid) and torch.equal(rng, e_rng)
        assert torch.equal(grid.cpu(), SR.make_grid(fresh, nrow=5, normalize=True))
        assert torch.equal(rng.cpu(), SR.image_range(fresh))


def test_save_image_writes_the_pixels_it_returns(S, tmp_path):
    from PIL import Image
    x = torch.randn((5, 3, 6, 7), generator=torch.Generator().manual_seed(2))
    path = str(tmp_path / "d" / "s.png")
    u8 = S.save_image(x.to(DEV), path, nrow=2, padding=1, normalize=True, pad_value=0.5)
    assert isinstance(u8, np.ndarray) and np.array_equal(u8, SR.sheet_u8(x, nrow=2, padding=1, normalize=True, pad_value=0.5).numpy())
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), u8)


def test_misuse_is_refused(S):
    from pcgan_amd import PcgError
    x = torch.zeros((4, 1, 8, 8), device=DEV)
    bad = [x.cpu(), x.half(), x.double(), torch.zeros((4, 1, 8, 16), device=DEV)[:, :, :, ::2], torch.zeros((4, 2, 8, 8), device=DEV),
           torch.zeros((0, 1, 8, 8), device=DEV), torch.zeros((2, 2, 1, 8, 8), device=DEV)]
    for t in bad:
        for call in (S.make_grid, S.sheet_u8):
            with pytest.raises(PcgError):
                call(t)
    for t in bad[:4]:
        with pytest.raises(PcgError):
            S.image_range(t)
    for kw in (dict(nrow=0), dict(padding=-1), dict(normalize=True, value_range=(1.0, 0.0))):
        with pytest.raises(PcgError):
            S.make_grid(x, **kw)
    with pytest.raises(PcgError):
        S.sheet_u8(torch.zeros((2, 3, 4, 4), device=DEV), gray=True)
    nan = torch.full((2, 1, 4, 4), float("nan"), device=DEV)                             # unspecified pixels, but no fault
    assert S.sheet_u8(nan, normalize=True).shape == (8, 14, 3)
    torch.cuda.synchronize()


# ---- the trainers' calls -----------------------------------------------------------------------------------------------------------------
def _dcgan_run(D, gold, grid):
    cfg = {"g_hidden": int(gold["meta.g_hidden"]), "d_hidden": int(gold["meta.d_hidden"]), "z_dim": int(gold["meta.z_dim"]),
           "batch_size": int(gold["meta.batch"]), "epochs": int(gold["meta.epochs"])}
    netG, netD = D.Generator(cfg), D.Discriminator(cfg)
    netG.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.G.")})
    netD.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in gold.items() if k.startswith("init.D.")})
    netG.to(DEV); netD.to(DEV)
    data = [(torch.from_numpy(gold[f"data.{k}"]),) for k in range(int(gold["meta.nbatches"]))]
    torch.manual_seed(int(gold["meta.loop_seed"]))
    return D.train(data, cfg, netG=netG, netD=netD, device=DEV, log=lambda s: None, grid=grid), data


def test_dcgan_train_keeps_the_grids(S, golden_dir):
    from pcgan_amd import dcgan as D
    gold = dict(np.load(os.path.join(golden_dir, "dcgan_loop_small.npz")))
    raw, data = _dcgan_run(D, gold, False)
    out, _ = _dcgan_run(D, gold, True)
    assert out["epoch_G_losses"] == raw["epoch_G_losses"] and out["epoch_D_losses"] == raw["epoch_D_losses"] and out["iters"] == raw["iters"]
    assert len(out["img_list"]) == len(raw["img_list"]) == 2
    for img, batch in zip(out["img_list"], raw["img_list"]):
        assert not img.is_cuda and img.shape == (3,) + S.grid_shape(batch.shape[0], 64, 64)
        assert torch.equal(img, SR.make_grid(batch, padding=2, normalize=True))
    real = data[0][0]
    assert torch.equal(D.real_grid(real, DEV).cpu(), SR.make_grid(real[:64], padding=5, normalize=True))


@pytest.mark.parametrize("module", ["gan_train", "countergan2"])
def test_save_examples(module, tmp_path):
    import importlib

    from PIL import Image
    T = importlib.import_module(f"pcgan_amd.{module}")
    torch.manual_seed(4)
    G = T.Generator().to(DEV)
    x = (torch.rand((16, 1, 28, 28), generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV)
    target = torch.full((16,), 3, dtype=torch.int64, device=DEV)
    got = T.save_examples(G, x, 3, str(tmp_path))
    cf, delta = T.counterfactual_batch(G, x, target)
    want = (SR.sheet_u8(x, nrow=4, normalize=True), SR.sheet_u8(cf, nrow=4, normalize=True),
            SR.sheet_u8(delta.reshape(16, 1, 28, 28), nrow=4, normalize=True, pre=(0.5, 0.5)))
    assert torch.equal(want[2], SR.sheet_u8(delta.reshape(16, 1, 28, 28).cpu() * 0.5 + 0.5, nrow=4, normalize=True))   # deltas * 0.5 + 0.5
    for name, g, w in zip(("original", "counterfactual", "delta"), got, want):
        assert g.shape == (122, 122, 3) and np.array_equal(g, w.numpy()), name
        with Image.open(str(tmp_path / f"{name}.png")) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), g), name


def test_wgan_class_grid_and_train_grids(S):
    from pcgan_amd import ops
    from pcgan_amd import wgan as W
    dev = torch.device(DEV)
    hp = W.Hyperparameter(critic_size=16, generator_size=16, critic_hidden_size=16, batchsize=8, n_critic=2)
    critic, generator = W.build(dev, hp, seed=1)
    noise = torch.randn((80, hp.latent_size), generator=torch.Generator().manual_seed(8)).to(DEV)
    grid = W.class_grid(generator, hp, noise)
    classes = torch.tensor([k for k in range(10) for _ in range(8)], dtype=torch.int64, device=DEV)      # [0] * 8 + [1] * 8 + ...
    with torch.no_grad():
        fake = generator(noise, ops.onehot(classes, 10))
        other = generator(noise, ops.onehot(classes.flip(0).contiguous(), 10))
    assert grid.shape == (3, 302, 242) and torch.equal(grid.cpu(), SR.make_grid(fake, padding=2, normalize=True))
    assert not torch.equal(grid.cpu(), SR.make_grid(other, padding=2, normalize=True))
    small = W.class_grid(generator, hp, noise[:20], per_class=2)
    assert small.shape == (3,) + S.grid_shape(20, 28, 28)
    data = [(torch.rand(8, 1, 28, 28) * 2 - 1, torch.randint(0, 10, (8,))) for _ in range(3)]
    grids = []
    hist = W.train(critic, generator, data, hp, dev, rng=ops.DeviceRNG(3), epochs=1, grid_every=2, img_list=grids, fixed_noise=noise)
    assert len(hist) == 1 and len(grids) == 2                                            # iterations 0 and 2 (also the last)
    assert all(not g.is_cuda and g.shape == (3, 302, 242) and float(g.max()) == 1.0 and float(g.min()) == 0.0 for g in grids)
    assert W.train(critic, generator, data, hp, dev, rng=ops.DeviceRNG(3), epochs=1) and len(grids) == 2
    with pytest.raises(W.PcgError):
        W.train(critic, generator, data, hp, dev, epochs=1, grid_every=2)


def test_mnist_gan_writes_the_epoch_sheet(tmp_path):
    from PIL import Image
    from pcgan_amd import mnist_gan as M
    from pcgan_amd.data import DeviceLoader
    torch.manual_seed(9)
    G, D = M.Generator().to(DEV), M.Discriminator().to(DEV)
    x = (torch.rand((96, 1, 28, 28), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    loader = DeviceLoader(x, torch.zeros(96, device=DEV), 32, shuffle=True, seed=2)
    losses = M.train(G, D, loader, epochs=1, image_dir=str(tmp_path / "images"))
    assert len(losses) == 1 and sorted(os.listdir(tmp_path / "images")) == ["1.png"]
    generated = M._workspace(G, D, 32, torch.device(DEV)).X[32:64].view(32, 1, 28, 28)   # the last step's generated batch
    with Image.open(str(tmp_path / "images" / "1.png")) as im:
        assert im.size == (152, 152) and np.array_equal(np.asarray(im), SR.sheet_u8(generated[:25], nrow=5, normalize=True).numpy())
