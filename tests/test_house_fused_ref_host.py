"""CPU, no device: (1) the float64 segment references of tests/house_fused_ref.py, chained, are oracle/house_ref.py's ResidualGenerator
and Discriminator to rtol 1e-9 (values, and float64 autograd for the critic's hand-written backward); (2) the case tables of
tests/test_hip_house_fused_edges.py hold their own conditions — every layout is one `_fused_ok` sends to the fused kernels, every row
count sits where its comment says against the block sizes of the constants block; (3) the hard-sample cases are decided: at most
0.5 % of their (row, head) pairs have a float64 top-two gap below max(1e-5, 100 max|p32 - p64|); (4) the derived bounds are no
looser than the 2e-5-of-scale tolerances tests/test_hip_house.py gives the same outputs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import house_fused_ref as R  # noqa: E402
from oracle import house_ref as HR  # noqa: E402


def _close(a, b, msg):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=msg)


_oracle, _oracle_run = R.oracle_generator, R.oracle_run


@pytest.mark.parametrize("name", list(R.LAYOUTS))
@pytest.mark.parametrize("rows", [17, 65, 129])
def test_chained_generator_segments_are_the_oracle_generator(name, rows):
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    G, cfg = _oracle(name, sd, torch.float64)
    cont, logits, soft = _oracle_run(G, cfg, x.double(), onehot.double(), mask.double(), noise.double())
    sd64 = {k: v.double() for k, v in sd.items()}
    out = R.generator_forward(sd64, x.double(), onehot.double(), mask.double(), noise.double(), 0.5)
    _close(out["cont"], cont, "cont"); _close(out["logits"], logits, "logits"); _close(out["soft"], soft, "soft")
    # the running statistics one forward leaves, against torch's BatchNorm1d (first layer: its input is the reference's own z1)
    _, h, _ = R.g_entry(sd64, x.double(), onehot.double(), mask.double())
    z1, _ = R.g_fc1(sd64, 0, h)
    st = R.bn_finish(R.block_sums(z1)[0], z1, rows, 1e-5, 0.1, sd64["blocks.0.bn1.running_mean"], sd64["blocks.0.bn1.running_var"])
    np.testing.assert_allclose(st["rm"].numpy(), G.blocks[0].bn1.running_mean.numpy(), rtol=1e-7, atol=1e-9)   # momentum is float32(0.1)
    np.testing.assert_allclose(st["rv"].numpy(), G.blocks[0].bn1.running_var.numpy(), rtol=1e-7, atol=1e-9)
    two = R.stats_bound(z1, 1e-5)
    _close(st["mean"], two["mean"], "mean from the pivoted sums"); _close(st["inv"], two["invstd"], "invstd from the pivoted sums")


@pytest.mark.parametrize("form", ["all", "training", "no-samples", "no-cont", "cont-only"])
@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_chained_backward_segments_are_float64_autograd_of_the_oracle(name, form):
    rows = 65
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    G, cfg = _oracle(name, sd, torch.float64)
    x, onehot, mask, noise = x.double(), onehot.double(), mask.double(), noise.double()
    cont, logits, soft = _oracle_run(G, cfg, x, onehot, mask, noise)
    g = torch.Generator().manual_seed(rows)
    dc, dl, ds = (torch.randn(v.shape, generator=g, dtype=torch.float64) for v in (cont, logits, soft))
    dc, dl, ds = R.cotangent_form(form, dc, dl, ds)
    outs, cots = zip(*[(o, c) for o, c in ((cont, dc), (logits, dl), (soft, ds)) if c is not None])
    torch.autograd.backward(list(outs), list(cots))
    sd64 = {k: v.double() for k, v in sd.items()}
    seg = R.seg_of(R.LAYOUTS[name][0])
    f = R.chain_forward_saved(sd64, x, onehot, mask)
    grads = R.chain_backward(sd64, seg, f, soft.detach(), dc, dl, ds, 0.5, 0.1)
    want = {n: p.grad if p.grad is not None else torch.zeros_like(p) for n, p in G.named_parameters()}      # no path: None
    assert set(grads) == set(want)
    scale = max(float(v.abs().max()) for v in want.values())      # (a bias in front of a BatchNorm has gradient 0 but for rounding)
    for n in want:
        np.testing.assert_allclose(grads[n].numpy(), want[n].numpy(), rtol=1e-9, atol=1e-9 * scale, err_msg=n)


def test_pivoted_block_sums_fold_back_to_the_plain_sums():
    g = torch.Generator().manual_seed(3)
    z = (40.0 + torch.randn(577, 32, generator=g)).double()
    s, q = R.fold_pivots(R.block_sums(z)[0], z, 577)
    _close(s, z.sum(0), "sum"); _close(q, (z * z).sum(0), "sum of squares")
    st = R.stats_bound(z, 1e-5)
    assert float(st["ratio"].min()) > 30 and float((st["invstd_bound"] / st["invstd"]).max()) < 2e-5 < R.plain_sums_invstd_rel_bound_at(30.0)
    assert abs(R.plain_sums_invstd_rel_bound_at(R.plain_sums_crossing()) - 2e-5) < 1e-12 and 4.8 < R.plain_sums_crossing() < 4.9


@pytest.mark.parametrize("rows", [5, 33])
def test_chained_critic_layers_are_the_oracle_critic(rows):
    torch.manual_seed(rows)
    D = HR.Discriminator(17, 32, 4).double().eval()
    for m in D.net:
        if isinstance(m, torch.nn.LeakyReLU):
            m.negative_slope = float(np.float32(0.2))           # the C float the kernel is handed
    g = torch.Generator().manual_seed(rows)
    x = torch.rand(rows, 17, generator=g, dtype=torch.float64).requires_grad_(True)
    onehot = F.one_hot(torch.randint(0, 4, (rows,), generator=g), 4).double()
    out = D(x, onehot)
    lin = [m for m in D.net if isinstance(m, torch.nn.Linear)]
    ws, bs = [m.weight.detach() for m in lin], [m.bias.detach() for m in lin]
    dout = torch.randn(rows, 1, generator=g, dtype=torch.float64)
    a, _ = R.critic_forward(ws, bs, x.detach(), onehot, 0.2)
    _close(a[4], out, "out")
    dx, = torch.autograd.grad(out, x, dout)
    d, _ = R.critic_backward(ws, a[1:4], dout, 0.2, 17)
    _close(d[3], dx, "dx")


@pytest.mark.parametrize("rows", [5, 33])
def test_chained_classifier_layers_are_the_folded_oracle_classifier(rows):
    """nn_classifier.py in eval mode, float64, BatchNorm statistics off their defaults; each BatchNorm folded into the Linear behind it."""
    torch.manual_seed(rows)
    clf = HR.NNClassifier(17, 4).double().eval()
    g = torch.Generator().manual_seed(rows)
    lin, bns = [m for m in clf.net if isinstance(m, torch.nn.Linear)], [m for m in clf.net if isinstance(m, torch.nn.BatchNorm1d)]
    for m in clf.net:
        if isinstance(m, torch.nn.LeakyReLU):
            m.negative_slope = R.CLS_SLOPE
    for bn in bns:
        bn.running_mean.copy_(0.2 * torch.randn(bn.num_features, generator=g, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g, dtype=torch.float64))
        bn.weight.data.copy_(1.0 + 0.2 * torch.randn(bn.num_features, generator=g, dtype=torch.float64))
        bn.bias.data.copy_(0.2 * torch.randn(bn.num_features, generator=g, dtype=torch.float64))
    ws, bs = [lin[0].weight.detach()], [lin[0].bias.detach()]
    for bn, l in zip(bns, lin[1:]):
        s = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        ws.append(l.weight.detach() * s)
        bs.append(l.bias.detach() + l.weight.detach() @ (bn.bias.detach() - bn.running_mean * s))
    assert [tuple(w.shape) for w in ws] == [(o, i) for i, o in zip(R.CLS_WIDTHS, R.CLS_WIDTHS[1:])]
    x = torch.rand(rows, 17, generator=g, dtype=torch.float64).requires_grad_(True)
    logits = clf(x)
    acts, _ = R.classifier_forward(ws, bs, x.detach())
    _close(acts[4], logits, "logits")
    dl = torch.randn(rows, 4, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(logits, x, dl)
    got, _ = R.classifier_backward(ws, acts[:4], dl)
    _close(got, dx, "dx")
    t = torch.randint(0, 4, (rows,), generator=g)
    rowsv, _, dz, _ = R.cross_entropy_rows(logits.detach(), t, 1.0)
    z = logits.detach().requires_grad_(True)
    loss = F.cross_entropy(z, t)
    _close(rowsv.mean(), loss, "cross-entropy")
    _close(dz, torch.autograd.grad(loss, z)[0], "cross-entropy gradient")
    km = R.pack_kmajor([w.float() for w in ws])
    assert [tuple(k.shape) for k in km] == [(20, 256), (256, 256), (256, 128), (128, 64), (4, 64)] and bool((km[0][17:] == 0).all())


def test_case_tables_hold_their_own_conditions():
    from pcgan_amd import house as H
    ceil = lambda a, b: (a + b - 1) // b  # noqa: E731
    for name, (widths, ncont) in R.LAYOUTS.items():
        cfg = R.layout_config(name)
        G = H.ResidualGenerator(R.DIN, R.HH, R.NCLS, cfg["continuous_idx"], cfg["categorical_info"]).train()
        assert G._fused_ok() and G._eval_dims_ok(), name
        assert [G.seg[i + 1] - G.seg[i] for i in range(len(widths))] == widths and len(G.continuous_idx) == ncont, name
        assert 1 <= len(widths) <= R.MAXHEADS and max(widths) <= R.MAXW and sum(widths) <= R.MAXT and sum(widths) + ncont <= R.MAXCOLS
    assert R.LAYOUTS["house"][0] == [H.CONFIG["categorical_info"][f]["n"] for f in H.CONFIG["categorical_info"]]
    assert R.layout_config("house")["continuous_idx"] == H.CONFIG["continuous_idx"]
    w, nc = R.LAYOUTS["full"]
    assert sum(w) + nc == R.MAXCOLS and ceil(sum(w) + nc, 16) == 6 and sorted((ceil(v, 2), v - ceil(v, 2)) for v in set(w)) == [(16, 15), (16, 16)]
    w, nc = R.LAYOUTS["narrow"]
    assert len(w) == R.MAXHEADS and len(w) * R.HEAD_ROWS == R.PAIRS_PER_ROUND and w.count(1) >= 2 and sum(w) < 16 < sum(w) + nc
    w, nc = R.LAYOUTS["single"]
    assert len(w) == 1 and w[0] > 16 and (w[0] + nc) % 16 == 1 and len(w) * R.HEAD_ROWS == 16 < 32     # waves 1-3 start past the last pair
    for rows, claim in R.GEN_ROWS.items():
        assert rows >= 2 and claim == (ceil(rows, R.SEG_ROWS), rows - (ceil(rows, R.SEG_ROWS) - 1) * R.SEG_ROWS,
                                       ceil(rows, R.HEAD_ROWS), rows - (ceil(rows, R.HEAD_ROWS) - 1) * R.HEAD_ROWS), rows
    assert max(R.GEN_ROWS) == 577 and R.GEN_ROWS[577][0] > R.PLOAD_PARTS
    for b in (R.HEAD_ROWS, R.SEG_ROWS):
        assert {b - 1, b, b + 1} <= set(R.GEN_ROWS)
    for table, b in ((R.CRITIC_ROWS_CASES, R.CRITIC_ROWS), (R.CLS_ROWS_CASES, R.CLS_ROWS)):
        for rows, claim in table.items():
            assert claim == (ceil(rows, b), rows - (ceil(rows, b) - 1) * b), rows
        assert {1, b - 1, b, b + 1} <= set(table)
    assert {(n, r) for n, r in R.GEN_FWD_CASES} >= {("house", r) for r in R.GEN_ROWS} | {(n, r) for n in R.LAYOUTS for r in (17, 65, 577)}
    assert all(r <= 577 for _, r in R.GEN_FWD_CASES + R.GEN_BWD_CASES)


@pytest.mark.parametrize("name,rows", R.GEN_FWD_CASES, ids=[f"{n}-{r}" for n, r in R.GEN_FWD_CASES])
def test_hard_sample_cases_are_decided_on_the_reference_alone(name, rows):
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    G32, cfg = _oracle(name, sd, torch.float32)
    G64, _ = _oracle(name, sd, torch.float64)
    with torch.no_grad():
        p32 = _oracle_run(G32, cfg, x, onehot, mask, noise)[2]
        p64 = _oracle_run(G64, cfg, x.double(), onehot.double(), mask.double(), noise.double())[2]
    und = R.undecided(p64, p32, R.seg_of(R.LAYOUTS[name][0]))
    assert und.float().mean().item() <= 0.005, (name, rows, int(und.sum()), und.numel())


@pytest.mark.parametrize("name,rows", R.GEN_FWD_CASES, ids=[f"{n}-{r}" for n, r in R.GEN_FWD_CASES])
def test_derived_bounds_are_no_looser_than_the_older_tolerances(name, rows):
    """tests/test_hip_house.py holds cont, logits and samples to rtol 2e-5 + 2e-5 max|tensor| and the BatchNorm buffers to
    rtol 1e-5 + 1e-6.  Every forward case; all ten BatchNorm layers: the rounding of the update (bn_finish) plus what the float32
    block sums add against the two-pass statistics (stats_bound)."""
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    sd64 = {k: v.double() for k, v in sd.items()}
    x, onehot, mask, noise = x.double(), onehot.double(), mask.double(), noise.double()
    f = R.chain_forward_saved(sd64, x, onehot, mask)
    h5 = f["H"][R.NBLK].float().double()
    logits, e_l, cont, e_c = R.g_heads(sd64, h5, 0.1)
    assert bool((e_l <= 2e-5 * logits.abs() + 2e-5 * float(logits.abs().max())).all())
    assert bool((e_c <= 2e-5 * cont.abs() + 2e-5 * float(cont.abs().max())).all())
    soft = R.soft_samples(logits, noise, 0.5, R.seg_of(R.LAYOUTS[name][0]))
    assert R.SOFT_RTOL <= 2e-5 and R.SOFT_ATOL <= 2e-5 * float(soft.max())
    m = float(np.float32(0.1))
    for k in range(R.NBLK):
        for j, z, bn in ((2 * k, f["Z1"][k], "bn1"), (2 * k + 1, f["Z2"][k], "bn2")):
            z = z.float().double()
            st = R.bn_finish(R.block_sums(z)[0], z, rows, 1e-5, 0.1, sd64[f"blocks.{k}.{bn}.running_mean"], sd64[f"blocks.{k}.{bn}.running_var"])
            two = R.stats_bound(z, 1e-5)
            assert bool((m * two["mean_bound"] + st["rm_bound"] <= 1e-5 * st["rm"].abs() + 1e-6).all()), (j, "running_mean")
            assert bool((m * two["var_bound"] * rows / (rows - 1.0) + st["rv_bound"] <= 1e-5 * st["rv"].abs() + 1e-6).all()), (j, "running_var")
