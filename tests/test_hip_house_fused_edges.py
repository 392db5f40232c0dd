"""GPU: the fused tabular MFMA kernels (csrc/house_fused.hip, house_critic_fused.hip, house_classifier_fused.hip) against float64, segment by segment, at the
block and head edges.  References and bounds: tests/house_fused_ref.py (teacher-forced: every segment is recomputed in float64 from
the device's own inputs of that segment and held to the bound derived from the kernel's arithmetic); the case tables and what each
row count and layout pins are there too, and tests/test_house_fused_ref_host.py checks them without a device.

Every float32 buffer the launches allocate is, for the duration of a launch, carved out of a sentinel-filled allocation with a
sentinel tail (`_Guarded`): an element the kernels were to write and did not shows as the sentinel, a write past the end shows in
the tail.  Inputs are compared with a copy afterwards.

Tolerances: derived in house_fused_ref.py (`within`), except
  soft samples              rtol 2e-5, atol 1e-7   test_gumbel_softmax_heads_and_residual_assembly (tests/test_hip_house.py)
  offset BatchNorm channel  house_fused_ref.stats_bound; measured figures in test_batchnorm_constant_and_offset_channels' docstring"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import house_fused_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0e30
TAIL = 64


@pytest.fixture(scope="module")
def pcg():
    import pcgan_amd
    from pcgan_amd import house  # noqa: F401
    return pcgan_amd


def _dev(t):
    return t.to(DEV).contiguous()


class _Guarded:
    """While active, every float32 torch.empty on the GPU is a view into a sentinel-filled allocation with TAIL sentinels behind it."""

    def __enter__(self):
        self.orig, self.flats = torch.empty, []
        torch.empty = self._empty
        return self

    def __exit__(self, *exc):
        torch.empty = self.orig

    def _empty(self, *size, **kw):
        dev = kw.get("device")
        if kw.get("dtype") is torch.float32 and dev is not None and torch.device(dev).type == "cuda" and set(kw) <= {"dtype", "device"}:
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
            n = int(np.prod(shape)) if shape else 1
            flat = self.orig(n + TAIL, **kw).fill_(SENT)
            self.flats.append((flat, n))
            return flat[:n].view(shape)
        return self.orig(*size, **kw)

    def check_tails(self, what, outputs=()):
        """The tails are intact, and every tensor of `outputs` is one of the guarded allocations (else its checks prove nothing)."""
        assert self.flats, what
        for flat, n in self.flats:
            assert bool((flat[n:] == SENT).all()), f"{what}: a write past the end of a buffer of {n} elements"
        mine = {(flat.data_ptr(), n) for flat, n in self.flats}
        for t in outputs:
            assert (t.data_ptr(), t.numel()) in mine, f"{what}: an output of {tuple(t.shape)} was not allocated between sentinels"


def _written(what, t):
    assert bool((t != SENT).all()), f"{what}: {int((t == SENT).sum())} elements were never written"


def within(what, dev, ref, bound, report=None):
    """|dev - ref| <= bound, element by element (bound 0: equal).  Prints the largest used share of the bound."""
    d = (R.d64(dev) - ref).abs()
    assert d.shape == bound.shape, (what, d.shape, bound.shape)
    share = float((d / bound.clamp_min(1e-300)).max())
    if report is not None:
        report.append((what, share))
    assert share <= 1.0, f"{what}: {share:.2f} x the bound at {int((d / bound.clamp_min(1e-300)).argmax())}, |diff| {float(d.max()):.3e}"


def _generator(pcg, name, sd):
    H = pcg.house
    cfg = R.layout_config(name)
    G = H.ResidualGenerator(R.DIN, R.HH, R.NCLS, cfg["continuous_idx"], cfg["categorical_info"], tau=0.5)
    G.load_state_dict(sd)
    G.to(DEV).train()
    G._ensure_flat()
    assert G._fused_ok(), name
    return G


def _bns(G):
    return [bn for blk in G.blocks for bn in (blk.bn1, blk.bn2)]


def _forward(G, x, onehot, mask, noise, hard):
    ins = [_dev(t) for t in (x, onehot, mask, noise)]
    keep = [t.clone() for t in ins]
    with _Guarded() as g:
        cont, logits, samples, saved = G._fused_forward(*ins, 0.5, hard)
        torch.cuda.synchronize()
    g.check_tails("forward", [t for t in saved[1].values() if t is not None])
    for a, b in zip(ins, keep):
        assert torch.equal(a, b), "the forward changed an input"
    buf = saved[1]
    for n, t in buf.items():
        if t is not None:
            _written(n, t)
    return buf, saved, ins


def _check_forward(sd, buf, x, onehot, mask, noise, B, running0, running1, seg, report):
    """Every saved tensor of one forward against its segment reference.  running0 / running1: the ten (mean, var, nbt) before / after."""
    sd = {k: v.double() for k, v in sd.items()}
    x, onehot, mask, noise = (t.double() for t in (x, onehot, mask, noise))
    cond = torch.cat([onehot, mask], 1)
    H, Z1, Z2, P, SM = (R.d64(buf[n]) for n in ("H", "Z1", "Z2", "P", "SM"))
    inp, h0, e = R.g_entry(sd, x, onehot, mask)
    assert torch.equal(R.d64(buf["inp"]), inp), "inp"
    within("H[0]", H[0], h0, e, report)
    for k in range(R.NBLK):
        z1, e = R.g_fc1(sd, k, H[k])
        within(f"Z1[{k}]", Z1[k], z1, e, report)
        for j, z in ((2 * k, Z1[k]), (2 * k + 1, Z2[k])):
            if j == 2 * k + 1:
                z2, e, _ = R.g_seg_a(sd, k, cond, Z1[k], SM[2 * k, 0], SM[2 * k, 1])
                within(f"Z2[{k}]", Z2[k], z2, e, report)
            p, e = R.block_sums(z)
            within(f"P[{j}]", P[j], p, e, report)
            st = R.bn_finish(P[j], z, B, 1e-5, 0.1, running0[j][0], running0[j][1])
            within(f"SM[{j}] mean", SM[j, 0], st["mean"], st["mean_bound"], report)
            within(f"SM[{j}] invstd", SM[j, 1], st["inv"], st["inv_bound"], report)
            within(f"running_mean[{j}]", running1[j][0], st["rm"], st["rm_bound"], report)
            within(f"running_var[{j}]", running1[j][1], st["rv"], st["rv_bound"], report)
            assert running1[j][2] == running0[j][2] + 1, f"num_batches_tracked[{j}]"
        hn, e = R.g_seg_b(sd, k, cond, Z2[k], SM[2 * k + 1, 0], SM[2 * k + 1, 1], H[k])
        within(f"H[{k + 1}]", H[k + 1], hn, e, report)
    logits, e_l, cont, e_c = R.g_heads(sd, H[R.NBLK], 0.1)
    within("logits", buf["logits"], logits, e_l, report)
    within("cont", buf["cont"], cont, e_c, report)
    soft = R.soft_samples(R.d64(buf["logits"]), noise, 0.5, seg)
    np.testing.assert_allclose(R.d64(buf["soft"]).numpy(), soft.numpy(), rtol=R.SOFT_RTOL, atol=R.SOFT_ATOL, err_msg="soft")
    for a, b in zip(seg, seg[1:]):
        if b - a == 1:
            assert bool((buf["soft"][:, a] == 1.0).all()), "a one-column head's soft sample is 1 exactly"


def _running(G):
    return [(R.d64(bn.running_mean), R.d64(bn.running_var), int(bn.num_batches_tracked)) for bn in _bns(G)]


def _check_hard(hard, soft, seg):
    hard, soft = hard.cpu(), soft.cpu()
    assert bool(((hard == 0) | (hard == 1)).all())
    for a, b in zip(seg, seg[1:]):
        assert bool((hard[:, a:b].sum(1) == 1).all()), f"head [{a}, {b}) is not one-hot"
    assert torch.equal(hard, R.first_max_onehot(soft, seg)), "hard is not the first maximum of the device's own soft sample"


@pytest.mark.parametrize("name,rows", R.GEN_FWD_CASES, ids=[f"{n}-{r}" for n, r in R.GEN_FWD_CASES])
def test_generator_forward_segments_vs_float64(pcg, name, rows):
    """Two forwards of one case: the first without hard samples, the second with them; the running statistics after one and after
    two, num_batches_tracked, every saved tensor, P per block, SM.  Hard samples: one-hot per head, the first maximum of the device's
    own soft sample exactly, and the float64 argmax on every decided pair."""
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    seg = R.seg_of(R.LAYOUTS[name][0])
    G = _generator(pcg, name, sd)
    report = []
    r0 = _running(G)
    assert all(r[2] == 3 for r in r0)
    buf, _, _ = _forward(G, x, onehot, mask, noise, False)
    assert buf["hard"] is None
    r1 = _running(G)
    _check_forward(sd, buf, x, onehot, mask, noise, rows, r0, r1, seg, report)
    buf2, _, _ = _forward(G, x, onehot, mask, noise, True)
    r2 = _running(G)
    _check_forward(sd, buf2, x, onehot, mask, noise, rows, r1, r2, seg, report)
    for n in ("inp", "H", "Z1", "Z2", "P", "SM", "cont", "logits", "soft"):
        assert torch.equal(buf[n], buf2[n]), f"{n}: the second forward of the same inputs differs"
    _check_hard(buf2["hard"], buf2["soft"], seg)
    G64, cfg = R.oracle_generator(name, sd, torch.float64)
    G32, _ = R.oracle_generator(name, sd, torch.float32)
    with torch.no_grad():
        p64 = R.oracle_run(G64, cfg, x.double(), onehot.double(), mask.double(), noise.double())[2]
        p32 = R.oracle_run(G32, cfg, x, onehot, mask, noise)[2]
    und = R.undecided(p64, p32, seg)
    want, got = R.first_max_onehot(p64, seg), buf2["hard"].cpu().double()
    for s, (a, b) in enumerate(zip(seg, seg[1:])):
        same = (want[:, a:b] == got[:, a:b]).all(1)
        assert bool((same | und[:, s]).all()), f"head {s}: a decided pair differs from the float64 argmax"
    worst = max(report, key=lambda t: t[1])
    print(f"\n{name}-{rows}: largest share of a bound {worst[1]:.3f} ({worst[0]})")


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_hard_sample_ties_pick_the_first_column_of_every_head(pcg, name):
    """Zero head weights, one bias per head, zero noise: every probability of a head is equal, in both lanes of the pair, and the
    first maximum is the head's first column — the `ob == best && oa < arg` exchange seen from the upper lane (which must give way)
    and from the lower (which must not)."""
    rows = 17
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    for i, k in enumerate(R.head_keys(sd)):
        sd[k + ".weight"] = torch.zeros_like(sd[k + ".weight"])
        sd[k + ".bias"] = torch.full_like(sd[k + ".bias"], 0.25 * (i + 1))
    seg = R.seg_of(R.LAYOUTS[name][0])
    G = _generator(pcg, name, sd)
    buf, _, _ = _forward(G, x, onehot, mask, torch.zeros_like(noise), True)
    for a, b in zip(seg, seg[1:]):
        assert bool((buf["soft"][:, a:b] == buf["soft"][:, a:a + 1]).all()), "the tie case is not a tie on the device"
    want = torch.zeros(rows, seg[-1])
    want[:, seg[:-1]] = 1.0
    assert torch.equal(buf["hard"].cpu(), want)


def _golden_ratio(pcg, golden_dir):
    """The largest |mean| / std over the ten BatchNorm inputs of the shipped generator on the golden batch, from the device's Z."""
    H = pcg.house
    hg = dict(np.load(os.path.join(golden_dir, "house_ref_b64.npz")))
    torch.manual_seed(0)
    G = H.ResidualGenerator(17, 32, 4, H.CONFIG["continuous_idx"], H.CONFIG["categorical_info"], tau=0.5)
    G.load_state_dict({k[7:]: torch.from_numpy(v.copy()) for k, v in hg.items() if k.startswith("init.G.")})
    G.to(DEV).train()
    G._ensure_flat()
    x, mask = torch.from_numpy(hg["in.x"]), torch.from_numpy(hg["in.mask"])
    onehot = torch.nn.functional.one_hot(torch.from_numpy(hg["in.target_y"]).long(), 4).float()
    noise = torch.cat([torch.from_numpy(hg[f"gumbel.{f}"]) for f in G.cat_idx], 1)
    buf, _, _ = _forward(G, x, onehot, mask, noise, False)
    z = torch.cat([R.d64(buf["Z1"]), R.d64(buf["Z2"])], 0)
    return float((z.mean(1).abs() / z.std(1, unbiased=False)).max())


def test_batchnorm_constant_and_offset_channels(pcg, golden_dir):
    """House layout, 129 rows, three doctored channels of the first BatchNorm (fc1 of block 0):
      3  constant: zero weight row, bias 0.5 — pivoted sums are exactly zero, mean 0.5 and var 0 exactly;
      5  constant, inexact: bias 1/3 — the segment's outputs are asserted (the whole forward check), invstd with them since the
         pivoted sums make var exactly 0 here too;
      7  offset: |mean| / std of the device's own Z in [20, 40] (asserted).  Its save_mean / invstd must meet stats_bound, the
         bound of the pivoted fp32 block sums, against the two-pass float64 statistics of the device's Z.
    Measured on an MI355X (ratio 29.37): relative error of invstd 3.35e-8 fused and 3.35e-8 for the fp64-summing chain
    (ops.bn_train_stats on the same Z; both one fp32 rounding), bound 6.4e-6; of the mean 1.1e-8 both, bound 1.2e-7.  The test prints
    the figures (DESIGN.md §3 has them too).  Plain fp32 sums of z and z^2 — the arithmetic before the pivot —
    are bounded by plain_sums_invstd_rel_bound_at: 7.5e-4 at ratio 30, 2e-5 at 4.85; the shipped nets reach 5.2 on the golden batch
    (asserted below), which is why the sums are pivoted."""
    rows, name = 129, "house"
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, h0, _ = R.g_entry(sd64, x.double(), onehot.double(), mask.double())
    W, b = sd["blocks.0.fc1.weight"], sd["blocks.0.fc1.bias"]
    W[3], b[3] = 0.0, 0.5
    W[5], b[5] = 0.0, 1.0 / 3.0
    W[7] *= 0.25
    zc = h0 @ W[7].double()
    b[7] = float(30.0 * zc.std(unbiased=False) - zc.mean())
    seg = R.seg_of(R.LAYOUTS[name][0])
    G = _generator(pcg, name, sd)
    r0 = _running(G)
    buf, _, _ = _forward(G, x, onehot, mask, noise, False)
    report = []
    _check_forward(sd, buf, x, onehot, mask, noise, rows, r0, _running(G), seg, report)
    Z, SM, P = R.d64(buf["Z1"][0]), R.d64(buf["SM"][0]), R.d64(buf["P"][0])
    assert bool((Z[:, 3] == 0.5).all()) and bool((P[:, :, 3] == 0).all()) and float(SM[0, 3]) == 0.5
    assert bool((P[:, :, 5] == 0).all()) and float(SM[0, 5]) == float(np.float32(1.0 / 3.0))
    inv0 = 1.0 / np.sqrt(float(np.float32(1e-5)))
    assert abs(float(SM[1, 3]) - inv0) <= R.U * inv0 and float(SM[1, 5]) == float(SM[1, 3])
    two = R.stats_bound(Z, 1e-5)
    ratio = float(two["ratio"][7])
    assert 20.0 <= ratio <= 40.0, ratio
    within("save_mean vs two-pass float64", SM[0], two["mean"], two["mean_bound"], report)
    within("invstd vs two-pass float64", SM[1], two["invstd"], two["invstd_bound"], report)
    ops = pcg.ops
    bn = torch.nn.BatchNorm1d(32).to(DEV)
    cm, ci = ops.bn_train_stats(buf["Z1"][0].contiguous(), 32, 1e-5, 0.1, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    rel = lambda a, ref: float(((R.d64(a) - ref).abs() / ref.abs())[7])  # noqa: E731
    print(f"\noffset channel: |mean|/std {ratio:.2f}; relative error of invstd: fused {rel(buf['SM'][0, 1], two['invstd']):.3e}, "
          f"fp64-summing chain {rel(ci, two['invstd']):.3e}, bound {float(two['invstd_bound'][7] / two['invstd'][7]):.3e}, "
          f"plain-sums bound {R.plain_sums_invstd_rel_bound_at(ratio):.3e}; of mean: fused {rel(buf['SM'][0, 0], two['mean']):.3e}, "
          f"chain {rel(cm, two['mean']):.3e}, bound {float(two['mean_bound'][7] / two['mean'][7].abs()):.3e}")
    gr = _golden_ratio(pcg, golden_dir)
    print(f"golden nets, golden batch: largest |mean|/std {gr:.3f}; plain fp32 sums reach 2e-5 at {R.plain_sums_crossing():.3f}")
    assert 5.0 < gr < 5.4 and gr > R.plain_sums_crossing() / 4.0          # the figures DESIGN.md §3 states


# ---- critic ------------------------------------------------------------------------------------------------------------------------
def _critic_case(rows, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(32, 21), (64, 32), (128, 64), (1, 128)]
    ws = [(2.0 * torch.rand(s, generator=g) - 1.0) / np.sqrt(s[1]) * 1.5 for s in shapes]
    x = torch.rand(rows, 17, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 4, (rows,), generator=g), 4).float()
    dout = torch.randn(rows, 1, generator=g)
    return ws, x, onehot, dout


def _critic_check(ws, bs, x, onehot, dout, acts, out, grads, need_dx, what):
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    dev_a = [R.d64(a) for a in acts]
    ref, e = R.critic_forward(w64, b64, x.double(), onehot.double(), 0.2, forced=dev_a)
    assert torch.equal(dev_a[0], ref[0]), f"{what}: a0"
    for l in (1, 2, 3):
        within(f"{what}: a{l}", acts[l], ref[l], e[l])
    within(f"{what}: out", out, ref[4], e[4])
    dev_d = [R.d64(d) for d in grads[:3]]
    dref, de = R.critic_backward(w64, dev_a[1:4], dout.double(), 0.2, 17, forced=dev_d)
    for i, n in enumerate(("d3", "d2", "d1")):
        within(f"{what}: {n}", grads[i], dref[i], de[i])
    if need_dx:
        within(f"{what}: dx", grads[3], dref[3], de[3])
    else:
        assert grads[3] is None


@pytest.mark.parametrize("need_dx", [True, False], ids=["dx", "no-dx"])
@pytest.mark.parametrize("rows", list(R.CRITIC_ROWS_CASES))
def test_critic_one_and_two_passes_vs_float64(pcg, rows, need_dx):
    """One pass, and two passes with different weights, inputs and cotangents in one launch (blockIdx.y): a0..a3, out, d3, d2, d1, dx
    within the derived bounds of float64 (LeakyReLU masks from the saved activations, as the kernel reads them), and the two-pass
    launch equal to two one-pass launches bit for bit."""
    ops = pcg.ops
    g = torch.Generator().manual_seed(7)
    bs = [0.1 * torch.randn(n, generator=g) for n in (32, 64, 128, 1)]
    cases = [_critic_case(rows, 100 + rows), _critic_case(rows, 200 + rows)]
    dbs = [_dev(b) for b in bs]
    dws = [[_dev(w) for w in c[0]] for c in cases]
    dx_, doh, ddo = ([_dev(c[i]) for c in cases] for i in (1, 2, 3))
    keep = [t.clone() for t in dx_ + doh + ddo + dws[0] + dws[1] + dbs]
    single = []
    for q in range(2):
        with _Guarded() as gd:
            (acts, out), = ops.house_critic_fwd([(dx_[q], doh[q])], dws[q], dbs)
            grads, = ops.house_critic_bwd([ddo[q]], dws[q], [acts], 17, need_dx)
            torch.cuda.synchronize()
        gd.check_tails(f"one pass {q}", acts + [out] + [t for t in grads if t is not None])
        for t in acts + [out] + [t for t in grads if t is not None]:
            _written(f"one pass {q}", t)
        _critic_check(cases[q][0], bs, cases[q][1], cases[q][2], cases[q][3], acts, out, grads, need_dx, f"pass {q} alone")
        single.append((acts, out, grads))
    with _Guarded() as gd:
        res = ops.house_critic_fwd([(dx_[0], doh[0]), (dx_[1], doh[1])], dws[0] + dws[1], dbs)
        gr = ops.house_critic_bwd(ddo, dws[0] + dws[1], [r[0] for r in res], 17, need_dx)
        torch.cuda.synchronize()
    gd.check_tails("two passes", [t for r, g_ in zip(res, gr) for t in r[0] + [r[1]] + [d for d in g_ if d is not None]])
    for q in range(2):
        _critic_check(cases[q][0], bs, cases[q][1], cases[q][2], cases[q][3], res[q][0], res[q][1], gr[q], need_dx, f"pass {q} of two")
        for a, b in zip(res[q][0] + [res[q][1]] + [t for t in gr[q] if t is not None],
                        single[q][0] + [single[q][1]] + [t for t in single[q][2] if t is not None]):
            assert torch.equal(a, b), f"pass {q} of the two-pass launch differs from its one-pass launch"
    for a, b in zip(dx_ + doh + ddo + dws[0] + dws[1] + dbs, keep):
        assert torch.equal(a, b), "a critic launch changed an input"


# ---- generator backward ---------------------------------------------------------------------------------------------------------------
G_NAMES = ("DH", "DZ1", "DZ2", "A1", "DG", "DB", "DN1", "DZIN", "DL", "DC", "Q")


def _backward(G, saved, cots):
    buf = saved[1]
    dcots = [None if c is None else _dev(c) for c in cots]
    watched = [buf[n] for n in ("inp", "H", "Z1", "Z2", "SM", "soft")] + [c for c in dcots if c is not None] + [saved[2], saved[3]]
    keep = [t.clone() for t in watched]
    with _Guarded() as g:
        gb = G._fused_backward(saved, *dcots)
        torch.cuda.synchronize()
    g.check_tails("backward", list(gb.values()))
    assert sorted(gb) == sorted(G_NAMES)
    for n in G_NAMES:
        _written(n, gb[n])
    for a, b in zip(watched, keep):
        assert torch.equal(a, b), "the backward changed an input"
    return gb


def _check_backward(sd, G, buf, gb, x, onehot, mask, cots, B, seg, report):
    """Every saved gradient tensor, Q per block and the BatchNorm gamma / beta gradients of one (non-accumulating) backward."""
    sd = {k: v.double() for k, v in sd.items()}
    cond = torch.cat([onehot.double(), mask.double()], 1)
    dc, dl, ds = (None if c is None else c.double() for c in cots)
    H, Z1, Z2, SM, soft = (R.d64(buf[n]) for n in ("H", "Z1", "Z2", "SM", "soft"))
    D = {n: R.d64(gb[n]) for n in G_NAMES}
    nb = (B + R.SEG_ROWS - 1) // R.SEG_ROWS
    Q = [D["Q"][j * nb:(j + 1) * nb] for j in range(9)] + [D["Q"][9 * nb:]]
    assert Q[9].shape[0] == (B + R.HEAD_ROWS - 1) // R.HEAD_ROWS
    grad = {n: R.d64(p.grad) for n, p in G.named_parameters()}
    DL, e_DL, DC, e_DC = R.g_bwd_first(sd, seg, soft, dc, dl, ds, 0.5, 0.1)
    within("DL", D["DL"], DL, e_DL, report)
    within("DC", D["DC"], DC, e_DC, report)
    dh, e = R.g_bwd_dh(sd, D["DL"], D["DC"])
    within("DH[4]", D["DH"][4], dh, e, report)
    q, e = R.part_a(sd, 4, cond, D["DH"][4], Z2[4], SM[9, 0], SM[9, 1], R.HEAD_ROWS)
    within("Q[9]", Q[9], q, e, report)
    for k in range(R.NBLK - 1, -1, -1):
        pre = f"blocks.{k}."
        out, aux = R.g_bwd_b(sd, k, cond, D["DH"][k], Z2[k], Z1[k], SM[2 * k], SM[2 * k + 1], Q[2 * k + 1], B, None)
        within(f"DZ2[{k}]", D["DZ2"][k], *out["DZ2"], report)
        within(f"A1[{k}]", D["A1"][k], *out["A1"], report)
        fv, e_fv = out["fv"]
        sure = fv.abs() > e_fv
        assert bool((((D["A1"][k] > 0) == (fv > 0)) | ~sure).all()), f"ReLU decision of block {k} differs from float64 outside its bound"
        within(pre + "bn2.weight.grad", grad[pre + "bn2.weight"], out["stats"]["dgamma"], out["stats"]["dgamma_bound"], report)
        within(pre + "bn2.bias.grad", grad[pre + "bn2.bias"], out["stats"]["dbeta"], out["stats"]["dbeta_bound"], report)
        tail = R.g_bwd_b_tail(sd, k, D["DH"][k], D["DZ2"][k], D["A1"][k], aux)
        within(f"DG[{k}]", D["DG"][k], *tail["DG"], report)
        within(f"DB[{k}]", D["DB"][k], *tail["DB"], report)
        dn1, e_dn1 = tail["DN1"]
        if k == 0:                                       # the scratch tensor holds the last block in flight
            within("DN1", D["DN1"], dn1, e_dn1, report)
        q, e = R.g_bwd_q1(dn1, aux["xh1"], e_dn1)
        within(f"Q[{2 * k}]", Q[2 * k], q, e, report)
        c = R.g_bwd_c(sd, k, dn1, Z1[k], SM[2 * k], D["DH"][k], Q[2 * k], B, e_dn1)
        within(f"DZ1[{k}]", D["DZ1"][k], *c["DZ1"], report)
        within(pre + "bn1.weight.grad", grad[pre + "bn1.weight"], c["stats"]["dgamma"], c["stats"]["dgamma_bound"], report)
        within(pre + "bn1.bias.grad", grad[pre + "bn1.bias"], c["stats"]["dbeta"], c["stats"]["dbeta_bound"], report)
        dhn, e = R.g_bwd_c_tail(sd, k, D["DZ1"][k], D["DH"][k], H[0] if k == 0 else None)
        if k == 0:
            within("DZIN", D["DZIN"], dhn, e, report)
        else:
            within(f"DH[{k - 1}]", D["DH"][k - 1], dhn, e, report)
            q, e = R.part_a(sd, k - 1, cond, D["DH"][k - 1], Z2[k - 1], SM[2 * k - 1, 0], SM[2 * k - 1, 1], R.SEG_ROWS)
            within(f"Q[{2 * k - 1}]", Q[2 * k - 1], q, e, report)


def _cotangents(buf, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(buf[n].shape, generator=g) for n in ("cont", "logits", "soft"))


def _no_grads(G):
    for p in G.parameters():
        p.grad = None


@pytest.mark.parametrize("form", R.COTANGENT_FORMS)
@pytest.mark.parametrize("name,rows", R.GEN_BWD_CASES, ids=[f"{n}-{r}" for n, r in R.GEN_BWD_CASES])
def test_generator_backward_segments_vs_float64(pcg, name, rows, form):
    """Every saved gradient tensor, Q per block and the BatchNorm gamma / beta gradients against the segment references, for each
    form of absent cotangents: all three present, d_logits absent (the training form), d_samples absent, d_cont absent, only d_cont."""
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    seg = R.seg_of(R.LAYOUTS[name][0])
    G = _generator(pcg, name, sd)
    buf, saved, _ = _forward(G, x, onehot, mask, noise, False)
    cots = R.cotangent_form(form, *_cotangents(buf, rows))
    gb = _backward(G, saved, cots)
    report = []
    _check_backward(sd, G, buf, gb, x, onehot, mask, cots, rows, seg, report)
    if cots[0] is None:
        assert bool((gb["DC"] == 0).all())
    if cots[1] is None and cots[2] is None:
        assert bool((gb["DL"] == 0).all())
    for a, b in zip(seg, seg[1:]):
        if b - a == 1 and cots[1] is None:
            assert bool((gb["DL"][:, a] == 0).all()), "a one-column head has dlogits 0 exactly"
    worst = max(report, key=lambda t: t[1])
    print(f"\n{name}-{rows}-{form}: largest share of a bound {worst[1]:.3f} ({worst[0]})")


@pytest.mark.parametrize("name,rows", [("house", 65), ("house", 577), ("narrow", 65), ("full", 65)], ids=lambda v: str(v))
def test_generator_backward_accumulates(pcg, name, rows):
    """accumulate = 1: a second backward (other cotangents) into the same flat gradient buffer leaves first + second within one
    rounding in EVERY parameter gradient: the BatchNorm gamma / beta gradients pcg_house_g_bwd writes itself under its accumulate
    flag, and the 35 Linear layers' weights and biases, whose accumulate flags _fused_backward hands to the grouped weight-gradient
    launch (a deterministic sum added to the old value once)."""
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    G = _generator(pcg, name, sd)
    buf, saved, _ = _forward(G, x, onehot, mask, noise, False)
    c1, c2 = _cotangents(buf, 1), _cotangents(buf, 2)
    alone = []
    for c in (c1, c2):
        _no_grads(G)
        _backward(G, saved, c)
        alone.append({n: R.d64(p.grad) for n, p in G.named_parameters()})
    assert any(bool((alone[0][n] != alone[1][n]).any()) for n in alone[0])
    _no_grads(G)
    _backward(G, saved, c1)
    _backward(G, saved, c2)
    for n, p in G.named_parameters():
        want = alone[0][n] + alone[1][n]
        within(f"{n}.grad accumulated", p.grad, want, R.U * want.abs() + 1e-30)


@pytest.mark.parametrize("name", list(R.LAYOUTS))
def test_generator_end_to_end_vs_float64_autograd(pcg, name):
    """65 rows through the module: the three outputs and every parameter gradient (after ops.linear_wgrad_grouped) against float64
    autograd of the chained reference (tests/test_house_fused_ref_host.py: it is the oracle), by the tolerance of
    test_fused_generator_kernels_match_the_op_chain.  The ReLU decisions are pinned to the device's; the pinned ones — where float64
    decides otherwise — are at most 0.1 % of the activations."""
    rows = 65
    sd, x, onehot, mask, noise = R.generator_case(name, rows)
    G = _generator(pcg, name, sd)
    buf, saved, _ = _forward(G, x, onehot, mask, noise, False)
    cots = _cotangents(buf, 3)
    gb = _backward(G, saved, cots)
    masks = [(buf["H"][0] > 0).cpu().double()] + [(gb["A1"][k] > 0).cpu().double() for k in range(R.NBLK)]
    leaf = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    out = R.generator_forward(leaf, x.double(), onehot.double(), mask.double(), noise.double(), 0.5, relu_masks=masks)
    pinned = sum(int(((p > 0).double() != m).sum()) for p, m in zip(out["relu_in"], masks))
    assert pinned <= 0.001 * sum(m.numel() for m in masks), pinned
    torch.autograd.backward([out["cont"], out["logits"], out["soft"]], [c.double() for c in cots])
    for n, ref in (("cont", out["cont"]), ("logits", out["logits"]), ("soft", out["soft"])):
        ref = ref.detach()
        np.testing.assert_allclose(R.d64(buf[n]).numpy(), ref.numpy(), rtol=2e-5, atol=2e-5 * float(ref.abs().max()), err_msg=n)
    want = {n: leaf[n].grad for n, _ in G.named_parameters()}
    scale = max(float(v.abs().max()) for v in want.values())
    for n, p in G.named_parameters():
        np.testing.assert_allclose(R.d64(p.grad).numpy(), want[n].numpy(), rtol=1e-4, atol=2e-5 * float(want[n].abs().max()) + 2e-6 * scale,
                                   err_msg=f"grad {n}")


# ---- classifier ------------------------------------------------------------------------------------------------------------------------
def _sn_case(seed):
    """Two small spectral-norm layers for the riders: (weights, u, v, eps)."""
    g = torch.Generator().manual_seed(seed)
    ws = [_dev(torch.randn(32, 21, generator=g)), _dev(torch.randn(64, 32, generator=g))]
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, generator=g), dim=0)  # noqa: E731
    return ws, [_dev(unit(w.shape[0])) for w in ws], [_dev(unit(w.shape[1])) for w in ws], 1e-12


def _clone(t):
    return t.clone() if torch.is_tensor(t) else type(t)(_clone(e) for e in t)


def _flat(t):
    return [t] if torch.is_tensor(t) else [f for e in t for f in _flat(e)]


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    return len(fa) == len(fb) and all(torch.equal(u, v) for u, v in zip(fa, fb))


@pytest.mark.parametrize("rows", list(R.CLS_ROWS_CASES))
def test_classifier_and_its_riders_vs_float64(pcg, rows):
    """Synthetic folded weights (k-major, zero-padded copies forward; as stored backward): logits, the four saved activations and dx
    within the derived bounds of float64.  The forward with a small spectral-norm-backward rider and the backward with a
    spectral-norm-forward rider: the classifier's outputs equal the plain launches bit for bit, the riders' outputs equal the separate
    spectral_norm_*_batched calls bit for bit.  The cross-entropy tail (rider launch only): ce_dlogits equals
    ops.cross_entropy_fwd_bwd's gradient on the same logits bit for bit, ce_row_loss that kernel's loss of each row alone, and both
    are within bound of float64."""
    ops = pcg.ops
    ws, bs = R.classifier_weights(11)
    g = torch.Generator().manual_seed(rows)
    x, dl = torch.rand(rows, 17, generator=g), torch.randn(rows, 4, generator=g)
    t = torch.randint(0, 4, (rows,), generator=g)
    t[0], t[-1] = 0, 3
    dws, dkm, dbs = [_dev(w) for w in ws], [_dev(w) for w in R.pack_kmajor(ws)], [_dev(b) for b in bs]
    dxin, ddl, dt = _dev(x), _dev(dl), t.to(DEV)
    keep = [v.clone() for v in dws + dkm + dbs + [dxin, ddl]]
    with _Guarded() as gd:
        logits, acts = ops.house_classifier_fwd(dxin, dkm, dbs)
        dx = ops.house_classifier_bwd(ddl, dws, acts)
        torch.cuda.synchronize()
    gd.check_tails("classifier", [logits, dx] + acts)
    for v in [logits, dx] + acts:
        _written("classifier", v)
    w64, b64 = [w.double() for w in ws], [b.double() for b in bs]
    dev_a = [R.d64(a) for a in acts]
    ref, e = R.classifier_forward(w64, b64, x.double(), forced=dev_a)
    for l in range(4):
        within(f"a{l + 1}", acts[l], ref[l], e[l])
    within("logits", logits, ref[4], e[4])
    rdx, edx = R.classifier_backward(w64, dev_a, dl.double())
    within("dx", dx, rdx, edx)
    # riders
    sw, su, sv, eps = _sn_case(rows)
    outs = ops.spectral_norm_fwd_batched(sw, _clone(su), _clone(sv), eps, True)
    gq = torch.Generator().manual_seed(rows + 1)
    passes = [[(_dev(torch.randn(w.shape, generator=gq)), o[0], o[2], o[3], o[1]) for w, o in zip(sw, outs[0])]]
    sep_dw, rid_dw = [torch.zeros_like(w) for w in sw], [torch.zeros_like(w) for w in sw]
    ops.spectral_norm_bwd_batched(passes, sep_dw, [False, False])
    scale = 1.7
    with _Guarded() as gd:
        logits2, acts2, ce_dz, ce_rows = ops.house_classifier_fwd(dxin, dkm, dbs, sn_bwd=ops.sn_bwd_batch(passes, rid_dw, [False, False]),
                                                                  ce=(dt, scale))
        torch.cuda.synchronize()
    gd.check_tails("classifier forward with its rider", [logits2, ce_dz, ce_rows] + acts2)
    assert _same([logits, acts], [logits2, acts2]), "the classifier's outputs under the rider launch"
    assert _same(sep_dw, rid_dw), "the spectral-norm backward as a rider"
    sep_uv, rid_uv = _clone((su, sv)), _clone((su, sv))
    sep_out = ops.spectral_norm_fwd_batched(sw, *sep_uv, eps, True)
    with _Guarded() as gd:
        dx2, rid_out = ops.house_classifier_bwd(ddl, dws, acts, sn_fwd=ops.sn_fwd_batch(sw, *rid_uv, eps)[1])
        torch.cuda.synchronize()
    gd.check_tails("classifier backward with its rider", [dx2])
    assert torch.equal(dx, dx2), "dx under the rider launch"
    assert _same(sep_out, rid_out) and _same(sep_uv, rid_uv), "the spectral-norm forward as a rider"
    # the cross-entropy tail
    _check_ce(ops, logits, dt, scale, ce_dz, ce_rows)
    for a, b in zip(dws + dkm + dbs + [dxin, ddl], keep):
        assert torch.equal(a, b), "a classifier launch changed an input"


def _check_ce(ops, logits, dt, scale, ce_dz, ce_rows):
    rows = logits.shape[0]
    _written("cross-entropy tail", ce_dz); _written("cross-entropy tail", ce_rows)
    _, dz = ops.cross_entropy_fwd_bwd(logits, dt, need_loss=False, grad_scale=scale)
    assert torch.equal(ce_dz, dz), "ce_dlogits is not pcg_cross_entropy_fwd_bwd's gradient on the same logits"
    for i in range(rows):
        li, _ = ops.cross_entropy_fwd_bwd(logits[i:i + 1], dt[i:i + 1], need_grad=False)
        assert torch.equal(li.reshape(()), ce_rows[i]), f"ce_row_loss[{i}] is not pcg_cross_entropy_fwd_bwd's loss of that row"
    r, er, d, ed = R.cross_entropy_rows(R.d64(logits), dt.cpu(), scale)
    within("ce_row_loss", ce_rows, r, er)
    within("ce_dlogits", ce_dz, d, ed)


def test_cross_entropy_tail_at_large_logits(pcg):
    """Every row has logits (60, -60, -60, 60) (zero last-layer weights): targets at each of the four classes, 0 and 3 among them —
    the row term is log 2 behind an lse of 60.7, or 120.7."""
    ops = pcg.ops
    rows = 17
    ws, bs = R.classifier_weights(12)
    ws[4] = torch.zeros_like(ws[4])
    bs[4] = torch.tensor([60.0, -60.0, -60.0, 60.0])
    g = torch.Generator().manual_seed(5)
    x = torch.rand(rows, 17, generator=g)
    t = torch.arange(rows) % 4
    t[-1] = 3
    sw, su, sv, eps = _sn_case(3)
    outs = ops.spectral_norm_fwd_batched(sw, _clone(su), _clone(sv), eps, True)
    passes = [[(_dev(torch.randn(w.shape, generator=g)), o[0], o[2], o[3], o[1]) for w, o in zip(sw, outs[0])]]
    dw = [torch.zeros_like(w) for w in sw]
    dt = t.to(DEV)
    logits, _, ce_dz, ce_rows = ops.house_classifier_fwd(_dev(x), [_dev(w) for w in R.pack_kmajor(ws)], [_dev(b) for b in bs],
                                                         sn_bwd=ops.sn_bwd_batch(passes, dw, [False, False]), ce=(dt, 1.0))
    assert torch.equal(logits.cpu(), bs[4].expand(rows, 4))
    _check_ce(ops, logits, dt, 1.0, ce_dz, ce_rows)
