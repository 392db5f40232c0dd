"""Float64 restatement of the fused tabular kernels (csrc/house_fused.hip, house_critic_fused.hip, house_classifier_fused.hip),
segment by segment, and the error bounds tests/test_hip_house_fused_edges.py holds them to.  Plain torch on the CPU.

The kernels park every segment's inputs and outputs in global memory, so the reference is TEACHER-FORCED: each function takes the
device's own inputs of one segment (float32 values, widened) and returns that segment's outputs in float64 beside a per-element
bound derived from the kernel's arithmetic.  An error can then not hide behind the error of the segment before it, and a bound
never has to cover more than one segment.  The chained forms at the end (`generator_forward`, `critic_forward`, ...) run the same
functions on their own outputs; tests/test_house_fused_ref_host.py pins them to float64 autograd of oracle/house_ref.py, so a wrong
reference fails there and not on the GPU.

u = 2^-24 (unit roundoff of float32).  Derivations:

  Linear on the MFMA chain.  acc starts at the bias and takes K products one after the other (v_mfma_f32_16x16x4_f32 /
  32x32x2_f32: fp32 products, fp32 accumulate, K / 4 or K / 2 dependent instructions; zero pad columns add exact zeros).  The
  classical bound of a length-K recursive sum is gamma_K (sum |a||w| + |b|); `linear` takes (K + 2) u: two more for the
  second-order terms and for an accumulation order inside one instruction that the ISA does not promise.

  Per-block column sums: four in-lane adds, two shuffle adds (distance 16, 32), two adds of the four waves' partial sums = DEPTH 8
  roundings on any path from a term to the result (colsums2_m, block_sums2); the forward's sums are pivoted and take a few more
  (colsums_m, block_sums).

  BatchNorm statistics (pload_piv, bn_finish_m) are float64 arithmetic on the float32 partial sums and pivots, then ONE rounding
  to float32: u |value|, with 1e-12 relative for the float64 arithmetic itself (its error is 1e-16 of q / B, which the
  subtraction q / B - mean^2 can magnify by (mean / std)^2 <= 1e4 here).  What the float32 partial sums cost against the true
  statistics of Z is `stats_bound`.

  Everything downstream of a rounded quantity gets that quantity's error to first order: |df| <= sum |df / dx_i| e_i."""
import math

import numpy as np
import torch

U = 2.0 ** -24
# ---- the constants block: block sizes of the kernels under test (rows per block) ---------------------------------------------
SEG_ROWS = 64          # FT: generator segment kernels (forward and backward)
HEAD_ROWS = 16         # HR: g_heads16 / g_bwd_first16
CRITIC_ROWS = 32       # MR: critic forward / backward
CLS_ROWS = 16          # classifier forward / backward
PLOAD_PARTS = 8        # NPART: pload's first trip covers this many 64-row blocks
PAIRS_PER_ROUND = 128  # (row, head) pairs one softmax round of a head block takes (256 threads, two lanes per pair)
MAXCOLS, MAXT, MAXHEADS, MAXW = 96, 96, 8, 32
HH, NBLK, DIN, NCLS = 32, 5, 17, 4
DEPTH = 8              # roundings between a term and its per-block column sum
K_IN, K_COND, K_HID = 40, 24, 32     # padded reduction depths of fc_in, the FiLM products, the hidden Linears

# ---- generator layouts: head widths in head order, number of continuous columns ------------------------------------------------
LAYOUTS = {
    "house": ([9, 30, 6, 2, 5, 5, 13], 10),      # the product configuration (the heads sit at the product's feature columns)
    "full": ([32, 32, 31], 1),                   # T + ncont = MAXCOLS: all six column tiles; half-splits 16/16 and 16/15
    "narrow": ([1, 2, 1, 3, 2, 1, 2, 1], 9),     # eight heads = 128 pairs = one full round; width-1 heads; heads + cont in one tile
    "single": ([17], 16),                        # a head straddling the tile boundary at 16; a last tile of one column; 16 pairs
}
HOUSE_CAT_COLS = [0, 1, 4, 5, 6, 7, 8]


def layout_config(name):
    """The config dict oracle/house_ref.py and pcgan_amd.house take, for a layout: heads first (or at the product's columns)."""
    widths, ncont = LAYOUTS[name]
    cols = HOUSE_CAT_COLS if name == "house" else list(range(len(widths)))
    cat = {c: w for c, w in zip(cols, widths)}
    cont = [i for i in range(DIN) if i not in cat][:ncont]
    return {"input_dim": DIN, "num_classes": NCLS, "hidden_dim": HH, "gumbel_tau": 0.5, "immutable_idx": [11, 12, 13, 14],
            "categorical_info": cat, "continuous_idx": cont}


def seg_of(widths):
    return [0] + [int(v) for v in np.cumsum(widths)]


def d64(t):
    return t.detach().cpu().double()


# ---- parameters ---------------------------------------------------------------------------------------------------------------------
def make_generator_state(name, seed):
    """A seeded float32 state dict with the key order of (oracle or device) ResidualGenerator: Linear weights U(-1, 1) / sqrt(fan_in),
    biases of the same scale, BatchNorm gamma 1 + 0.2 N, beta 0.2 N, running statistics off their defaults (the kernel must read them)."""
    from oracle import house_ref as HR
    cfg = layout_config(name)
    ref = HR.ResidualGenerator(DIN, HH, NCLS, cfg["continuous_idx"], cfg["categorical_info"])
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in ref.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3, dtype=torch.int64)
        elif k.endswith("running_mean"):
            sd[k] = 0.3 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif ".bn" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.2 * torch.randn(v.shape, generator=g)
        elif ".bn" in k:
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
        else:
            mod = k.rsplit(".", 1)[0]
            fan_in = ref.state_dict()[mod + ".weight"].shape[1]
            sd[k] = (2.0 * torch.rand(v.shape, generator=g) - 1.0) / math.sqrt(fan_in)
    return sd


def head_keys(sd):
    return [k[:-7] for k in sd if k.startswith("fc_cat_logits.") and k.endswith(".weight")]


# ---- building blocks -----------------------------------------------------------------------------------------------------------------
def linear(a, W, b, K, e_a=None):
    """y = a W^T + b and its bound (K + 2) u (|a||W|^T + |b|) [+ |W| e_a to first order when the operand a carries the error e_a]."""
    y = a @ W.T + (b if b is not None else 0.0)
    mag = a.abs() @ W.abs().T + (b.abs() if b is not None else 0.0)
    bound = (K + 2) * U * mag
    if e_a is not None:
        bound = bound + e_a @ W.abs().T
    return y, bound


DEPTH_S, DEPTH_Q = 12, 17   # roundings behind a pivoted block sum / sum of squares (block_sums' docstring)


def block_sums(z, rows_per_block=SEG_ROWS):
    """colsums_m: per-block PIVOTED column sums [nblocks][2][C] = (sum (z - p), sum (z - p)^2) over the block's live rows, p = the
    block's first row.  On the device every 16-row wave subtracts its own first row p_w, adds, and is then moved to p
    (d = p_w - p: s_w + n_w d, q_w + d (2 s_w + n_w d)) before the four waves are added.  Roundings on a path to the sum: z - p_w [1],
    four in-lane adds, two shuffle adds, d [1] and the fma [1], two wave adds = 11, DEPTH_S = 12 with the second order, relative to
    M_s = sum_w (sum |z - p_w| + n_w |d_w|).  To the sum of squares: z - p_w counts twice, the square, 4 + 2 adds, d twice, n d, two
    fmas, two wave adds = 16, DEPTH_Q = 17, relative to M_q = sum_w 2 (sum (z - p_w)^2 + n_w d_w^2)  (2 |d| sum|x| <= sum x^2 + n d^2)."""
    B, C = z.shape
    nb = (B + rows_per_block - 1) // rows_per_block
    out, bound = torch.zeros(nb, 2, C, dtype=torch.float64), torch.zeros(nb, 2, C, dtype=torch.float64)
    for b in range(nb):
        blk = z[b * rows_per_block:min(B, (b + 1) * rows_per_block)]
        x = blk - blk[0]
        out[b, 0], out[b, 1] = x.sum(0), (x * x).sum(0)
        for w in range(0, blk.shape[0], 16):
            xw = blk[w:w + 16] - blk[w]
            d, n = blk[w] - blk[0], xw.shape[0]
            bound[b, 0] += DEPTH_S * U * (xw.abs().sum(0) + n * d.abs())
            bound[b, 1] += DEPTH_Q * U * 2.0 * ((xw * xw).sum(0) + n * d * d)
    return out, bound


def block_sums2(v, w, rows_per_block=SEG_ROWS, e_v=None, e_w=None):
    """colsums2_m (backward) and the tail of g_bwd_first16: plain per-block column sums of (v, w), w = v * xhat a rounded product:
    four in-lane adds, two shuffles, two wave adds = DEPTH 8, + 1 second order, on top of the terms' own errors e_v, e_w."""
    B, C = v.shape
    nb = (B + rows_per_block - 1) // rows_per_block
    out, bound = torch.zeros(nb, 2, C, dtype=torch.float64), torch.zeros(nb, 2, C, dtype=torch.float64)
    for b in range(nb):
        sl = slice(b * rows_per_block, min(B, (b + 1) * rows_per_block))
        out[b, 0], out[b, 1] = v[sl].sum(0), w[sl].sum(0)
        bound[b, 0], bound[b, 1] = (DEPTH + 1) * U * v[sl].abs().sum(0), (DEPTH + 1) * U * w[sl].abs().sum(0)
        if e_v is not None:
            bound[b, 0] += e_v[sl].sum(0)
        if e_w is not None:
            bound[b, 1] += e_w[sl].sum(0)
    return out, bound


def fold_pivots(P, z, B, rows_per_block=SEG_ROWS):
    """pload_piv: (sum z, sum z^2) over the batch from the pivoted block sums and the pivots (row 0 of every block of z), float64."""
    nb = P.shape[0]
    piv = z[0:B:rows_per_block]
    n = torch.tensor([min(rows_per_block, B - b * rows_per_block) for b in range(nb)], dtype=torch.float64)[:, None]
    return (P[:, 0] + n * piv).sum(0), (P[:, 1] + piv * (2.0 * P[:, 0] + n * piv)).sum(0)


def bn_finish(P, z, B, eps, momentum, rm0=None, rv0=None):
    """pload_piv + bn_finish_m on the device's partial sums P [nblocks][2][C] and the device's z: float64 sums, mean = s / B,
    var = max(q / B - mean^2, 0), invstd = 1 / sqrt(var + eps), each rounded once to float32; running statistics (1 - m) r + m s in
    float64, rounded once."""
    eps, m = float(np.float32(eps)), float(np.float32(momentum))
    s, q = fold_pivots(P, z, B)
    mean = s / B
    var = (q / B - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    rel = U + 1e-12
    out = dict(mean=mean, inv=inv, var=var, mean_bound=rel * mean.abs() + 1e-30,
               # d inv / d var = -inv^3 / 2; var carries 1e-12 (q / B + mean^2) of float64 noise
               inv_bound=rel * inv + 0.5 * inv ** 3 * 1e-12 * (q / B + mean * mean))
    if rm0 is not None:
        unb = var * (B / (B - 1.0) if B > 1 else 1.0)
        out.update(rm=(1.0 - m) * rm0 + m * mean, rv=(1.0 - m) * rv0 + m * unb)
        out.update(rm_bound=rel * out["rm"].abs() + 1e-12, rv_bound=rel * out["rv"].abs() + 1e-12)
    return out


def stats_bound(z, eps):
    """What the fused path's mean / invstd may differ by from the two-pass float64 statistics of the same z: the float32 block sums.
    With e_s(b), e_q(b) the bounds of block_sums: mean: sum_b e_s(b) / B + u |mean|.  var = Q / B - (S / B)^2 with S, Q folded from
    the pivots in float64: d var / d s_b = 2 (p_b - mean) / B, d var / d q_b = 1 / B, so e_var = sum_b (e_q(b) + 2 |p_b - mean| e_s(b)) / B
    — a multiple of u (var + (p_b - mean)^2): the distance of the PIVOT from the mean in units of std, a few for any row of the
    batch, where plain sums of z and z^2 had (mean / std)^2 (plain_sums_invstd_rel_bound_at).  invstd = (var + eps)^-1/2: relative
    e_var / (2 (var + eps)) + u.  Returns dict(mean, invstd, var, mean_bound, invstd_bound, var_bound, ratio = |mean| / std)."""
    B = z.shape[0]
    eps = float(np.float32(eps))
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    inv = 1.0 / torch.sqrt(var + eps)
    _, e = block_sums(z)
    piv = z[0:B:SEG_ROWS]
    e_var = (e[:, 1] + 2.0 * (piv - mean).abs() * e[:, 0]).sum(0) / B
    return dict(mean=mean, invstd=inv, mean_bound=e[:, 0].sum(0) / B + U * mean.abs() + 1e-30,
                invstd_bound=inv * (0.5 * e_var * inv * inv + U), var=var, var_bound=e_var, ratio=mean.abs() * inv)


def plain_sums_invstd_rel_bound_at(ratio):
    """The relative invstd bound of UNPIVOTED float32 block sums (sum z: (DEPTH + 1) u sum|z|, sum z^2: (DEPTH + 2) u sum z^2 — the
    arithmetic before the pivot) for a column of constant sign with |mean| / std = ratio:
    e_var = (DEPTH + 2) u (var + mean^2) + 2 |mean| (DEPTH + 1) u |mean|, relative e_var / (2 var) + u."""
    return 0.5 * ((DEPTH + 2) * U * (1.0 + ratio * ratio) + 2.0 * (DEPTH + 1) * U * ratio * ratio) + U


def plain_sums_crossing(tol=2e-5):
    """The ratio at which plain_sums_invstd_rel_bound_at reaches tol."""
    return math.sqrt((2.0 * (tol - U) / U - (DEPTH + 2)) / ((DEPTH + 2) + 2.0 * (DEPTH + 1)))


def film(sd, k, cond):
    gam, e_gam = linear(cond, sd[f"blocks.{k}.film.gamma.weight"], sd[f"blocks.{k}.film.gamma.bias"], K_COND)
    bet, e_bet = linear(cond, sd[f"blocks.{k}.film.beta.weight"], sd[f"blocks.{k}.film.beta.bias"], K_COND)
    return gam, bet, e_gam, e_bet


def bn_film(z, mean, inv, g, b, gam, bet, e_gam, e_bet):
    """fv = fma(gam, n, bet), n = fma((z - mean) * inv, g, b) on float32 mean / inv (the device's own).  Roundings: z - mean [1],
    * inv [1], fma [1]: e_n = u (2 |xh g| + |n|); fv: |gam| e_n + |n| e_gam + e_bet + u |fv|.  Returns (fv, e_fv, n, xh)."""
    xh = (z - mean) * inv
    n = xh * g + b
    e_n = U * (2.0 * (xh * g).abs() + n.abs())
    fv = gam * n + bet
    e_fv = gam.abs() * e_n + n.abs() * e_gam + e_bet + U * fv.abs()
    return fv, e_fv, n, xh


# ---- generator forward segments ----------------------------------------------------------------------------------------------------
def g_entry(sd, x, onehot, mask):
    """g_fwd_first4: inp = (x, onehot, mask) [exact]; H[0] = relu(fc_in(inp)) (ReLU is 1-Lipschitz: the Linear's bound)."""
    inp = torch.cat([x, onehot, mask], 1)
    h, e = linear(inp, sd["fc_in.weight"], sd["fc_in.bias"], K_IN)
    return inp, h.clamp_min(0.0), e


def g_fc1(sd, k, h):
    """Z1[k] = fc1_k(H[k]) from the device's H[k] (the registers the kernel multiplies are the values it stored)."""
    return linear(h, sd[f"blocks.{k}.fc1.weight"], sd[f"blocks.{k}.fc1.bias"], K_HID)


def g_seg_a(sd, k, cond, z1, mean, inv):
    """kind A: a1 = relu(film(bn1(z1))) [in LDS only], Z2[k] = fc2(a1).  Returns (z2, e_z2, fv) — fv for the backward's masks."""
    gam, bet, e_gam, e_bet = film(sd, k, cond)
    fv, e_fv, _, _ = bn_film(z1, mean, inv, sd[f"blocks.{k}.bn1.weight"], sd[f"blocks.{k}.bn1.bias"], gam, bet, e_gam, e_bet)
    z2, e_z2 = linear(fv.clamp_min(0.0), sd[f"blocks.{k}.fc2.weight"], sd[f"blocks.{k}.fc2.bias"], K_HID, e_a=e_fv)
    return z2, e_z2, fv


def g_seg_b(sd, k, cond, z2, mean, inv, h):
    """kind B: H[k + 1] = h + film(bn2(z2)) [one more rounding]."""
    gam, bet, e_gam, e_bet = film(sd, k, cond)
    fv, e_fv, _, _ = bn_film(z2, mean, inv, sd[f"blocks.{k}.bn2.weight"], sd[f"blocks.{k}.bn2.bias"], gam, bet, e_gam, e_bet)
    hn = h + fv
    return hn, e_fv + U * hn.abs()


def packed_heads(sd):
    keys = head_keys(sd)
    return torch.cat([sd[k + ".weight"] for k in keys], 0), torch.cat([sd[k + ".bias"] for k in keys], 0)


def g_heads(sd, h5, res_scale):
    """g_heads16's product: packed logits and cont = fc_cont(h5) * res_scale [one more rounding, on the float32 res_scale]."""
    W, b = packed_heads(sd)
    logits, e_l = linear(h5, W, b, K_HID)
    rs = float(np.float32(res_scale))
    c, e_c = linear(h5, sd["fc_cont.weight"], sd["fc_cont.bias"], K_HID)
    return logits, e_l, c * rs, e_c * rs + U * (c * rs).abs()


def soft_samples(logits, noise, tau, seg):
    """softmax((logits + noise) / tau) per head, float64, from the device's logits.  Held at rtol 2e-5, atol 1e-7 (expf): the
    tolerance test_gumbel_softmax_heads_and_residual_assembly gives the same quantity."""
    t = (logits + noise) / float(np.float32(tau))
    return torch.cat([torch.softmax(t[:, a:b], 1) for a, b in zip(seg, seg[1:])], 1)


SOFT_RTOL, SOFT_ATOL = 2e-5, 1e-7


def first_max_onehot(soft, seg):
    out = torch.zeros_like(soft)
    for a, b in zip(seg, seg[1:]):
        out[torch.arange(soft.shape[0]), a + soft[:, a:b].argmax(1)] = 1.0     # torch.argmax: the first maximum
    return out


def undecided(p64, p32, seg):
    """[rows][heads] bool: the float64 top-two probability gap of the pair is below max(1e-5, 100 max|p32 - p64|) (the project's rule
    for discrete outputs: such a pair may fall either way in float32).  A one-column head is always decided."""
    thr = max(1e-5, 100.0 * float((p32.double() - p64).abs().max()))
    cols = []
    for a, b in zip(seg, seg[1:]):
        if b - a == 1:
            cols.append(torch.zeros(p64.shape[0], dtype=torch.bool))
            continue
        top = p64[:, a:b].topk(2, dim=1).values
        cols.append((top[:, 0] - top[:, 1]) < thr)
    return torch.stack(cols, 1)


# ---- the chained forward (host test: equals oracle/house_ref.py) ----------------------------------------------------------------
def generator_forward(sd, x, onehot, mask, noise, tau, eps=1e-5, res_scale=0.1, relu_masks=None):
    """Every segment function on the outputs of the one before.  Returns dict(cont, logits, soft, h5, relu_in).  relu_masks =
    [mask of fc_in's ReLU, mask of block 0's, ...] pins the ReLU decisions (the end-to-end gradient check pins them to the device's);
    relu_in are the six pre-activations.  Differentiable (float64 autograd) when sd's tensors require grad."""
    B = x.shape[0]
    cond = torch.cat([onehot, mask], 1)
    inp = torch.cat([x, onehot, mask], 1)
    pre, _ = linear(inp, sd["fc_in.weight"], sd["fc_in.bias"], K_IN)
    relu_in = [pre]
    h = pre.clamp_min(0.0) if relu_masks is None else pre * relu_masks[0]
    for k in range(NBLK):
        z1, _ = g_fc1(sd, k, h)
        st = bn_finish(block_sums(z1)[0], z1, B, eps, 0.1)
        gam, bet, e_gam, e_bet = film(sd, k, cond)
        fv, _, _, _ = bn_film(z1, st["mean"], st["inv"], sd[f"blocks.{k}.bn1.weight"], sd[f"blocks.{k}.bn1.bias"], gam, bet, e_gam, e_bet)
        relu_in.append(fv)
        a1 = fv.clamp_min(0.0) if relu_masks is None else fv * relu_masks[k + 1]
        z2, _ = linear(a1, sd[f"blocks.{k}.fc2.weight"], sd[f"blocks.{k}.fc2.bias"], K_HID)
        st = bn_finish(block_sums(z2)[0], z2, B, eps, 0.1)
        h, _ = g_seg_b(sd, k, cond, z2, st["mean"], st["inv"], h)
    logits, _, cont, _ = g_heads(sd, h, res_scale)
    seg = seg_of([sd[k + ".bias"].shape[0] for k in head_keys(sd)])
    return dict(cont=cont, logits=logits, soft=soft_samples(logits, noise, tau, seg), h5=h, relu_in=relu_in)


# ---- generator backward segments ------------------------------------------------------------------------------------------------------
def _xhat(z, mean, inv):
    return (z - mean) * inv                         # two roundings on the device: 2 u |xhat|


def part_a(sd, k, cond, dh, z2, m2, i2, rows_per_block):
    """Part "a" of block k (tail of g_bwd_first16 at 16-row blocks, of g_bwd_c4 at 64): dn2 = dh * gam from the device's dh, and the
    per-block sums of (dn2, dn2 * xhat2).  e_v = |dh| e_gam + u |v|; w = v * xhat: e_w = |xhat| e_v + 3 u |w|."""
    gam, e_gam = linear(cond, sd[f"blocks.{k}.film.gamma.weight"], sd[f"blocks.{k}.film.gamma.bias"], K_COND)
    xh = _xhat(z2, m2, i2)
    v = dh * gam
    e_v = dh.abs() * e_gam + U * v.abs()
    w = v * xh
    return block_sums2(v, w, rows_per_block, e_v, xh.abs() * e_v + 3 * U * w.abs())


def g_bwd_first(sd, seg, soft, d_cont, d_logits, d_samples, tau, res_scale):
    """g_bwd_first16 up to dh: DL = d_logits + soft (d_samples - <d_samples, soft>_head) / tau, DC = d_cont res_scale (absent
    cotangents are zeros).  dot: an fma chain over the lane's <= 16 columns and one shuffle add: (w + 2) u sum |ds| |y| for a head of
    width w; dl_s = y (ds - dot) / tau: three roundings + |y| e_dot / tau; + the add to d_logits.  Then (see g_bwd_dh) DH[4]."""
    B, T = soft.shape
    it = 1.0 / float(np.float32(tau))
    dl = torch.zeros(B, T, dtype=torch.float64) if d_logits is None else d_logits.clone()
    e = torch.zeros(B, T, dtype=torch.float64)
    if d_samples is not None:
        for a, b in zip(seg, seg[1:]):
            y, ds = soft[:, a:b], d_samples[:, a:b]
            dot = (ds * y).sum(1, keepdim=True)
            e_dot = (b - a + 2) * U * (ds * y).abs().sum(1, keepdim=True)
            t = y * (ds - dot) * it
            e_t = y.abs() * it * (e_dot + U * (ds.abs() + dot.abs())) + 3 * U * t.abs()
            dl[:, a:b] += t
            e[:, a:b] = e_t + (U * dl[:, a:b].abs() if d_logits is not None else 0.0)
    rs = float(np.float32(res_scale))
    ncont = sd["fc_cont.bias"].shape[0]
    dc = torch.zeros(B, ncont, dtype=torch.float64) if d_cont is None else d_cont * rs
    return dl, e, dc, U * dc.abs()


def g_bwd_dh(sd, DL, DC):
    """DH[4] = [DL, DC] W over the packed head + continuous weight rows, from the device's DL / DC (the MFMA operand is the tile it
    stores): K = 96 columns in 24 steps, no bias."""
    W, _ = packed_heads(sd)
    Wp = torch.cat([W, sd["fc_cont.weight"]], 0)
    G = torch.cat([DL, DC], 1)
    return G @ Wp, (MAXCOLS + 2) * U * (G.abs() @ Wp.abs())


def bn_bwd_sums(Q, B):
    """bnb_finish_m: float64 sums of the partial rows, / B, one rounding each; dgamma = sum of dn * xhat, dbeta = sum of dn."""
    s1, s2 = Q[:, 0].sum(0), Q[:, 1].sum(0)
    rel = U + 1e-12
    return dict(su=s1 / B, sx=s2 / B, su_bound=rel * (s1 / B).abs() + 1e-30, sx_bound=rel * (s2 / B).abs() + 1e-30,
                dgamma=s2, dbeta=s1, dgamma_bound=rel * s2.abs() + 1e-30, dbeta_bound=rel * s1.abs() + 1e-30)


def bn_bwd_dz(dn, e_dn, z, mean, inv, g, su, sx):
    """dz = g inv (dn - su - xhat sx) on the float32 su, sx the device used (recomputed from ITS partial sums: one rounding each,
    carried here as u |su|, u |sx|).  t = dn - su - xhat sx: e_t = e_dn + 4 u (|dn| + |su| + |xhat sx|) [xhat: 2, the product: 1, sx: 1,
    two subtractions]; dz = (g inv) t: two more roundings."""
    xh = _xhat(z, mean, inv)
    t = dn - su - xh * sx
    e_t = e_dn + 4 * U * (dn.abs() + su.abs() + (xh * sx).abs())
    dz = g * inv * t
    return dz, (g * inv).abs() * e_t + 2 * U * dz.abs(), xh


def g_bwd_b(sd, k, cond, dh, z2, z1, sm1, sm2, Q, B, a1_dev):
    """kind B of block k from the device's DH[k], Z2[k], Z1[k], SM and the partial sums Q of (dn2, dn2 xhat2).  The ReLU mask is the
    device's own decision, read from the A1 it stored (a1 > 0 <=> fv > 0); fv is returned so the caller can see that the decision is
    the float64 one wherever |fv| exceeds its bound.  Returns dict name -> (value, bound)."""
    gam, bet, e_gam, e_bet = film(sd, k, cond)
    g2, b2 = sd[f"blocks.{k}.bn2.weight"], sd[f"blocks.{k}.bn2.bias"]
    g1, b1 = sd[f"blocks.{k}.bn1.weight"], sd[f"blocks.{k}.bn1.bias"]
    st = bn_bwd_sums(Q, B)
    dn2 = dh * gam
    e_dn2 = dh.abs() * e_gam + U * dn2.abs()
    # (the device's su / sx are the float32 roundings of its own float64 sums: su_bound + |xhat| sx_bound more on t)
    dz2, e_dz2, xh2 = bn_bwd_dz(dn2, e_dn2 + st["su_bound"] + _xhat(z2, sm2[0], sm2[1]).abs() * st["sx_bound"], z2, sm2[0], sm2[1], g2,
                                st["su"], st["sx"])
    n2 = xh2 * g2 + b2
    e_n2 = U * (2.0 * (xh2 * g2).abs() + n2.abs())
    out = dict(DZ2=(dz2, e_dz2), stats=st)
    fv, e_fv, n1, xh1 = bn_film(z1, sm1[0], sm1[1], g1, b1, gam, bet, e_gam, e_bet)
    e_n1 = U * (2.0 * (xh1 * g1).abs() + n1.abs())
    out["A1"] = (fv.clamp_min(0.0), e_fv)
    out["fv"] = (fv, e_fv)
    return out, dict(gam=gam, e_gam=e_gam, n1=n1, e_n1=e_n1, n2=n2, e_n2=e_n2, xh1=xh1)


def g_bwd_b_tail(sd, k, dh, dz2_dev, a1_dev, aux):
    """The second half of kind B from the device's DZ2: da1 = dz2 fc2_w (K = 32, no bias), df1 = da1 where the device's a1 > 0;
    DG = fma(df1, n1, dh n2), DB = dh + df1, DN1 = df1 gam."""
    W = sd[f"blocks.{k}.fc2.weight"]
    m = (a1_dev > 0).double()
    da1 = dz2_dev @ W
    e_da1 = (K_HID + 2) * U * (dz2_dev.abs() @ W.abs())
    df1, e_df1 = da1 * m, e_da1 * m
    p = dh * aux["n2"]
    dg = df1 * aux["n1"] + p
    e_dg = df1.abs() * aux["e_n1"] + aux["n1"].abs() * e_df1 + dh.abs() * aux["e_n2"] + U * p.abs() + U * dg.abs()
    db = dh + df1
    dn1 = df1 * aux["gam"]
    return dict(DG=(dg, e_dg), DB=(db, e_df1 + U * db.abs()), DN1=(dn1, aux["gam"].abs() * e_df1 + df1.abs() * aux["e_gam"] + U * dn1.abs()))


def g_bwd_q1(dn1, xh1, e_dn1=None):
    """Q[2k]: 64-row block sums of (dn1, dn1 xhat1).  DN1 is one scratch tensor, rewritten by every block: only block 0's survives
    the launch, so the caller passes the reference dn1 with its bound e_dn1 for the others."""
    w = dn1 * xh1
    e_w = 3 * U * w.abs() + (xh1.abs() * e_dn1 if e_dn1 is not None else 0.0)
    return block_sums2(dn1, w, SEG_ROWS, e_dn1, e_w)


def g_bwd_c(sd, k, dn1, z1, sm1, dh, Q, B, e_dn1=None):
    """kind C of block k: bn1 backward from DN1 (+ its bound where it is the reference's, see g_bwd_q1) and the device's Q[2k] -> DZ1."""
    st = bn_bwd_sums(Q, B)
    g1 = sd[f"blocks.{k}.bn1.weight"]
    xh = _xhat(z1, sm1[0], sm1[1])
    e = st["su_bound"] + xh.abs() * st["sx_bound"] + (e_dn1 if e_dn1 is not None else 0.0)
    dz1, e, _ = bn_bwd_dz(dn1, e, z1, sm1[0], sm1[1], g1, st["su"], st["sx"])
    return dict(DZ1=(dz1, e), stats=st)


def g_bwd_c_tail(sd, k, dz1_dev, dh, h0_dev=None):
    """dh_{k-1} = dh_k + dz1 fc1_w from the device's DZ1 (K = 32, no bias, one more add); for k = 0 the fc_in ReLU on the device's H[0]."""
    W = sd[f"blocks.{k}.fc1.weight"]
    t = dz1_dev @ W
    out = dh + t
    e = (K_HID + 2) * U * (dz1_dev.abs() @ W.abs()) + U * out.abs()
    if h0_dev is not None:
        m = (h0_dev > 0).double()
        out, e = out * m, e * m
    return out, e


def chain_forward_saved(sd, x, onehot, mask, eps=1e-5):
    """The forward's saved tensors (H, Z1, Z2, SM as lists) from the segment functions on their own outputs."""
    B = x.shape[0]
    cond = torch.cat([onehot, mask], 1)
    inp, h, _ = g_entry(sd, x, onehot, mask)
    H, Z1, Z2, SM = [h], [], [], []
    for k in range(NBLK):
        z1, _ = g_fc1(sd, k, H[k])
        s1 = bn_finish(block_sums(z1)[0], z1, B, eps, 0.1)
        z2, _, _ = g_seg_a(sd, k, cond, z1, s1["mean"], s1["inv"])
        s2 = bn_finish(block_sums(z2)[0], z2, B, eps, 0.1)
        hn, _ = g_seg_b(sd, k, cond, z2, s2["mean"], s2["inv"], H[k])
        Z1.append(z1); Z2.append(z2); H.append(hn); SM += [(s1["mean"], s1["inv"]), (s2["mean"], s2["inv"])]
    return dict(inp=inp, cond=cond, H=H, Z1=Z1, Z2=Z2, SM=SM)


def chain_backward(sd, seg, f, soft, d_cont, d_logits, d_samples, tau, res_scale):
    """The backward segment functions on their own outputs: the parameter gradients (as the grouped weight-gradient launch forms
    them: dW = dY^T X, db = column sums of dY) by parameter name."""
    B = soft.shape[0]
    cond, H, Z1, Z2, SM = f["cond"], f["H"], f["Z1"], f["Z2"], f["SM"]
    DL, _, DC, _ = g_bwd_first(sd, seg, soft, d_cont, d_logits, d_samples, tau, res_scale)
    dh, _ = g_bwd_dh(sd, DL, DC)
    g = {"fc_cont.weight": DC.T @ H[NBLK], "fc_cont.bias": DC.sum(0)}
    for key, a, b in zip(head_keys(sd), seg, seg[1:]):
        g[key + ".weight"], g[key + ".bias"] = DL[:, a:b].T @ H[NBLK], DL[:, a:b].sum(0)
    Q2, _ = part_a(sd, NBLK - 1, cond, dh, Z2[NBLK - 1], *SM[2 * NBLK - 1], HEAD_ROWS)
    for k in range(NBLK - 1, -1, -1):
        out, aux = g_bwd_b(sd, k, cond, dh, Z2[k], Z1[k], SM[2 * k], SM[2 * k + 1], Q2, B, None)
        a1 = out["A1"][0]
        tail = g_bwd_b_tail(sd, k, dh, out["DZ2"][0], a1, aux)
        Q1, _ = g_bwd_q1(tail["DN1"][0], aux["xh1"])
        c = g_bwd_c(sd, k, tail["DN1"][0], Z1[k], SM[2 * k], dh, Q1, B)
        pre = f"blocks.{k}."
        g[pre + "bn2.weight"], g[pre + "bn2.bias"] = out["stats"]["dgamma"], out["stats"]["dbeta"]
        g[pre + "bn1.weight"], g[pre + "bn1.bias"] = c["stats"]["dgamma"], c["stats"]["dbeta"]
        g[pre + "fc2.weight"], g[pre + "fc2.bias"] = out["DZ2"][0].T @ a1, out["DZ2"][0].sum(0)
        g[pre + "fc1.weight"], g[pre + "fc1.bias"] = c["DZ1"][0].T @ H[k], c["DZ1"][0].sum(0)
        g[pre + "film.gamma.weight"], g[pre + "film.gamma.bias"] = tail["DG"][0].T @ cond, tail["DG"][0].sum(0)
        g[pre + "film.beta.weight"], g[pre + "film.beta.bias"] = tail["DB"][0].T @ cond, tail["DB"][0].sum(0)
        dh, _ = g_bwd_c_tail(sd, k, c["DZ1"][0], dh, H[0] if k == 0 else None)
        if k > 0:
            Q2, _ = part_a(sd, k - 1, cond, dh, Z2[k - 1], *SM[2 * k - 1], SEG_ROWS)
    g["fc_in.weight"], g["fc_in.bias"] = dh.T @ f["inp"], dh.sum(0)
    return g


# ---- critic ----------------------------------------------------------------------------------------------------------------------
C_WIDTHS = (21, 32, 64, 128)
C_K = (22, 32, 64)                  # padded reduction depths of the three MFMA layers


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def critic_layer(a, W, b, K, slope):
    """One Linear + LeakyReLU from the device's input activation: the Linear's bound, + u |v| for the slope product (<= 1-Lipschitz)."""
    y, e = linear(a, W, b, K)
    v = lrelu(y, slope)
    return v, e + U * v.abs()


def critic_out(a3, w4, b4):
    """Linear(128 -> 1): eight fma chains of 16 and a three-level tree of them, then + bias: (16 + 3 + 1 + 1) u (|a3||w4| + |b4|)."""
    y = a3 @ w4.T + b4
    return y, (16 + 3 + 2) * U * (a3.abs() @ w4.abs().T + b4.abs())


def critic_forward(ws, bs, x, onehot, slope, forced=None):
    """[a0, a1, a2, a3, out] and their bounds; forced = the device's [a0..a3]: every layer starts from the device's input of it."""
    s = float(np.float32(slope))
    a = [torch.cat([x, onehot], 1)]
    e = [torch.zeros_like(a[0])]
    for l in range(3):
        src = forced[l] if forced is not None else a[l]
        v, ev = critic_layer(src, ws[l], bs[l], C_K[l], s)
        a.append(v); e.append(ev)
    o, eo = critic_out(forced[3] if forced is not None else a[3], ws[3], bs[3])
    return a + [o], e + [eo]


def critic_backward(ws, acts, dout, slope, D, forced=None):
    """d3 = dout w4 LeakyReLU'(a3) [2 roundings, 3 with the slope]; d2 = (d3 W3) LeakyReLU'(a2): K = 128 in two MFMA halves + 1 add
    + the slope product; d1: K = 64 in quarters + 3 adds + slope; dx = d1 W1[:, :D]: K = 32 in quarters + 3 adds.  The masks are the
    saved activations' signs (a > 0), as the kernel reads them.  forced = the device's (d3, d2, d1)."""
    s = float(np.float32(slope))
    m = [torch.where(a > 0, torch.ones_like(a), torch.full_like(a, s)) for a in acts]       # a1, a2, a3
    d3 = dout * ws[3] * m[2]
    e3 = 3 * U * d3.abs()
    src = forced[0] if forced is not None else d3
    d2 = (src @ ws[2]) * m[1]
    e2 = (128 // 2 + 2 + 2) * U * (src.abs() @ ws[2].abs()) * m[1]
    src = forced[1] if forced is not None else d2
    d1 = (src @ ws[1]) * m[0]
    e1 = (64 // 4 + 2 + 4) * U * (src.abs() @ ws[1].abs()) * m[0]
    src = forced[2] if forced is not None else d1
    dx = src @ ws[0][:, :D]
    ex = (32 // 4 + 2 + 3) * U * (src.abs() @ ws[0][:, :D].abs())
    return [d3, d2, d1, dx], [e3, e2, e1, ex]


# ---- case tables (tests/test_house_fused_ref_host.py checks every claim against the constants block) --------------------------------
# generator rows -> (64-row segment blocks, rows in the last one, 16-row head blocks, rows in the last one)
GEN_ROWS = {
    2: (1, 2, 1, 2),          # the fewest rows a training BatchNorm takes
    15: (1, 15, 1, 15),       # one short of a head block
    16: (1, 16, 1, 16),       # exactly one head block
    17: (1, 17, 2, 1),        # a second head block of one row
    63: (1, 63, 4, 15),       # one short of a segment block
    64: (1, 64, 4, 16),       # exactly one segment block
    65: (2, 1, 5, 1),         # a second segment block of one row
    129: (3, 1, 9, 1),        # three segment blocks, odd
    577: (10, 1, 37, 1),      # ten segment blocks: pload's second trip (> PLOAD_PARTS); last segment and head block hold one row
}
GEN_FWD_CASES = [("house", r) for r in GEN_ROWS] + [(n, r) for n in ("full", "narrow", "single") for r in (17, 65, 577)]
GEN_BWD_CASES = [("house", r) for r in (2, 17, 65, 577)] + [(n, 65) for n in ("full", "narrow", "single")]
CRITIC_ROWS_CASES = {1: (1, 1), 31: (1, 31), 32: (1, 32), 33: (2, 1), 97: (4, 1)}         # rows -> (32-row blocks, rows in the last)
CLS_ROWS_CASES = {1: (1, 1), 15: (1, 15), 16: (1, 16), 17: (2, 1), 33: (3, 1), 257: (17, 1)}   # rows -> (16-row blocks, rows in the last)


COTANGENT_FORMS = ("all", "training", "no-samples", "no-cont", "cont-only")


def cotangent_form(form, dc, dl, ds):
    """(d_cont, d_logits, d_samples) of a form: "training" has no d_logits (the training step never uses the logits)."""
    return {"all": (dc, dl, ds), "training": (dc, None, ds), "no-samples": (dc, dl, None), "no-cont": (None, dl, ds),
            "cont-only": (dc, None, None)}[form]


def case_seed(name, rows):
    return 1000 * (1 + list(LAYOUTS).index(name)) + rows


def generator_case(name, rows):
    """(state dict, x, onehot, mask, packed noise [rows][T]) of a case, float32, seeded."""
    from oracle import house_ref as HR
    cfg = layout_config(name)
    sd = make_generator_state(name, case_seed(name, rows))
    x, _, t, mask, gumbel = HR.synthetic_batch(rows, seed=case_seed(name, rows), config=cfg)
    onehot = torch.nn.functional.one_hot(t, NCLS).float()
    noise = torch.cat([gumbel[f] for f in cfg["categorical_info"]], 1).contiguous()
    return sd, x, onehot, mask, noise


# ---- the oracle (oracle/house_ref.py) on a case ------------------------------------------------------------------------------------
def oracle_generator(name, sd, dtype):
    from oracle import house_ref as HR
    cfg = layout_config(name)
    G = HR.ResidualGenerator(DIN, HH, NCLS, cfg["continuous_idx"], cfg["categorical_info"], tau=0.5)
    G.load_state_dict(sd)
    G.residual_scaling = float(np.float32(0.1))       # the C floats the kernel is handed
    for m in G.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.eps, m.momentum = float(np.float32(m.eps)), float(np.float32(m.momentum))
    return G.to(dtype).train(), cfg


def oracle_run(G, cfg, x, onehot, mask, noise, hard=False):
    seg = seg_of(list(cfg["categorical_info"].values()))
    gum = {f: noise[:, a:b] for f, a, b in zip(cfg["categorical_info"], seg, seg[1:])}
    cont, logits, samples = G(x, onehot, mask, gum, hard=hard)
    return cont, torch.cat([logits[f] for f in cfg["categorical_info"]], 1), torch.cat([samples[f] for f in cfg["categorical_info"]], 1)


# ---- classifier (csrc/house_classifier_fused.hip): the BatchNorm-folded five layers ------------------------------------------------------
CLS_WIDTHS = (17, 256, 256, 128, 64, 4)
CLS_K = (20, 256, 256, 128, 64)          # reduction depths (layer 0 zero-padded to 20); a split reduction of KS parts takes K / KS + KS
CLS_SLOPE = float(np.float32(0.1))       # roundings, never more than the K + 2 of `linear`


def classifier_weights(seed):
    """Synthetic folded weights (as stored, [out][in]) and biases, float32."""
    g = torch.Generator().manual_seed(seed)
    ws = [(2.0 * torch.rand(o, i, generator=g) - 1.0) * (1.7 / math.sqrt(i)) for i, o in zip(CLS_WIDTHS, CLS_WIDTHS[1:])]
    bs = [0.1 * torch.randn(o, generator=g) for o in CLS_WIDTHS[1:]]
    return ws, bs


def pack_kmajor(ws):
    """What NNClassifier._pack_kmajor makes: [K][N] copies, layer 0 zero-padded to K = 20; the last layer as stored."""
    km = [w.t().contiguous() for w in ws[:4]]
    km[0] = torch.cat([km[0], torch.zeros(3, km[0].shape[1], dtype=km[0].dtype)], 0).contiguous()
    return km + [ws[4]]


def classifier_forward(ws, bs, x, forced=None):
    """([a1, a2, a3, a4, logits], bounds); forced = the device's [a1..a4]: every layer starts from the device's input."""
    acts, e, src = [], [], x
    for l in range(4):
        y, ey = linear(src, ws[l], bs[l], CLS_K[l])
        v = lrelu(y, CLS_SLOPE)
        acts.append(v); e.append(ey + U * v.abs())
        src = forced[l] if forced is not None else v
    y, ey = linear(src, ws[4], bs[4], CLS_K[4])
    return acts + [y], e + [ey]


def classifier_backward(ws, acts, dlogits):
    """dx of the frozen classifier from the device's saved activations (masks a > 0) — the intermediate gradients stay in LDS, so
    every layer's error is carried into the next to first order.  d4: four fmas and the slope product."""
    m = [torch.where(a > 0, torch.ones_like(a), torch.full_like(a, CLS_SLOPE)) for a in acts]
    d = (dlogits @ ws[4]) * m[3]
    e = (4 + 2) * U * (dlogits.abs() @ ws[4].abs()) * m[3]
    for l in (3, 2, 1):
        t = d @ ws[l]
        et = (ws[l].shape[0] + 2) * U * (d.abs() @ ws[l].abs()) + e @ ws[l].abs()
        d, e = t * m[l - 1], et * m[l - 1] + U * (t * m[l - 1]).abs()
    dx = d @ ws[0]
    return dx, (ws[0].shape[0] + 2) * U * (d.abs() @ ws[0].abs()) + e @ ws[0].abs()


CE_GRAD_RTOL, CE_GRAD_ATOL, CE_LOSS_RTOL = 2e-5, 1e-8, 2e-6      # tests/test_hip_small_ops.py


def cross_entropy_rows(logits, target, grad_scale):
    """(row terms lse - z[t], their bound, gradient grad_scale / B (softmax - onehot), its bound) in float64 from the device's logits.
    Gradient: the tolerance of tests/test_hip_small_ops.py.  Row term: that file's relative loss tolerance, plus u |lse| — the term is
    fl(fl(max + logf(sum)) - z[t]), and the rounding of lse is relative to lse, which a row whose term is far smaller cannot absorb."""
    B = logits.shape[0]
    lse = torch.logsumexp(logits, 1)
    rows = lse - logits[torch.arange(B), target]
    onehot = torch.nn.functional.one_hot(target, logits.shape[1]).double()
    dz = float(np.float32(grad_scale)) / B * (torch.exp(logits - lse[:, None]) - onehot)
    return rows, CE_LOSS_RTOL * rows.abs() + U * lse.abs(), dz, CE_GRAD_RTOL * dz.abs() + CE_GRAD_ATOL
