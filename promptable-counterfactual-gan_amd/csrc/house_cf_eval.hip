// house_cf_eval.hip — the tabular ("prompted") CounteRGAN's counterfactual queries and evaluation in ONE launch:
// conditional_counteRGAN/house_sales_kc_usa eval_utils.py:25-181 (build_counterfactuals), :185-289 (compute_metrics_per_target),
// :351-434 (analyze_class_pair_sensitivity), gradio_app.py:144-169 (the per-request feature mask), models/generator.py:38-92 and
// models/nn_classifier.py:4-32 in eval mode.
//
// In eval mode BatchNorm uses the running statistics, so every row is independent of every other: one work item is (target slot t,
// row i).  A workgroup of 512 threads owns a tile of 16 rows and ALL T target slots, i.e. up to 64 items:
//   generator   on the vector ALU, one thread per (item, hidden unit): a thread keeps its unit's weight row in registers for its four
//               items, the activations of all items sit in LDS ([item][32]) between layers, the FiLM gamma / beta of the thread's
//               (item, unit) stay in registers over the block.  Heads: one thread per (item, logit column), then one per (item, head)
//               for the hard Gumbel-softmax sample with gumbel_softmax_fwd_kernel's expressions (tabular.hip), then one per
//               (item, feature) for the residual row.
//   classifier  94 % of the MACs: the T + 1 row tiles (x once, then one counterfactual tile per slot) run one after the other
//               through the dense layers of house_classifier_body.h on v_mfma_f32_16x16x4_f32, weights straight from L2 — the
//               body of the training step's classifier launch, so a row's logits are the bits that launch gives.
//   sums        per tile, by one thread per output in ascending row order: no atomics, bitwise repeatable.
// The generator's LDS image aliases the classifier's (the phases do not overlap); what crosses the phases (the classifier inputs,
// the logits, |masked| per item) has its own block.  A row's values do not depend on its place in a tile, on the other rows of the
// tile or on the other slots: the per-row form, the sweep and every `group` give the same bits.
#include <cstdint>
#include "pcg_common.h"
#include "house_classifier_body.h"

namespace pcg {
namespace {

constexpr int CE_D = 17, CE_NC = 4, CE_H = 32, CE_NB = 5, CE_COND = CE_D + CE_NC, CE_IN = CE_D + CE_COND;
constexpr int CE_TMAX = 4, CE_ITEMS = CE_TMAX * CL_R, CE_TCAT = 96, CE_HEADS = 8;
constexpr int CE_IPT = CE_ITEMS * CE_H / CL_NT;          // items per thread in the (item, unit) layers: 4

struct GenSmem {                                          // the generator phase: aliases ClsSmem
  float inp[CE_ITEMS * CE_IN];                            // [item][x 17 | onehot 4 | mask 17]
  float h[CE_ITEMS * CE_H];                               // block input / output; after the heads: masked [item][17]
  float a[CE_ITEMS * 3 * CE_H];                           // [item][32] inside a block; after the blocks: logits [item][Tcat <= 96]
};
static_assert(sizeof(GenSmem) <= sizeof(ClsSmem), "the generator image must fit the classifier's");

struct KeepSmem {                                         // what crosses the phases
  float xin[(CE_TMAX + 1) * CL_R * CE_D];                 // classifier inputs: tile 0 = x, tile 1 + t = the counterfactual of slot t
  float cont[CE_ITEMS * CE_D];
  float lg[(CE_TMAX + 1) * CL_R * CE_NC];
  float absm[CE_ITEMS];                                   // sum over the 17 columns of |masked|
  float stat[CE_ITEMS * 4];                               // included, flipped, gain (tile sums)
  int chosen[CE_ITEMS * CE_HEADS];
  int colw[CE_TCAT], colb[CE_TCAT];                       // per packed logit column: offset of its weight row / bias in the flat buffer
  int tgt[CE_ITEMS];
};

struct HouseCfK {                                         // the kernel's view of the arguments (device pointers only)
  pcg_house_cf_eval_args a;
  ClsFwdW w;
  int tiles_per_group, n_tiles;
};

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

// out[j] = bias + sum_k in[item_j][k] * w[k], ascending k, for the thread's CE_IPT items (item = i0 + 16 j)
template <int K>
__device__ __forceinline__ void dot_items(const float* __restrict__ W, float bias, const float* in, int pitch, int i0, int items,
                                          float (&out)[CE_IPT]) {
  float w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) w[k] = W[k];
#pragma unroll
  for (int j = 0; j < CE_IPT; ++j) {
    const int it = i0 + 16 * j;
    float acc = 0.f;
    if (it < items) {
      const float* r = in + it * pitch;
#pragma unroll
      for (int k = 0; k < K; ++k) acc = fmaf(r[k], w[k], acc);
    }
    out[j] = acc + bias;
  }
}

__global__ void __launch_bounds__(CL_NT) house_cf_eval_kernel(const pcg_house_g_desc d, const HouseCfK kk) {
  __shared__ __attribute__((aligned(16))) unsigned char lds_alias[sizeof(ClsSmem)];
  __shared__ KeepSmem keep;
  GenSmem& gs = *reinterpret_cast<GenSmem*>(lds_alias);
  ClsSmem& cs = *reinterpret_cast<ClsSmem*>(lds_alias);
  const pcg_house_cf_eval_args& a = kk.a;
  const int tid = threadIdx.x;
  const int T = a.T, items = T * CL_R;
  const int64_t N = a.N;
  const int q = blockIdx.x;
  const int64_t grp = q / kk.tiles_per_group;
  const int64_t row0 = grp * a.group + (int64_t)(q - grp * kk.tiles_per_group) * CL_R;
  const int64_t gend = (grp + 1) * a.group < N ? (grp + 1) * a.group : N;
  const int rows = (int)(gend - row0 < CL_R ? gend - row0 : CL_R);
  const int Tcat = d.seg[d.nheads], ncont = d.ncont, nheads = d.nheads;
  if (rows <= 0) {                                        // a tile past the end of a short last group (uniform): empty sums
    if (a.tile_sums && tid < T * 4) a.tile_sums[((size_t)(tid >> 2) * kk.n_tiles + q) * 4 + (tid & 3)] = 0.f;
    if (a.class_sums)
      for (int e = tid; e < T * CE_NC * (CE_D + 1); e += CL_NT) {
        const int t = e / (CE_NC * (CE_D + 1)), r = e - t * (CE_NC * (CE_D + 1)), c = r / (CE_D + 1), f = r - c * (CE_D + 1);
        if (f < CE_D) a.class_sums[(((size_t)t * kk.n_tiles + q) * CE_NC + c) * CE_D + f] = 0.f;
        else a.class_counts[((size_t)t * kk.n_tiles + q) * CE_NC + c] = 0.f;
      }
    return;
  }
  const float* __restrict__ G = a.g_flat;

  // ---- inputs: [x, onehot(target), mask] per item; rows past the tile's end repeat its last row (computed, never written) --------
  if (tid < items) {
    const int t = tid / CL_R, m = tid - t * CL_R;
    int tg = t;
    if (a.target) { const int64_t v = a.target[row0 + min(m, rows - 1)]; tg = v < 0 ? 0 : (v >= CE_NC ? CE_NC - 1 : (int)v); }
    keep.tgt[tid] = tg;
  }
  if (tid < Tcat) {
    int s = 0;
    while (s + 1 < nheads && tid >= d.seg[s + 1]) ++s;
    keep.colw[tid] = d.head_w[s] + (tid - d.seg[s]) * CE_H;
    keep.colb[tid] = d.head_b[s] + (tid - d.seg[s]);
  }
  __syncthreads();
  for (int e = tid; e < items * CE_IN; e += CL_NT) {
    const int it = e / CE_IN, k = e - it * CE_IN, m = it & (CL_R - 1);
    const int64_t r = row0 + min(m, rows - 1);
    float v;
    if (k < CE_D) v = a.x[r * CE_D + k];
    else if (k < CE_COND) v = (k - CE_D) == keep.tgt[it] ? 1.f : 0.f;
    else v = a.mask_rows ? a.mask[r * CE_D + (k - CE_COND)] : a.mask[k - CE_COND];
    gs.inp[e] = v;
    if (it < CL_R && k < CE_D) keep.xin[m * CE_D + k] = v;
  }
  __syncthreads();

  // ---- generator.py:73-79: fc_in + ReLU, five FiLM-conditioned residual blocks ---------------------------------------------------
  const int o = tid & (CE_H - 1), i0 = tid >> 5;           // unit, first item (items i0, i0 + 16, i0 + 32, i0 + 48)
  {
    float z[CE_IPT];
    dot_items<CE_IN>(G + d.fc_in_w + o * CE_IN, G[d.fc_in_b + o], gs.inp, CE_IN, i0, items, z);
#pragma unroll
    for (int j = 0; j < CE_IPT; ++j) gs.h[(i0 + 16 * j) * CE_H + o] = relu(z[j]);
  }
  __syncthreads();
#pragma unroll 1
  for (int b = 0; b < CE_NB; ++b) {
    float gam[CE_IPT], bet[CE_IPT], z[CE_IPT];
    dot_items<CE_COND>(G + d.film_gamma_w[b] + o * CE_COND, G[d.film_gamma_b[b] + o], gs.inp + CE_D, CE_IN, i0, items, gam);
    dot_items<CE_COND>(G + d.film_beta_w[b] + o * CE_COND, G[d.film_beta_b[b] + o], gs.inp + CE_D, CE_IN, i0, items, bet);
    dot_items<CE_H>(G + d.fc1_w[b] + o * CE_H, G[d.fc1_b[b] + o], gs.h, CE_H, i0, items, z);
    {
      const float mu = a.bn_mean[2 * b][o], inv = 1.f / sqrtf(a.bn_var[2 * b][o] + a.bn_eps);
      const float ga = G[d.bn1_g[b] + o], be = G[d.bn1_b[b] + o];
#pragma unroll
      for (int j = 0; j < CE_IPT; ++j) gs.a[(i0 + 16 * j) * CE_H + o] = relu(fmaf(gam[j], fmaf(ga, (z[j] - mu) * inv, be), bet[j]));
    }
    __syncthreads();                                       // every read of h above is done: h may be rewritten below
    dot_items<CE_H>(G + d.fc2_w[b] + o * CE_H, G[d.fc2_b[b] + o], gs.a, CE_H, i0, items, z);
    {
      const float mu = a.bn_mean[2 * b + 1][o], inv = 1.f / sqrtf(a.bn_var[2 * b + 1][o] + a.bn_eps);
      const float ga = G[d.bn2_g[b] + o], be = G[d.bn2_b[b] + o];
#pragma unroll
      for (int j = 0; j < CE_IPT; ++j) {
        const int e = (i0 + 16 * j) * CE_H + o;
        gs.h[e] = gs.h[e] + fmaf(gam[j], fmaf(ga, (z[j] - mu) * inv, be), bet[j]);
      }
    }
    __syncthreads();
  }

  // ---- heads (generator.py:81-90): cont = res_scale * fc_cont(h); the packed logits ----------------------------------------------
  if (o < ncont) {
    float z[CE_IPT];
    dot_items<CE_H>(G + d.cont_w + o * CE_H, G[d.cont_b + o], gs.h, CE_H, i0, items, z);
#pragma unroll
    for (int j = 0; j < CE_IPT; ++j) {
      const int it = i0 + 16 * j, m = it & (CL_R - 1);
      if (it >= items) continue;
      const float v = a.res_scale * z[j];
      keep.cont[it * CE_D + o] = v;
      if (a.cont && m < rows) a.cont[((size_t)(it / CL_R) * N + row0 + m) * ncont + o] = v;
    }
  }
  for (int c = o; c < Tcat; c += CE_H) {
    float z[CE_IPT];
    dot_items<CE_H>(G + keep.colw[c], G[keep.colb[c]], gs.h, CE_H, i0, items, z);
#pragma unroll
    for (int j = 0; j < CE_IPT; ++j) {
      const int it = i0 + 16 * j, m = it & (CL_R - 1);
      if (it >= items) continue;
      gs.a[it * CE_TCAT + c] = z[j];
      if (a.logits && m < rows) a.logits[((size_t)(it / CL_R) * N + row0 + m) * Tcat + c] = z[j];
    }
  }
  __syncthreads();
  // the hard Gumbel-softmax sample of each (item, head): gumbel_softmax_fwd_kernel's expressions, first maximum of the soft-max
  if (tid < items * nheads) {
    const int it = tid / nheads, s = tid - it * nheads, m = it & (CL_R - 1);
    const int c0 = d.seg[s], c1 = d.seg[s + 1];
    const float inv_tau = 1.f / a.tau;
    const float* l = gs.a + it * CE_TCAT;
    const float* g = a.noise + ((size_t)(it / CL_R) * N + row0 + min(m, rows - 1)) * Tcat;
    float mx = -INFINITY;
    for (int c = c0; c < c1; ++c) mx = fmaxf(mx, (l[c] + g[c]) * inv_tau);
    float se = 0.f;
    for (int c = c0; c < c1; ++c) se += expf((l[c] + g[c]) * inv_tau - mx);
    const float inv = 1.f / se;
    float best = -1.f;
    int arg = c0;
    for (int c = c0; c < c1; ++c) {
      const float p = expf((l[c] + g[c]) * inv_tau - mx) * inv;
      if (p > best) { best = p; arg = c; }
    }
    keep.chosen[it * CE_HEADS + s] = arg - c0;
    if (a.chosen && m < rows) a.chosen[((size_t)(it / CL_R) * N + row0 + m) * nheads + s] = arg - c0;
  }
  __syncthreads();

  // ---- residual row (eval_utils.py:127-180): two roundings for x + residual * mask, as the reference's two tensor ops ------------
  for (int e = tid; e < items * CE_D; e += CL_NT) {
    const int it = e / CE_D, f = e - it * CE_D, t = it / CL_R, m = it & (CL_R - 1);
    const float x = gs.inp[it * CE_IN + f], mk = gs.inp[it * CE_IN + CE_COND + f];
    const int src = a.col_src[f];
    float res;
    if (src >= 0) res = keep.cont[it * CE_D + src];
    else { const int s = -src - 1; res = a.norm_vals[d.seg[s] + keep.chosen[it * CE_HEADS + s]] - x; }
    const float md = __fmul_rn(res, mk);
    const float raw = __fadd_rn(x, md);
    const float cf = fminf(fmaxf(raw, 0.f), 1.f);
    gs.h[it * CE_D + f] = md;
    keep.xin[((1 + t) * CL_R + m) * CE_D + f] = a.clamp_cls ? cf : raw;
    if (m < rows) {
      const size_t oi = ((size_t)t * N + row0 + m) * CE_D + f;
      if (a.masked) a.masked[oi] = md;
      if (a.x_cf) a.x_cf[oi] = cf;
      if (a.x_cf_raw) a.x_cf_raw[oi] = raw;
    }
  }
  __syncthreads();
  if (tid < items) {
    float s = 0.f;
    for (int f = 0; f < CE_D; ++f) s += fabsf(gs.h[tid * CE_D + f]);
    keep.absm[tid] = s;
  }
  // per source class the sum of |masked| per feature and the row count: one thread per (slot, class, feature | count)
  if (a.class_sums)
    for (int e = tid; e < T * CE_NC * (CE_D + 1); e += CL_NT) {
      const int t = e / (CE_NC * (CE_D + 1)), r = e - t * (CE_NC * (CE_D + 1)), c = r / (CE_D + 1), f = r - c * (CE_D + 1);
      float s = 0.f;
      for (int m = 0; m < rows; ++m)
        if (a.y[row0 + m] == (int64_t)c) s += f < CE_D ? fabsf(gs.h[(t * CL_R + m) * CE_D + f]) : 1.f;
      if (f < CE_D) a.class_sums[(((size_t)t * kk.n_tiles + q) * CE_NC + c) * CE_D + f] = s;
      else a.class_counts[((size_t)t * kk.n_tiles + q) * CE_NC + c] = s;
    }
  __syncthreads();                                         // the generator's image is dead from here: the classifier's takes its place

  // ---- nn_classifier.py:4-32 (eval, BatchNorm folded): T + 1 row tiles through the MFMA layers -----------------------------------
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
#pragma unroll 1
  for (int p = 0; p <= T; ++p) {
    if (tid < CL_R * CL_INP) {
      const int m = tid / CL_INP, k = tid - m * CL_INP;
      cs.X[0][k * CL_P + m] = k < CL_IN ? keep.xin[(p * CL_R + m) * CE_D + min(k, CL_IN - 1)] : 0.f;
    }
    __syncthreads();
    // the weight pointers pass through an opaque copy per tile: the layers' first weight loads do not depend on the tile and would
    // otherwise all be hoisted out of this loop and held (spilled) across it
    const float *w0 = kk.w.wt[0], *w1 = kk.w.wt[1], *w2 = kk.w.wt[2], *w3 = kk.w.wt[3];
    asm volatile("" : "+s"(w0), "+s"(w1), "+s"(w2), "+s"(w3));
    cl_dense_fwd<CL_INP, CL_H1, true>(cs.X[0], cs.X[1], w0, kk.w.b[0], nullptr, cs.part, 0, rows, wave, li, lq);
    __syncthreads();
    cl_dense_fwd<CL_H1, CL_H2, true>(cs.X[1], cs.X[0], w1, kk.w.b[1], nullptr, cs.part, 0, rows, wave, li, lq);
    __syncthreads();
    cl_dense_fwd<CL_H2, CL_H3, true>(cs.X[0], cs.X[1], w2, kk.w.b[2], nullptr, cs.part, 0, rows, wave, li, lq);
    __syncthreads();
    cl_dense_fwd<CL_H3, CL_H4, true>(cs.X[1], cs.X[0], w3, kk.w.b[3], nullptr, cs.part, 0, rows, wave, li, lq);
    __syncthreads();
    if (tid < CL_R * CL_OUT) {                             // Linear(64 -> 4), classifier_fwd_body's expression
      const int m = tid >> 2, col = tid & 3;
      float acc = kk.w.b[4][col];
      const float* wr = kk.w.wt[4] + col * CL_H4;
#pragma unroll 8
      for (int k = 0; k < CL_H4; ++k) acc = fmaf(cs.X[0][k * CL_P + m], wr[k], acc);
      keep.lg[(p * CL_R + m) * CE_NC + col] = acc;
    }
    __syncthreads();
  }

  // ---- per item: predicted classes (first maximum), gain = softmax(logits_cf)[t] - softmax(logits_x)[t] -------------------------
  if (tid < items) {
    const int t = tid / CL_R, m = tid - t * CL_R, tg = keep.tgt[tid];
    const float* lx = keep.lg + m * CE_NC;
    const float* lc = keep.lg + ((1 + t) * CL_R + m) * CE_NC;
    int px = 0, pc = 0;
    float mxx = lx[0], mxc = lc[0];
    for (int k = 1; k < CE_NC; ++k) {
      if (lx[k] > mxx) { mxx = lx[k]; px = k; }
      if (lc[k] > mxc) { mxc = lc[k]; pc = k; }
    }
    float sx = 0.f, sc = 0.f, ex = 0.f, ec = 0.f;
    for (int k = 0; k < CE_NC; ++k) {
      const float vx = expf(lx[k] - mxx), vc = expf(lc[k] - mxc);
      sx += vx; sc += vc;
      if (k == tg) { ex = vx; ec = vc; }
    }
    const float gain = ec / sc - ex / sx;
    bool inc = false;
    if (m < rows) {
      const size_t oi = (size_t)t * N + row0 + m;
      if (a.logits_cf) for (int k = 0; k < CE_NC; ++k) a.logits_cf[oi * CE_NC + k] = lc[k];
      if (a.pred_cf) a.pred_cf[oi] = pc;
      if (a.gain) a.gain[oi] = gain;
      if (t == 0) {
        if (a.logits_x) for (int k = 0; k < CE_NC; ++k) a.logits_x[(size_t)(row0 + m) * CE_NC + k] = lx[k];
        if (a.pred_x) a.pred_x[row0 + m] = px;
      }
      inc = !a.y || a.y[row0 + m] != (int64_t)tg;         // eval_utils.py:226
    }
    keep.stat[tid * 4] = inc ? 1.f : 0.f;
    keep.stat[tid * 4 + 1] = inc && pc == tg ? 1.f : 0.f;
    keep.stat[tid * 4 + 2] = inc ? gain : 0.f;
    keep.stat[tid * 4 + 3] = inc ? keep.absm[tid] : 0.f;
  }
  if (!a.tile_sums) return;                                // (uniform)
  __syncthreads();
  if (tid < T * 4) {
    const int t = tid >> 2, k = tid & 3;
    float s = 0.f;
    for (int m = 0; m < rows; ++m) s += keep.stat[(t * CL_R + m) * 4 + k];
    a.tile_sums[((size_t)t * kk.n_tiles + q) * 4 + k] = s;
  }
}

bool span_ok(int off, int n, int total) { return off >= 0 && n >= 0 && off <= total - n; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_house_cf_eval(const pcg_house_g_desc* desc, const pcg_house_cf_eval_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(desc && args, "pcg_house_cf_eval: null descriptor or arguments");
  const pcg_house_g_desc& d = *desc;
  const pcg_house_cf_eval_args& a = *args;
  PCG_REQUIRE(d.D == CE_D && d.NC == CE_NC && d.hidden == CE_H && d.nblocks == CE_NB,
              "pcg_house_cf_eval: built for input_dim %d, %d classes, hidden %d, %d blocks (got %d, %d, %d, %d)", CE_D, CE_NC, CE_H, CE_NB, d.D,
              d.NC, d.hidden, d.nblocks);
  PCG_REQUIRE(d.nheads >= 0 && d.nheads <= CE_HEADS && d.ncont >= 0 && d.ncont + d.nheads == CE_D && d.seg[0] == 0,
              "pcg_house_cf_eval: %d heads (<= %d) and %d continuous columns must cover the %d features", d.nheads, CE_HEADS, d.ncont, CE_D);
  for (int s = 0; s < d.nheads; ++s) PCG_REQUIRE(d.seg[s + 1] > d.seg[s], "pcg_house_cf_eval: head %d is empty", s);
  const int Tcat = d.seg[d.nheads];
  PCG_REQUIRE(Tcat <= CE_TCAT, "pcg_house_cf_eval: %d packed categories (<= %d)", Tcat, CE_TCAT);
  PCG_REQUIRE(a.N >= 1 && a.group >= 1 && a.T >= 1 && a.T <= CE_TMAX, "pcg_house_cf_eval: N %lld, group %d, T %d (N, group >= 1, 1 <= T <= %d)",
              (long long)a.N, a.group, a.T, CE_TMAX);
  PCG_REQUIRE(!a.target || a.T == 1, "pcg_house_cf_eval: the per-row form (target [N]) takes T = 1, got %d", a.T);
  PCG_REQUIRE(a.g_flat && a.nG > 0 && a.x && a.mask && a.noise && a.norm_vals && a.c_w_kmajor && a.c_bias,
              "pcg_house_cf_eval: null generator, x, mask, noise, norm_vals or classifier image");
  PCG_REQUIRE(a.tau > 0.f, "pcg_house_cf_eval: tau %g", (double)a.tau);
  // every tensor of the generator inside its flat buffer
  {
    const int nG = a.nG;
    bool ok = span_ok(d.fc_in_w, CE_H * CE_IN, nG) && span_ok(d.fc_in_b, CE_H, nG) && span_ok(d.cont_w, d.ncont * CE_H, nG) &&
              span_ok(d.cont_b, d.ncont, nG);
    for (int b = 0; b < CE_NB; ++b)
      ok = ok && span_ok(d.fc1_w[b], CE_H * CE_H, nG) && span_ok(d.fc1_b[b], CE_H, nG) && span_ok(d.fc2_w[b], CE_H * CE_H, nG) &&
           span_ok(d.fc2_b[b], CE_H, nG) && span_ok(d.bn1_g[b], CE_H, nG) && span_ok(d.bn1_b[b], CE_H, nG) && span_ok(d.bn2_g[b], CE_H, nG) &&
           span_ok(d.bn2_b[b], CE_H, nG) && span_ok(d.film_gamma_w[b], CE_H * CE_COND, nG) && span_ok(d.film_gamma_b[b], CE_H, nG) &&
           span_ok(d.film_beta_w[b], CE_H * CE_COND, nG) && span_ok(d.film_beta_b[b], CE_H, nG);
    for (int s = 0; s < d.nheads; ++s)
      ok = ok && span_ok(d.head_w[s], (d.seg[s + 1] - d.seg[s]) * CE_H, nG) && span_ok(d.head_b[s], d.seg[s + 1] - d.seg[s], nG);
    PCG_REQUIRE(ok, "pcg_house_cf_eval: a generator tensor leaves the flat buffer of %d elements", nG);
  }
  for (int l = 0; l < 2 * CE_NB; ++l) PCG_REQUIRE(a.bn_mean[l] && a.bn_var[l], "pcg_house_cf_eval: null BatchNorm buffer %d", l);
  {
    int seen_c[CE_D] = {0}, seen_h[CE_HEADS] = {0};
    for (int f = 0; f < CE_D; ++f) {
      const int s = a.col_src[f];
      PCG_REQUIRE(s >= 0 ? s < d.ncont : -s - 1 < d.nheads, "pcg_house_cf_eval: col_src[%d] = %d names no output", f, s);
      int& seen = s >= 0 ? seen_c[s] : seen_h[-s - 1];
      PCG_REQUIRE(!seen, "pcg_house_cf_eval: col_src[%d] = %d is used twice", f, s);
      seen = 1;
    }
  }
  HouseCfK k{};
  for (int l = 0; l < 5; ++l) {
    PCG_REQUIRE(a.c_w_kmajor[l] && a.c_bias[l], "pcg_house_cf_eval: null classifier layer %d", l);
    k.w.wt[l] = a.c_w_kmajor[l]; k.w.b[l] = a.c_bias[l];
  }
  PCG_REQUIRE(!a.class_sums == !a.class_counts && (!a.class_sums || a.y), "pcg_house_cf_eval: class_sums and class_counts come together and need y");
  PCG_REQUIRE(a.cont || a.logits || a.chosen || a.masked || a.x_cf || a.x_cf_raw || a.logits_cf || a.logits_x || a.pred_cf || a.pred_x ||
                  a.gain || a.tile_sums || a.class_sums, "pcg_house_cf_eval: no output");
  const int64_t span = a.group < a.N ? a.group : a.N;
  const int64_t tpg = ceil_div64(span, CL_R), n_tiles = ceil_div64(a.N, a.group) * tpg;
  PCG_REQUIRE(n_tiles <= INT32_MAX, "pcg_house_cf_eval: %lld tiles exceed the grid", (long long)n_tiles);
  k.a = a;
  k.a.c_w_kmajor = nullptr; k.a.c_bias = nullptr;          // host arrays: the kernel reads k.w
  k.tiles_per_group = (int)tpg; k.n_tiles = (int)n_tiles;
  hipLaunchKernelGGL(house_cf_eval_kernel, dim3((unsigned)n_tiles), dim3(CL_NT), 0, (hipStream_t)stream, d, k);
  return launch_status("house_cf_eval_kernel");
}
