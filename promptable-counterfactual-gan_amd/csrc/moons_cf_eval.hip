// moons_cf_eval.hip — the moons CounteRGAN's counterfactual queries and evaluation (conditional_counteRGAN/moons eval_utils.py:29-106,
// :114-124, :196-206, gradio_app.py:79-95) in ONE launch over many workgroups.
//
// In eval mode BatchNorm uses the running statistics, so every row is independent of every other: one work item is
// (mask slot m, target slot t, row i), and the grid is (groups of rows) x T x M.  Layout:
//   LDS        the generator's and the classifier's weights, staged once per workgroup, BatchNorm as mean and 1 / sqrt(var + eps);
//              the matrices that are consumed column by column are stored transposed, so that every read is a same-address
//              broadcast of 16 bytes
//   registers  one thread per row, the activations of the row in registers: layer l's unit o is formed by a runtime loop over o and
//              fed at once into layer l+1's accumulators, which are the only arrays (static indices, no scratch)
//   global     x, y, masks / targets in; per-row outputs and the group sums out.  The nets are read only.
// The summation order of every dot product is lin_fwd's of moons_cf.hip (ascending input index from 0, then the bias), the
// BatchNorm expressions are g_forward's eval branch.  Group sums: thread partials over rows tid, tid + nt, ..., a wave butterfly,
// then the waves in order — no atomics, bitwise repeatable.  Launch and latency bound at the reference's sizes: no MFMA, no
// roofline claim.
#include "epoch_wg.h"

namespace pcg {
namespace {

constexpr int NT = 256;
constexpr int F = 2, NC = 3, GIN = 2 * F + NC, CH = 32;
constexpr int MAX_GROUP = 1 << 24;                       // the included / flip counts are float sums: exact up to 2^24

// LDS image of both nets, offsets in floats (every block 16-byte aligned).
template <int H>
struct Lds {
  static constexpr int H2 = H / 2;
  static constexpr int W1 = 0;                // [H][8]   net.0.weight row o (7 inputs), 0
  static constexpr int P1 = W1 + H * 8;       // [H][8]   net.0.bias, BN mean, invstd, gamma, beta, 0, 0, 0
  static constexpr int W2T = P1 + H * 8;      // [H][H]   net.3.weight transposed: [in][out]
  static constexpr int P2 = W2T + H * H;      // [5][H]   net.3.bias, BN mean, invstd, gamma, beta
  static constexpr int W3 = P2 + 5 * H;       // [H2][H]  net.6.weight
  static constexpr int P3 = W3 + H2 * H;      // [H2][8]  net.6.bias, BN mean, invstd, gamma, beta, net.9.weight[0][o], [1][o], 0
  static constexpr int B4 = P3 + H2 * 8;      // [4]      net.9.bias
  static constexpr int C1 = B4 + 4;           // [CH][4]  classifier net.0.weight row o, net.0.bias[o], 0
  static constexpr int C2T = C1 + CH * 4;     // [CH][CH] classifier net.2.weight transposed
  static constexpr int CB2 = C2T + CH * CH;   // [CH]
  static constexpr int C3 = CB2 + CH;         // [NC][CH] classifier net.4.weight
  static constexpr int CB3 = C3 + NC * CH;    // [4]
  static constexpr int RED = CB3 + 4;         // [4 waves][4]
  static constexpr int TOTAL = RED + 16;
};

// The weights are invariant and the scheduler would otherwise issue the LDS reads of several phases of a row (and of the next row)
// at once, which costs more registers than the row's activations: reads stay inside the phase that uses them.
#define PHASE_FENCE() asm volatile("" ::: "memory")
// ... and the arithmetic on them too: a value that passes through a fence is formed before the next fence's reads are issued
// (otherwise the reads stay put and the arithmetic sinks below all of them, every weight of the phase live at once)
#define FENCE4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : : "memory")
#define FENCE1(a) asm volatile("" : "+v"(a) : : "memory")

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }
// g_forward's eval branch (moons_cf.hip): x-hat = (z - mean) * invstd, then fmaf(gamma, x-hat, beta), ReLU
__device__ __forceinline__ float bn_relu(float z, float mean, float inv, float gamma, float beta) {
  return relu(fmaf(gamma, (z - mean) * inv, beta));
}

template <int H>
__device__ void stage(float* sm, const pcg_moons_cf_desc& d, const pcg_moons_cf_eval_args& a, bool gen) {
  using L = Lds<H>;
  const int tid = threadIdx.x, nt = blockDim.x;
  if (gen) {
    const float* G = a.g_flat;
    for (int idx = tid; idx < H * 8; idx += nt) {
      const int o = idx >> 3, k = idx & 7;
      sm[L::W1 + idx] = k < GIN ? G[d.g_off[0] + o * GIN + k] : 0.f;
      float v = 0.f;
      if (k == 0) v = G[d.g_off[1] + o];
      else if (k == 1) v = a.bn_mean[0][o];
      else if (k == 2) v = 1.f / sqrtf(a.bn_var[0][o] + d.bn_eps);
      else if (k == 3) v = G[d.g_off[2] + o];
      else if (k == 4) v = G[d.g_off[3] + o];
      sm[L::P1 + idx] = v;
    }
    for (int idx = tid; idx < H * H; idx += nt) {
      const int i = idx / H, j = idx - i * H;
      sm[L::W2T + idx] = G[d.g_off[4] + j * H + i];
    }
    for (int c = tid; c < H; c += nt) {
      sm[L::P2 + c] = G[d.g_off[5] + c];
      sm[L::P2 + H + c] = a.bn_mean[1][c];
      sm[L::P2 + 2 * H + c] = 1.f / sqrtf(a.bn_var[1][c] + d.bn_eps);
      sm[L::P2 + 3 * H + c] = G[d.g_off[6] + c];
      sm[L::P2 + 4 * H + c] = G[d.g_off[7] + c];
    }
    for (int idx = tid; idx < L::H2 * H; idx += nt) sm[L::W3 + idx] = G[d.g_off[8] + idx];
    for (int idx = tid; idx < L::H2 * 8; idx += nt) {
      const int o = idx >> 3, k = idx & 7;
      float v = 0.f;
      if (k == 0) v = G[d.g_off[9] + o];
      else if (k == 1) v = a.bn_mean[2][o];
      else if (k == 2) v = 1.f / sqrtf(a.bn_var[2][o] + d.bn_eps);
      else if (k == 3) v = G[d.g_off[10] + o];
      else if (k == 4) v = G[d.g_off[11] + o];
      else if (k == 5) v = G[d.g_off[12] + o];
      else if (k == 6) v = G[d.g_off[12] + L::H2 + o];
      sm[L::P3 + idx] = v;
    }
    if (tid < 4) sm[L::B4 + tid] = tid < F ? G[d.g_off[13] + tid] : 0.f;
  }
  const float* C = a.c_flat;
  for (int idx = tid; idx < CH * 4; idx += nt) {
    const int o = idx >> 2, k = idx & 3;
    sm[L::C1 + idx] = k < F ? C[d.c_off[0] + o * F + k] : (k == 2 ? C[d.c_off[1] + o] : 0.f);
  }
  for (int idx = tid; idx < CH * CH; idx += nt) {
    const int i = idx / CH, j = idx - i * CH;
    sm[L::C2T + idx] = C[d.c_off[2] + j * CH + i];
  }
  for (int c = tid; c < CH; c += nt) sm[L::CB2 + c] = C[d.c_off[3] + c];
  for (int idx = tid; idx < NC * CH; idx += nt) sm[L::C3 + idx] = C[d.c_off[4] + idx];
  if (tid < 4) sm[L::CB3 + tid] = tid < NC ? C[d.c_off[5] + tid] : 0.f;
}

// models/generator.py:20-24 in eval mode for one row: h = [x, onehot(t), mask] (h[7] unused) -> raw residual.
template <int H>
__device__ __forceinline__ void gen_row(const float* sm, const float (&h)[8], float (&raw)[F]) {
  using L = Lds<H>;
  float z[H];
#pragma unroll
  for (int j = 0; j < H; ++j) z[j] = 0.f;
#pragma unroll 2
  for (int o = 0; o < H; ++o) {                      // Linear 0 unit o -> BN 1 -> ReLU, fed into Linear 3's accumulators
    const float4 wa = ld4(sm + L::W1 + o * 8), wb = ld4(sm + L::W1 + o * 8 + 4);
    const float4 p = ld4(sm + L::P1 + o * 8);
    const float beta = sm[L::P1 + o * 8 + 4];
    float acc = 0.f;
    acc = fmaf(h[0], wa.x, acc); acc = fmaf(h[1], wa.y, acc); acc = fmaf(h[2], wa.z, acc); acc = fmaf(h[3], wa.w, acc);
    acc = fmaf(h[4], wb.x, acc); acc = fmaf(h[5], wb.y, acc); acc = fmaf(h[6], wb.z, acc);
    acc += p.x;
    const float act = bn_relu(acc, p.y, p.z, p.w, beta);
    const float* w2 = sm + L::W2T + o * H;
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 w = ld4(w2 + j);
      z[j] = fmaf(act, w.x, z[j]); z[j + 1] = fmaf(act, w.y, z[j + 1]);
      z[j + 2] = fmaf(act, w.z, z[j + 2]); z[j + 3] = fmaf(act, w.w, z[j + 3]);
    }
  }
  PHASE_FENCE();
#pragma unroll
  for (int j = 0; j < H; j += 4) {                   // Linear 3's bias -> BN 4 -> ReLU
    const float4 b = ld4(sm + L::P2 + j), mu = ld4(sm + L::P2 + H + j), is = ld4(sm + L::P2 + 2 * H + j);
    const float4 ga = ld4(sm + L::P2 + 3 * H + j), be = ld4(sm + L::P2 + 4 * H + j);
    z[j] = bn_relu(z[j] + b.x, mu.x, is.x, ga.x, be.x);
    z[j + 1] = bn_relu(z[j + 1] + b.y, mu.y, is.y, ga.y, be.y);
    z[j + 2] = bn_relu(z[j + 2] + b.z, mu.z, is.z, ga.z, be.z);
    z[j + 3] = bn_relu(z[j + 3] + b.w, mu.w, is.w, ga.w, be.w);
    FENCE4(z[j], z[j + 1], z[j + 2], z[j + 3]);
  }
  float r0 = 0.f, r1 = 0.f;
#pragma unroll 2
  for (int o = 0; o < L::H2; ++o) {                  // Linear 6 unit o -> BN 7 -> ReLU, fed into Linear 9's two accumulators
    const float* w3 = sm + L::W3 + o * H;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 w = ld4(w3 + j);
      acc = fmaf(z[j], w.x, acc); acc = fmaf(z[j + 1], w.y, acc); acc = fmaf(z[j + 2], w.z, acc); acc = fmaf(z[j + 3], w.w, acc);
    }
    const float4 p = ld4(sm + L::P3 + o * 8), q = ld4(sm + L::P3 + o * 8 + 4);
    acc += p.x;
    const float act = bn_relu(acc, p.y, p.z, p.w, q.x);
    r0 = fmaf(act, q.y, r0);
    r1 = fmaf(act, q.z, r1);
  }
  raw[0] = r0 + sm[L::B4];
  raw[1] = r1 + sm[L::B4 + 1];
}

// models/nn_classifier.py:14-15 for NR rows at once (they share every weight read).  LO: Lds<H>::C1 (the classifier's base).
template <int NR, int LO>
__device__ __forceinline__ void clf_rows(const float* sm, const float (&x)[NR][F], float (&lg)[NR][NC]) {
  constexpr int C1 = LO, C2T = C1 + CH * 4, CB2 = C2T + CH * CH, C3 = CB2 + CH, CB3 = C3 + NC * CH;
  float z[NR][CH];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int j = 0; j < CH; ++j) z[r][j] = 0.f;
#pragma unroll 2
  for (int o = 0; o < CH; ++o) {
    const float4 c = ld4(sm + C1 + o * 4);
    float act[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) act[r] = relu(fmaf(x[r][1], c.y, fmaf(x[r][0], c.x, 0.f)) + c.z);
    const float* w2 = sm + C2T + o * CH;
#pragma unroll
    for (int j = 0; j < CH; j += 4) {
      const float4 w = ld4(w2 + j);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        z[r][j] = fmaf(act[r], w.x, z[r][j]); z[r][j + 1] = fmaf(act[r], w.y, z[r][j + 1]);
        z[r][j + 2] = fmaf(act[r], w.z, z[r][j + 2]); z[r][j + 3] = fmaf(act[r], w.w, z[r][j + 3]);
      }
    }
  }
  PHASE_FENCE();
#pragma unroll
  for (int j = 0; j < CH; j += 4) {
    const float4 b = ld4(sm + CB2 + j);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      z[r][j] = relu(z[r][j] + b.x); z[r][j + 1] = relu(z[r][j + 1] + b.y);
      z[r][j + 2] = relu(z[r][j + 2] + b.z); z[r][j + 3] = relu(z[r][j + 3] + b.w);
      FENCE4(z[r][j], z[r][j + 1], z[r][j + 2], z[r][j + 3]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
#pragma unroll
    for (int j = 0; j < CH; j += 4) {
      const float4 w = ld4(sm + C3 + c * CH + j);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        acc[r] = fmaf(z[r][j], w.x, acc[r]); acc[r] = fmaf(z[r][j + 1], w.y, acc[r]);
        acc[r] = fmaf(z[r][j + 2], w.z, acc[r]); acc[r] = fmaf(z[r][j + 3], w.w, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      lg[r][c] = acc[r] + sm[CB3 + c];
      FENCE1(lg[r][c]);
    }
  }
}

// torch.argmax: the first index of the maximum
__device__ __forceinline__ int argmax3(const float (&l)[NC]) {
  int p = 0;
  float m = l[0];
  if (l[1] > m) { m = l[1]; p = 1; }
  if (l[2] > m) p = 2;
  return p;
}

// softmax(l)[t] as torch forms it in fp32: exp(l - max) / sum.  t selected by comparison: no index leaves the registers.
__device__ __forceinline__ float softmax_at(const float (&l)[NC], int t) {
  const float mx = fmaxf(fmaxf(l[0], l[1]), l[2]);
  const float e0 = expf(l[0] - mx), e1 = expf(l[1] - mx), e2 = expf(l[2] - mx);
  const float et = t == 0 ? e0 : (t == 1 ? e1 : e2);
  return et / (e0 + e1 + e2);
}

template <int H>
__global__ void __launch_bounds__(NT) moons_cf_eval_kernel(const pcg_moons_cf_desc d, const pcg_moons_cf_eval_args a, int n_groups) {
  using L = Lds<H>;
  __shared__ __attribute__((aligned(16))) float sm[L::TOTAL];
  const bool gen = a.g_flat != nullptr;
  stage<H>(sm, d, a, gen);
  __syncthreads();
  const int tid = threadIdx.x, nt = blockDim.x;
  const int m = blockIdx.z, tb = blockIdx.y;
  const int64_t N = a.N;
  const int64_t first = (int64_t)blockIdx.x * a.group;
  const int64_t last = first + a.group < N ? first + a.group : N;
  const size_t slot = (size_t)m * a.T + tb;                // per-row form: M = T = 1, slot 0
  const bool base = m == 0 && tb == 0;                      // the workgroups that write logits_x / pred_x
  float s[4] = {0.f, 0.f, 0.f, 0.f};                        // included rows, flips, sum gain, sum |masked|
  for (int64_t i = first + tid; i < last; i += nt) {
    PHASE_FENCE();
    float x[2][F], lg[2][NC];
    x[0][0] = a.x[2 * i];
    x[0][1] = a.x[2 * i + 1];
    if (!gen) {                                             // the classifier alone (the decision grid)
      float x1[1][F] = {{x[0][0], x[0][1]}}, l1[1][NC];
      clf_rows<1, L::C1>(sm, x1, l1);
      if (a.logits_x) { a.logits_x[3 * i] = l1[0][0]; a.logits_x[3 * i + 1] = l1[0][1]; a.logits_x[3 * i + 2] = l1[0][2]; }
      if (a.pred_x) a.pred_x[i] = argmax3(l1[0]);
      continue;
    }
    const int t = a.target ? (int)a.target[i] : tb;
    const float* mk = a.row_mask ? a.row_mask + 2 * i : a.masks + 2 * m;
    const float m0 = mk[0], m1 = mk[1];
    const float h[8] = {x[0][0], x[0][1], t == 0 ? 1.f : 0.f, t == 1 ? 1.f : 0.f, t == 2 ? 1.f : 0.f, m0, m1, 0.f};
    float raw[F];
    gen_row<H>(sm, h, raw);
    // two roundings each, as the reference's `raw * mask` and `x + masked_residual` (no contraction into one fma)
    const float md0 = __fmul_rn(raw[0], m0), md1 = __fmul_rn(raw[1], m1);
    x[1][0] = __fadd_rn(x[0][0], md0);
    x[1][1] = __fadd_rn(x[0][1], md1);
    clf_rows<2, L::C1>(sm, x, lg);
    const int px = argmax3(lg[0]), pc = argmax3(lg[1]);
    const float gain = softmax_at(lg[1], t) - softmax_at(lg[0], t);
    const size_t oi = slot * (size_t)N + (size_t)i;
    if (a.raw) { a.raw[2 * oi] = raw[0]; a.raw[2 * oi + 1] = raw[1]; }
    if (a.masked) { a.masked[2 * oi] = md0; a.masked[2 * oi + 1] = md1; }
    if (a.x_cf) { a.x_cf[2 * oi] = x[1][0]; a.x_cf[2 * oi + 1] = x[1][1]; }
    if (a.logits_cf) { a.logits_cf[3 * oi] = lg[1][0]; a.logits_cf[3 * oi + 1] = lg[1][1]; a.logits_cf[3 * oi + 2] = lg[1][2]; }
    if (a.pred_cf) a.pred_cf[oi] = pc;
    if (a.gain) a.gain[oi] = gain;
    if (base) {
      if (a.logits_x) { a.logits_x[3 * i] = lg[0][0]; a.logits_x[3 * i + 1] = lg[0][1]; a.logits_x[3 * i + 2] = lg[0][2]; }
      if (a.pred_x) a.pred_x[i] = px;
    }
    if (!a.y || a.y[i] != (int64_t)t) {                     // eval_utils.py:57
      s[0] += 1.f;
      s[1] += pc == t ? 1.f : 0.f;
      s[2] += gain;
      s[3] += fabsf(md0) + fabsf(md1);
    }
  }
  if (!a.sums) return;                                      // (uniform)
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
  float* red = sm + L::RED;
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[4 * (tid >> 6) + k] = s[k];
  }
  __syncthreads();
  if (tid < 4) {
    float v = red[tid];
    for (int w = 1; w < (nt >> 6); ++w) v += red[4 * w + tid];
    a.sums[(slot * (size_t)n_groups + blockIdx.x) * 4 + tid] = v;
  }
}

bool span_ok(int off, int n, int total) { return off >= 0 && n >= 0 && off <= total - n; }

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" int pcg_moons_cf_eval(const pcg_moons_cf_desc* desc, const pcg_moons_cf_eval_args* args, pcg_stream_t stream) {
  PCG_REQUIRE(desc && args, "pcg_moons_cf_eval: null descriptor or arguments");
  const pcg_moons_cf_desc& d = *desc;
  const pcg_moons_cf_eval_args& a = *args;
  PCG_REQUIRE(d.hidden == 32 || d.hidden == 64, "pcg_moons_cf_eval: hidden_dim %d (built for 32 and 64)", d.hidden);
  PCG_REQUIRE(d.clf_hidden == CH, "pcg_moons_cf_eval: classifier hidden width %d (built for %d)", d.clf_hidden, CH);
  PCG_REQUIRE(a.N >= 1 && a.group >= 1 && a.group <= MAX_GROUP, "pcg_moons_cf_eval: N %lld, group %d (N >= 1, 1 <= group <= %d)",
              (long long)a.N, a.group, MAX_GROUP);
  const int64_t n_groups = ceil_div64(a.N, a.group);
  PCG_REQUIRE(n_groups <= INT32_MAX, "pcg_moons_cf_eval: %lld groups exceed the grid", (long long)n_groups);
  PCG_REQUIRE(a.x && a.c_flat, "pcg_moons_cf_eval: null x or classifier parameters");
  const int H = d.hidden;
  const int csz[6] = {CH * F, CH, CH * CH, CH, NC * CH, NC};
  for (int k = 0; k < 6; ++k)
    PCG_REQUIRE(span_ok(d.c_off[k], csz[k], d.nC), "pcg_moons_cf_eval: classifier tensor %d at %d (+%d) leaves the flat buffer of %d", k,
                d.c_off[k], csz[k], d.nC);
  const bool gen = a.g_flat != nullptr;
  if (gen) {
    const int gsz[14] = {H * GIN, H, H, H, H * H, H, H, H, (H / 2) * H, H / 2, H / 2, H / 2, F * (H / 2), F};
    for (int k = 0; k < 14; ++k)
      PCG_REQUIRE(span_ok(d.g_off[k], gsz[k], d.nG), "pcg_moons_cf_eval: generator tensor %d at %d (+%d) leaves the flat buffer of %d", k,
                  d.g_off[k], gsz[k], d.nG);
    for (int l = 0; l < 3; ++l) PCG_REQUIRE(a.bn_mean[l] && a.bn_var[l], "pcg_moons_cf_eval: null BatchNorm buffer");
    if (a.target || a.row_mask) {
      PCG_REQUIRE(a.target && a.row_mask && !a.masks && a.M == 1 && a.T == 1,
                  "pcg_moons_cf_eval: the per-row form takes target [N] and row_mask [N][2], no masks, M = T = 1");
    } else {
      PCG_REQUIRE(a.masks && a.M >= 1 && a.M <= 65535 && a.T >= 1 && a.T <= NC,
                  "pcg_moons_cf_eval: the sweep form takes masks [M][2], 1 <= M <= 65535, 1 <= T <= %d (got M %d, T %d)", NC, a.M, a.T);
    }
    PCG_REQUIRE(a.raw || a.masked || a.x_cf || a.logits_cf || a.logits_x || a.pred_cf || a.pred_x || a.gain || a.sums,
                "pcg_moons_cf_eval: no output");
  } else {
    PCG_REQUIRE(!a.raw && !a.masked && !a.x_cf && !a.logits_cf && !a.pred_cf && !a.gain && !a.sums && !a.masks && !a.target && !a.row_mask &&
                    a.M == 1 && a.T == 1,
                "pcg_moons_cf_eval: without a generator only logits_x / pred_x are produced (M = T = 1)");
    PCG_REQUIRE(a.logits_x || a.pred_x, "pcg_moons_cf_eval: no output");
  }
  const int64_t rows = a.group < a.N ? a.group : a.N;
  const int nt = rows >= NT ? NT : (int)((rows + 63) / 64) * 64;
  const dim3 grid((unsigned)n_groups, (unsigned)a.T, (unsigned)a.M);
  hipStream_t s = (hipStream_t)stream;
  if (H == 32) hipLaunchKernelGGL(moons_cf_eval_kernel<32>, grid, dim3(nt), 0, s, d, a, (int)n_groups);
  else hipLaunchKernelGGL(moons_cf_eval_kernel<64>, grid, dim3(nt), 0, s, d, a, (int)n_groups);
  return launch_status("moons_cf_eval_kernel");
}
