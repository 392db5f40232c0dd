// moons_cf.hip — the moons CounteRGAN (conditional_counteRGAN/moons) as whole training iterations in ONE launch of ONE workgroup.
//
// The step is launch-latency bound (batch 64, 2 features, 3 classes, ~4.3 k parameters over three nets): eager PyTorch issues
// 150+ kernels per iteration, each of which does almost nothing.  Here one workgroup of 256 threads runs n_steps iterations of
// trainer.py:58-113 back to back.  Layout:
//   LDS        G and D parameters and gradients, D's W/sigma and dW/sigma staging, u / v of the three power iterations of an
//              iteration, BatchNorm statistics, reduction scratch; the activations too when they fit (batch 64 at hidden 32),
//              otherwise a global scratch buffer the caller allocates (generic pointers: the same code serves both)
//   registers  the Adam moments of G and D, element i held by thread i % 256 (slot i / 256)
//   global     the training set, the per-step rows / targets / masks, the frozen classifier's parameters (read through L2)
// Every reduction has a fixed order (wave butterflies, then waves in order; column sums in fixed row partitions): a launch of
// n steps is bit-identical to n launches of one.
#include "epoch_wg.h"

namespace pcg {
namespace {

constexpr int NT = 256;                                  // four waves; wave l runs layer l's power iteration
constexpr int F = 2, NC = 3, GIN = 2 * F + NC, DIN = F + NC, CH = 32;
constexpr int NLOG = 9;

// K block-wide sums in one pair of barriers; every thread receives all K.  red: 4*K floats.
template <int K>
__device__ __forceinline__ void block_sums(float (&v)[K], float* red) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[4 * k + w] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[4 * k] + red[4 * k + 1]) + (red[4 * k + 2] + red[4 * k + 3]);
}

// Column reductions over B rows of [B][ld] matrices, fixed partition: thread t sums rows p, p + P, ... of column t % C
// (p = t / C, P = NT / C), then thread c < C adds the P partials in order.  mode 0: sum A; 1: sum (A - sub[c])^2; 2: sum A * Bm.
// red: 2 * NT floats.  Two barriers; out0 / out1 valid after return.  mode 3: both sum A (out0) and sum A * Bm (out1).
__device__ void col_sums(int mode, const float* A, const float* Bm, const float* sub, int ld, int C, int B, float* red, float* out0,
                         float* out1) {
  const int t = threadIdx.x, P = NT / C, c = t % C, p = t / C;
  float s0 = 0.f, s1 = 0.f;
  if (p < P) {
    const float m = (mode == 1) ? sub[c] : 0.f;
    for (int b = p; b < B; b += P) {
      const float a = A[(size_t)b * ld + c];
      if (mode == 0) s0 += a;
      else if (mode == 1) { const float d = a - m; s0 = fmaf(d, d, s0); }
      else if (mode == 2) s0 = fmaf(a, Bm[(size_t)b * ld + c], s0);
      else { s0 += a; s1 = fmaf(a, Bm[(size_t)b * ld + c], s1); }
    }
    red[p * C + c] = s0;
    red[NT + p * C + c] = s1;
  }
  __syncthreads();
  if (t < C) {
    float a0 = 0.f, a1 = 0.f;
    for (int q = 0; q < P; ++q) { a0 += red[q * C + t]; a1 += red[NT + q * C + t]; }
    out0[t] = a0;
    if (mode == 3) out1[t] = a1;
  }
  __syncthreads();
}

// Y[b][o] = act(bias[o] + sum_i X[b][i] W[o][i]); act: neg < 0 none, else v > 0 ? v : v * neg.  X row stride ldx, Y [B][O].
__device__ void lin_fwd(const float* X, int ldx, int I, const float* W, const float* bias, float* Y, int O, int B, float neg) {
  for (int idx = threadIdx.x; idx < B * O; idx += NT) {
    const int b = idx / O, o = idx - b * O;
    const float* x = X + (size_t)b * ldx;
    const float* w = W + o * I;
    float acc = 0.f;
#pragma unroll 4
    for (int i = 0; i < I; ++i) acc = fmaf(x[i], w[i], acc);
    acc += bias[o];
    if (neg >= 0.f) acc = acc > 0.f ? acc : acc * neg;
    Y[idx] = acc;
  }
}

// dX[b][i] = (sum_o dZ[b][o] W[o][i]) * act'(A[b][i]) (A: the layer input as the previous activation produced it; nullptr: no
// activation), dX [B][ldo], columns [0, Iout).  act'(a) = a > 0 ? 1 : neg (ReLU: neg 0; LeakyReLU: 0.2 — the sign of a LeakyReLU
// output is its input's).
__device__ void lin_dx(const float* dZ, int O, const float* W, int I, const float* A, float neg, float* dX, int ldo, int Iout, int B) {
  for (int idx = threadIdx.x; idx < B * Iout; idx += NT) {
    const int b = idx / Iout, i = idx - b * Iout;
    const float* dz = dZ + (size_t)b * O;
    float acc = 0.f;
#pragma unroll 4
    for (int o = 0; o < O; ++o) acc = fmaf(dz[o], W[o * I + i], acc);
    if (A) acc = A[(size_t)b * I + i] > 0.f ? acc : acc * neg;
    dX[(size_t)b * ldo + i] = acc;
  }
}

// dW[o][i] = sum_b dZ[b][o] X[b][i], db[o] = sum_b dZ[b][o] (overwrite).  X row stride ldx.
__device__ void lin_dw(const float* dZ, int O, const float* X, int ldx, int I, float* dW, float* db, int B) {
  for (int idx = threadIdx.x; idx < O * I + O; idx += NT) {
    if (idx < O * I) {
      const int o = idx / I, i = idx - o * I;
      float acc = 0.f;
#pragma unroll 4
      for (int b = 0; b < B; ++b) acc = fmaf(dZ[(size_t)b * O + o], X[(size_t)b * ldx + i], acc);
      dW[idx] = acc;
    } else {
      const int o = idx - O * I;
      float acc = 0.f;
#pragma unroll 4
      for (int b = 0; b < B; ++b) acc += dZ[(size_t)b * O + o];
      db[o] = acc;
    }
  }
}

template <int H>
struct Dims {
  static constexpr int GO[4] = {H, H, H / 2, F}, GI[4] = {GIN, H, H, H / 2};
  static constexpr int DO[4] = {H, H / 2, H / 2, 1}, DI[4] = {DIN, H, H / 2, H / 2};
  static constexpr int gmax() { return 7 * H + H + 2 * H + H * H + H + 2 * H + H * (H / 2) + H / 2 + H + (H / 2) * F + F + 4 * 14; }
  static constexpr int dmax() { return DIN * H + H + H * (H / 2) + H / 2 + (H / 2) * (H / 2) + H / 2 + H / 2 + 1 + 4 * 8; }
  static constexpr int SG = (gmax() + NT - 1) / NT, SD = (dmax() + NT - 1) / NT;
};

// Activation layout, floats, every matrix row-major [B][width].  The classifier's three matrices of the generator step overlay
// the real pass's critic activations, dead by then.
struct ActLayout {
  int hin, gz[3], ga[3], raw, xcf, tgt, dxc, dxd, dinR, rA[3], rO, dinF, fA[3], fO, dP, dQ, c0, c1, cl, total;
};
__host__ __device__ inline ActLayout act_layout(int H, int B) {
  ActLayout L;
  int o = 0;
  auto take = [&](int w) { const int r = o; o += r4(w * B); return r; };
  L.hin = take(GIN);
  L.gz[0] = take(H); L.ga[0] = take(H); L.gz[1] = take(H); L.ga[1] = take(H); L.gz[2] = take(H / 2); L.ga[2] = take(H / 2);
  L.raw = take(F); L.xcf = take(F); L.tgt = take(1); L.dxc = take(F); L.dxd = take(F);
  const int rbase = o;
  L.dinR = take(DIN); L.rA[0] = take(H); L.rA[1] = take(H / 2); L.rA[2] = take(H / 2); L.rO = take(1);
  const int rend = o;
  L.dinF = take(DIN); L.fA[0] = take(H); L.fA[1] = take(H / 2); L.fA[2] = take(H / 2); L.fO = take(1);
  const int dw = H > CH ? H : CH;
  L.dP = take(dw); L.dQ = take(dw);
  L.c0 = rbase; L.c1 = rbase + r4(CH * B); L.cl = L.c1 + r4(CH * B);
  if (L.cl + r4(NC * B) > rend) { L.c0 = take(CH); L.c1 = take(CH); L.cl = take(NC); }   // (never at F = 2, NC = 3)
  L.total = o;
  return L;
}

// Fixed LDS part of the train kernel, floats.
struct SmemLayout {
  int gP, dP, gG, dG, wbar, tmp, su, sv, sig, bnrm, bnrv, bnmean, bninv, red, misc, total;
};
__host__ __device__ inline SmemLayout smem_layout(int H, int nG, int nD) {
  SmemLayout S;
  int o = 0;
  auto take = [&](int n) { const int r = o; o += r4(n); return r; };
  S.gP = take(nG); S.dP = take(nD); S.gG = take(nG); S.dG = take(nD); S.wbar = take(nD); S.tmp = take(nD);
  S.su = take(3 * 4 * H); S.sv = take(3 * 4 * H); S.sig = take(3 * 4);
  S.bnrm = take(3 * H); S.bnrv = take(3 * H); S.bnmean = take(3 * H); S.bninv = take(3 * H);
  S.red = take(2 * NT); S.misc = take(32);
  S.total = o;
  return S;
}

// Spectral norm of the four critic layers, wave l on layer l (torch.nn.utils.spectral_norm, n_power_iterations = 1):
//   power:  v = normalize(W^T u_in), u = normalize(W v)   (F.normalize: x / max(||x||, eps)), written to u_out / v_out
//   sigma = u . (W v);  wbar = W / sigma  (at the layer's offset inside the D-shaped buffer `wbar`)
// Vectors of layer l at base + l * H.  Without power, u_out / v_out must equal u_in (v_in unused; eval mode: the stored vectors).
// dW: the critic's flat parameters; woff: LDS copy of the four weight offsets (no private arrays: a wave-indexed one is scratch).
template <int H>
__device__ void sn_forward(const float* dW, const int* woff, const float* u_in, const float* v_in, float* u_out, float* v_out, float* sig,
                           float* wbar, bool power, float eps) {
  using Dm = Dims<H>;
  const int l = threadIdx.x >> 6, j = threadIdx.x & 63;
  const int O = l == 0 ? Dm::DO[0] : l == 1 ? Dm::DO[1] : l == 2 ? Dm::DO[2] : Dm::DO[3];
  const int I = l == 0 ? Dm::DI[0] : l == 1 ? Dm::DI[1] : l == 2 ? Dm::DI[2] : Dm::DI[3];
  const int wo = woff[l];
  const float* W = dW + wo;
  const float* ui = u_in + l * H;
  float* uo = u_out + l * H;
  float* vo = v_out + l * H;
  if (power) {
    float t = 0.f;
    if (j < I) for (int o = 0; o < O; ++o) t = fmaf(W[o * I + j], ui[o], t);
    const float n1 = sqrtf(wave_sum(t * t));
    if (j < I) vo[j] = t / fmaxf(n1, eps);
    __syncthreads();
    float s = 0.f;
    if (j < O) for (int i = 0; i < I; ++i) s = fmaf(W[j * I + i], vo[i], s);
    const float n2 = sqrtf(wave_sum(s * s));
    if (j < O) uo[j] = s / fmaxf(n2, eps);
    __syncthreads();
  }
  float wv = 0.f;
  if (j < O) for (int i = 0; i < I; ++i) wv = fmaf(W[j * I + i], vo[i], wv);
  const float sigma = wave_sum(j < O ? uo[j] * wv : 0.f);
  if (j == 0) sig[l] = sigma;
  for (int k = j; k < O * I; k += 64) wbar[wo + k] = W[k] / sigma;
  __syncthreads();
}

// Critic forward on din [B][DIN] with the normalised weights wbar (D-shaped buffer): A[0..2] post-LeakyReLU, out [B][1].
template <int H>
__device__ void d_forward(const float* din, const float* wbar, const float* dparams, const int* woff, const int* boff, float* const* A,
                          float* out, int B, float slope) {
  using Dm = Dims<H>;
  const float* x = din;
  int ld = DIN;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    float* y = l < 3 ? A[l] : out;
    lin_fwd(x, ld, Dm::DI[l], wbar + woff[l], dparams + boff[l], y, Dm::DO[l], B, l < 3 ? slope : -1.f);
    __syncthreads();
    x = y; ld = Dm::DO[l];
  }
}

// Critic backward from dout = c (the same constant for every row: the gradient of +-mean(D)).  With weights: dW-bar of every layer
// into tmp (D-shaped), db into dgrad (overwrite or add).  dx: the gradient of the first `nx` input columns ([B][nx]), or nullptr.
template <int H>
__device__ void d_backward(float c, const float* din, const float* wbar, const int* woff, const int* boff, float* const* A, float* dP,
                           float* dQ, float* tmp, float* dgrad, bool accumulate_b, float* dx, int nx, int B, float slope, bool weights) {
  using Dm = Dims<H>;
  for (int b = threadIdx.x; b < B; b += NT) dP[b] = c;
  __syncthreads();
  float* dz = dP;
  float* nxt = dQ;
#pragma unroll
  for (int l = 3; l >= 0; --l) {
    const int O = Dm::DO[l], I = Dm::DI[l];
    const float* X = l > 0 ? A[l - 1] : din;
    if (weights) {
      for (int idx = threadIdx.x; idx < O * I + O; idx += NT) {
        if (idx < O * I) {
          const int o = idx / I, i = idx - o * I;
          float acc = 0.f;
          for (int b = 0; b < B; ++b) acc = fmaf(dz[(size_t)b * O + o], X[(size_t)b * I + i], acc);
          tmp[woff[l] + idx] = acc;
        } else {
          const int o = idx - O * I;
          float acc = 0.f;
          for (int b = 0; b < B; ++b) acc += dz[(size_t)b * O + o];
          dgrad[boff[l] + o] = accumulate_b ? dgrad[boff[l] + o] + acc : acc;
        }
      }
    }
    if (l > 0) lin_dx(dz, O, wbar + woff[l], I, A[l - 1], slope, nxt, I, I, B);
    else if (dx) lin_dx(dz, O, wbar + woff[l], I, nullptr, 0.f, dx, nx, nx, B);
    __syncthreads();
    float* t = dz; dz = nxt; nxt = t;
  }
}

// dW += dWbar / sigma - (<dWbar, W> / sigma^2) u v^T for the four layers (the path through sigma = u . W v, u and v constant).
template <int H>
__device__ void sn_backward(const float* tmp, const float* W, const int* woff, const float* u, const float* v, const float* sig,
                            float* dW, bool accumulate, float* red) {
  using Dm = Dims<H>;
  float dots[4];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const int n = Dm::DO[l] * Dm::DI[l];
    float a = 0.f;
    for (int k = threadIdx.x; k < n; k += NT) a = fmaf(tmp[woff[l] + k], W[woff[l] + k], a);
    dots[l] = a;
  }
  block_sums<4>(dots, red);
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const int O = Dm::DO[l], I = Dm::DI[l];
    const float s = sig[l], gs = -dots[l] / (s * s);
    for (int k = threadIdx.x; k < O * I; k += NT) {
      const int o = k / I, i = k - o * I;
      const float g = fmaf(gs, u[l * H + o] * v[l * H + i], tmp[woff[l] + k] / s);
      dW[woff[l] + k] = accumulate ? dW[woff[l] + k] + g : g;
    }
  }
  __syncthreads();
}

// Generator forward.  train: batch statistics (biased variance for the normalisation, unbiased into the running variance,
// momentum), else the running statistics.  gz[l] = x-hat, ga[l] = ReLU(gamma x-hat + beta).  raw [B][2].
template <int H>
__device__ void g_forward(const float* hin, const float* P, const int* go, float* const* gz, float* const* ga, float* raw, int B, bool train,
                          float* rm, float* rv, float* mean, float* inv, float eps, float mom, float* red) {
  using Dm = Dims<H>;
  const float* x = hin;
  int ld = GIN;
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int O = Dm::GO[l];
    lin_fwd(x, ld, Dm::GI[l], P + go[4 * l], P + go[4 * l + 1], gz[l], O, B, -1.f);
    __syncthreads();
    float* mu = mean + l * H;
    float* is = inv + l * H;
    if (train) {
      col_sums(0, gz[l], nullptr, nullptr, O, O, B, red, mu, nullptr);
      if (threadIdx.x < O) mu[threadIdx.x] = mu[threadIdx.x] / (float)B;
      __syncthreads();
      col_sums(1, gz[l], nullptr, mu, O, O, B, red, is, nullptr);
      if (threadIdx.x < O) {
        const int c = threadIdx.x;
        const float var = is[c] / (float)B;
        const float unbiased = is[c] / (float)(B - 1);
        rm[l * H + c] = (1.f - mom) * rm[l * H + c] + mom * mu[c];
        rv[l * H + c] = (1.f - mom) * rv[l * H + c] + mom * unbiased;
        is[c] = 1.f / sqrtf(var + eps);
      }
    } else if (threadIdx.x < O) {
      const int c = threadIdx.x;
      mu[c] = rm[l * H + c];
      is[c] = 1.f / sqrtf(rv[l * H + c] + eps);
    }
    __syncthreads();
    const float* gamma = P + go[4 * l + 2];
    const float* beta = P + go[4 * l + 3];
    for (int idx = threadIdx.x; idx < B * O; idx += NT) {
      const int c = idx % O;
      const float xh = (gz[l][idx] - mu[c]) * is[c];
      gz[l][idx] = xh;
      const float a = fmaf(gamma[c], xh, beta[c]);
      ga[l][idx] = a > 0.f ? a : 0.f;
    }
    __syncthreads();
    x = ga[l]; ld = O;
  }
  lin_fwd(x, ld, Dm::GI[3], P + go[12], P + go[13], raw, F, B, -1.f);
  __syncthreads();
}

// Classifier forward (eval): c0 = ReLU, c1 = ReLU, logits.
__device__ void c_forward(const float* x, int ldx, const float* P, const int* co, float* c0, float* c1, float* cl, int B) {
  lin_fwd(x, ldx, F, P + co[0], P + co[1], c0, CH, B, 0.f);
  __syncthreads();
  lin_fwd(c0, CH, CH, P + co[2], P + co[3], c1, CH, B, 0.f);
  __syncthreads();
  lin_fwd(c1, CH, CH, P + co[4], P + co[5], cl, NC, B, -1.f);
  __syncthreads();
}

// beta^t for adam_corr: pow() on every thread (moons_gan.hip has binary exponentiation on one thread; each kernel keeps its own)
__device__ __forceinline__ double pow_t(double beta, int64_t t) { return pow(beta, (double)t); }

template <int H>
__global__ void __launch_bounds__(NT) moons_cf_train_kernel(const pcg_moons_cf_desc d, const pcg_moons_cf_train_args a, int n_steps,
                                                            int act_in_lds) {
  using Dm = Dims<H>;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, B = d.B;
  const SmemLayout S = smem_layout(H, d.nG, d.nD);
  const ActLayout L = act_layout(H, B);
  float* act = act_in_lds ? sm + S.total : a.scratch;
  float *gP = sm + S.gP, *dP = sm + S.dP, *gG = sm + S.gG, *dG = sm + S.dG, *wbar = sm + S.wbar, *tmp = sm + S.tmp;
  float *red = sm + S.red, *sig = sm + S.sig;
  const float* cP = a.c_flat;
  // the descriptor's offset tables, copied to LDS: a runtime index into a by-value kernel argument would live in scratch
  int* go = reinterpret_cast<int*>(sm + S.misc);
  int* co = go + 14;
  int* woff = go + 20;                      // the critic's weight_orig offsets, then its bias offsets
  int* boff = go + 24;
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 14; ++k) go[k] = d.g_off[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) co[k] = d.c_off[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) woff[k] = d.d_off[k];
  }
  // u / v of the three power iterations of an iteration (slot 0: D(real), 1: D(fake), 2: the generator step's = the state)
  float* su[3] = {sm + S.su, sm + S.su + 4 * H, sm + S.su + 8 * H};
  float* sv[3] = {sm + S.sv, sm + S.sv + 4 * H, sm + S.sv + 8 * H};
  float *hin = act + L.hin, *raw = act + L.raw, *xcf = act + L.xcf, *tgt = act + L.tgt, *dinR = act + L.dinR, *dinF = act + L.dinF;
  float* gz[3] = {act + L.gz[0], act + L.gz[1], act + L.gz[2]};
  float* ga[3] = {act + L.ga[0], act + L.ga[1], act + L.ga[2]};
  float* rA[3] = {act + L.rA[0], act + L.rA[1], act + L.rA[2]};
  float* fA[3] = {act + L.fA[0], act + L.fA[1], act + L.fA[2]};
  float *dxc = act + L.dxc, *dxd = act + L.dxd;
  float *rO = act + L.rO, *fO = act + L.fO, *bP = act + L.dP, *bQ = act + L.dQ, *c0 = act + L.c0, *c1 = act + L.c1, *cl = act + L.cl;

  // ---- state in: parameters and buffers to LDS, moments to registers ------------------------------------------------------
  for (int i = tid; i < d.nG; i += NT) { gP[i] = a.g_flat[i]; gG[i] = 0.f; }
  for (int i = tid; i < d.nD; i += NT) { dP[i] = a.d_flat[i]; dG[i] = 0.f; tmp[i] = 0.f; wbar[i] = 0.f; }
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    for (int k = tid; k < Dm::DO[l]; k += NT) su[2][l * H + k] = a.sn_u[l][k];
    for (int k = tid; k < Dm::DI[l]; k += NT) sv[2][l * H + k] = a.sn_v[l][k];
  }
#pragma unroll
  for (int l = 0; l < 3; ++l)
    for (int k = tid; k < Dm::GO[l]; k += NT) { sm[S.bnrm + l * H + k] = a.bn_mean[l][k]; sm[S.bnrv + l * H + k] = a.bn_var[l][k]; }
  float mG[Dm::SG], vG[Dm::SG], mD[Dm::SD], vD[Dm::SD];
#pragma unroll
  for (int s = 0; s < Dm::SG; ++s) {
    const int i = tid + s * NT;
    mG[s] = i < d.nG_adam ? a.g_exp_avg[i] : 0.f;
    vG[s] = i < d.nG_adam ? a.g_exp_avg_sq[i] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < Dm::SD; ++s) {
    const int i = tid + s * NT;
    mD[s] = i < d.nD_adam ? a.d_exp_avg[i] : 0.f;
    vD[s] = i < d.nD_adam ? a.d_exp_avg_sq[i] : 0.f;
  }
  const int64_t g_step0 = a.g_step[0], d_step0 = a.d_step[0];
  const AdamK ak = adam_k(d);
  const float inv_b = 1.f / (float)B;
  __syncthreads();

  for (int it = 0; it < n_steps; ++it) {
    // ---- 1. batch (trainer.py:58-69; draws made by the caller) ------------------------------------------------------------
    const int64_t* rows = a.rows + (size_t)it * B;
    const int64_t* ty = a.target_y + (size_t)it * B;
    const float* mk = a.mask + (size_t)it * B * F;
    for (int b = tid; b < B; b += NT) {
      const int64_t r = rows[b];
      const int y = (int)a.Y[r], t = (int)ty[b];
      const float x0 = a.X[2 * r], x1 = a.X[2 * r + 1];
      float* h = hin + b * GIN;
      h[0] = x0; h[1] = x1;
      for (int c = 0; c < NC; ++c) h[F + c] = c == t ? 1.f : 0.f;
      h[F + NC] = mk[2 * b]; h[F + NC + 1] = mk[2 * b + 1];
      float* dr = dinR + b * DIN;
      dr[0] = x0; dr[1] = x1;
      for (int c = 0; c < NC; ++c) dr[F + c] = c == y ? 1.f : 0.f;
      tgt[b] = (float)t;
    }
    __syncthreads();
    // ---- 2. generator forward, training mode (:70-73) ------------------------------------------------------------------------
    g_forward<H>(hin, gP, go, gz, ga, raw, B, true, sm + S.bnrm, sm + S.bnrv, sm + S.bnmean, sm + S.bninv, d.bn_eps, d.bn_momentum, red);
    for (int b = tid; b < B; b += NT) {
      const float* h = hin + b * GIN;
      float* df = dinF + b * DIN;
      for (int j = 0; j < F; ++j) {
        const float xc = h[j] + raw[b * F + j] * h[F + NC + j];
        xcf[b * F + j] = xc;
        df[j] = xc;
      }
      for (int c = 0; c < NC; ++c) df[F + c] = h[F + c];
    }
    // ---- 3. critic step (:76-80): two power iterations, two passes, backward through both, Adam D -------------------------
    sn_forward<H>(dP, woff, su[2], sv[2], su[0], sv[0], sig, wbar, true, d.sn_eps);         // (its first barrier orders dinF)
    d_forward<H>(dinR, wbar, dP, woff, boff, rA, rO, B, d.slope);
    sn_forward<H>(dP, woff, su[0], sv[0], su[1], sv[1], sig + 4, wbar, true, d.sn_eps);
    d_forward<H>(dinF, wbar, dP, woff, boff, fA, fO, B, d.slope);
    float lr[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = tid; b < B; b += NT) {
      const float r = rO[b], f = fO[b];
      lr[0] += r; lr[1] += f;
      lr[2] += 1.f / (1.f + expf(-r)); lr[3] += 1.f / (1.f + expf(-f));
    }
    block_sums<4>(lr, red);
    const float mean_real = lr[0] * inv_b, mean_fake = lr[1] * inv_b;
    const float d_loss = -mean_real + mean_fake;
    // backward of the fake pass (wbar holds its W / sigma), then the real pass
    d_backward<H>(inv_b, dinF, wbar, woff, boff, fA, bP, bQ, tmp, dG, false, nullptr, 0, B, d.slope, true);
    sn_backward<H>(tmp, dP, woff, su[1], sv[1], sig + 4, dG, false, red);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const float s = sig[l];
      for (int k = tid; k < Dm::DO[l] * Dm::DI[l]; k += NT) wbar[woff[l] + k] = dP[woff[l] + k] / s;
    }
    __syncthreads();
    d_backward<H>(-inv_b, dinR, wbar, woff, boff, rA, bP, bQ, tmp, dG, true, nullptr, 0, B, d.slope, true);
    sn_backward<H>(tmp, dP, woff, su[0], sv[0], sig, dG, true, red);
    {
      float ss, bc2;
      adam_corr(d.lr_D, d.beta1, d.beta2, d_step0 + it + 1, pow_t, ss, bc2);
#pragma unroll
      for (int s = 0; s < Dm::SD; ++s) {
        const int i = tid + s * NT;
        if (i < d.nD_adam) { float p = dP[i]; adam_upd(p, dG[i], mD[s], vD[s], ak, ss, bc2); dP[i] = p; }
      }
    }
    __syncthreads();
    // ---- 4. generator step (:83-99) ----------------------------------------------------------------------------------------
    sn_forward<H>(dP, woff, su[1], sv[1], su[2], sv[2], sig + 8, wbar, true, d.sn_eps);
    d_forward<H>(dinF, wbar, dP, woff, boff, fA, fO, B, d.slope);
    c_forward(xcf, F, cP, co, c0, c1, cl, B);
    float gl[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // sum D, sum CE, sum l1, sum l2, sum |raw (1 - m)|
    for (int b = tid; b < B; b += NT) {
      gl[0] += fO[b];
      const float* lg = cl + b * NC;
      const float mx = fmaxf(fmaxf(lg[0], lg[1]), lg[2]);
      const float se = expf(lg[0] - mx) + expf(lg[1] - mx) + expf(lg[2] - mx);
      const int t = (int)tgt[b];
      gl[1] += mx + logf(se) - lg[t];
      const float* h = hin + b * GIN;
      float l1 = 0.f, l2 = 0.f, mp = 0.f;
      for (int j = 0; j < F; ++j) {
        const float r = raw[b * F + j], m = h[F + NC + j], q = r * m;
        l1 += fabsf(q); l2 = fmaf(q, q, l2); mp += fabsf(r * (1.f - m));
      }
      gl[2] += l1; gl[3] += sqrtf(l2); gl[4] += mp;
    }
    block_sums<5>(gl, red);
    const float g_adv = -gl[0] * inv_b, g_cls = gl[1] * inv_b, reg_l1 = gl[2] * inv_b, reg_l2 = gl[3] * inv_b;
    const float mask_pen = gl[4] / (float)(B * F);
    const float g_loss = g_adv + d.lambda_cls * g_cls + d.lambda_l1 * reg_l1 + d.lambda_l2 * reg_l2 + d.lambda_mask * mask_pen;
    // d x_cf, classifier path: dlogits = lambda_cls (softmax - onehot) / B (into cl in place), back to dxc [B][2]
    for (int b = tid; b < B; b += NT) {
      float* lg = cl + b * NC;
      const float mx = fmaxf(fmaxf(lg[0], lg[1]), lg[2]);
      const float e0 = expf(lg[0] - mx), e1 = expf(lg[1] - mx), e2 = expf(lg[2] - mx);
      const float se = e0 + e1 + e2;
      const int t = (int)tgt[b];
      const float sc = d.lambda_cls * inv_b;
      lg[0] = sc * (e0 / se - (t == 0 ? 1.f : 0.f));
      lg[1] = sc * (e1 / se - (t == 1 ? 1.f : 0.f));
      lg[2] = sc * (e2 / se - (t == 2 ? 1.f : 0.f));
    }
    __syncthreads();
    lin_dx(cl, NC, cP + co[4], CH, c1, 0.f, bP, CH, CH, B);
    __syncthreads();
    lin_dx(bP, CH, cP + co[2], CH, c0, 0.f, bQ, CH, CH, B);
    __syncthreads();
    lin_dx(bQ, CH, cP + co[0], F, nullptr, 0.f, dxc, F, F, B);
    __syncthreads();
    // d x_cf, critic path (G_adv = -mean D: -1/B per row), no weight gradients, to dxd [B][2]
    d_backward<H>(-inv_b, dinF, wbar, woff, boff, fA, bP, bQ, tmp, dG, false, dxd, F, B, d.slope, false);
    // d raw (the four loss terms), into raw's twin buffer bP [B][F]
    {
      const float s1 = d.lambda_l1 * inv_b, s2 = d.lambda_l2 * inv_b, sm_ = d.lambda_mask / (float)(B * F);
      for (int b = tid; b < B; b += NT) {
        const float* h = hin + b * GIN;
        float q[F], n2 = 0.f;
        for (int j = 0; j < F; ++j) { q[j] = raw[b * F + j] * h[F + NC + j]; n2 = fmaf(q[j], q[j], n2); }
        const float nrm = sqrtf(n2);
        for (int j = 0; j < F; ++j) {
          const float m = h[F + NC + j], r = raw[b * F + j];
          const float sg = q[j] > 0.f ? 1.f : (q[j] < 0.f ? -1.f : 0.f);
          float dm = dxd[b * F + j] + dxc[b * F + j] + s1 * sg;
          if (nrm > 0.f) dm += s2 * q[j] / nrm;             // torch: the norm's backward is 0 at a zero row (masked_fill)
          const float p = r * (1.f - m);
          const float sp = p > 0.f ? 1.f : (p < 0.f ? -1.f : 0.f);
          bP[b * F + j] = dm * m + sm_ * sp * (1.f - m);
        }
      }
    }
    __syncthreads();
    // generator backward: Linear 9, then (ReLU, BN, Linear) x 3
    {
      const float* dz = bP;
      int O = F;
#pragma unroll
      for (int l = 3; l >= 0; --l) {
        const int I = Dm::GI[l];
        const float* X = l > 0 ? ga[l - 1] : hin;
        lin_dw(dz, O, X, I, I, gG + go[4 * l], gG + go[4 * l + 1], B);   // (l = 3: go[12], go[13], the last Linear)
        if (l == 0) break;
        float* dy = dz == bP ? bQ : bP;                     // d (BN output) of layer l-1 after the ReLU
        lin_dx(dz, O, gP + go[4 * l], I, ga[l - 1], 0.f, dy, I, I, B);
        __syncthreads();
        // BN l-1 backward: dz = gamma invstd / B (B dy - sum dy - xhat sum dy xhat); dgamma, dbeta
        const int bl = l - 1, C = Dm::GO[bl];
        float* s_dy = tmp;                                  // D's dW-bar staging is free in the generator step
        float* s_dyx = tmp + 64;
        col_sums(3, dy, gz[bl], nullptr, C, C, B, red, s_dy, s_dyx);
        if (tid < C) { gG[go[4 * bl + 2] + tid] = s_dyx[tid]; gG[go[4 * bl + 3] + tid] = s_dy[tid]; }
        const float* gamma = gP + go[4 * bl + 2];
        const float* is = sm + S.bninv + bl * H;
        for (int idx = tid; idx < B * C; idx += NT) {
          const int c = idx % C;
          dy[idx] = gamma[c] * is[c] * inv_b * ((float)B * dy[idx] - s_dy[c] - gz[bl][idx] * s_dyx[c]);
        }
        __syncthreads();
        dz = dy; O = C;
      }
      __syncthreads();
    }
    {
      float ss, bc2;
      adam_corr(d.lr_G, d.beta1, d.beta2, g_step0 + it + 1, pow_t, ss, bc2);
#pragma unroll
      for (int s = 0; s < Dm::SG; ++s) {
        const int i = tid + s * NT;
        if (i < d.nG_adam) { float p = gP[i]; adam_upd(p, gG[i], mG[s], vG[s], ak, ss, bc2); gP[i] = p; }
      }
    }
    if (tid == 0) {
      float* lg = a.logs + (size_t)it * NLOG;
      lg[0] = d_loss; lg[1] = g_loss; lg[2] = lr[2] * inv_b; lg[3] = lr[3] * inv_b;
      lg[4] = g_adv; lg[5] = g_cls; lg[6] = reg_l1; lg[7] = reg_l2; lg[8] = mask_pen;
    }
    __syncthreads();
  }

  // ---- state out -------------------------------------------------------------------------------------------------------------
  for (int i = tid; i < d.nG; i += NT) a.g_flat[i] = gP[i];
  for (int i = tid; i < d.nD; i += NT) a.d_flat[i] = dP[i];
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    for (int k = tid; k < Dm::DO[l]; k += NT) a.sn_u[l][k] = su[2][l * H + k];
    for (int k = tid; k < Dm::DI[l]; k += NT) a.sn_v[l][k] = sv[2][l * H + k];
  }
#pragma unroll
  for (int l = 0; l < 3; ++l)
    for (int k = tid; k < Dm::GO[l]; k += NT) { a.bn_mean[l][k] = sm[S.bnrm + l * H + k]; a.bn_var[l][k] = sm[S.bnrv + l * H + k]; }
#pragma unroll
  for (int s = 0; s < Dm::SG; ++s) {
    const int i = tid + s * NT;
    if (i < d.nG_adam) { a.g_exp_avg[i] = mG[s]; a.g_exp_avg_sq[i] = vG[s]; }
  }
#pragma unroll
  for (int s = 0; s < Dm::SD; ++s) {
    const int i = tid + s * NT;
    if (i < d.nD_adam) { a.d_exp_avg[i] = mD[s]; a.d_exp_avg_sq[i] = vD[s]; }
  }
  if (tid == 0) {
    a.g_step[0] = g_step0 + n_steps;
    a.d_step[0] = d_step0 + n_steps;
#pragma unroll
    for (int l = 0; l < 3; ++l) a.bn_nbt[l][0] += n_steps;
  }
}

// ---- forwards (one workgroup; parameters and activations in global memory) ------------------------------------------------
template <int H>
__global__ void __launch_bounds__(NT) moons_cf_forward_kernel(const pcg_moons_cf_desc d, const pcg_moons_cf_fwd_args a) {
  using Dm = Dims<H>;
  __shared__ float red[2 * NT];
  __shared__ float bn[4 * 3 * H];
  __shared__ float snu[8 * H], snv[8 * H], sig[4];
  __shared__ int offs[28];                  // the descriptor's g_off / c_off (a runtime index into a kernel argument is scratch)
  const int B = a.B, tid = threadIdx.x;
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 14; ++k) offs[k] = d.g_off[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) offs[14 + k] = d.c_off[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) offs[20 + k] = d.d_off[k];
  }
  __syncthreads();
  float* act = a.scratch;
  if (a.which == 0) {
    // hin, then gz/ga of three layers
    float* hin = act;
    float* gz[3];
    float* ga[3];
    int o = r4(GIN * B);
#pragma unroll
    for (int l = 0; l < 3; ++l) { gz[l] = act + o; o += r4(Dm::GO[l] * B); ga[l] = act + o; o += r4(Dm::GO[l] * B); }
    for (int b = tid; b < B; b += NT) {
      float* h = hin + b * GIN;
      for (int j = 0; j < F; ++j) { h[j] = a.x[b * F + j]; h[F + NC + j] = a.mask[b * F + j]; }
      for (int c = 0; c < NC; ++c) h[F + c] = a.onehot[b * NC + c];
    }
    float* rm = bn;
    float* rv = bn + 3 * H;
#pragma unroll
    for (int l = 0; l < 3; ++l)
      for (int k = tid; k < Dm::GO[l]; k += NT) { rm[l * H + k] = a.bn_mean[l][k]; rv[l * H + k] = a.bn_var[l][k]; }
    __syncthreads();
    g_forward<H>(hin, a.params, offs, gz, ga, a.out0, B, a.train != 0, rm, rv, bn + 6 * H, bn + 9 * H, d.bn_eps, d.bn_momentum, red);
    for (int i = tid; i < B * F; i += NT) a.out1[i] = a.out0[i] * a.mask[i];
    if (a.train) {
#pragma unroll
      for (int l = 0; l < 3; ++l)
        for (int k = tid; k < Dm::GO[l]; k += NT) { a.bn_mean[l][k] = rm[l * H + k]; a.bn_var[l][k] = rv[l * H + k]; }
      if (tid == 0) { a.bn_nbt[0][0] += 1; a.bn_nbt[1][0] += 1; a.bn_nbt[2][0] += 1; }
    }
  } else if (a.which == 1) {
    float* din = act;
    float* wbar = act + r4(DIN * B);
    float* A[3];
    int o = r4(DIN * B) + r4(d.nD);
#pragma unroll
    for (int l = 0; l < 3; ++l) { A[l] = act + o; o += r4(Dm::DO[l] * B); }
    for (int b = tid; b < B; b += NT) {
      for (int j = 0; j < F; ++j) din[b * DIN + j] = a.x[b * F + j];
      for (int c = 0; c < NC; ++c) din[b * DIN + F + c] = a.onehot[b * NC + c];
    }
    int* woff = offs + 20;
    int* boff = offs + 24;
    // stored u / v to LDS slot 0; a training-mode pass iterates into slot 1 and writes that back
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      for (int k = tid; k < Dm::DO[l]; k += NT) snu[l * H + k] = a.sn_u[l][k];
      for (int k = tid; k < Dm::DI[l]; k += NT) snv[l * H + k] = a.sn_v[l][k];
    }
    __syncthreads();
    const int so = a.train ? 4 * H : 0;
    sn_forward<H>(a.params, woff, snu, snv, snu + so, snv + so, sig, wbar, a.train != 0, d.sn_eps);
    d_forward<H>(din, wbar, a.params, woff, boff, A, a.out0, B, d.slope);
    if (a.train) {
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        for (int k = tid; k < Dm::DO[l]; k += NT) a.sn_u[l][k] = snu[4 * H + l * H + k];
        for (int k = tid; k < Dm::DI[l]; k += NT) a.sn_v[l][k] = snv[4 * H + l * H + k];
      }
    }
  } else {
    c_forward(a.x, F, a.params, offs + 14, act, act + r4(CH * B), a.out0, B);
  }
}

size_t fixed_bytes(const pcg_moons_cf_desc& d) { return sizeof(float) * (size_t)smem_layout(d.hidden, d.nG, d.nD).total; }

size_t act_bytes(const pcg_moons_cf_desc& d) { return sizeof(float) * (size_t)act_layout(d.hidden, d.B).total; }

size_t fwd_bytes(const pcg_moons_cf_desc& d, int B) {
  const int H = d.hidden;
  const size_t g = r4(GIN * B) + 2 * (size_t)(r4(H * B) * 2 + r4((H / 2) * B));
  const size_t dd = r4(DIN * B) + r4(d.nD) + r4(H * B) + 2 * (size_t)r4((H / 2) * B);
  const size_t c = 2 * (size_t)r4(CH * B);
  size_t m = g > dd ? g : dd;
  m = m > c ? m : c;
  return sizeof(float) * m;
}

int check_desc(const pcg_moons_cf_desc* d) {
  PCG_REQUIRE(d, "pcg_moons_cf: null descriptor");
  PCG_REQUIRE(d->hidden == 32 || d->hidden == 64, "pcg_moons_cf: hidden_dim %d (built for 32 and 64)", d->hidden);
  PCG_REQUIRE(d->clf_hidden == CH, "pcg_moons_cf: classifier hidden width %d (built for %d)", d->clf_hidden, CH);
  PCG_REQUIRE(d->B >= 2 && d->B <= 512, "pcg_moons_cf: batch %d outside [2, 512]", d->B);
  const bool h32 = d->hidden == 32;
  PCG_REQUIRE(d->nG > 0 && d->nG <= (h32 ? Dims<32>::gmax() : Dims<64>::gmax()) && d->nD > 0 &&
                  d->nD <= (h32 ? Dims<32>::dmax() : Dims<64>::dmax()) && d->nG_adam <= d->nG && d->nD_adam <= d->nD && d->nC > 0,
              "pcg_moons_cf: flat sizes G %d D %d C %d do not fit hidden %d", d->nG, d->nD, d->nC, d->hidden);
  return PCG_OK;
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_moons_cf_scratch_bytes(const pcg_moons_cf_desc* desc, int32_t forward) {
  if (check_desc(desc) != PCG_OK) return 0;
  if (forward) return fwd_bytes(*desc, desc->B);
  return acts_fit_lds(fixed_bytes(*desc), act_bytes(*desc)) ? 0 : act_bytes(*desc);
}

extern "C" int pcg_moons_cf_train_steps(const pcg_moons_cf_desc* desc, const pcg_moons_cf_train_args* args, int32_t n_steps,
                                        pcg_stream_t stream) {
  if (int rc = check_desc(desc)) return rc;
  PCG_REQUIRE(args && n_steps >= 1, "pcg_moons_cf_train_steps: bad arguments");
  const pcg_moons_cf_train_args& a = *args;
  PCG_REQUIRE(a.X && a.Y && a.rows && a.target_y && a.mask && a.g_flat && a.d_flat && a.c_flat && a.g_exp_avg && a.g_exp_avg_sq &&
                  a.g_step && a.d_exp_avg && a.d_exp_avg_sq && a.d_step && a.logs,
              "pcg_moons_cf_train_steps: null pointer");
  for (int l = 0; l < 3; ++l) PCG_REQUIRE(a.bn_mean[l] && a.bn_var[l] && a.bn_nbt[l], "pcg_moons_cf_train_steps: null BatchNorm buffer");
  for (int l = 0; l < 4; ++l) PCG_REQUIRE(a.sn_u[l] && a.sn_v[l], "pcg_moons_cf_train_steps: null spectral-norm vector");
  bool in_lds;
  size_t lds;
  if (int rc = place_acts("pcg_moons_cf_train_steps", fixed_bytes(*desc), act_bytes(*desc), a.scratch, a.scratch_bytes, sizeof(float), in_lds, lds))
    return rc;
  return launch_one_wg(desc->hidden == 32 ? moons_cf_train_kernel<32> : moons_cf_train_kernel<64>, "moons_cf_train_kernel", NT, lds,
                       (hipStream_t)stream, *desc, a, (int)n_steps, (int)in_lds);
}

extern "C" int pcg_moons_cf_forward(const pcg_moons_cf_desc* desc, const pcg_moons_cf_fwd_args* args, pcg_stream_t stream) {
  if (int rc = check_desc(desc)) return rc;
  PCG_REQUIRE(args && args->which >= 0 && args->which <= 2 && args->B >= 2 && args->B <= 512 && args->x && args->params && args->out0,
              "pcg_moons_cf_forward: bad arguments");
  const pcg_moons_cf_fwd_args& a = *args;
  if (a.which == 0) {
    PCG_REQUIRE(a.onehot && a.mask && a.out1, "pcg_moons_cf_forward: the generator needs onehot, mask and out1");
    for (int l = 0; l < 3; ++l) PCG_REQUIRE(a.bn_mean[l] && a.bn_var[l] && (!a.train || a.bn_nbt[l]), "pcg_moons_cf_forward: null BatchNorm buffer");
  }
  if (a.which == 1) {
    PCG_REQUIRE(a.onehot, "pcg_moons_cf_forward: the critic needs onehot");
    for (int l = 0; l < 4; ++l) PCG_REQUIRE(a.sn_u[l] && a.sn_v[l], "pcg_moons_cf_forward: null spectral-norm vector");
  }
  PCG_REQUIRE(a.scratch && a.scratch_bytes >= fwd_bytes(*desc, a.B), "pcg_moons_cf_forward: scratch %zu bytes < %zu needed", a.scratch_bytes,
              fwd_bytes(*desc, a.B));
  hipStream_t s = (hipStream_t)stream;
  if (desc->hidden == 32) hipLaunchKernelGGL(moons_cf_forward_kernel<32>, dim3(1), dim3(NT), 0, s, *desc, a);
  else hipLaunchKernelGGL(moons_cf_forward_kernel<64>, dim3(1), dim3(NT), 0, s, *desc, a);
  return launch_status("moons_cf_forward_kernel");
}
