// moons_gan.hip — the moons GAN (simple_gan/moons/make_moons_gan.py) and the one-hot conditional GAN
// (conditional_gan/moons/make_moons_cgan.py) as whole training iterations in ONE launch of ONE workgroup.
//
// Both scripts train two 2-layer MLPs, G: Linear(Z+L -> H) ReLU Linear(H -> 2) and D: Linear(2+L -> H) ReLU Linear(H -> 1) Sigmoid,
// L = label_dim (0: the simple GAN).  An iteration is a few hundred kFLOP: launch latency is all there is, so one workgroup of 512
// threads runs n_steps iterations back to back, six barrier-separated phases each:
//   1  rows     16 lanes own a batch row (two in the G passes, so that one LDS read of a weight serves both): G(z_d) -> fake, D(real), D(fake) (hidden stored), logits, the row's loss_D term and
//               d loss / d logit — the whole forward chain of a row stays inside its lane group (shuffles, no barrier)
//   2  columns  thread (j, p) sums its row partition's share of dV1[j][:], dc1[j], dV2[j] (and dc2)
//   3  params   thread i adds the partitions of D's parameter i in order and applies Adam; the last wave adds up loss_D
//   4  rows     G(z_g) -> fake, D(fake) with the updated D (hidden recomputed, not stored), the row's loss_G term, d fake, and
//               d hidden of G; G's hidden and its gradient are stored
//   5  columns  dW1 as 1 x 4 register tiles over all rows, db1 / dW2 / db2
//   6  params   Adam on G, the last wave adds up loss_G, and the inputs of the next iteration are staged
// Layout: parameters and gradients in LDS (W1 transposed, [in][H], so that the 16 lanes of a row read consecutive words), the Adam
// moments in registers (element i in thread i % 512, slot i / 512), activations in LDS when they fit (50 x 128 does), else in a
// global scratch buffer the caller allocates (generic pointers: one code path).  fp32 on the vector ALU, every sum in a fixed order
// (lane butterflies, rows in order, partitions in order): n steps in one launch are bit-identical to n launches of one step.
// The losses are taken from the logit a of D: -log D = softplus(-a), -log(1 - D) = softplus(a), finite where the reference's
// log(sigmoid(a)) gives inf.
#include "epoch_wg.h"

namespace pcg {
namespace {

constexpr int NT = 512, LPR = 16, GROUPS = NT / LPR;      // 8 waves (256 registers each); 16 lanes per batch row, 32 rows per pass
constexpr int RT = 2;                                      // batch rows per lane group in the G passes: one weight read, two rows
constexpr int MAXB = 256, MAXZ = 64, MAXL = 2, NQ = 6;    // NQ: per-j partial sums of phase 2 (dV1[j][0..3], dc1[j], dV2[j])
constexpr int FWD_NT = 256, FWD_ROWS = 64;                // forward: 16 lane groups, four passes per block

template <int H>
struct Dims {
  static constexpr int JL = H / LPR;                      // hidden units per lane, in runs of JV consecutive ones (unit<H>(l, k))
  // Run length 1 (unit = l + 16 k).  Measured at 50 x 128 with runs of 4 (one 16-byte LDS read per run): phase 1 8.0 -> 7.0 us
  // without labels, but 8.7 -> 11.5 us with them (D's first layer [H][4] is then read with a 16-word stride across the lanes).
  static constexpr int JV = 1;
  static constexpr int gmax = r4(H * (MAXZ + MAXL)) + r4(H) + r4(2 * H) + 4;
  static constexpr int dmax = r4(H * (2 + MAXL)) + r4(H) + r4(H) + 4;
  static constexpr int SG = (gmax + NT - 1) / NT, SD = (dmax + NT - 1) / NT;
};

__device__ __forceinline__ float group_sum(float v) {    // over the 16 lanes of a row; every lane receives the sum
  v += __shfl_xor(v, 8, LPR);
  v += __shfl_xor(v, 4, LPR);
  v += __shfl_xor(v, 2, LPR);
  v += __shfl_xor(v, 1, LPR);
  return v;
}

// Hidden unit k of lane l: runs of JV consecutive units, the lanes' runs side by side, JL / JV such blocks.
template <int H>
__device__ __forceinline__ int unit(int l, int k) {
  constexpr int JV = Dims<H>::JV;
  return JV * l + (LPR * JV) * (k / JV) + (k % JV);
}

// w[k] = v[unit(l, k)] for a vector v of H floats in LDS, 16-byte aligned: one read per run.
template <int H>
__device__ __forceinline__ void load_units(const float* v, int l, float (&w)[Dims<H>::JL]) {
  constexpr int JV = Dims<H>::JV, JL = Dims<H>::JL;
#pragma unroll
  for (int kk = 0; kk < JL / JV; ++kk) {
    const float* q = v + JV * l + (LPR * JV) * kk;
    if constexpr (JV == 1) {
      w[kk] = q[0];
    } else if constexpr (JV == 4) {
      const float4 t = *reinterpret_cast<const float4*>(q);
      w[4 * kk] = t.x; w[4 * kk + 1] = t.y; w[4 * kk + 2] = t.z; w[4 * kk + 3] = t.w;
    } else {
      const float2 t = *reinterpret_cast<const float2*>(q);
      w[2 * kk] = t.x; w[2 * kk + 1] = t.y;
    }
  }
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// beta^t by binary exponentiation in double: a function of t alone, so a launch of n steps and n launches of one step form the
// same corrections bit for bit, at a few dozen multiplications where pow() costs hundreds of fp64 instructions per call.  Within
// an ulp or two (of double) of pow(beta, t): far below the fp32 rounding of the two corrections it feeds.
__device__ __forceinline__ double ipow(double b, int64_t t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) {
    if (t & 1) r *= b;
    b *= b;
  }
  return r;
}

// Where flat element idx of G lives in LDS: W1 [H][GI] is kept transposed, [GI][H]; everything else at its flat offset.
__device__ __forceinline__ int g_pos(int idx, int oW1, int H, int GI) {
  const int r = idx - oW1;
  if (r < 0 || r >= H * GI) return idx;
  const int j = r / GI, i = r - j * GI;
  return oW1 + i * H + j;
}

// G's hidden pre-activations of R rows for this lane's units j = l + 16 k: every weight read from LDS serves R rows.
// zrow[r]: Z floats, 16-byte aligned; o0 / o1: the one-hot.
template <int H, int R>
__device__ __forceinline__ void g_hidden(const float* const (&zrow)[R], const float (&o0)[R], const float (&o1)[R], const float* W1T,
                                         const float* b1, int Z, int L, int l, float (&h)[R][Dims<H>::JL]) {
  constexpr int JL = Dims<H>::JL;
  float w0[JL], w1[JL], w2[JL], w3[JL];
  load_units<H>(b1, l, w0);
#pragma unroll
  for (int k = 0; k < JL; ++k) {
#pragma unroll
    for (int r = 0; r < R; ++r) h[r][k] = w0[k];
  }
  for (int i = 0; i < Z; i += 4) {
    float4 x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = *reinterpret_cast<const float4*>(zrow[r] + i);
    const float* w = W1T + i * H;
    load_units<H>(w, l, w0); load_units<H>(w + H, l, w1); load_units<H>(w + 2 * H, l, w2); load_units<H>(w + 3 * H, l, w3);
#pragma unroll
    for (int k = 0; k < JL; ++k) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        h[r][k] = fmaf(x[r].x, w0[k], h[r][k]);
        h[r][k] = fmaf(x[r].y, w1[k], h[r][k]);
        h[r][k] = fmaf(x[r].z, w2[k], h[r][k]);
        h[r][k] = fmaf(x[r].w, w3[k], h[r][k]);
      }
    }
  }
  if (L) {
    load_units<H>(W1T + Z * H, l, w0); load_units<H>(W1T + (Z + 1) * H, l, w1);
#pragma unroll
    for (int k = 0; k < JL; ++k) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        h[r][k] = fmaf(o0[r], w0[k], h[r][k]);
        h[r][k] = fmaf(o1[r], w1[k], h[r][k]);
      }
    }
  }
}

// ReLU and G's output layer: h becomes post-ReLU; (f0, f1) on every lane of the row.
template <int H>
__device__ __forceinline__ void g_out(float (&h)[Dims<H>::JL], const float* W2, const float* b2, int l, float& f0, float& f1) {
  float s0 = 0.f, s1 = 0.f, u0[Dims<H>::JL], u1[Dims<H>::JL];
  load_units<H>(W2, l, u0); load_units<H>(W2 + H, l, u1);
#pragma unroll
  for (int k = 0; k < Dims<H>::JL; ++k) {
    h[k] = fmaxf(h[k], 0.f);
    s0 = fmaf(h[k], u0[k], s0);
    s1 = fmaf(h[k], u1[k], s1);
  }
  f0 = group_sum(s0) + b2[0];
  f1 = group_sum(s1) + b2[1];
}

// D's hidden layer (post-ReLU) of one row for this lane's units, and the logit on every lane of the row.
template <int H>
__device__ __forceinline__ float d_row(float x0, float x1, float o0, float o1, const float* V1, const float* c1, const float* V2, float c2,
                                       int L, int l, float (&hd)[Dims<H>::JL]) {
  const int DI = 2 + L;
  float s = 0.f, cc[Dims<H>::JL], vv[Dims<H>::JL];
  load_units<H>(c1, l, cc); load_units<H>(V2, l, vv);
#pragma unroll
  for (int k = 0; k < Dims<H>::JL; ++k) {
    const float* v = V1 + unit<H>(l, k) * DI;
    float p = cc[k];
    p = fmaf(v[0], x0, p);
    p = fmaf(v[1], x1, p);
    if (L) { p = fmaf(v[2], o0, p); p = fmaf(v[3], o1, p); }
    hd[k] = fmaxf(p, 0.f);
    s = fmaf(hd[k], vv[k], s);
  }
  return group_sum(s) + c2;
}

// LDS of the train kernel, floats.  The `act` part follows when it fits.
struct SmemLayout { int gP, gG, dP, part, pc2, corr, dinR, dinF, dlr, dlf, lrow, dfk, total; };
__host__ __device__ inline SmemLayout smem_layout(int nG, int nD, int B) {
  SmemLayout S;
  int o = 0;
  auto take = [&](int n) { const int r = o; o += r4(n); return r; };
  S.gP = take(nG); S.gG = take(nG); S.dP = take(nD); S.part = take(NQ * NT); S.pc2 = take(NT / 32); S.corr = take(4);
  S.dinR = take(4 * B); S.dinF = take(4 * B); S.dlr = take(B); S.dlf = take(B); S.lrow = take(B); S.dfk = take(2 * B);
  S.total = o;
  return S;
}
struct ActLayout { int hA, hB, gd, gg, total; };
__host__ __device__ inline ActLayout act_layout(int H, int B, int GIS) {
  ActLayout A;
  A.hA = 0; A.hB = r4(B * H); A.gd = 2 * r4(B * H); A.gg = A.gd + B * GIS; A.total = A.gg + B * GIS;
  return A;
}

template <int H, bool ACT_LDS>
__global__ void __launch_bounds__(NT) moons_gan_train_kernel(const pcg_moons_gan_desc d, const pcg_moons_gan_train_args a, int n_steps) {
  using Dm = Dims<H>;
  constexpr int JL = Dm::JL, P = NT / H;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, l = tid & (LPR - 1), grp = tid / LPR;
  const int B = d.B, Z = d.z_dim, L = d.label_dim, GI = Z + L, DI = 2 + L, GIS = Z + (L ? 4 : 0);
  const SmemLayout S = smem_layout(d.nG, d.nD, B);
  const ActLayout A = act_layout(H, B, GIS);
  float* act = ACT_LDS ? sm + S.total : a.scratch;      // a template switch: LDS addressing stays 32-bit
  float *gP = sm + S.gP, *gG = sm + S.gG, *dP = sm + S.dP, *part = sm + S.part, *pc2 = sm + S.pc2, *corr = sm + S.corr;
  float *dinR = sm + S.dinR, *dinF = sm + S.dinF, *dlr = sm + S.dlr, *dlf = sm + S.dlf, *lrow = sm + S.lrow, *dfk = sm + S.dfk;
  float *hA = act + A.hA, *hB = act + A.hB, *gin_d = act + A.gd, *gin_g = act + A.gg;
  const int oW1 = d.g_off[0], ob1 = d.g_off[1], oW2 = d.g_off[2], ob2 = d.g_off[3];
  const int oV1 = d.d_off[0], oc1 = d.d_off[1], oV2 = d.d_off[2], oc2 = d.d_off[3];
  const float *W1T = gP + oW1, *b1 = gP + ob1, *W2 = gP + oW2, *b2 = gP + ob2;
  const float *V1 = dP + oV1, *c1 = dP + oc1, *V2 = dP + oV2;
  const float inv_b = 1.f / (float)B;

  // ---- state in: parameters to LDS, moments to registers ----------------------------------------------------------------------
  float mG[Dm::SG], vG[Dm::SG];
#pragma unroll
  for (int s = 0; s < Dm::SG; ++s) {
    const int i = tid + s * NT;
    if (i < d.nG) { gP[g_pos(i, oW1, H, GI)] = a.g_flat[i]; gG[i] = 0.f; }
    mG[s] = i < d.nG_adam ? a.g_exp_avg[i] : 0.f;
    vG[s] = i < d.nG_adam ? a.g_exp_avg_sq[i] : 0.f;
  }
  // which sum of phase 2 is the gradient of D's flat element i: q < NQ at hidden unit j; q == NQ: c2; -1: padding
  float mD[Dm::SD], vD[Dm::SD];
  int qD[Dm::SD], jD[Dm::SD];
#pragma unroll
  for (int s = 0; s < Dm::SD; ++s) {
    const int i = tid + s * NT;
    if (i < d.nD) dP[i] = a.d_flat[i];
    mD[s] = i < d.nD_adam ? a.d_exp_avg[i] : 0.f;
    vD[s] = i < d.nD_adam ? a.d_exp_avg_sq[i] : 0.f;
    qD[s] = -1; jD[s] = 0;
    int r = i - oV1;
    if (r >= 0 && r < H * DI) { jD[s] = r / DI; qD[s] = r - jD[s] * DI; }
    r = i - oc1;
    if (r >= 0 && r < H) { jD[s] = r; qD[s] = 4; }
    r = i - oV2;
    if (r >= 0 && r < H) { jD[s] = r; qD[s] = 5; }
    if (i == oc2) qD[s] = NQ;
  }
  const int64_t g_step0 = a.g_step[0], d_step0 = a.d_step[0];
  // adam_k(d), spelled out as it was: through the function the compiler reuses 1 - beta1 for 1 - (1 - beta1) (the same value, one
  // fp64 add fewer), which moves the code of the six train kernels and their time with it (measured: -1.4 %); not in a refactor
  const AdamK ak{(float)(1.0 - d.beta1), (float)(1.0 - (1.0 - d.beta1)), (float)d.beta2, (float)(1.0 - d.beta2), (float)d.adam_eps};

  // inputs of iteration `it`: both noise draws with their one-hot labels ([B][GIS], zero padded), the real rows with theirs
  auto stage = [&](int it) {
    const float* zd = a.z + (size_t)(2 * it) * B * Z;
    const float* zg = zd + (size_t)B * Z;
    const int64_t* ld = L ? a.labels + (size_t)(2 * it) * B : nullptr;
    for (int idx = tid; idx < B * GIS; idx += NT) {
      const int b = idx / GIS, i = idx - b * GIS;
      float vd, vg;
      if (i < Z) { vd = zd[b * Z + i]; vg = zg[b * Z + i]; }
      else { vd = (ld[b] == (int64_t)(i - Z)) ? 1.f : 0.f; vg = (ld[B + b] == (int64_t)(i - Z)) ? 1.f : 0.f; }
      gin_d[idx] = vd; gin_g[idx] = vg;
    }
    for (int b = tid; b < B; b += NT) {
      int64_t r = a.rows[(size_t)it * B + b];
      r = r < 0 ? 0 : (r >= d.N ? d.N - 1 : r);               // the caller checks the range; never read outside X
      const int64_t y = L ? a.Y[r] : -1;
      dinR[4 * b] = a.X[2 * r]; dinR[4 * b + 1] = a.X[2 * r + 1];
      dinR[4 * b + 2] = y == 0 ? 1.f : 0.f; dinR[4 * b + 3] = y == 1 ? 1.f : 0.f;
    }
  };
  stage(0);
  __syncthreads();

  for (int it = 0; it < n_steps; ++it) {
    PCG_T(0);                                             // (phase stamps: compiled out of the library, pcg_common.h)
    // ---- 1. rows: G(z_d), D(real), D(fake), loss_D terms (make_moons_gan.py:63-70, make_moons_cgan.py:94-107) ----------------
    for (int b0 = 0; b0 < B; b0 += GROUPS) {              // D(real)
      const bool valid = b0 + grp < B;
      const int b = valid ? b0 + grp : B - 1;
      const float4 xr = *reinterpret_cast<const float4*>(dinR + 4 * b);
      float hr[JL];
      const float ar = d_row<H>(xr.x, xr.y, xr.z, xr.w, V1, c1, V2, dP[oc2], L, l, hr);
      if (valid) {
#pragma unroll
        for (int k = 0; k < JL; ++k) hA[b * H + unit<H>(l, k)] = hr[k];
        if (l == 0) {
          lrow[b] = softplus(-ar);
          dlr[b] = -inv_b / (1.f + expf(ar));                 // d/da softplus(-a) = sigmoid(a) - 1
        }
      }
    }
    for (int b0 = 0; b0 < B; b0 += RT * GROUPS) {         // G(z_d), D(fake); the same lane wrote lrow[b] above
      const float* gr[RT];
      float o0[RT], o1[RT], h[RT][JL];
      int bb[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const int b = b0 + r * GROUPS + grp;
        bb[r] = b < B ? b : -1;
        gr[r] = gin_d + (b < B ? b : B - 1) * GIS;
        o0[r] = L ? gr[r][Z] : 0.f; o1[r] = L ? gr[r][Z + 1] : 0.f;
      }
      g_hidden<H, RT>(gr, o0, o1, W1T, b1, Z, L, l, h);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        float f0, f1;
        g_out<H>(h[r], W2, b2, l, f0, f1);
        const float af = d_row<H>(f0, f1, o0[r], o1[r], V1, c1, V2, dP[oc2], L, l, h[r]);
        const int b = bb[r];
        if (b >= 0) {
#pragma unroll
          for (int k = 0; k < JL; ++k) hB[b * H + unit<H>(l, k)] = h[r][k];
          if (l == 0) {
            *reinterpret_cast<float4*>(dinF + 4 * b) = make_float4(f0, f1, o0[r], o1[r]);
            lrow[b] += softplus(af);
            dlf[b] = inv_b / (1.f + expf(-af));               // d/da softplus(a)  = sigmoid(a)
          }
        }
      }
    }
    __syncthreads();
    PCG_T(1);
    // ---- 2. columns: D's gradients, one partial per row partition (:73 / :110) ---------------------------------------------
    {
      const int j = tid % H, p = tid / H;
      float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f, sc1 = 0.f, sv2 = 0.f, sc2 = 0.f;
      for (int b = p; b < B; b += P) {
        const float er = dlr[b], ef = dlf[b], yr = hA[b * H + j], yf = hB[b * H + j];
        const float4 xr = *reinterpret_cast<const float4*>(dinR + 4 * b);
        const float4 xf = *reinterpret_cast<const float4*>(dinF + 4 * b);
        const float gr = yr > 0.f ? er : 0.f, gf = yf > 0.f ? ef : 0.f;
        sv2 = fmaf(er, yr, sv2); sv2 = fmaf(ef, yf, sv2);
        sc1 += gr; sc1 += gf;
        w0 = fmaf(gr, xr.x, w0); w0 = fmaf(gf, xf.x, w0);
        w1 = fmaf(gr, xr.y, w1); w1 = fmaf(gf, xf.y, w1);
        w2 = fmaf(gr, xr.z, w2); w2 = fmaf(gf, xf.z, w2);
        w3 = fmaf(gr, xr.w, w3); w3 = fmaf(gf, xf.w, w3);
        sc2 += er; sc2 += ef;
      }
      const float v2 = V2[j];
      float* q = part + (p * NQ) * H + j;
      q[0] = w0 * v2; q[H] = w1 * v2; q[2 * H] = w2 * v2; q[3 * H] = w3 * v2; q[4 * H] = sc1 * v2; q[5 * H] = sv2;
      if (j == 0) pc2[p] = sc2;
      if (tid == NT - 1) {                 // this iteration's Adam bias corrections, once (fp64), for phases 3 and 6
        adam_corr(d.lr_D, d.beta1, d.beta2, d_step0 + it + 1, ipow, corr[0], corr[1]);
        adam_corr(d.lr_G, d.beta1, d.beta2, g_step0 + it + 1, ipow, corr[2], corr[3]);
      }
    }
    __syncthreads();
    PCG_T(2);
    // ---- 3. params: partitions added in order, Adam on D (:74 / :111); loss_D ---------------------------------------------------
    float loss_D = 0.f;
    {
      const float ss = corr[0], bc2 = corr[1];
#pragma unroll
      for (int s = 0; s < Dm::SD; ++s) {
        const int i = tid + s * NT;
        if (i < d.nD_adam && qD[s] >= 0) {
          float g = 0.f;
          if (qD[s] < NQ) for (int p = 0; p < P; ++p) g += part[(p * NQ + qD[s]) * H + jD[s]];
          else for (int p = 0; p < P; ++p) g += pc2[p];
          float pv = dP[i];
          adam_upd(pv, g, mD[s], vD[s], ak, ss, bc2);
          dP[i] = pv;
        }
      }
      if (tid >= NT - 64) {
        float s = 0.f;
        for (int b = tid & 63; b < B; b += 64) s += lrow[b];
        loss_D = wave_sum(s) * inv_b;
      }
    }
    __syncthreads();
    PCG_T(3);
    // ---- 4. rows: G(z_g), D(fake) with the updated D, loss_G terms, backward to G's hidden (:78-86 / :116-126) ---------------
    for (int b0 = 0; b0 < B; b0 += RT * GROUPS) {
      const float* gr[RT];
      float o0[RT], o1[RT], h[RT][JL];
      int bb[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        const int b = b0 + r * GROUPS + grp;
        bb[r] = b < B ? b : -1;
        gr[r] = gin_g + (b < B ? b : B - 1) * GIS;
        o0[r] = L ? gr[r][Z] : 0.f; o1[r] = L ? gr[r][Z + 1] : 0.f;
      }
      g_hidden<H, RT>(gr, o0, o1, W1T, b1, Z, L, l, h);
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        float hd[JL], f0, f1;
        g_out<H>(h[r], W2, b2, l, f0, f1);
        const float af = d_row<H>(f0, f1, o0[r], o1[r], V1, c1, V2, dP[oc2], L, l, hd);
        const float e = -inv_b / (1.f + expf(af));           // d loss_G / d logit
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < JL; ++k) {
          const int j = unit<H>(l, k);
          const float g = hd[k] > 0.f ? V2[j] : 0.f;
          s0 = fmaf(g, V1[j * DI], s0);
          s1 = fmaf(g, V1[j * DI + 1], s1);
        }
        const float dx0 = group_sum(s0) * e, dx1 = group_sum(s1) * e;
        const int b = bb[r];
        if (b >= 0) {
#pragma unroll
          for (int k = 0; k < JL; ++k) {
            const int j = unit<H>(l, k);
            hA[b * H + j] = h[r][k];
            hB[b * H + j] = h[r][k] > 0.f ? fmaf(dx1, W2[H + j], dx0 * W2[j]) : 0.f;
          }
          if (l == 0) { dfk[2 * b] = dx0; dfk[2 * b + 1] = dx1; lrow[b] = softplus(-af); }
        }
      }
    }
    __syncthreads();
    PCG_T(4);
    // ---- 5. columns: G's gradients (:86 / :126) -----------------------------------------------------------------------------------
    {
      const int nt1 = H * (GIS / 4);
      for (int t = tid; t < nt1 + H; t += NT) {
        if (t < nt1) {
          const int j = t % H, i4 = (t / H) * 4;
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
          for (int b = 0; b < B; ++b) {
            const float g = hB[b * H + j];
            const float4 x = *reinterpret_cast<const float4*>(gin_g + b * GIS + i4);
            acc.x = fmaf(g, x.x, acc.x); acc.y = fmaf(g, x.y, acc.y); acc.z = fmaf(g, x.z, acc.z); acc.w = fmaf(g, x.w, acc.w);
          }
          float* o = gG + oW1 + j * GI + i4;
          o[0] = acc.x; o[1] = acc.y;
          if (i4 + 2 < GI) { o[2] = acc.z; o[3] = acc.w; }   // (the last tile of a labelled G has two columns of padding)
        } else {
          const int j = t - nt1;
          float sb = 0.f, u0 = 0.f, u1 = 0.f, t0 = 0.f, t1 = 0.f;
          for (int b = 0; b < B; ++b) {
            const float y = hA[b * H + j], e0 = dfk[2 * b], e1 = dfk[2 * b + 1];
            sb += hB[b * H + j];
            u0 = fmaf(e0, y, u0); u1 = fmaf(e1, y, u1);
            t0 += e0; t1 += e1;
          }
          gG[ob1 + j] = sb; gG[oW2 + j] = u0; gG[oW2 + H + j] = u1;
          if (j == 0) { gG[ob2] = t0; gG[ob2 + 1] = t1; }
        }
      }
    }
    __syncthreads();
    PCG_T(5);
    // ---- 6. params: Adam on G (:87 / :127), loss_G, the next iteration's inputs ----------------------------------------------------
    {
      const float ss = corr[2], bc2 = corr[3];
#pragma unroll
      for (int s = 0; s < Dm::SG; ++s) {
        const int i = tid + s * NT;
        if (i < d.nG_adam) { const int q = g_pos(i, oW1, H, GI); float pv = gP[q]; adam_upd(pv, gG[i], mG[s], vG[s], ak, ss, bc2); gP[q] = pv; }
      }
      if (tid >= NT - 64) {
        float s = 0.f;
        for (int b = tid & 63; b < B; b += 64) s += lrow[b];
        const float loss_G = wave_sum(s) * inv_b;
        if (tid == NT - 64) { a.logs[2 * (size_t)it] = loss_D; a.logs[2 * (size_t)it + 1] = loss_G; }
      }
      if (it + 1 < n_steps) stage(it + 1);
    }
    __syncthreads();
    PCG_T(6);
  }

  // ---- state out -----------------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int s = 0; s < Dm::SG; ++s) {
    const int i = tid + s * NT;
    if (i < d.nG) a.g_flat[i] = gP[g_pos(i, oW1, H, GI)];
    if (i < d.nG_adam) { a.g_exp_avg[i] = mG[s]; a.g_exp_avg_sq[i] = vG[s]; }
  }
#pragma unroll
  for (int s = 0; s < Dm::SD; ++s) {
    const int i = tid + s * NT;
    if (i < d.nD) a.d_flat[i] = dP[i];
    if (i < d.nD_adam) { a.d_exp_avg[i] = mD[s]; a.d_exp_avg_sq[i] = vD[s]; }
  }
  if (tid == 0) { a.g_step[0] = g_step0 + n_steps; a.d_step[0] = d_step0 + n_steps; }
}

// ---- forward of one net over any number of rows: a grid over blocks of 64 rows, the parameters staged in LDS --------------------
template <int H>
__global__ void __launch_bounds__(FWD_NT) moons_gan_forward_kernel(const pcg_moons_gan_desc d, const pcg_moons_gan_fwd_args a) {
  constexpr int JL = Dims<H>::JL;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, l = tid & (LPR - 1), grp = tid / LPR;
  const int Z = d.z_dim, L = d.label_dim, GI = Z + L;
  const int64_t R = a.R;
  if (a.which == 0) {
    for (int i = tid; i < d.nG; i += FWD_NT) sm[g_pos(i, d.g_off[0], H, GI)] = a.params[i];
  } else {
    for (int i = tid; i < d.nD; i += FWD_NT) sm[i] = a.params[i];
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * FWD_ROWS;
  for (int b0 = 0; b0 < FWD_ROWS; b0 += FWD_NT / LPR) {
    const int64_t r = base + b0 + grp;
    const bool valid = r < R;
    const int64_t rr = valid ? r : R - 1;
    const float o0 = L ? a.onehot[rr * L] : 0.f, o1 = L ? a.onehot[rr * L + 1] : 0.f;
    if (a.which == 0) {
      float h[1][JL], f0, f1;
      const float* const zr[1] = {a.x + rr * Z};
      const float oa[1] = {o0}, ob[1] = {o1};
      g_hidden<H, 1>(zr, oa, ob, sm + d.g_off[0], sm + d.g_off[1], Z, L, l, h);
      g_out<H>(h[0], sm + d.g_off[2], sm + d.g_off[3], l, f0, f1);
      if (valid && l == 0) { a.out[2 * r] = f0; a.out[2 * r + 1] = f1; }
    } else {
      float hd[JL];
      const float af = d_row<H>(a.x[2 * rr], a.x[2 * rr + 1], o0, o1, sm + d.d_off[0], sm + d.d_off[1], sm + d.d_off[2], sm[d.d_off[3]], L, l, hd);
      if (valid && l == 0) a.out[r] = 1.f / (1.f + expf(-af));
    }
  }
}

int check_desc(const pcg_moons_gan_desc* d, bool train) {
  PCG_REQUIRE(d, "pcg_moons_gan: null descriptor");
  const int H = d->hidden, Z = d->z_dim, L = d->label_dim;
  PCG_REQUIRE(H == 32 || H == 64 || H == 128, "pcg_moons_gan: hidden_dim %d (built for 32, 64 and 128)", H);
  PCG_REQUIRE(Z >= 4 && Z <= MAXZ && Z % 4 == 0, "pcg_moons_gan: z_dim %d (a multiple of 4 in [4, %d])", Z, MAXZ);
  PCG_REQUIRE(L == 0 || L == 2, "pcg_moons_gan: label_dim %d (0: unconditional, or 2)", L);
  const int gsz[4] = {H * (Z + L), H, 2 * H, 2}, dsz[4] = {H * (2 + L), H, H, 1};
  int go = 0, dd = 0;
  for (int k = 0; k < 4; ++k) {         // tensors in flat order, not overlapping, inside the buffers
    PCG_REQUIRE(d->g_off[k] >= go && d->g_off[k] % 4 == 0 && d->d_off[k] >= dd && d->d_off[k] % 4 == 0,
                "pcg_moons_gan: parameter offset %d out of order or unaligned (G %d, D %d)", k, d->g_off[k], d->d_off[k]);
    go = d->g_off[k] + gsz[k];
    dd = d->d_off[k] + dsz[k];
  }
  const int gmax = H == 32 ? Dims<32>::gmax : H == 64 ? Dims<64>::gmax : Dims<128>::gmax;
  const int dmax = H == 32 ? Dims<32>::dmax : H == 64 ? Dims<64>::dmax : Dims<128>::dmax;
  PCG_REQUIRE(go <= d->nG && d->nG <= gmax && dd <= d->nD && d->nD <= dmax, "pcg_moons_gan: flat sizes G %d D %d do not fit hidden %d, z_dim %d, label_dim %d",
              d->nG, d->nD, H, Z, L);
  if (train) {
    PCG_REQUIRE(d->B >= 1 && d->B <= MAXB, "pcg_moons_gan: batch %d outside [1, %d]", d->B, MAXB);
    PCG_REQUIRE(d->N >= 1, "pcg_moons_gan: %d training rows", d->N);
    PCG_REQUIRE(d->nG_adam >= 0 && d->nG_adam <= d->nG && d->nD_adam >= 0 && d->nD_adam <= d->nD, "pcg_moons_gan: Adam spans %d / %d exceed the flat sizes",
                d->nG_adam, d->nD_adam);
  }
  return PCG_OK;
}

size_t fixed_bytes(const pcg_moons_gan_desc& d) { return sizeof(float) * (size_t)smem_layout(d.nG, d.nD, d.B).total; }
size_t act_bytes(const pcg_moons_gan_desc& d) {
  return sizeof(float) * (size_t)act_layout(d.hidden, d.B, d.z_dim + (d.label_dim ? 4 : 0)).total;
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_moons_gan_scratch_bytes(const pcg_moons_gan_desc* desc) {
  if (check_desc(desc, true) != PCG_OK) return 0;
  return acts_fit_lds(fixed_bytes(*desc), act_bytes(*desc)) ? 0 : act_bytes(*desc);
}

extern "C" int pcg_moons_gan_train_steps(const pcg_moons_gan_desc* desc, const pcg_moons_gan_train_args* args, int32_t n_steps,
                                         pcg_stream_t stream) {
  if (int rc = check_desc(desc, true)) return rc;
  PCG_REQUIRE(args && n_steps >= 1, "pcg_moons_gan_train_steps: bad arguments");
  const pcg_moons_gan_train_args& a = *args;
  PCG_REQUIRE(a.X && a.rows && a.z && a.g_flat && a.d_flat && a.g_exp_avg && a.g_exp_avg_sq && a.g_step && a.d_exp_avg && a.d_exp_avg_sq &&
                  a.d_step && a.logs, "pcg_moons_gan_train_steps: null pointer");
  PCG_REQUIRE(desc->label_dim == 0 || (a.Y && a.labels), "pcg_moons_gan_train_steps: label_dim %d needs Y and labels", desc->label_dim);
  bool in_lds;
  size_t lds;
  if (int rc = place_acts("pcg_moons_gan_train_steps", fixed_bytes(*desc), act_bytes(*desc), a.scratch, a.scratch_bytes, 16, in_lds, lds))
    return rc;
  const int H = desc->hidden;
  auto launch = [&](auto kernel) {
    return launch_one_wg(kernel, "moons_gan_train_kernel", NT, lds, (hipStream_t)stream, *desc, a, (int)n_steps);
  };
  if (in_lds) return H == 32 ? launch(moons_gan_train_kernel<32, true>) : H == 64 ? launch(moons_gan_train_kernel<64, true>) : launch(moons_gan_train_kernel<128, true>);
  return H == 32 ? launch(moons_gan_train_kernel<32, false>) : H == 64 ? launch(moons_gan_train_kernel<64, false>) : launch(moons_gan_train_kernel<128, false>);
}

extern "C" int pcg_moons_gan_forward(const pcg_moons_gan_desc* desc, const pcg_moons_gan_fwd_args* args, pcg_stream_t stream) {
  if (int rc = check_desc(desc, false)) return rc;
  PCG_REQUIRE(args && (args->which == 0 || args->which == 1) && args->R >= 1 && args->R <= (int64_t)1 << 30 && args->x && args->params && args->out,
              "pcg_moons_gan_forward: bad arguments");
  PCG_REQUIRE(desc->label_dim == 0 || args->onehot, "pcg_moons_gan_forward: label_dim %d needs onehot", desc->label_dim);
  PCG_REQUIRE(args->which == 1 || ((uintptr_t)args->x & 15) == 0, "pcg_moons_gan_forward: z must be 16-byte aligned");
  const size_t lds = sizeof(float) * (size_t)(args->which == 0 ? desc->nG : desc->nD);
  const unsigned blocks = (unsigned)((args->R + FWD_ROWS - 1) / FWD_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const int H = desc->hidden;
  if (H == 32) hipLaunchKernelGGL(moons_gan_forward_kernel<32>, dim3(blocks), dim3(FWD_NT), lds, s, *desc, *args);
  else if (H == 64) hipLaunchKernelGGL(moons_gan_forward_kernel<64>, dim3(blocks), dim3(FWD_NT), lds, s, *desc, *args);
  else hipLaunchKernelGGL(moons_gan_forward_kernel<128>, dim3(blocks), dim3(FWD_NT), lds, s, *desc, *args);
  return launch_status("moons_gan_forward_kernel");
}
