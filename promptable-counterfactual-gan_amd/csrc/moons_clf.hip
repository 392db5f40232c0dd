// moons_clf.hip — the moons CounteRGAN's classifier fit (conditional_counteRGAN/moons/trainer.py:22-25: full-batch Adam steps of
// cross-entropy on Linear(2,32)-ReLU-Linear(32,32)-ReLU-Linear(32,3)) as whole iterations in ONE launch of ONE workgroup
// (DESIGN.md §3.15).
//
// An iteration is about 3.4 M fused multiply-adds over N rows (the reference: 960) and 1251 parameters; as an op chain it is a
// dozen launches.  One workgroup of 512 threads runs n_steps iterations back to back.  The rows are walked in chunks of 512 whose
// activations live in two LDS buffers; per chunk two thread mappings alternate, six barriers:
//   A1 rows     thread = row: forward, the row's loss term, d logits, backward through both ReLUs down to d z1 — every weight is
//               a broadcast read from LDS.  h2 and d z2 go to the two chunk buffers unit by unit, as the loops over the 32 units
//               of the second layer produce them; h1 and d z1 stay in the thread's registers
//   C1 columns  thread = one element of dW3 / db3 / db2 and one half of the chunk's rows; the last wave adds up the loss terms
//   A2 rows     h1 from the registers over h2
//   B2 columns  wave w = rows 64 w .. 64 w + 63 of the chunk, lane = a 4 x 4 tile of dW2
//   A3 rows     d z1 from the registers over d z2
//   C3 columns  thread = one element of dW1 / db1 and one half of the chunk's rows
// The column threads keep their sums in registers from chunk to chunk.  After the last chunk they go to LDS (into the first chunk
// buffer, free by then), a thread per parameter adds the partitions in order and applies Adam (moments in registers, element i
// in thread i % 512), and the next iteration starts.  Layout: parameters in LDS at their flat offsets; the chunk buffers are
// unit-major, [32][RS] with RS = 516 (a row phase stores one dword per lane to consecutive addresses; a column phase reads four
// rows of a unit as one 16-byte word, and RS % 16 == 4 puts the four units of a tile 16 banks apart).  fp32 on the vector ALU,
// every sum in an order fixed by N alone (rows in order within a partition, partitions in order, lane butterflies): n steps in
// one launch are bit-identical to any split into several launches.
//
// The loops over the second layer's units are real loops (two units per trip), not unrolled: unrolled, the compiler starts all 256
// weight reads of a 32 x 32 product at the top of the block and spills them (1035 VGPRs, 3.9 KB of scratch per thread).
#include "epoch_wg.h"

namespace pcg {
namespace {

constexpr int NT = 512, WAVES = NT / 64;                  // 8 waves, two per SIMD: 256 registers each
constexpr int H = 32, NCLS = 3, IN = 2;
constexpr int CH = NT, RS = CH + 4;                       // rows per chunk (one per thread); row stride of the unit-major buffers
constexpr int MAXN = 4096, MAXC = 2048;                   // rows; floats of the flat parameter buffer
constexpr int SLOTS = (MAXC + NT - 1) / NT;               // Adam moments per thread
constexpr int PC = 2, OC = NT / PC;                       // C1 / C3: row partitions, output slots per partition
// C1's output slots: dW3 [3][32], db3 [3], db2 [32]; C3's: dW1 [32][2], db1 [32]
constexpr int O_W3 = 0, O_B3 = O_W3 + NCLS * H, O_B2 = 128, O1_END = O_B2 + H;
constexpr int O_W1 = 0, O_B1 = O_W1 + H * IN, O3_END = O_B1 + H;
// where the partitions' sums lie (floats, from the start of the first chunk buffer) when Adam reads them
constexpr int PART_W2 = 0, PART_C1 = PART_W2 + WAVES * H * H, PART_C3 = PART_C1 + PC * OC, PART_END = PART_C3 + PC * OC;
static_assert(O_B3 + NCLS <= O_B2 && O1_END <= OC && O3_END <= OC && PART_END <= H * RS, "partition sums must fit the first chunk buffer");

// LDS, floats
struct Smem { int P, buf0, buf1, dl, x, lrow, corr, cnt, total; };
__host__ __device__ constexpr Smem smem_layout() {
  Smem S{};
  int o = 0;
  S.P = o; o += r4(MAXC);
  S.buf0 = o; o += r4(H * RS);
  S.buf1 = o; o += r4(H * RS);
  S.dl = o; o += r4(NCLS * RS);
  S.x = o; o += r4(IN * RS);
  S.lrow = o; o += r4(CH);
  S.corr = o; o += 4;
  S.cnt = o; o += r4(WAVES);
  S.total = o;
  return S;
}
static_assert(sizeof(float) * (size_t)smem_layout().total <= LDS_CAP, "the fixed LDS state must fit the CU's");

// beta^t by binary exponentiation in double, a function of t alone (as moons_gan.hip's: each kernel keeps its own)
__device__ __forceinline__ double ipow(double b, int64_t t) {
  double r = 1.0;
  for (; t > 0; t >>= 1) {
    if (t & 1) r *= b;
    b *= b;
  }
  return r;
}

struct Net { const float *W1, *b1, *W2, *b2, *W3, *b3; };     // in LDS

// Forward of one row; every weight is the same LDS address on all lanes (a broadcast read).  h1 post-ReLU; bit j of live2: unit j
// of the second layer is positive.  STORE: h2 (post-ReLU, 0 for a row that does not exist) goes to h2col[j * RS].
template <bool STORE>
__device__ __forceinline__ void forward_row(float x0, float x1, const Net& n, float (&h1)[H], float (&lg)[NCLS], unsigned& live2, float* h2col,
                                            bool valid) {
#pragma unroll
  for (int j4 = 0; j4 < H; j4 += 4) {
    const float4 wa = *reinterpret_cast<const float4*>(n.W1 + 2 * j4), wb = *reinterpret_cast<const float4*>(n.W1 + 2 * j4 + 4);
    const float4 b = *reinterpret_cast<const float4*>(n.b1 + j4);
    h1[j4] = fmaxf(fmaf(wa.y, x1, fmaf(wa.x, x0, b.x)), 0.f);
    h1[j4 + 1] = fmaxf(fmaf(wa.w, x1, fmaf(wa.z, x0, b.y)), 0.f);
    h1[j4 + 2] = fmaxf(fmaf(wb.y, x1, fmaf(wb.x, x0, b.z)), 0.f);
    h1[j4 + 3] = fmaxf(fmaf(wb.w, x1, fmaf(wb.z, x0, b.w)), 0.f);
  }
  lg[0] = n.b3[0]; lg[1] = n.b3[1]; lg[2] = n.b3[2];
  live2 = 0;
#pragma unroll 1
  for (int j = 0; j < H; j += 2) {
    const float2 bb = *reinterpret_cast<const float2*>(n.b2 + j);
    float s0 = bb.x, s1 = bb.y;
    const float* w = n.W2 + j * H;
#pragma unroll
    for (int i = 0; i < H; i += 4) {
      const float4 u = *reinterpret_cast<const float4*>(w + i), t = *reinterpret_cast<const float4*>(w + H + i);
      s0 = fmaf(u.x, h1[i], s0); s0 = fmaf(u.y, h1[i + 1], s0); s0 = fmaf(u.z, h1[i + 2], s0); s0 = fmaf(u.w, h1[i + 3], s0);
      s1 = fmaf(t.x, h1[i], s1); s1 = fmaf(t.y, h1[i + 1], s1); s1 = fmaf(t.z, h1[i + 2], s1); s1 = fmaf(t.w, h1[i + 3], s1);
    }
    s0 = fmaxf(s0, 0.f); s1 = fmaxf(s1, 0.f);
    live2 |= ((s0 > 0.f ? 1u : 0u) | (s1 > 0.f ? 2u : 0u)) << j;
    if (STORE) { h2col[j * RS] = valid ? s0 : 0.f; h2col[(j + 1) * RS] = valid ? s1 : 0.f; }
#pragma unroll
    for (int c = 0; c < NCLS; ++c) {
      const float2 w3 = *reinterpret_cast<const float2*>(n.W3 + c * H + j);
      lg[c] = fmaf(w3.y, s1, fmaf(w3.x, s0, lg[c]));
    }
  }
}

// sum over rows r0 .. r1 (a multiple of 4 apart from r0) of pa[r] * pb[r] (pb null: of pa[r]), rows in order, added to acc
__device__ __forceinline__ float column_sum(const float* pa, const float* pb, int r0, int r1, float acc) {
  if (pb) {
    for (int r = r0; r < r1; r += 4) {
      const float4 u = *reinterpret_cast<const float4*>(pa + r), w = *reinterpret_cast<const float4*>(pb + r);
      acc = fmaf(u.x, w.x, acc); acc = fmaf(u.y, w.y, acc); acc = fmaf(u.z, w.z, acc); acc = fmaf(u.w, w.w, acc);
    }
  } else {
    for (int r = r0; r < r1; r += 4) {
      const float4 u = *reinterpret_cast<const float4*>(pa + r);
      acc += u.x; acc += u.y; acc += u.z; acc += u.w;
    }
  }
  return acc;
}

__global__ void __launch_bounds__(NT) moons_clf_fit_kernel(const pcg_moons_clf_fit_desc d, const pcg_moons_clf_fit_args a, int n_steps) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr Smem S = smem_layout();
  float *P = sm + S.P, *buf0 = sm + S.buf0, *buf1 = sm + S.buf1, *dlT = sm + S.dl, *xT = sm + S.x, *lrow = sm + S.lrow, *corr = sm + S.corr;
  const int N = d.N, nchunks = (N + CH - 1) / CH;
  const int oW1 = d.c_off[0], ob1 = d.c_off[1], oW2 = d.c_off[2], ob2 = d.c_off[3], oW3 = d.c_off[4], ob3 = d.c_off[5];
  const Net net{P + oW1, P + ob1, P + oW2, P + ob2, P + oW3, P + ob3};
  const float fN = (float)N;

  // ---- state in: parameters to LDS, moments to registers; where the gradient of flat element i will lie -------------------------
  float m[SLOTS], v[SLOTS];
  int gsrc[SLOTS];                                        // offset of partition 0's sum of this element; -1: padding, no update
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int i = tid + s * NT;
    if (i < d.nC) P[i] = a.c_flat[i];
    m[s] = i < d.nC_adam ? a.exp_avg[i] : 0.f;
    v[s] = i < d.nC_adam ? a.exp_avg_sq[i] : 0.f;
    int g = -1, r = i - oW2;
    if (r >= 0 && r < H * H) g = PART_W2 + r;
    r = i - ob2;
    if (r >= 0 && r < H) g = PART_C1 + O_B2 + r;
    r = i - oW3;
    if (r >= 0 && r < NCLS * H) g = PART_C1 + O_W3 + r;
    r = i - ob3;
    if (r >= 0 && r < NCLS) g = PART_C1 + O_B3 + r;
    r = i - oW1;
    if (r >= 0 && r < H * IN) g = PART_C3 + O_W1 + r;
    r = i - ob1;
    if (r >= 0 && r < H) g = PART_C3 + O_B1 + r;
    gsrc[s] = i < d.nC_adam ? g : -1;
  }
  const int64_t step0 = a.step[0];
  const AdamK ak = adam_k(d);

  // B2: this lane's 4 x 4 tile of dW2 (units 4 jt .., inputs 4 it ..).  C1 / C3: this thread's element and its operand rows
  const int jt = lane >> 3, it = lane & 7;
  const int oc = tid & (OC - 1), pc = tid / OC;
  const float *c1a = nullptr, *c1b = nullptr, *c3a = nullptr, *c3b = nullptr;
  if (oc < O_B3) { c1a = buf0 + (oc & (H - 1)) * RS; c1b = dlT + (oc / H) * RS; }               // dW3[c][j] = sum h2[r][j] dl[r][c]
  else if (oc < O_B3 + NCLS) c1a = dlT + (oc - O_B3) * RS;                                        // db3[c]
  else if (oc >= O_B2 && oc < O1_END) c1a = buf1 + (oc - O_B2) * RS;                              // db2[j] = sum d z2[r][j]
  if (oc < O_B1) { c3a = buf1 + (oc >> 1) * RS; c3b = xT + (oc & 1) * RS; }                       // dW1[j][k] = sum d z1[r][j] x[r][k]
  else if (oc < O3_END) c3a = buf1 + (oc - O_B1) * RS;                                            // db1[j]
  __syncthreads();

  for (int step = 0; step < n_steps; ++step) {
    PCG_T(0);
    float acc2[4][4], acc1 = 0.f, acc3 = 0.f, loss_sum = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc2[p][q] = 0.f;
    }
    for (int c = 0; c < nchunks; ++c) {
      const int nv = min(CH, N - c * CH);                  // rows of this chunk
      const int cr0 = pc * (CH / PC), cr1 = min(cr0 + CH / PC, nv);
      // ---- A1. rows: forward, loss term, backward to d z1 (trainer.py:23-25) ----------------------------------------------------
      float h1[H], dz1[H];
      {
        const int r = c * CH + tid;
        const bool valid = tid < nv;
        const float2 xr = valid ? *reinterpret_cast<const float2*>(a.X + 2 * (size_t)r) : make_float2(0.f, 0.f);
        const int y = valid ? (int)a.Y[r] : -1;
        float lg[NCLS], dl[NCLS];
        unsigned live2;
        forward_row<true>(xr.x, xr.y, net, h1, lg, live2, buf0 + tid, valid);
        // log-softmax with the row maximum subtracted, as torch; d loss / d logits = (softmax - onehot) / N
        const float mx = fmaxf(lg[0], fmaxf(lg[1], lg[2]));
        const float e0 = expf(lg[0] - mx), e1 = expf(lg[1] - mx), e2 = expf(lg[2] - mx);
        const float se = e0 + e1 + e2;
        const float ly = y == 0 ? lg[0] : y == 1 ? lg[1] : lg[2];
        lrow[tid] = valid ? (mx + logf(se)) - ly : 0.f;
        dl[0] = valid ? (e0 / se - (y == 0 ? 1.f : 0.f)) / fN : 0.f;
        dl[1] = valid ? (e1 / se - (y == 1 ? 1.f : 0.f)) / fN : 0.f;
        dl[2] = valid ? (e2 / se - (y == 2 ? 1.f : 0.f)) / fN : 0.f;
        xT[tid] = xr.x; xT[RS + tid] = xr.y;
        dlT[tid] = dl[0]; dlT[RS + tid] = dl[1]; dlT[2 * RS + tid] = dl[2];
#pragma unroll
        for (int i = 0; i < H; ++i) dz1[i] = 0.f;
#pragma unroll 1
        for (int j = 0; j < H; j += 2) {
          const float2 wa = *reinterpret_cast<const float2*>(net.W3 + j), wb = *reinterpret_cast<const float2*>(net.W3 + H + j);
          const float2 wc = *reinterpret_cast<const float2*>(net.W3 + 2 * H + j);
          const float g0 = fmaf(wc.x, dl[2], fmaf(wb.x, dl[1], wa.x * dl[0])), g1 = fmaf(wc.y, dl[2], fmaf(wb.y, dl[1], wa.y * dl[0]));
          const float z0 = (live2 >> j) & 1u ? g0 : 0.f, z1 = (live2 >> j) & 2u ? g1 : 0.f;      // (dl = 0 where the row does not exist)
          buf1[j * RS + tid] = z0; buf1[(j + 1) * RS + tid] = z1;
          const float* w = net.W2 + j * H;
#pragma unroll
          for (int i = 0; i < H; i += 4) {
            const float4 u = *reinterpret_cast<const float4*>(w + i), t = *reinterpret_cast<const float4*>(w + H + i);
            dz1[i] = fmaf(t.x, z1, fmaf(u.x, z0, dz1[i])); dz1[i + 1] = fmaf(t.y, z1, fmaf(u.y, z0, dz1[i + 1]));
            dz1[i + 2] = fmaf(t.z, z1, fmaf(u.z, z0, dz1[i + 2])); dz1[i + 3] = fmaf(t.w, z1, fmaf(u.w, z0, dz1[i + 3]));
          }
        }
#pragma unroll
        for (int i = 0; i < H; ++i) dz1[i] = h1[i] > 0.f ? dz1[i] : 0.f;
      }
      __syncthreads();
      PCG_T(1);
      // ---- C1. columns: dW3, db3, db2; the chunk's loss -------------------------------------------------------------------------
      if (c1a) acc1 = column_sum(c1a, c1b, cr0, cr1, acc1);
      if (wave == WAVES - 1) {
        float s = 0.f;
        for (int r = lane; r < nv; r += 64) s += lrow[r];
        loss_sum += wave_sum(s);
      }
      __syncthreads();
      PCG_T(2);
      // ---- A2. rows: h1 over h2 ---------------------------------------------------------------------------------------------------
#pragma unroll
      for (int j = 0; j < H; ++j) buf0[j * RS + tid] = h1[j];
      __syncthreads();
      PCG_T(3);
      // ---- B2. columns: dW2 as 4 x 4 tiles (d z2 = 0 where the row does not exist) -----------------------------------------------
      {
        const int r0 = wave * 64, r1 = min(r0 + 64, nv);
        const float* pz = buf1 + (4 * jt) * RS;
        const float* ph = buf0 + (4 * it) * RS;
        for (int r = r0; r < r1; r += 4) {
          float4 z[4], hh[4];
#pragma unroll
          for (int p = 0; p < 4; ++p) { z[p] = *reinterpret_cast<const float4*>(pz + p * RS + r); hh[p] = *reinterpret_cast<const float4*>(ph + p * RS + r); }
#pragma unroll
          for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float s = acc2[p][q];
              s = fmaf(z[p].x, hh[q].x, s); s = fmaf(z[p].y, hh[q].y, s); s = fmaf(z[p].z, hh[q].z, s); s = fmaf(z[p].w, hh[q].w, s);
              acc2[p][q] = s;
            }
          }
        }
      }
      __syncthreads();
      PCG_T(4);
      // ---- A3. rows: d z1 over d z2 -----------------------------------------------------------------------------------------------
#pragma unroll
      for (int j = 0; j < H; ++j) buf1[j * RS + tid] = dz1[j];
      __syncthreads();
      PCG_T(5);
      // ---- C3. columns: dW1, db1 --------------------------------------------------------------------------------------------------
      if (c3a) acc3 = column_sum(c3a, c3b, cr0, cr1, acc3);
      __syncthreads();
      PCG_T(6);
    }
    // ---- the partitions' sums to LDS (the chunk buffers are free), this iteration's bias corrections ----------------------------
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<float4*>(buf0 + PART_W2 + wave * H * H + (4 * jt + p) * H + 4 * it) = make_float4(acc2[p][0], acc2[p][1], acc2[p][2], acc2[p][3]);
    buf0[PART_C1 + pc * OC + oc] = acc1;
    buf0[PART_C3 + pc * OC + oc] = acc3;
    if (tid == 0) adam_corr(d.lr, d.beta1, d.beta2, step0 + step + 1, ipow, corr[0], corr[1]);
    if (tid == NT - 64) a.losses[step] = loss_sum / fN;   // the loss before this iteration's update (trainer.py:23)
    __syncthreads();
    PCG_T(7);
    // ---- params: partitions added in order, Adam (trainer.py:25) ----------------------------------------------------------------
    {
      const float ss = corr[0], bc2 = corr[1];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int i = tid + s * NT, g0 = gsrc[s];
        if (g0 >= 0) {
          const int np = g0 < PART_C1 ? WAVES : PC, st = g0 < PART_C1 ? H * H : OC;
          float g = 0.f;
          for (int p = 0; p < np; ++p) g += buf0[g0 + p * st];
          float pv = P[i];
          adam_upd(pv, g, m[s], v[s], ak, ss, bc2);
          P[i] = pv;
        }
      }
    }
    __syncthreads();
    PCG_T(8);
  }

  // ---- rows the final weights classify as their label (ties: the lower index, as torch.argmax) ----------------------------------
  if (a.correct) {
    int cnt = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int r = c * CH + tid;
      const bool valid = r < N;
      const float2 xr = valid ? *reinterpret_cast<const float2*>(a.X + 2 * (size_t)r) : make_float2(0.f, 0.f);
      float h1[H], lg[NCLS];
      unsigned live2;
      forward_row<false>(xr.x, xr.y, net, h1, lg, live2, nullptr, valid);
      const int best = lg[2] > fmaxf(lg[0], lg[1]) ? 2 : lg[1] > lg[0] ? 1 : 0;
      if (valid && (int64_t)best == a.Y[r]) ++cnt;
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    int* wc = reinterpret_cast<int*>(sm + S.cnt);
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < WAVES; ++w) t += wc[w];
      a.correct[0] = t;
    }
  }

  // ---- state out -----------------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int i = tid + s * NT;
    if (i < d.nC) a.c_flat[i] = P[i];
    if (i < d.nC_adam) { a.exp_avg[i] = m[s]; a.exp_avg_sq[i] = v[s]; }
  }
  if (tid == 0) a.step[0] = step0 + n_steps;
}

int check_desc(const pcg_moons_clf_fit_desc* d) {
  PCG_REQUIRE(d, "pcg_moons_clf_fit: null desc");
  PCG_REQUIRE(d->hidden == H, "pcg_moons_clf_fit: hidden %d (built for %d)", d->hidden, H);
  PCG_REQUIRE(d->N >= 1 && d->N <= MAXN, "pcg_moons_clf_fit: N %d outside [1, %d]", d->N, MAXN);
  PCG_REQUIRE(d->nC >= 1 && d->nC <= MAXC, "pcg_moons_clf_fit: nC %d outside [1, %d]", d->nC, MAXC);
  const int sz[6] = {H * IN, H, H * H, H, NCLS * H, NCLS};
  int end = 0;
  for (int k = 0; k < 6; ++k) {           // tensors in flat order, 16-byte aligned, not overlapping, inside the buffer
    PCG_REQUIRE(d->c_off[k] >= end && d->c_off[k] % 4 == 0 && d->c_off[k] <= d->nC - sz[k],
                "pcg_moons_clf_fit: c_off[%d] = %d out of order, unaligned or outside nC %d", k, d->c_off[k], d->nC);
    end = d->c_off[k] + sz[k];
  }
  PCG_REQUIRE(d->nC_adam >= 0 && d->nC_adam <= d->nC, "pcg_moons_clf_fit: nC_adam %d outside [0, nC %d]", d->nC_adam, d->nC);
  return PCG_OK;
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_moons_clf_fit_scratch_bytes(const pcg_moons_clf_fit_desc* desc) {
  (void)desc;
  return 0;                               // the chunks' activations live in LDS
}

extern "C" int pcg_moons_clf_fit(const pcg_moons_clf_fit_desc* desc, const pcg_moons_clf_fit_args* args, int32_t n_steps, pcg_stream_t stream) {
  if (int rc = check_desc(desc)) return rc;
  PCG_REQUIRE(args, "pcg_moons_clf_fit: null args");
  PCG_REQUIRE(n_steps >= 1, "pcg_moons_clf_fit: n_steps %d < 1", n_steps);
  const pcg_moons_clf_fit_args& a = *args;
#define PCG_CLF_PTR(f) PCG_REQUIRE(a.f, "pcg_moons_clf_fit: null pointer %s", #f)
  PCG_CLF_PTR(X); PCG_CLF_PTR(Y); PCG_CLF_PTR(c_flat); PCG_CLF_PTR(exp_avg); PCG_CLF_PTR(exp_avg_sq); PCG_CLF_PTR(step); PCG_CLF_PTR(losses);
#undef PCG_CLF_PTR
  PCG_REQUIRE(((uintptr_t)a.X & 7) == 0, "pcg_moons_clf_fit: X must be 8-byte aligned");
  const size_t need = pcg_moons_clf_fit_scratch_bytes(desc);
  PCG_REQUIRE(a.scratch_bytes >= need && (a.scratch || a.scratch_bytes == 0) && ((uintptr_t)a.scratch & 15) == 0,
              "pcg_moons_clf_fit: scratch of %zu bytes: %zu needed, not NULL unless 0 bytes, 16-byte aligned", a.scratch_bytes, need);
  const size_t lds = sizeof(float) * (size_t)smem_layout().total;
  return launch_one_wg(moons_clf_fit_kernel, "moons_clf_fit_kernel", NT, lds, (hipStream_t)stream, *desc, a, (int)n_steps);
}
