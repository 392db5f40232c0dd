// conv_igemm.hip — Conv2d / ConvTranspose2d forward, grad-input and grad-weight as fp32-MFMA implicit
// GEMMs over NHWC activations and OHWI weights (see include/pcgan_hip.h for the layer <-> op mapping).
//
//   fwd   : M = B*OH*OW        N = Cout          K = (kh,kw,ci)     A = im2col(x) gathered, B = w rows
//   dgrad : per sub-pixel phase (ih%s, iw%s):  M = B*PHh*PHw  N = Cin  K = (taps of the phase, co)
//           A = dy gathered, B = w^T slices.  For k4 s2 p1 every phase sees exactly 2x2 taps: no MAC is
//           spent on the zeros a "dilate then convolve" formulation would insert.
//   wgrad : M = Cout  N = (kh,kw,ci)  K = B*OH*OW split over gridDim.y; partial slabs reduced in a
//           fixed order by a second kernel (deterministic; also implements .grad accumulation).
//
// Replaces ATen conv forward/backward behind nn.Conv2d / nn.ConvTranspose2d at
// dconv_gan/mnist/mnist_dcgan.py:76-88,100-111 and conditional_counteRGAN/mnist/models/*.py.
#include <string.h>
#include <array>
#include <map>
#include <mutex>
#include <vector>
#include "conv_loaders.h"
#include "conv_pixtab.h"
#include "conv_cliptab.h"
#include "thin_conv.h"

namespace pcg {
namespace {

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// role of this wave, provably wave-uniform for the compiler (scalar branch, no exec masking)
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Issue priority at the edges of a workgroup's life (ConvP::edge_prio).  The main loops run producers at 3 and consumers at 1-2
// (igemm_core.h); everything outside them — loader set-up with its divisions, the first gathers, the LDS-staged epilogue — used to
// run at priority 0 and was handed an issue slot only when no wave of the CU's other workgroups wanted one: in-kernel stamps
// (r04, 3x3 64->64 forward, three workgroups per CU) read 4.0 us from entry to the first k-tile and 7.1 us for a ~150-instruction
// epilogue, 17 % of the workgroup's life.
__device__ __forceinline__ void prio_entry(const ConvP& p) { if (p.edge_prio & 1) __builtin_amdgcn_s_setprio(3); }
__device__ __forceinline__ void prio_epilogue(const ConvP& p) { if (p.edge_prio & 2) __builtin_amdgcn_s_setprio(3); }

// grouped launches (EpiAux::group_rows): float offset of the tile's group inside the [G][N] BatchNorm statistics
__device__ __forceinline__ int epi_group_off(const ConvP& p, int m_block) {
  return p.epi.group_rows > 0 ? __builtin_amdgcn_readfirstlane(m_block / p.epi.group_rows) * p.N : 0;
}

// XF (here and below): the activation operand carries an input transform (ConvP::in_sc) — a separate instantiation, so the
// plain kernels pay nothing for it.
// CLIP: position-major rows, each tile iterating only the taps that are not padding at its position (conv_cliptab.h): a 1-D grid of
// whole tiles, no K-slices.  Same products in the same order for every output element, zeros left out: bit-identical outputs.
template <class Cfg, bool XF, bool CLIP = false>
__global__ void __launch_bounds__(IG_THREADS, Cfg::MINW) conv_fwd_kernel(ConvP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  prio_entry(p);
  if constexpr (CLIP) {
    uint32_t nt, idx;
    clip_block_tile(blockIdx.x, (uint32_t)p.tilesN, gridDim.x / (uint32_t)p.tilesN, p.clip_order, false, 0u, nt, idx);
    nt = __builtin_amdgcn_readfirstlane(nt); idx = __builtin_amdgcn_readfirstlane(idx);   // (the divisions ran on the vector unit)
    const ClipTile t = clip_tile(p, 0, idx, Cfg::BM);
    const int n_block = (int)nt * Cfg::BN;
    const int ktiles = t.nh * t.nw * ((p.Cin + IG_BK - 1) / IG_BK);
    if (wave_id() >= 4) {  // producers
      const int tid = threadIdx.x - IG_LOADERS;
      FwdALoader<Cfg::BM, XF, true> la(p, t, tid);
      FwdBLoader<Cfg::BN, true> lb(p, n_block, tid);
      lb.it.clip(t.h0, t.nh, t.w0, t.nw);
      igemm_produce<Cfg>(la, lb, ktiles, smem, tid, ClockStamp{p.stamps, p.stamp_slots});
      return;
    }
    f32x16 acc[Cfg::TM][Cfg::TN];
    ClockStamp cs{p.stamps, p.stamp_slots};
    cs.phase(0);
    igemm_consume<Cfg, true, true>(ktiles, acc, smem, cs);
    prio_epilogue(p);
    const size_t npix = (size_t)p.OH * p.OW;
    igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
      const int b = t.img0 + row;
      return b < p.B ? p.out + ((size_t)b * npix + t.pos) * p.N + n_block : nullptr;
    }, p.stat_partial ? p.stat_partial + (size_t)t.stat_tile * Cfg::WAVES_M * 2 * p.N : nullptr, p.act, p.slope, &p.epi,
       p.epi.group_rows > 0 ? t.group * p.N : 0);
    cs.phase(3);
    return;
  }
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = tile / p.tilesN, nt = tile % p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  // split-K (few output tiles, long K): slab blockIdx.y covers k-tiles [kt_begin, kt_begin + ktiles)
  const int kt_begin = blockIdx.y * p.ktiles_per_split;
  int ktiles = p.ktiles - kt_begin;
  if (ktiles > p.ktiles_per_split) ktiles = p.ktiles_per_split;

  if (wave_id() >= 4) {  // producers
    const int tid = threadIdx.x - IG_LOADERS;
    FwdALoader<Cfg::BM, XF> la(p, m_block, tid);
    FwdBLoader<Cfg::BN> lb(p, n_block, tid);
    if (kt_begin) { la.seek(kt_begin); lb.seek(kt_begin); }
    igemm_produce<Cfg>(la, lb, ktiles, smem, tid, ClockStamp{p.stamps, p.stamp_slots});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  ClockStamp cs{p.stamps, p.stamp_slots};
  cs.phase(0);
  igemm_consume<Cfg, true, true>(ktiles, acc, smem, cs);
  prio_epilogue(p);
  float* out = p.out + (size_t)blockIdx.y * (size_t)p.M * (size_t)p.N;
#ifdef PCG_ABL_NO_EPILOGUE   // timing-only ablation: keep one store so the accumulators stay live
  if (acc[0][0][0] == 12345.678f) out[0] = acc[0][0][1];
  return;
#endif
  igemm_store_tile<Cfg>(acc, smem, n_block, p.N, blockIdx.y == 0 ? p.bias : nullptr, [&](int row) -> float* {
    const int m = m_block + row;
    return m < p.M ? out + (size_t)m * p.N + n_block : nullptr;
  }, p.stat_partial ? p.stat_partial + (size_t)mt * Cfg::WAVES_M * 2 * p.N : nullptr, p.act, p.slope, &p.epi, epi_group_off(p, m_block));
  cs.phase(3);
}

template <class Cfg, bool XF, bool CLIP = false>
__global__ void __launch_bounds__(IG_THREADS, Cfg::MINW) conv_dgrad_kernel(ConvP p, DgradPhases phases) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int rowpix[Cfg::BM];
  prio_entry(p);
  if constexpr (CLIP) {   // (see conv_fwd_kernel) equal phases, either interleaved in the 1-D grid or one per blockIdx.y
    const uint32_t nil = phases.interleave ? (uint32_t)phases.interleave : 1u, per = nil * (uint32_t)p.tilesN;
    uint32_t within, idx;
    clip_block_tile(blockIdx.x, per, gridDim.x / per, p.clip_order, !phases.interleave, blockIdx.y, within, idx);
    idx = __builtin_amdgcn_readfirstlane(idx);   // (the divisions ran on the vector unit: back to scalar registers, like the phase below)
    const uint32_t py = __builtin_amdgcn_readfirstlane(phases.interleave ? within % nil : blockIdx.y), nt = __builtin_amdgcn_readfirstlane(within / nil);
    const PhaseInfo& f = phases.p[py];
    const ClipTile t = clip_tile(p, 1 + 2 * f.ph + f.pw, idx, Cfg::BM);
    const int n_block = (int)nt * Cfg::BN;
    const int ktiles = t.nh * t.nw * ((p.Cout + IG_BK - 1) / IG_BK);
    if (wave_id() >= 4) {
      const int tid = threadIdx.x - IG_LOADERS;
      uint32_t aa, cc;
      f.dPHw.divmod((uint32_t)t.pos, aa, cc);
      const int pix0 = ((int)aa * p.stride + f.ph) * p.IW + (int)cc * p.stride + f.pw;
      for (int r = tid; r < Cfg::BM; r += IG_LOADERS) rowpix[r] = t.img0 + r < p.B ? (t.img0 + r) * p.IH * p.IW + pix0 : -1;
      DgradALoader<Cfg::BM, XF, true> la(p, f, t, tid);
      DgradBLoader<Cfg::BN, true> lb(p, f, n_block, tid);
      lb.it.clip(t.h0, t.nh, t.w0, t.nw);
      igemm_produce<Cfg>(la, lb, ktiles, smem, tid, ClockStamp{p.stamps, p.stamp_slots});
      return;
    }
    f32x16 acc[Cfg::TM][Cfg::TN];
    ClockStamp cs{p.stamps, p.stamp_slots};
    cs.phase(0);
    igemm_consume<Cfg, true, false>(ktiles, acc, smem, cs);
    prio_epilogue(p);
    igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
      const int pix = rowpix[row];
      return pix >= 0 ? p.out + (size_t)pix * p.Cin + n_block : nullptr;
    }, p.stat_partial ? p.stat_partial + (size_t)(f.prow0 + t.stat_tile * Cfg::WAVES_M) * 2 * p.N : nullptr, p.act, p.slope, &p.epi,
       p.epi.group_rows > 0 ? t.group * p.N : 0);
    cs.phase(3);
    return;
  }
  // phases.interleave (all phases the same size, 1-D grid): the sub-pixel phases of one tile are neighbours in launch order and
  // on one XCD — they gather the same dy rows, which then come from HBM once and from that XCD's L2 for the other phases
  uint32_t bx = blockIdx.x, py = blockIdx.y;
  if (phases.interleave) {
    const uint32_t l = xcd_remap(blockIdx.x, gridDim.x);
    py = l % (uint32_t)phases.interleave; bx = l / (uint32_t)phases.interleave;
  }
  const PhaseInfo& f = phases.p[py];
  const int tilesM = (f.Mp + Cfg::BM - 1) / Cfg::BM;
  const uint32_t ntiles = (uint32_t)tilesM * p.tilesN;
  if (bx >= ntiles) return;  // phases can differ in size (odd IH/IW); uniform per block
  const uint32_t tile = phases.interleave ? bx : xcd_remap(bx, ntiles);
  const int mt = tile / p.tilesN, nt = tile % p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  const int ktiles = f.nth * f.ntw * ((p.Cout + IG_BK - 1) / IG_BK);

  if (wave_id() >= 4) {  // producers: also publish the output pixel of every tile row (visible after barrier 0)
    const int tid = threadIdx.x - IG_LOADERS;
    for (int r = tid; r < Cfg::BM; r += IG_LOADERS) {
      const int m = m_block + r;
      int pix = -1;
      if (m < f.Mp) {
        uint32_t t, cc, b, aa;
        f.dPHw.divmod((uint32_t)m, t, cc);
        f.dPHh.divmod(t, b, aa);
        pix = ((int)b * p.IH + (int)aa * p.stride + f.ph) * p.IW + (int)cc * p.stride + f.pw;
      }
      rowpix[r] = pix;
    }
    DgradALoader<Cfg::BM, XF> la(p, f, m_block, tid);
    DgradBLoader<Cfg::BN> lb(p, f, n_block, tid);
    igemm_produce<Cfg>(la, lb, ktiles, smem, tid, ClockStamp{p.stamps, p.stamp_slots});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  ClockStamp cs{p.stamps, p.stamp_slots};
  cs.phase(0);
  igemm_consume<Cfg, true, false>(ktiles, acc, smem, cs);
  prio_epilogue(p);
  igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
    const int pix = rowpix[row];
    return pix >= 0 ? p.out + (size_t)pix * p.Cin + n_block : nullptr;
  }, p.stat_partial ? p.stat_partial + (size_t)(f.prow0 + mt * Cfg::WAVES_M) * 2 * p.N : nullptr, p.act, p.slope, &p.epi, epi_group_off(p, m_block));
  cs.phase(3);
}

// ======================================================================================================================
// Hybrid stream-K launches (r03).  The one-tile-per-workgroup kernels above run in rounds of 512 workgroups (2 per CU); a launch
// whose tile count is not a multiple of that pays a whole extra round for the remainder — the in-kernel stamps of WGAN-GP's
// 288-tile grad-input GEMM (1024 x 4608, K = 1024) show 224 CUs finishing their single tile at 69 us and 32 CUs running two tiles
// side by side until 124 us: 66 TFLOP/s.  Here the first `dp_tiles` tiles (whole rounds) keep one workgroup each, and the k-tiles
// of the remaining `sk_tiles` tiles form ONE iteration space that is cut into `sk_blocks` equal contiguous ranges, one per
// workgroup; a range covers the tail of one tile and the head of the next (at most two segments: sk_blocks >= sk_tiles).
// A segment that is not a whole tile leaves its accumulators as a partial tile in the scratch buffer (register layout, coalesced
// 16-byte stores) and bumps the arrival counter of (tile, consumer wave); the wave that arrives LAST adds the partial tiles of its
// quadrant in K order — its own included, from memory: the order of the sum never depends on who arrives when, results are
// bit-reproducible — and runs the ordinary epilogue (bias, activation, statistics, backward riders: nothing is lost to the
// split, unlike the slab form of plan_fwd).  Counters return to zero behind the last arrival; visibility across the XCDs' L2s
// comes from the agent-scope release / acquire fences around the counter update.
// ======================================================================================================================
struct SkPlan {
  int dp_tiles, sk_tiles, sk_blocks, ktiles;   // ktiles: per tile
  float* parts;                                // [2 * sk_blocks][BM * BN]
  int* arrivals;                               // [sk_tiles][4], zero between launches
};
struct SkSeg { int tile, kt_begin, nkt, nparts, first_block; };   // tile: index among ALL tiles of the launch

// (wave-uniform values; the divisions run on the vector unit, readfirstlane puts the results back into scalar registers.
//  32-bit: the host keeps sk_tiles * ktiles * sk_blocks below 2^31)
__device__ __forceinline__ int sk_start(int g, const SkPlan& sk) {
  return __builtin_amdgcn_readfirstlane((int)((uint32_t)g * (uint32_t)(sk.sk_tiles * sk.ktiles) / (uint32_t)sk.sk_blocks));
}
__device__ __forceinline__ int sk_owner(int x, const SkPlan& sk) {     // the block whose range holds iteration x
  return __builtin_amdgcn_readfirstlane((int)((((uint32_t)x + 1u) * (uint32_t)sk.sk_blocks - 1u) / (uint32_t)(sk.sk_tiles * sk.ktiles)));
}
// b: the block's place in the launch order — blockIdx.x, or a permutation of it (wgrad_pair_block)
__device__ __forceinline__ int sk_segments(const SkPlan& sk, SkSeg& s0, SkSeg& s1, int b) {
  if (b < sk.dp_tiles) { s0 = SkSeg{(int)xcd_remap((uint32_t)b, (uint32_t)sk.dp_tiles), 0, sk.ktiles, 1, 0}; return 1; }
  // neighbouring ranges (neighbouring tiles: shared operand rows) on ONE XCD, like the tiles of the data-parallel part
  const int g = (int)xcd_remap((uint32_t)(b - sk.dp_tiles), (uint32_t)sk.sk_blocks), KT = sk.ktiles;
  const int it0 = sk_start(g, sk), it1 = sk_start(g + 1, sk);
  const int j0 = __builtin_amdgcn_readfirstlane(it0 / KT), e0 = it1 < (j0 + 1) * KT ? it1 : (j0 + 1) * KT;
  auto fill = [&](SkSeg& sg, int j, int from, int to) {
    const int f = sk_owner(j * KT, sk), l = sk_owner((j + 1) * KT - 1, sk);
    sg = SkSeg{sk.dp_tiles + j, from - j * KT, to - from, l - f + 1, f};
  };
  fill(s0, j0, it0, e0);
  if (it1 <= e0) return 1;
  fill(s1, j0 + 1, e0, it1);
  return 2;
}
// Partial tiles cross XCDs (each has its own L2).  Their stores and loads carry sc1 (agent scope: written through / read past
// the non-coherent lines; raw-buffer builtins with aux 16, so the compiler counts them) instead of an agent-scope release /
// acquire fence pair around the counter, which writes back and invalidates whole caches once per wave and arrival (measured r03:
// with the fences the 288-tile GEMM went from 137 to 203 us).  Each storing wave drains its stores (vmcnt(0)) before ITS add to
// the (tile, wave) counter; the wave whose add returns nparts - 1 loads only behind that return.
// PER-ARCHITECTURE REQUIREMENT: this protocol (sc1 stores drained by vmcnt(0), then a relaxed agent-scope atomic, no fences) is
// what gfx950's memory model guarantees for agent-scope visibility; another target has to re-derive it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "stream-K partial-tile exchange (sc1 stores + relaxed agent-scope counters) is written for gfx950 only"
#endif
__device__ __forceinline__ void sk_store4(rsrc_t r, uint32_t off, float a, float b, float c, float d) {
  const u32x4 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 16);
}
__device__ __forceinline__ float4 sk_load4(rsrc_t r, uint32_t off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// consumer waves, after the main loop of a segment: true when this wave holds the finished sum of its quadrant in `acc`.
//   g: this workgroup's range index, j: arrival-counter index of the tile, nparts / first_block: the ranges that touch the tile,
//   first_of(blk): does range blk START inside this tile (its partial is then in the range's slot 0, else in slot 1)
template <class Cfg, class FirstOf>
__device__ __forceinline__ bool sk_combine_core(float* parts, int* arrivals, int nblocks, int g, int j, int nparts, int first_block,
                                                FirstOf first_of, f32x16 (&acc)[Cfg::TM][Cfg::TN]) {
  if (nparts == 1) return true;
  constexpr uint32_t TILE_BYTES = Cfg::BM * Cfg::BN * 4;
  auto slot_of = [&](int blk) { return (uint32_t)(2 * blk + (first_of(blk) ? 0 : 1)); };
  const rsrc_t rs = make_rsrc(parts, (uint32_t)(2 * nblocks) * TILE_BYTES);
  const uint32_t toff = threadIdx.x * 16u;                 // consumer threads 0..255: one 16-byte column of each 4 KB row of the partial tile
  const uint32_t mine = slot_of(g) * TILE_BYTES + toff;
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int jj = 0; jj < Cfg::TN; ++jj)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        sk_store4(rs, mine + (uint32_t)(((i * Cfg::TN + jj) * 4 + q) * IG_LOADERS * 16),
                  acc[i][jj][4 * q], acc[i][jj][4 * q + 1], acc[i][jj][4 * q + 2], acc[i][jj][4 * q + 3]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's partial quadrant has left for memory
  int* cnt = arrivals + j * 4 + (int)(threadIdx.x >> 6);
  int old = 0;
  if ((threadIdx.x & 63) == 0) old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = __builtin_amdgcn_readfirstlane(old);
  if (old != nparts - 1) return false;
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int jj = 0; jj < Cfg::TN; ++jj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][jj][r] = 0.f;
  for (int k = 0; k < nparts; ++k) {
    const uint32_t src = slot_of(first_block + k) * TILE_BYTES + toff;
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int jj = 0; jj < Cfg::TN; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = sk_load4(rs, src + (uint32_t)(((i * Cfg::TN + jj) * 4 + q) * IG_LOADERS * 16));
          acc[i][jj][4 * q] += v.x; acc[i][jj][4 * q + 1] += v.y; acc[i][jj][4 * q + 2] += v.z; acc[i][jj][4 * q + 3] += v.w;
        }
  }
  return true;
}
template <class Cfg>
__device__ __forceinline__ bool sk_combine(const SkPlan& sk, const SkSeg& sg, f32x16 (&acc)[Cfg::TM][Cfg::TN], int b) {
  const int g = (int)xcd_remap((uint32_t)(b - sk.dp_tiles), (uint32_t)sk.sk_blocks), j = sg.tile - sk.dp_tiles, KT = sk.ktiles;
  return sk_combine_core<Cfg>(sk.parts, sk.arrivals, sk.sk_blocks, g, j, sg.nparts, sg.first_block,
                              [&](int blk) { return sk_start(blk, sk) >= j * KT; }, acc);
}

// One segment = the base kernel's body over k-tiles [kt_begin, kt_begin + nkt) of one tile.  A workgroup runs it once or twice;
// the two runs are two inlined copies, not a loop (as a loop the compiler kept both segments' state live across the body: 60-80
// spilled VGPRs and a scratch access inside the k-tile loop; the all-data-parallel cost of that kernel was +13..21 % on grad-input
// launches, scripts/probes/streamk_dp_cost.py).
template <class Cfg, bool XF>
__device__ __forceinline__ void fwd_sk_segment(const ConvP& p, const SkPlan& sk, const SkSeg& sg, float* smem) {
  const int mt = __builtin_amdgcn_readfirstlane(sg.tile / p.tilesN), nt = sg.tile - mt * p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  if (wave_id() >= 4) {  // producers
    const int tid = threadIdx.x - IG_LOADERS;
    FwdALoader<Cfg::BM, XF> la(p, m_block, tid);
    FwdBLoader<Cfg::BN> lb(p, n_block, tid);
    if (sg.kt_begin) { la.seek(sg.kt_begin); lb.seek(sg.kt_begin); }
    igemm_produce<Cfg>(la, lb, sg.nkt, smem, tid, ClockStamp{nullptr, 0});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  igemm_consume<Cfg, true, true>(sg.nkt, acc, smem);
  if (sk_combine<Cfg>(sk, sg, acc, (int)blockIdx.x))
    igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
      const int m = m_block + row;
      return m < p.M ? p.out + (size_t)m * p.N + n_block : nullptr;
    }, p.stat_partial ? p.stat_partial + (size_t)mt * Cfg::WAVES_M * 2 * p.N : nullptr, p.act, p.slope, &p.epi, epi_group_off(p, m_block));
}
template <class Cfg, bool XF>
__global__ void __launch_bounds__(IG_THREADS, Cfg::MINW) conv_fwd_sk_kernel(ConvP p, SkPlan sk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  SkSeg s0, s1{};
  const int nseg = sk_segments(sk, s0, s1, (int)blockIdx.x);
  fwd_sk_segment<Cfg, XF>(p, sk, s0, smem);
  if (nseg == 1) return;
  lds_barrier();   // the epilogue staged through the LDS stages: the second segment's producers wait for it
  fwd_sk_segment<Cfg, XF>(p, sk, s1, smem);
}

// grad-input: the tiles of all sub-pixel phases are numbered phase-major (phase = tile / tiles_per_phase); the host only takes
// this form when every phase has the same number of rows and taps (one iteration space)
template <class Cfg, bool XF>
__device__ __forceinline__ void dgrad_sk_segment(const ConvP& p, const DgradPhases& phases, const SkPlan& sk, const SkSeg& sg, int tiles_per_phase,
                                                 float* smem, int* rowpix) {
  const int py = __builtin_amdgcn_readfirstlane(sg.tile / tiles_per_phase), tile = sg.tile - py * tiles_per_phase;
  const PhaseInfo& f = phases.p[py];
  const int mt = __builtin_amdgcn_readfirstlane(tile / p.tilesN), nt = tile - mt * p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  if (wave_id() >= 4) {
    const int tid = threadIdx.x - IG_LOADERS;
    for (int r = tid; r < Cfg::BM; r += IG_LOADERS) {
      const int m = m_block + r;
      int pix = -1;
      if (m < f.Mp) {
        uint32_t t, cc, b, aa;
        f.dPHw.divmod((uint32_t)m, t, cc);
        f.dPHh.divmod(t, b, aa);
        pix = ((int)b * p.IH + (int)aa * p.stride + f.ph) * p.IW + (int)cc * p.stride + f.pw;
      }
      rowpix[r] = pix;
    }
    DgradALoader<Cfg::BM, XF> la(p, f, m_block, tid);
    DgradBLoader<Cfg::BN> lb(p, f, n_block, tid);
    if (sg.kt_begin) { la.seek(sg.kt_begin); lb.seek(sg.kt_begin); }
    igemm_produce<Cfg>(la, lb, sg.nkt, smem, tid, ClockStamp{nullptr, 0});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  igemm_consume<Cfg, true, false>(sg.nkt, acc, smem);
  if (sk_combine<Cfg>(sk, sg, acc, (int)blockIdx.x))
    igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
      const int pix = rowpix[row];
      return pix >= 0 ? p.out + (size_t)pix * p.Cin + n_block : nullptr;
    }, p.stat_partial ? p.stat_partial + (size_t)(f.prow0 + mt * Cfg::WAVES_M) * 2 * p.N : nullptr, p.act, p.slope, &p.epi, epi_group_off(p, m_block));
}
template <class Cfg, bool XF>
__global__ void __launch_bounds__(IG_THREADS, Cfg::MINW) conv_dgrad_sk_kernel(ConvP p, DgradPhases phases, SkPlan sk, int tiles_per_phase) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int rowpix[Cfg::BM];
  SkSeg s0, s1{};
  const int nseg = sk_segments(sk, s0, s1, (int)blockIdx.x);
  dgrad_sk_segment<Cfg, XF>(p, phases, sk, s0, tiles_per_phase, smem, rowpix);
  if (nseg == 1) return;
  lds_barrier();
  dgrad_sk_segment<Cfg, XF>(p, phases, sk, s1, tiles_per_phase, smem, rowpix);
}

// The padding skip of the weight-gradient consumers (igemm_core.h PadSkip) for this wave's columns [n_block + wn * WTN, .. + WTN) and a
// K range that starts at k-tile kt_begin.  The host takes these kernels only for k4 s2 p1 geometries with IH = 2 OH, IW = 2 OW, OH and
// OW powers of two >= 4 and Cin a multiple of 64 (wgrad_padskip_geom), so a wave tile never straddles two tap rows, nor two taps
// where OW = 4.  Columns past N belong to "tap row 4": nothing is skipped for them.
template <class Cfg>
__device__ __forceinline__ PadSkip wgrad_padskip(const ConvP& p, int n_block, int kt_begin) {
  const int wn = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) % Cfg::WAVES_N;
  const int tap = __builtin_amdgcn_readfirstlane((int)((uint32_t)(n_block + wn * Cfg::WTN) / (uint32_t)p.Cin));
  const int kh = tap >> 2, kw = tap & 3;
  PadSkip ps;
  ps.q0 = kt_begin * IG_BK;
  ps.lgw = 31 - __builtin_clz((unsigned)p.OW); ps.ohm = p.OH - 1;
  const bool w4 = p.OW == 4;
  ps.tmask = w4 && tap < 16 ? (kw == 0 ? 1 : kw == 3 ? 8 : 0) : 0;
  ps.oh_zero = w4 ? -1 : kh == 0 ? 0 : kh == 3 ? p.OH - 1 : -1;
  return ps;
}
// Block order of the skipping kernels (pair_xor != 0): the schedule model puts blocks b and b + 256 on one CU, and in today's orders
// those two own tiles of the same tap class — both skip or neither does.  Within every odd round of 256 blocks the block ids are
// permuted by b ^ pair_xor (a permutation of the round, so every tile is still computed exactly once, by one block, in the same K
// order); the host picks the bit that pairs a skipping tile with a full one (wgrad_pair_xor).  Rounds that are not whole keep their order.
__device__ __forceinline__ uint32_t wgrad_pair_block(uint32_t b, uint32_t nblocks, int pair_xor) {
  return ((b >> 8) & 1u) && (b | 255u) < nblocks ? b ^ (uint32_t)pair_xor : b;
}

// XFA: the dy operand is a transformed activation (ConvTranspose2d layers); XFB: x is; TAB: the x gather reads its pixels from the
// geometry's descriptor table (ConvP::pixtab != nullptr); PS (1: OW = 4, 2: OW >= 8): the consumers skip all-padding MFMAs (wgrad_padskip) — launched as a 1-D
// grid in today's dispatch order (tile-major: x = tile fastest), optionally paired (pair_xor, unused without PS)
template <class Cfg, bool XFA, bool XFB, bool TAB = false, int PS = 0>
__global__ void __launch_bounds__(IG_THREADS, 4) conv_wgrad_kernel(ConvP p, int ktiles_total, int ktiles_per_split, int tiles,
                                                                   int slice_major, int pair_xor) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  prio_entry(p);
  // slice_major: 1-D grid, the output tiles of one K-slice are consecutive on ONE XCD, so the slice of dy / x they all read
  // comes from HBM once and from that XCD's L2 afterwards (layers with few output tiles re-read their operands per tile)
  uint32_t tile, split;
  if constexpr (PS) {
    const uint32_t b = wgrad_pair_block(blockIdx.x, gridDim.x, pair_xor);
    if (slice_major) {
      const uint32_t l = xcd_remap(b, gridDim.x);
      split = l / (uint32_t)tiles; tile = l - split * (uint32_t)tiles;
    } else {
      split = b / (uint32_t)tiles; tile = xcd_remap(b - split * (uint32_t)tiles, (uint32_t)tiles);
    }
  } else if (slice_major) {
    const uint32_t l = xcd_remap(blockIdx.x, gridDim.x);
    split = l / (uint32_t)tiles; tile = l - split * (uint32_t)tiles;
  } else {
    tile = xcd_remap(blockIdx.x, gridDim.x); split = blockIdx.y;
  }
  const int mt = tile / p.tilesN, nt = tile % p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  const int kt_begin = split * ktiles_per_split;
  int ktiles = ktiles_total - kt_begin;
  if (ktiles > ktiles_per_split) ktiles = ktiles_per_split;

  if (wave_id() >= 4) {
    const int tid = threadIdx.x - IG_LOADERS;
    WgradALoader<Cfg::BM, XFA> la(p, m_block, kt_begin, tid);
    WgradBLoader<Cfg::BN, XFB, TAB> lb(p, n_block, kt_begin, tid);
    igemm_produce<Cfg>(la, lb, ktiles, smem, tid, ClockStamp{p.stamps, p.stamp_slots});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  if constexpr (PS) igemm_consume_padskip<Cfg, false, false, PS>(ktiles, acc, smem, ClockStamp{p.stamps, p.stamp_slots}, wgrad_padskip<Cfg>(p, n_block, kt_begin));
  else igemm_consume<Cfg, false, false>(ktiles, acc, smem, ClockStamp{p.stamps, p.stamp_slots});
  prio_epilogue(p);
  float* slab = p.out + (size_t)split * (size_t)p.M * (size_t)p.N;
  igemm_store_tile<Cfg>(acc, smem, n_block, p.N, nullptr, [&](int row) -> float* {
    const int m = m_block + row;
    return m < p.M ? slab + (size_t)m * p.N + n_block : nullptr;
  });
}


// Grad-input whose sub-pixel phases differ in rows AND taps (k3 s2: 4 : 2 : 2 : 1 taps; the longest phase's tiles alone are as
// long as the whole launch should be): ALL tiles are stream-K.  The k-tiles of every tile of every phase, phase-major, form one
// iteration space cut into `blocks` equal ranges; a range covers any number of tiles — a loop over segments, whose descriptors are
// derived from the iteration index inside the loop (nothing but the index is carried: the loop form costs ~40 spilled registers in
// the segments' prologue / epilogue and none in the k-tile loops).  Only a range's first and last segment can be partial tiles:
// two partial slots per range as before.  Replaces the GEMM + col2im detour where it was only there for balance.
struct SkNPlan {
  int nph, blocks, total;        // sub-pixel phases, workgroups, k-tile iterations of the launch
  int tile0[5], it0[5], kt[4];   // per phase: first tile (arrival-counter index), first iteration, k-tiles per tile; [nph]: totals
  float* parts; int* arrivals;
};
__device__ __forceinline__ int skn_start(int g, const SkNPlan& sk) {
  return __builtin_amdgcn_readfirstlane((int)((uint32_t)g * (uint32_t)sk.total / (uint32_t)sk.blocks));
}
__device__ __forceinline__ int skn_owner(int x, const SkNPlan& sk) {
  return __builtin_amdgcn_readfirstlane((int)((((uint32_t)x + 1u) * (uint32_t)sk.blocks - 1u) / (uint32_t)sk.total));
}
// one segment of a range: which tile, which of its k-tiles, who shares the tile (all wave-uniform, derived from the iteration index)
struct SkNSeg { int py, tin, t_begin, e, kt_begin, nkt, fb, nparts, mt, nt; };
__device__ __forceinline__ SkNSeg skn_segment(int it, int it1, const SkNPlan& sk, int tilesN) {
  SkNSeg s;
  s.py = 0;
  if (sk.nph > 1 && it >= sk.it0[1]) s.py = 1;
  if (sk.nph > 2 && it >= sk.it0[2]) s.py = 2;
  if (sk.nph > 3 && it >= sk.it0[3]) s.py = 3;
  const int KT = sk.kt[s.py], local = it - sk.it0[s.py];
  s.tin = __builtin_amdgcn_readfirstlane(local / KT);                  // tile inside the phase
  s.t_begin = sk.it0[s.py] + s.tin * KT;                               // the tile's iterations: [t_begin, t_begin + KT)
  const int t_end = s.t_begin + KT;
  s.e = it1 < t_end ? it1 : t_end;
  s.kt_begin = it - s.t_begin; s.nkt = s.e - it;
  s.fb = skn_owner(s.t_begin, sk); s.nparts = skn_owner(t_end - 1, sk) - s.fb + 1;
  s.mt = __builtin_amdgcn_readfirstlane(s.tin / tilesN); s.nt = s.tin - s.mt * tilesN;
  return s;
}
// The segment loop exists TWICE, once per role (r04): as one loop holding both roles' bodies the register allocator had to carry the
// union of the producers' loader state and the consumers' accumulators / epilogue temporaries across the back edge — 61 spilled
// VGPRs and 208 bytes of scratch.  Both loops derive the same segments from the same indices and meet at the same
// barriers.
template <class Cfg, bool XF>
__global__ void __launch_bounds__(IG_THREADS, Cfg::MINW) conv_dgrad_skn_kernel(ConvP p, DgradPhases phases, SkNPlan sk) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int rowpix[Cfg::BM];
  const int g = (int)xcd_remap(blockIdx.x, (uint32_t)sk.blocks);
  const int it1 = skn_start(g + 1, sk);
  if (wave_id() >= 4) {
    const int tid = threadIdx.x - IG_LOADERS;
#pragma unroll 1
    for (int it = skn_start(g, sk); it < it1;) {
      const SkNSeg sg = skn_segment(it, it1, sk, p.tilesN);
      const PhaseInfo& f = phases.p[sg.py];
      const int m_block = sg.mt * Cfg::BM, n_block = sg.nt * Cfg::BN;
      for (int r = tid; r < Cfg::BM; r += IG_LOADERS) {
        const int m = m_block + r;
        int pix = -1;
        if (m < f.Mp) {
          uint32_t t, cc, b, aa;
          f.dPHw.divmod((uint32_t)m, t, cc);
          f.dPHh.divmod(t, b, aa);
          pix = ((int)b * p.IH + (int)aa * p.stride + f.ph) * p.IW + (int)cc * p.stride + f.pw;
        }
        rowpix[r] = pix;
      }
      DgradALoader<Cfg::BM, XF> la(p, f, m_block, tid);
      DgradBLoader<Cfg::BN> lb(p, f, n_block, tid);
      if (sg.kt_begin) { la.seek(sg.kt_begin); lb.seek(sg.kt_begin); }
      igemm_produce<Cfg>(la, lb, sg.nkt, smem, tid, ClockStamp{nullptr, 0});
      it = sg.e;
      if (it < it1) lds_barrier();   // the consumers' epilogue staged through the LDS stages / read rowpix: wait for it
    }
    return;
  }
#pragma unroll 1
  for (int it = skn_start(g, sk); it < it1;) {
    const SkNSeg sg = skn_segment(it, it1, sk, p.tilesN);
    const PhaseInfo& f = phases.p[sg.py];
    const int m_block = sg.mt * Cfg::BM, n_block = sg.nt * Cfg::BN;
    {
      f32x16 acc[Cfg::TM][Cfg::TN];
      igemm_consume<Cfg, true, false>(sg.nkt, acc, smem);
      const int t_begin = sg.t_begin;
      if (sk_combine_core<Cfg>(sk.parts, sk.arrivals, sk.blocks, g, sk.tile0[sg.py] + sg.tin, sg.nparts, sg.fb,
                               [&](int blk) { return skn_start(blk, sk) >= t_begin; }, acc))
        igemm_store_tile<Cfg>(acc, smem, n_block, p.N, p.bias, [&](int row) -> float* {
          const int pix = rowpix[row];
          return pix >= 0 ? p.out + (size_t)pix * p.Cin + n_block : nullptr;
        }, p.stat_partial ? p.stat_partial + (size_t)(f.prow0 + sg.mt * Cfg::WAVES_M) * 2 * p.N : nullptr, p.act, p.slope, &p.epi, epi_group_off(p, m_block));
    }
    it = sg.e;
    if (it < it1) lds_barrier();
  }
}

// weight gradient as a stream-K launch: the K = B*OH*OW loops of ALL tiles form the iteration space (a gradient has at most a few
// hundred tiles), the last arrival of a (tile, wave) writes dw itself — with the .grad accumulation as an EPI_ADD on dw — so
// neither slabs nor the slab_reduce pass exist (288-tile gradients of the WGAN-GP critic: one workgroup per tile left 224 CUs
// with one tile and 32 with two).
template <class Cfg, bool XFA, bool XFB, bool TAB, int PS>
__device__ __forceinline__ void wgrad_sk_segment(const ConvP& p, const SkPlan& sk, const SkSeg& sg, float* smem, int b) {
  const int mt = __builtin_amdgcn_readfirstlane(sg.tile / p.tilesN), nt = sg.tile - mt * p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  if (wave_id() >= 4) {
    const int tid = threadIdx.x - IG_LOADERS;
    WgradALoader<Cfg::BM, XFA> la(p, m_block, sg.kt_begin, tid);
    WgradBLoader<Cfg::BN, XFB, TAB> lb(p, n_block, sg.kt_begin, tid);
    igemm_produce<Cfg>(la, lb, sg.nkt, smem, tid, ClockStamp{nullptr, 0});
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  if constexpr (PS) igemm_consume_padskip<Cfg, false, false, PS>(sg.nkt, acc, smem, ClockStamp{nullptr, 0}, wgrad_padskip<Cfg>(p, n_block, sg.kt_begin));
  else igemm_consume<Cfg, false, false>(sg.nkt, acc, smem);
  if (sk_combine<Cfg>(sk, sg, acc, b))
    igemm_store_tile<Cfg>(acc, smem, n_block, p.N, nullptr, [&](int row) -> float* {
      const int m = m_block + row;
      return m < p.M ? p.out + (size_t)m * p.N + n_block : nullptr;
    }, nullptr, PCG_ACT_NONE, 0.f, &p.epi);
}
// PS: as in conv_wgrad_kernel; the permuted block id stands in for blockIdx.x everywhere (ranges, partial slots, arrival counters)
template <class Cfg, bool XFA, bool XFB, bool TAB = false, int PS = 0>
__global__ void __launch_bounds__(IG_THREADS, 4) conv_wgrad_sk_kernel(ConvP p, SkPlan sk, int pair_xor) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  SkSeg s0, s1{};
  const int b = PS ? (int)wgrad_pair_block(blockIdx.x, gridDim.x, pair_xor) : (int)blockIdx.x;
  const int nseg = sk_segments(sk, s0, s1, b);
  wgrad_sk_segment<Cfg, XFA, XFB, TAB, PS>(p, sk, s0, smem, b);
  if (nseg == 1) return;
  lds_barrier();
  wgrad_sk_segment<Cfg, XFA, XFB, TAB, PS>(p, sk, s1, smem, b);
}

// 64x192 tile of the weight gradient (Cout <= 64, N = KH*KW*Cin a multiple of 192): the same pipeline with the 192-column B loader
using Cfg64x192 = TileCfg<64, 192, 2, 2>;
template <class Cfg, bool TAB = false>
__global__ void __launch_bounds__(IG_THREADS, 4) conv_wgrad192_kernel(ConvP p, int ktiles_total, int ktiles_per_split, int tiles,
                                                                      int slice_major) {
  static_assert(Cfg::BM == 64 && Cfg::BN == 192, "the 192-column weight-gradient tile");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  prio_entry(p);
  uint32_t tile, split;
  if (slice_major) {
    const uint32_t l = xcd_remap(blockIdx.x, gridDim.x);
    split = l / (uint32_t)tiles; tile = l - split * (uint32_t)tiles;
  } else {
    tile = xcd_remap(blockIdx.x, gridDim.x); split = blockIdx.y;
  }
  const int mt = tile / p.tilesN, nt = tile % p.tilesN;
  const int m_block = mt * Cfg::BM, n_block = nt * Cfg::BN;
  const int kt_begin = split * ktiles_per_split;
  int ktiles = ktiles_total - kt_begin;
  if (ktiles > ktiles_per_split) ktiles = ktiles_per_split;
  if (wave_id() >= 4) {
    const int tid = threadIdx.x - IG_LOADERS;
    WgradALoader<Cfg::BM, false> la(p, m_block, kt_begin, tid);
    WgradBLoader192<TAB> lb(p, n_block, kt_begin, tid);
    igemm_produce<Cfg>(la, lb, ktiles, smem, tid);
    return;
  }
  f32x16 acc[Cfg::TM][Cfg::TN];
  igemm_consume<Cfg, false, false>(ktiles, acc, smem, ClockStamp{p.stamps, p.stamp_slots});
  prio_epilogue(p);
  float* slab = p.out + (size_t)split * (size_t)p.M * (size_t)p.N;
  igemm_store_tile<Cfg>(acc, smem, n_block, p.N, nullptr, [&](int row) -> float* {
    const int m = m_block + row;
    return m < p.M ? slab + (size_t)m * p.N + n_block : nullptr;
  });
}

// col2im for the "one GEMM + scatter" form of the grad-input (see dgrad_as_gemm): dx[b,ih,iw,ci] = bias[ci] + sum over the taps
// (kh,kw) that reach (ih,iw) of dcol[b,oh,ow][(kh,kw,ci)], taps added in (kh,kw) order.  Every dcol element is read once.
__global__ void __launch_bounds__(256) col2im_kernel(const float4* __restrict__ dcol, float4* __restrict__ dx, const float* __restrict__ bias,
                                                     int B, int IH, int IW, int CQ, int OH, int OW, int KH, int KW, int stride, int pad,
                                                     FastDiv dCQ, FastDiv dIW, FastDiv dIH, int act, float neg) {
  const uint32_t total = (uint32_t)B * IH * IW * CQ;
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    uint32_t pix, cq, t, iw, b, ih;
    dCQ.divmod(idx, pix, cq);
    dIW.divmod(pix, t, iw);
    dIH.divmod(t, b, ih);
    float4 acc = bias ? *reinterpret_cast<const float4*>(bias + 4 * cq) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kh = 0; kh < KH; ++kh) {
      const int th = (int)ih + pad - kh;
      if (th < 0 || th % stride) continue;
      const int oh = th / stride;
      if (oh >= OH) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int tw = (int)iw + pad - kw;
        if (tw < 0 || tw % stride) continue;
        const int ow = tw / stride;
        if (ow >= OW) continue;
        const float4 v = dcol[((size_t)(((int)b * OH + oh) * OW + ow) * (KH * KW) + (kh * KW + kw)) * CQ + cq];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    if (act != PCG_ACT_NONE) {
      acc.x = act_neg_scale(acc.x, neg); acc.y = act_neg_scale(acc.y, neg); acc.z = act_neg_scale(acc.z, neg); acc.w = act_neg_scale(acc.w, neg);
    }
    dx[idx] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
using Cfg128x128 = TileCfg<128, 128, 2, 2>;
#ifndef PCG_PAD_CLIP_DEFAULT
#define PCG_PAD_CLIP_DEFAULT 1
#endif
#ifndef PCG_TILE64_SWZ
#define PCG_TILE64_SWZ 1     // 128x64 tiles: swizzled unpadded LDS images, three workgroups per CU (0: the r01 layout, two per CU)
#endif
using Cfg128x64P = TileCfg<128, 64, 2, 2>;                 // padded images, two workgroups per CU, two k-tiles of gathers in flight
#if PCG_TILE64_SWZ
using Cfg128x64 = TileCfg<128, 64, 2, 2, true, 6, 1>;      // measured r02: 3x3 s1 64->64 forward 97.7 -> 101.1, grad-input 106.0 -> 111.5
#else                                                      // TFLOP/s; the k4 s2 grad-input (four interleaved phases, K = 512) LOSES
using Cfg128x64 = Cfg128x64P;                              // 9 % (105.7 -> 96.6) and therefore keeps the padded config
#endif

// The bf16-operand twin of a tile configuration (pcg_conv_precision_set): same tile, prefetch depth and launch bounds,
// so the same plans, grids and workspace.  Its LDS images are its own (igemm_core.h), so SWZ does not apply.
template <class C>
using Bf16Twin = TileCfg<C::BM, C::BN, C::WAVES_M, C::WAVES_N, false, C::MINW, C::PF, true>;

// (r04: 192x64 tiles — four consumer waves of 96x32, two workgroups per CU, 1.5x the MFMAs per workgroup — were built and measured:
//  bit-identical results, no gain: 3x3 64->64 forward 0.4867 -> 0.4943 ms, its grad-input 0.4969 -> 0.5227, D2's k4 s2 grad-input
//  0.2875 -> 0.2877.  The epilogue is per-OUTPUT work, not per-workgroup work; only the ~4 us entry is amortised.  Removed)

int check_geom(const pcg_conv_geom* g) {
  PCG_REQUIRE(g != nullptr, "conv geometry is null");
  PCG_REQUIRE(g->B > 0 && g->IH > 0 && g->IW > 0 && g->Cin > 0 && g->OH > 0 && g->OW > 0 && g->Cout > 0,
              "conv geometry: non-positive extent");
  PCG_REQUIRE(g->KH > 0 && g->KW > 0 && g->stride > 0 && g->pad >= 0, "conv geometry: bad kernel/stride/pad");
  PCG_REQUIRE(g->OH == (g->IH + 2 * g->pad - g->KH) / g->stride + 1 && g->OW == (g->IW + 2 * g->pad - g->KW) / g->stride + 1,
              "conv geometry: OH/OW inconsistent with IH/IW, kernel %dx%d stride %d pad %d", g->KH, g->KW, g->stride, g->pad);
  PCG_REQUIRE((int64_t)g->B * g->IH * g->IW * g->Cin * 4 < (1ll << 31) && (int64_t)g->B * g->OH * g->OW * g->Cout * 4 < (1ll << 31) &&
                  (int64_t)g->Cout * g->KH * g->KW * g->Cin * 4 < (1ll << 31),
              "conv geometry: an operand tensor reaches 2 GiB (32-bit buffer offsets); split the batch");
  PCG_REQUIRE(g->KH * g->KW <= 32, "conv geometry: more than 32 taps (%dx%d) unsupported", g->KH, g->KW);
  return PCG_OK;
}

// Tuning switches for A/B measurements in ONE process (pcg_tune_set; scripts/conv_microbench.py --ab): -1 = the built-in choice.
struct Tune { int edge_prio = -1, dgrad_swz3 = -1, wgrad_rounds = -1, korder = -1, wgrad_order = -1, dgrad_interleave = -1, fwd_splits = -1, stream_k = -1, sk_blocks = -1, dgrad_gemm = -1, t64 = -1, wgrad_pixtab = -1, pad_clip = -1, pad_clip_dgrad = -1, wgrad_padskip = -1; unsigned long long* stamps = nullptr; int stamp_slots = 0; };
Tune g_tune;

ConvP make_params(const pcg_conv_geom* g) {
  ConvP p{};
  static const int korder_env = getenv("PCG_KORDER") ? atoi(getenv("PCG_KORDER")) : 1;
  p.korder = g_tune.korder >= 0 ? g_tune.korder : korder_env;
  // default 2: the epilogue at priority 3, the entry left alone (measured r04, CounteRGAN step, one process, interleaved:
  // 0: 27.15 ms, 2: 26.49, 3: 27.62 — raising the entry as well lets every new workgroup's set-up cut into the running loops)
  static const int edge_env = getenv("PCG_EDGE_PRIO") ? atoi(getenv("PCG_EDGE_PRIO")) : 2;
  p.edge_prio = g_tune.edge_prio >= 0 ? g_tune.edge_prio : edge_env;
  p.stamps = g_tune.stamps; p.stamp_slots = g_tune.stamp_slots;
  p.B = g->B; p.IH = g->IH; p.IW = g->IW; p.Cin = g->Cin; p.OH = g->OH; p.OW = g->OW; p.Cout = g->Cout;
  p.KH = g->KH; p.KW = g->KW; p.stride = g->stride; p.pad = g->pad;
  p.dOW = FastDiv((uint32_t)g->OW);
  p.dOH = FastDiv((uint32_t)g->OH);
  p.dOHW = FastDiv((uint32_t)(g->OH * g->OW));
  p.x_bytes = (uint32_t)((int64_t)g->B * g->IH * g->IW * g->Cin * 4);
  p.dy_bytes = (uint32_t)((int64_t)g->B * g->OH * g->OW * g->Cout * 4);
  p.w_bytes = (uint32_t)((int64_t)g->Cout * g->KH * g->KW * g->Cin * 4);
  return p;
}

// validate an input transform for an operand with C channels and put it into the kernel parameters
int check_xform(const char* who, const pcg_in_xform* xf, int C) {
  if (!xf || !xf->scale) return PCG_OK;
  PCG_REQUIRE(xf->shift != nullptr, "%s: input transform without shift", who);
  PCG_REQUIRE(xf->act == PCG_ACT_NONE || xf->act == PCG_ACT_RELU || xf->act == PCG_ACT_LRELU,
              "%s: input transform activation %d is not none / ReLU / LeakyReLU", who, xf->act);
  PCG_REQUIRE(C % 4 == 0 && (((uintptr_t)xf->scale | (uintptr_t)xf->shift) & 15) == 0,
              "%s: input transform needs a channel count %% 4 == 0 and 16-byte aligned scale / shift", who);
  return PCG_OK;
}
int set_xform(const char* who, const pcg_in_xform* xf, int C, ConvP* p) {
  if (!xf || !xf->scale) return PCG_OK;
  if (int e = check_xform(who, xf, C)) return e;
  p->in_sc = xf->scale; p->in_sh = xf->shift; p->in_neg = act_neg_of(xf->act, xf->slope); p->in_c_bytes = (uint32_t)C * 4u;
  return PCG_OK;
}

template <class Cfg, bool AK, bool BK_>
constexpr size_t smem_bytes() {
  constexpr int a = igemm_smem_floats<Cfg, AK, BK_>(), b = epilogue_smem_floats<Cfg>();
  return sizeof(float) * (size_t)(a > b ? a : b);
}

template <class K>
int set_smem(K kernel, size_t bytes) {
  // > 64 KB of dynamic LDS needs the opt-in attribute; harmless otherwise
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(max dynamic LDS=%zu): %s", bytes, hipGetErrorString(e)); return PCG_ERR_LAUNCH; }
  return PCG_OK;
}

// ---- stream-K scratch: caller-owned, registered per stream (pcg_conv_set_scratch) --------------------------------------
constexpr int SK_MAX_BLOCKS = 512, SK_MAX_TILES = 4096;
constexpr size_t SK_PARTS_BYTES = (size_t)2 * SK_MAX_BLOCKS * 128 * 128 * sizeof(float);
constexpr size_t SK_ARRIVALS_BYTES = (size_t)SK_MAX_TILES * 4 * sizeof(int);
// keyed by (device, stream): the default stream has handle 0 on EVERY device, so the handle alone would let a second GPU's
// registration overwrite the first one's
struct SkScratch { int device; hipStream_t stream; float* parts; int* arrivals; };
SkScratch g_sk_scratch[64];
int g_sk_scratch_n = 0;
std::mutex g_sk_mutex;
int current_device() { int d = 0; return hipGetDevice(&d) == hipSuccess ? d : 0; }
bool sk_scratch_of(hipStream_t s, SkPlan* sk) {
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_sk_mutex);
  for (int i = 0; i < g_sk_scratch_n; ++i)
    if (g_sk_scratch[i].stream == s && g_sk_scratch[i].device == dev) {
      if (sk) { sk->parts = g_sk_scratch[i].parts; sk->arrivals = g_sk_scratch[i].arrivals; }
      return true;
    }
  return false;
}
// ---- pixel descriptor tables (conv_pixtab.h): caller-owned device memory, registered per (device, geometry without B and Cout) ----
struct PixTabReg { int device, IH, IW, OH, OW, stride, pad, KH, KW, Cin; const uint32_t* tab; };
constexpr int PIXTAB_MAX = 256;
PixTabReg g_pixtab[PIXTAB_MAX];
int g_pixtab_n = 0;
std::mutex g_pixtab_mutex;
bool pixtab_same(const PixTabReg& r, int dev, const pcg_conv_geom* g) {
  return r.device == dev && r.IH == g->IH && r.IW == g->IW && r.OH == g->OH && r.OW == g->OW && r.stride == g->stride && r.pad == g->pad &&
         r.KH == g->KH && r.KW == g->KW && r.Cin == g->Cin;
}
// the table the weight gradient of `g` reads on the current device, or nullptr (none registered, or switched off): the loaders that
// derive the pixels per k-tile.  On by default (DCGAN step 10.01 -> 9.89 ms, same process, three runs);
// pcg_tune_set("wgrad_pixtab", 0) or PCG_WGRAD_PIXTAB=0 for the A/B.
const uint32_t* pixtab_of(const pcg_conv_geom* g) {
  static const int env = getenv("PCG_WGRAD_PIXTAB") ? atoi(getenv("PCG_WGRAD_PIXTAB")) : 1;
  if (!(g_tune.wgrad_pixtab >= 0 ? g_tune.wgrad_pixtab : env)) return nullptr;
  std::lock_guard<std::mutex> lock(g_pixtab_mutex);
  if (g_pixtab_n == 0) return nullptr;
  const int dev = current_device();
  for (int i = 0; i < g_pixtab_n; ++i)
    if (pixtab_same(g_pixtab[i], dev, g)) return g_pixtab[i].tab;
  return nullptr;
}
// ---- tile descriptor tables of the clipped path (conv_cliptab.h): caller-owned device memory, registered per (device, OH, OW) ----
struct ClipTabReg { int device, OH, OW; const uint32_t* tab; };
constexpr int CLIPTAB_MAX = 64;
ClipTabReg g_cliptab[CLIPTAB_MAX];
int g_cliptab_n = 0;
std::mutex g_clip_mutex;
// 0: off.  1: the launches the schedule model takes.  2 / 3 / 4 (measurements, tests): every eligible launch, tiles long first / short
// first / in pairs, at today's tile height; 5 / 6 / 7: the same with 64-row tiles where the forward kernel has them.
// pcg_tune_set("pad_clip", v) or PCG_PAD_CLIP=v.
int clip_mode() {
  static const int env = getenv("PCG_PAD_CLIP") ? atoi(getenv("PCG_PAD_CLIP")) : PCG_PAD_CLIP_DEFAULT;
  return g_tune.pad_clip >= 0 ? g_tune.pad_clip : env;
}
// What switch 1 of pad_clip does with grad-input launches.  1 (default): those the schedule model takes.  0: none, forward-kernel
// launches only (the A/B's other side and an escape hatch).  2 (measurements): every eligible one, in the model's best order.  The
// forced modes 2-7 of pad_clip are not affected.  pcg_tune_set("pad_clip_dgrad", v) or PCG_PAD_CLIP_DGRAD=v.
int clip_dgrad_mode() {
  static const int env0 = getenv("PCG_PAD_CLIP_DGRAD") ? atoi(getenv("PCG_PAD_CLIP_DGRAD")) : 1;
  static const int env = env0 >= 0 && env0 <= 2 ? env0 : 1;       // (anything else in the environment: the default)
  return g_tune.pad_clip_dgrad >= 0 ? g_tune.pad_clip_dgrad : env;
}
const uint32_t* cliptab_of(const pcg_conv_geom* g) {
  std::lock_guard<std::mutex> lock(g_clip_mutex);
  if (g_cliptab_n == 0) return nullptr;
  const int dev = current_device();
  for (int i = 0; i < g_cliptab_n; ++i)
    if (g_cliptab[i].device == dev && g_cliptab[i].OH == g->OH && g_cliptab[i].OW == g->OW) return g_cliptab[i].tab;
  return nullptr;
}
// One eligible launch as the schedule model sees it, and what the model says.  form 0: forward kernel, 1: grad-input kernel (four equal
// phases, `interleave`d in a 1-D grid or one per blockIdx.y).  bm0: today's tile height; the forward kernel's 128-column tiles may also
// run 64 rows high (`alt64`), at 254 us against 479 / 2 per tile (D4 forward).
struct ClipShape { int form, OH, OW, B, tilesN, interleave, bm0, alt64; };
struct ClipPlan { bool take; int order, bm; double ratio; };   // ratio: predicted time of the chosen clipped launch / today's
constexpr double CLIP_UNIT64 = 254.0 / (479.0 / 2.0) / 2.0;    // a 64-row tile's k-tile in units of a 128-row tile's
constexpr double CLIP_TAKE = 0.95;
// The clipped grad-input kernel's k-tile in units of today's: the median, over D3 / D4 at batch 512 and 1024 and the three orders, of
// (clipped / today's time) / (the model's ratio without this factor) — 0.927 .. 0.984, profiles/dgrad_clip_ab.json.  It was 1.21 (D4:
// 0.2514 -> 0.3053 ms) while the tap walk's early-return chain kept both loaders in private memory, 304-352 bytes read and written in
// every k-tile of the producers' loop; with the walk in registers (conv_loaders.h, DgradTapIterT<true>::advance) the clipped kernel is
// the faster one at equal work.
constexpr double CLIP_DGRAD_COST = 0.98;
// The grad-input form is taken wherever the prediction, unit cost included, is no loss — not only below CLIP_TAKE: the model saw no round
// to save in D3 / D4 at either batch (ratio 1.000 in every order) where the clipped launches measured 2-7 % faster, and the DCGAN step
// gains 0.035 ms with CLIP_TAKE and 0.137 ms with every grad-input launch clipped (profiles/dgrad_clip_ab.json).  Only launches of at
// least one round of 512 workgroups, the smallest measured (D4 at batch 512); below that nothing was measured and the launch stays.
// With a unit cost below 1 the ratio test is at present VACUOUS for this form — the model's best ratio never exceeds 1.0, so 0.98 times it
// never exceeds CLIP_TAKE_DGRAD — and the rule comes down to "at least 512 workgroups"; it is kept so that a re-measured cost above 1
// decides again.  Launches of 512 workgroups or more that are not whole rounds were not measured.
constexpr double CLIP_TAKE_DGRAD = 1.0;
constexpr int CLIP_DGRAD_MIN_TILES = 512;
double clip_predict(const ClipShape& c, int bm, int order) {     // order < 0: today's launch (every tile iterates every tap)
  const int npos = c.OH * c.OW, tpp = c.B / bm, tilesM = npos * tpp, nph = c.form ? 4 : 1;
  const int per = (c.form && c.interleave ? nph : 1) * c.tilesN, gx = tilesM * per, gy = c.form && !c.interleave ? nph : 1;
  std::vector<uint32_t> tab(cliptab_words(c.OH, c.OW));
  cliptab_build(c.OH, c.OW, tab.data());
  std::vector<int> len((size_t)gx * gy);
  for (int y = 0; y < gy; ++y)
    for (int b = 0; b < gx; ++b) {
      uint32_t within, idx;
      clip_block_tile((uint32_t)b, (uint32_t)per, (uint32_t)tilesM, order < 0 ? 0 : order, gy > 1, (uint32_t)y, within, idx);
      const int py = c.form ? (c.interleave ? (int)(within % (uint32_t)nph) : y) : 0;
      len[(size_t)y * gx + b] = order < 0 ? (c.form ? 4 : 16) : clip_desc_taps(tab[(size_t)(c.form ? 1 + py : 0) * npos + idx / (uint32_t)tpp]);
    }
  return clip_sched_model(len.data(), (int)len.size()) * (bm == 64 ? CLIP_UNIT64 : 1.0) * (c.form && order >= 0 ? CLIP_DGRAD_COST : 1.0);
}
ClipPlan plan_clip(const ClipShape& c) {
  static std::map<std::array<int, 9>, ClipPlan> cache;
  const int mode = clip_mode();
  const std::array<int, 9> key = {c.form, c.OH, c.OW, c.B, c.tilesN, c.interleave, c.bm0, c.alt64, mode};
  std::lock_guard<std::mutex> lock(g_clip_mutex);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  ClipPlan best{false, 0, c.bm0, 1.0};
  const double t0 = clip_predict(c, c.B % c.bm0 ? 64 : c.bm0, -1);     // (B % bm0 != 0: forced 64-row modes only)
  if (mode >= 2) {
    const bool rows64 = mode >= 5 && c.alt64 && c.B % 64 == 0 && (c.OH * c.OW * (c.B / 64)) % 8 == 0;
    best = ClipPlan{true, (mode - 2) % 3, rows64 ? 64 : c.bm0, 0.0};
    best.ratio = clip_predict(c, best.bm, best.order) / t0;
  } else {
    for (int h = 0; h < 2; ++h) {
      const int bm = h ? 64 : 128;
      if (bm != c.bm0 && !(bm == 64 && c.alt64)) continue;
      if (c.B % bm || (c.OH * c.OW * (c.B / bm)) % 8) continue;
      for (int order = 0; order < 3; ++order) {
        const double r = clip_predict(c, bm, order) / t0;
        if (r < best.ratio - 1e-9) best = ClipPlan{false, order, bm, r};
      }
    }
    const int blocks = c.OH * c.OW * (c.B / best.bm) * c.tilesN * (c.form ? 4 : 1);
    best.take = c.form ? best.ratio <= CLIP_TAKE_DGRAD + 1e-9 && blocks >= CLIP_DGRAD_MIN_TILES : best.ratio <= CLIP_TAKE + 1e-9;
  }
  cache[key] = best;
  return best;
}
// geometry and batch alone (what the query reports); the launch also needs one group's images to be whole tiles, a table and the
// plain data-parallel form
bool clip_shape_ok(const pcg_conv_geom* g, int groups, int bm) {
  return clip_geom_ok(g->IH, g->IW, g->OH, g->OW, g->stride, g->pad, g->KH, g->KW) && groups >= 1 && g->B % groups == 0 &&
         (g->B / groups) % bm == 0 && (g->OH * g->OW * (g->B / bm)) % 8 == 0;
}

int sk_mode() {      // 0 off, 1 where the model sees > 10 % to gain (default), 2 wherever the form is valid (tests, scans)
  static const int env = getenv("PCG_STREAM_K") ? atoi(getenv("PCG_STREAM_K")) : 1;
  return g_tune.stream_k >= 0 ? g_tune.stream_k : env;
}
// Decide between whole rounds + stream-K remainder and the plain launch.  Times in us from the r03 stamps of the 128x128 kernels:
// a k-tile takes a workgroup 3.5 us when two share a CU (the matrix pipe's rate) and 2.2 us when it has the CU alone; a whole
// tile costs ~6 us outside its main loop, a stream-K segment ~12 (partial tile out, counter, the next segment's cold start); the
// last arrival reads ~1.5 us per partial tile.  Checked against scripts/probes/streamk_scan.py: the model takes the launches
// that gained 7-24 % there and leaves the K = 512 grad-input GEMMs (16 k-tiles per tile: no gain) data-parallel.
bool plan_sk_shape(int tiles, int ktiles, SkPlan* sk) {       // the decision alone (no scratch, no stream): host logic, CPU-testable
  const int mode = sk_mode();
  if (mode == 3) {                       // diagnostic: every tile data-parallel, but through the stream-K kernels (their cost as such)
    sk->dp_tiles = tiles; sk->sk_tiles = 0; sk->sk_blocks = 0; sk->ktiles = ktiles;
    return true;
  }
  if (mode == 0 || ktiles < 8) return false;
  const int dp = tiles / 512 * 512, r = tiles - dp;
  if (r == 0 || r > SK_MAX_TILES || (int64_t)r * ktiles * 512 >= (1ll << 31)) return false;
  const double t_dp = (r <= 256 ? 2.2 : 3.5) * ktiles + 6.0;
  double best = 1e30;
  int bg = 0;
  for (int G = 512; G >= 64; G >>= 1) {
    if (g_tune.sk_blocks > 0 && G != g_tune.sk_blocks) continue;
    if (G < r) break;
    const int it = ceil_div(r * ktiles, G);
    if (it < 4) continue;
    const int parts = ceil_div(ktiles, it) + 1;
    if (parts > 8) continue;
    const double t = it * (G == 512 ? 3.5 : 2.2) + 2 * 12.0 + 3.0 + 1.5 * parts;
    if (t < best) { best = t; bg = G; }
  }
  if (!bg || (mode == 1 && best > 0.9 * t_dp)) return false;
  sk->dp_tiles = dp; sk->sk_tiles = r; sk->sk_blocks = bg; sk->ktiles = ktiles;
  return true;
}
bool plan_sk(int tiles, int ktiles, hipStream_t s, SkPlan* sk) { return plan_sk_shape(tiles, ktiles, sk) && sk_scratch_of(s, sk); }
// workspace queries carry no stream: they assume scratch when ANY stream of this device has it (an upper bound on what a launch
// may need; a launch on a stream without scratch plans with stream_has_sk and falls back to the plain forms)
bool have_sk_scratch() {
  if (sk_mode() == 0) return false;
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_sk_mutex);
  for (int i = 0; i < g_sk_scratch_n; ++i) if (g_sk_scratch[i].device == dev) return true;
  return false;
}
int stream_has_sk(hipStream_t s) { return sk_mode() != 0 && sk_scratch_of(s, nullptr) ? 1 : 0; }

template <class Cfg, bool XF>
int launch_fwd_x(ConvP p, int splits, hipStream_t s) {
  p.tilesN = ceil_div(p.N, Cfg::BN);
  const int tilesM = ceil_div(p.M, Cfg::BM);
  constexpr size_t smem = smem_bytes<Cfg, true, true>();
  if constexpr (Cfg::BM == 128 && Cfg::BN == 128) {
    SkPlan sk{};
    if (splits == 1 && plan_sk(tilesM * p.tilesN, p.ktiles, s, &sk)) {
      static int once_sk = set_smem(conv_fwd_sk_kernel<Cfg, XF>, smem);
      if (once_sk != PCG_OK) return once_sk;
      hipLaunchKernelGGL((conv_fwd_sk_kernel<Cfg, XF>), dim3((unsigned)(sk.dp_tiles + sk.sk_blocks)), dim3(IG_THREADS), smem, s, p, sk);
      return launch_status("conv_fwd_sk_kernel");
    }
  }
  static int once = set_smem(conv_fwd_kernel<Cfg, XF>, smem);
  if (once != PCG_OK) return once;
  hipLaunchKernelGGL((conv_fwd_kernel<Cfg, XF>), dim3((unsigned)tilesM * p.tilesN, splits), dim3(IG_THREADS), smem, s, p);
  return launch_status("conv_fwd_kernel");
}
template <class Cfg>
int launch_fwd(const ConvP& p, int splits, hipStream_t s) {
  if (conv_bf16()) return p.in_sc ? launch_fwd_x<Bf16Twin<Cfg>, true>(p, splits, s) : launch_fwd_x<Bf16Twin<Cfg>, false>(p, splits, s);
  return p.in_sc ? launch_fwd_x<Cfg, true>(p, splits, s) : launch_fwd_x<Cfg, false>(p, splits, s);
}

// the clipped launch (ConvP::cliptab set by clip_fwd_setup): a 1-D grid of whole position-major tiles
template <class Cfg, bool XF>
int launch_fwd_clip_x(ConvP p, hipStream_t s) {
  p.tilesN = ceil_div(p.N, Cfg::BN);
  constexpr size_t smem = smem_bytes<Cfg, true, true>();
  static int once = set_smem(conv_fwd_kernel<Cfg, XF, true>, smem);
  if (once != PCG_OK) return once;
  hipLaunchKernelGGL((conv_fwd_kernel<Cfg, XF, true>), dim3((unsigned)(p.clip_npos * p.clip_tpp * p.tilesN)), dim3(IG_THREADS), smem, s, p);
  return launch_status("conv_fwd_kernel (clipped)");
}
template <class Cfg>
int launch_fwd_clip(const ConvP& p, hipStream_t s) { return p.in_sc ? launch_fwd_clip_x<Cfg, true>(p, s) : launch_fwd_clip_x<Cfg, false>(p, s); }

// Forward split-K: when M*N gives far fewer tiles than the chip has CUs and K is long (small-batch layers with big weights:
// the WGAN-GP critic's conv3 / 8192->1024 Linear, the generator's 1x1 -> 4x4 ConvT backward), K is cut into slabs that are
// summed in slab order by slab_reduce — the same deterministic scheme as the weight gradient.
struct FwdPlan { int splits, ktiles_per_split; };
FwdPlan plan_fwd(const pcg_conv_geom* g, int have_sk = -1) {
  if (have_sk < 0) have_sk = have_sk_scratch() ? 1 : 0;
  const int M = g->B * g->OH * g->OW, N = g->Cout;
  const int tiles = ceil_div(M, 128) * ceil_div(N, N > 64 ? 128 : 64);
  const int ktiles = g->KH * g->KW * ceil_div(g->Cin, IG_BK);
  FwdPlan f{1, ktiles};
  if (g_tune.fwd_splits > 0) {               // A/B override (pcg_tune_set("fwd_splits", s)): s K-slices whatever the shape
    f.ktiles_per_split = ceil_div(ktiles, g_tune.fwd_splits);
    f.splits = ceil_div(ktiles, f.ktiles_per_split);
    return f;
  }
  if (tiles > 256 && tiles < 448 && ktiles >= 32 && !have_sk) {     // (stream-K takes these when it has scratch)
    // a little over one block per CU (288 tiles: 32 CUs get two full-K blocks, the others one — the critic's conv2 at batch 256
    // ran at 73 TFLOP/s): a few K-slices bring the blocks per CU to ceil(tiles*s/256)/s.  Each slice also costs a slab of M*N
    // floats written and read: measured r03 (scripts/probes/fwd_splits_scan.py, 288 tiles x 72 k-tiles) 1: 283, 2: 241, 3: 221,
    // 4: 256 us — the slab term is worth ~0.1 of a block per slice.
    int best = 1;
    double bc = 2.0;
    for (int s = 2; s <= 4; ++s) {
      const double c = (double)ceil_div(tiles * s, 256) / s + 0.1 * s;
      if (c < bc - 1e-9) { bc = c; best = s; }
    }
    f.ktiles_per_split = ceil_div(ktiles, best);
    f.splits = ceil_div(ktiles, f.ktiles_per_split);
    return f;
  }
  if (tiles > 96 || ktiles < 32) return f;
  int splits = ceil_div(tiles >= 48 ? 512 : 384, tiles);     // (64 tiles x 144 k-tiles, r03 scan: 6 slices 115 us, 8 slices 101)
  if (splits > ktiles / 8) splits = ktiles / 8;
  if (splits < 2) return f;
  f.ktiles_per_split = ceil_div(ktiles, splits);
  f.splits = ceil_div(ktiles, f.ktiles_per_split);
  return f;
}

// every tile stream-K over phases of different length (conv_dgrad_skn_kernel): the decision alone
bool plan_skn_shape(const DgradPhases& ph, int nphases, int BM, int tilesN, int Cout, SkNPlan* sn) {
  if (sk_mode() == 0 || nphases < 2) return false;
  sn->nph = nphases;
  bool ok = true;
  int tiles = 0, total = 0, ktmax = 0;
  for (int i = 0; i < nphases && ok; ++i) {
    const int kt = ph.p[i].nth * ph.p[i].ntw * ceil_div(Cout, IG_BK), t = ceil_div(ph.p[i].Mp, BM) * tilesN;
    ok = ph.p[i].nth > 0 && ph.p[i].ntw > 0 && ph.p[i].Mp > 0 && kt > 0;
    sn->tile0[i] = tiles; sn->it0[i] = total; sn->kt[i] = kt;
    tiles += t; total += t * kt;
    if (kt > ktmax) ktmax = kt;
  }
  sn->tile0[nphases] = tiles; sn->it0[nphases] = total;
  int blocks = total / 512 >= 16 ? 512 : 256;
  if (g_tune.sk_blocks > 0) blocks = g_tune.sk_blocks;
  // (measured: pays where the tiles are long — 72-79 k-tiles on average: 309 -> 201 and 363 -> 237 us — and loses where they
  //  are short — 38 on average, 13x13 -> 6x6 at 512 channels: 236 -> 261 us: ~2.7 segments per range, each with its fixed cost)
  ok = ok && tiles <= SK_MAX_TILES && blocks <= SK_MAX_BLOCKS && total / blocks >= 8 && (int64_t)total * blocks < (1ll << 31) &&
       ktmax <= 8 * (total / blocks) && (sk_mode() == 2 || g_tune.sk_blocks > 0 || total >= 48 * tiles);
  sn->blocks = blocks; sn->total = total;
  return ok;
}

// equal phases share a 1-D grid, neighbours in launch order — only for small weight tensors: interleaved phases keep ALL phases' weight
// slices live in an XCD's 4 MB L2 at once (measured: WGAN-GP's 8 MB ConvT weights ran 20 % slower interleaved, DCGAN's 0.5 MB D2 / G4
// layers 1-3 % faster)
bool dgrad_interleaved(uint32_t w_bytes, const DgradPhases& ph, int nphases) {
  static const int il_env0 = getenv("PCG_DGRAD_INTERLEAVE") ? atoi(getenv("PCG_DGRAD_INTERLEAVE")) : 1;   // A/B switch
  const int il_env = g_tune.dgrad_interleave >= 0 ? g_tune.dgrad_interleave : il_env0;
  bool same = nphases > 1 && il_env && w_bytes <= (1u << 20);
  for (int i = 1; i < nphases; ++i) same = same && ph.p[i].Mp == ph.p[0].Mp;
  return same;
}

template <class Cfg, bool XF>
int launch_dgrad_x(ConvP p, const DgradPhases& ph, int nphases, int maxMp, hipStream_t s) {
  p.tilesN = ceil_div(p.N, Cfg::BN);
  const int tilesM = ceil_div(maxMp, Cfg::BM);
  constexpr size_t smem = smem_bytes<Cfg, true, false>();
  if constexpr (!Cfg::BF16) {
    if (p.cliptab) {       // the clipped launch (clip_dgrad_setup): whole position-major tiles of four equal phases
      static int once_c = set_smem(conv_dgrad_kernel<Cfg, XF, true>, smem);
      if (once_c != PCG_OK) return once_c;
      DgradPhases phc = ph;
      phc.interleave = dgrad_interleaved(p.w_bytes, ph, nphases) ? nphases : 0;
      const unsigned tiles = (unsigned)(p.clip_npos * p.clip_tpp * p.tilesN);
      hipLaunchKernelGGL((conv_dgrad_kernel<Cfg, XF, true>), phc.interleave ? dim3(tiles * nphases) : dim3(tiles, nphases), dim3(IG_THREADS), smem, s, p, phc);
      return launch_status("conv_dgrad_kernel (clipped)");
    }
  }
  if constexpr (Cfg::BM == 128 && Cfg::BN == 128) {
    bool uniform = true;
    for (int i = 0; i < nphases; ++i)
      uniform = uniform && ph.p[i].Mp == ph.p[0].Mp && ph.p[i].nth * ph.p[i].ntw == ph.p[0].nth * ph.p[0].ntw && ph.p[i].nth > 0 && ph.p[i].ntw > 0;
    if (!uniform && nphases > 1 && sk_mode() != 0) {
      // phases of different length: every tile stream-K (conv_dgrad_skn_kernel).  512 ranges, or 256 for small launches (>= 16
      // k-tiles per range, at most 8 ranges per tile)
      SkNPlan sn{};
      SkPlan scratch{};
      if (plan_skn_shape(ph, nphases, Cfg::BM, p.tilesN, p.Cout, &sn) && sk_scratch_of(s, &scratch)) {
        sn.parts = scratch.parts; sn.arrivals = scratch.arrivals;
        static int once_sn = set_smem(conv_dgrad_skn_kernel<Cfg, XF>, smem);
        if (once_sn != PCG_OK) return once_sn;
        DgradPhases phs = ph;
        phs.interleave = 0;
        hipLaunchKernelGGL((conv_dgrad_skn_kernel<Cfg, XF>), dim3((unsigned)sn.blocks), dim3(IG_THREADS), smem, s, p, phs, sn);
        return launch_status("conv_dgrad_skn_kernel");
      }
    }
    SkPlan sk{};
    const int tpp = tilesM * p.tilesN;
    if (uniform && plan_sk(tpp * nphases, ph.p[0].nth * ph.p[0].ntw * ceil_div(p.Cout, IG_BK), s, &sk)) {
      static int once_sk = set_smem(conv_dgrad_sk_kernel<Cfg, XF>, smem);
      if (once_sk != PCG_OK) return once_sk;
      DgradPhases phs = ph;
      phs.interleave = 0;
      hipLaunchKernelGGL((conv_dgrad_sk_kernel<Cfg, XF>), dim3((unsigned)(sk.dp_tiles + sk.sk_blocks)), dim3(IG_THREADS), smem, s, p, phs, sk, tpp);
      return launch_status("conv_dgrad_sk_kernel");
    }
  }
  static int once = set_smem(conv_dgrad_kernel<Cfg, XF>, smem);
  if (once != PCG_OK) return once;
  DgradPhases phl = ph;
  const bool same = dgrad_interleaved(p.w_bytes, ph, nphases);
  phl.interleave = same ? nphases : 0;
  if (same)
    hipLaunchKernelGGL((conv_dgrad_kernel<Cfg, XF>), dim3((unsigned)tilesM * p.tilesN * nphases), dim3(IG_THREADS), smem, s, p, phl);
  else
    hipLaunchKernelGGL((conv_dgrad_kernel<Cfg, XF>), dim3((unsigned)tilesM * p.tilesN, nphases), dim3(IG_THREADS), smem, s, p, phl);
  return launch_status("conv_dgrad_kernel");
}
template <class Cfg>
int launch_dgrad(const ConvP& p, const DgradPhases& ph, int nphases, int maxMp, hipStream_t s) {
  if (conv_bf16())
    return p.in_sc ? launch_dgrad_x<Bf16Twin<Cfg>, true>(p, ph, nphases, maxMp, s) : launch_dgrad_x<Bf16Twin<Cfg>, false>(p, ph, nphases, maxMp, s);
  return p.in_sc ? launch_dgrad_x<Cfg, true>(p, ph, nphases, maxMp, s) : launch_dgrad_x<Cfg, false>(p, ph, nphases, maxMp, s);
}

struct WgradPlan { int splits, ktiles_total, ktiles_per_split, tiles; bool narrow, wide192; };

// ---- weight gradients that skip their all-padding MFMAs (igemm_core.h PadSkip) ----
// Which geometries: k4 s2 p1 with IH = 2 OH and IW = 2 OW (the last tap row / column is padding at the last output row / column), OH and
// OW powers of two >= 4 (output row of a k-group by shift and mask; OW = 4: ow of an MFMA's two positions), Cin a multiple of 64 (a
// wave tile of 32 or 64 columns lies inside one tap).  Plain host code.
bool wgrad_padskip_geom(const pcg_conv_geom* g) {
  auto pow2 = [](int v) { return v >= 4 && (v & (v - 1)) == 0; };
  return g->KH == 4 && g->KW == 4 && g->stride == 2 && g->pad == 1 && g->IH == 2 * g->OH && g->IW == 2 * g->OW && pow2(g->OH) && pow2(g->OW) &&
         g->Cin % 64 == 0 && !thin_is_cin(g) && !thin_is_cout(g);
}
// share of the launch's MFMAs left out: OW = 4: one MFMA in four for the taps kw = 0 and 3; OW >= 8: one k-group in OH for kh = 0 and 3
double wgrad_padskip_fraction(const pcg_conv_geom* g) { return g->OW == 4 ? 0.125 : 0.5 / g->OH; }
// pcg_tune_set("wgrad_padskip", v) or PCG_WGRAD_PADSKIP=v: 0 today's launches; 1 (default) the skipping consumers in the paired block
// order for the classes that measured a gain, OW = 4 and OW = 8 (OW = 16 lost 1.7 % and stays on today's
// kernels); 2 / 3 (measurements) every eligible launch, in the paired order / in today's order.
// Returns what a launch of `g` does: 0 today's kernel, 1 skipping in today's order, 2 skipping in the paired order.
constexpr int WGRAD_PADSKIP_DEFAULT = 1;
int wgrad_padskip_mode(const pcg_conv_geom* g) {
  static const int env0 = getenv("PCG_WGRAD_PADSKIP") ? atoi(getenv("PCG_WGRAD_PADSKIP")) : WGRAD_PADSKIP_DEFAULT;
  static const int env = env0 >= 0 && env0 <= 3 ? env0 : WGRAD_PADSKIP_DEFAULT;      // a value outside 0 .. 3: the built-in default
  const int v = g_tune.wgrad_padskip >= 0 ? g_tune.wgrad_padskip : env;
  return v == 1 ? (g->OW <= 8 ? 2 : 0) : v == 2 ? 2 : v == 3 ? 1 : 0;
}
// The paired order's bit (wgrad_pair_block).  A tile's class is the number of its wave-tile columns that skip; the bit m in {1, 2, ..,
// 128} (or 0: none) is the one for which the blocks b ^ m of the odd rounds and b - 256 of the even ones, which share a CU in the
// schedule model, come closest to one skipping class per CU.  PairForm says which output tile block b works on in today's order:
//   sk = 0  conv_wgrad_kernel: n0 = tiles, n1 = K-slices, n2 = slice_major
//   sk = 1  conv_wgrad_sk_kernel: n0 = dp_tiles, n1 = sk_tiles, n2 = sk_blocks, n3 = k-tiles per tile (the tile of the block's first segment)
// The bit depends on nothing but its arguments; the answers are kept (a training step asks for the same few over and over).
struct PairForm { int sk, n0, n1, n2, n3; };
int wgrad_pair_xor(int waves_n, int wtn, int tilesN, int Cin, int OW, const PairForm& f) {
  struct Entry { int key[10]; int bit; };
  static std::vector<Entry> cache;
  static std::mutex cache_mutex;
  const int key[10] = {waves_n, wtn, tilesN, Cin, OW, f.sk, f.n0, f.n1, f.n2, f.n3};
  std::lock_guard<std::mutex> lock(cache_mutex);
  for (const Entry& e : cache)
    if (!memcmp(e.key, key, sizeof(key))) return e.bit;
  const int blocks = f.sk ? f.n0 + f.n2 : f.n0 * f.n1;
  auto tile_of = [&](int b) {
    if (!f.sk) return f.n2 ? (int)(xcd_remap((uint32_t)b, (uint32_t)blocks) % (uint32_t)f.n0) : (int)xcd_remap((uint32_t)(b % f.n0), (uint32_t)f.n0);
    if (b < f.n0) return (int)xcd_remap((uint32_t)b, (uint32_t)f.n0);
    const uint32_t g = xcd_remap((uint32_t)(b - f.n0), (uint32_t)f.n2);
    return f.n0 + (int)(g * (uint32_t)(f.n1 * f.n3) / (uint32_t)f.n2 / (uint32_t)f.n3);
  };
  auto cls = [&](int b) {
    const int nt = tile_of(b) % tilesN;
    int c = 0;
    for (int wn = 0; wn < waves_n; ++wn) {
      const int tap = (nt * 128 + wn * wtn) / Cin, kh = tap >> 2, kw = tap & 3;      // (128-column tiles)
      c += tap < 16 && (OW == 4 ? (kw == 0 || kw == 3) : (kh == 0 || kh == 3)) ? 1 : 0;
    }
    return c;
  };
  int best_m = 0, best = -1;
  for (int m = 0; m <= 128; m = m ? 2 * m : 1) {
    int score = 0;
    for (int b = 256; (b | 255) < blocks; b += (b & 255) == 255 ? 257 : 1)
      score += waves_n - abs(cls(b ^ m) + cls(b - 256) - waves_n);
    if (score > best) { best = score; best_m = m; }
  }
  if (cache.size() < 256) cache.push_back(Entry{{key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7], key[8], key[9]}, best_m});
  return best_m;
}

WgradPlan plan_wgrad(const pcg_conv_geom* g) {
  WgradPlan w{};
  const int M = g->Cout, N = g->KH * g->KW * g->Cin;
  w.narrow = (M <= 64);
  static const int t192_env = getenv("PCG_WGRAD_192") ? atoi(getenv("PCG_WGRAD_192")) : 1;   // A/B switch
  // 64x192 tile: N = 576 (3x3, 64 channels) is 4.5 tiles of 128 columns — the fifth one is half empty, 11 % of the MFMAs
  w.wide192 = w.narrow && t192_env && N % 192 == 0 && (N % 128) != 0;
  const int BM = w.narrow ? 64 : 128;
  w.tiles = ceil_div(M, BM) * (w.wide192 ? N / 192 : ceil_div(N, 128));
  const int64_t K = (int64_t)g->B * g->OH * g->OW;
  w.ktiles_total = (int)ceil_div64(K, IG_BK);
  // fill the 512 block slots (2 per CU) in ONE round — 515 blocks would run as 512 + a second round of 3 — but keep
  // >= 8 k-tiles (256 pixels) per slice
  const int slots = 512 * (g_tune.wgrad_rounds > 0 ? g_tune.wgrad_rounds : 1);      // (A/B: more, shorter K-slices = more than one round of workgroups)
  int splits = w.tiles <= slots ? slots / w.tiles : 1;
  const int max_splits = w.ktiles_total / 8 > 0 ? w.ktiles_total / 8 : 1;
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  // When the tiles do not divide the chip (288 tiles of a 1024 x 4608 gradient: 32 CUs get two full-K blocks, the rest one) a few
  // more K-slices balance the CUs at the price of slab traffic.  Cost model per candidate s, in us: n = blocks per CU (ceil),
  // n * k-tiles per slice * time per k-tile (one block alone on a CU exposes its latencies: x1.2) + s slabs written and read
  // at ~4 TB/s.  The 512-slot rule above stands unless the model sees > 5 % to gain (it agrees on every DCGAN / counteRGAN layer).
  auto cost = [&](int s, int* s_eff) {
    const int kps = ceil_div(w.ktiles_total, s), se = ceil_div(w.ktiles_total, kps);
    const int n = ceil_div(w.tiles * se, 256);
    *s_eff = se;
    return (double)n * kps * (w.wide192 ? 1.5 : w.narrow ? 1.0 : 1.95) * (n == 1 ? 1.2 : 1.0) + (double)se * M * N * 8.0 / 4.0e6;
  };
  int se = 0;
  const double c0 = cost(splits, &se);
  double cb = c0;
  int sb = splits;
  for (int s = 1; s <= max_splits && s <= 64; ++s) {
    const double c = cost(s, &se);
    if (se == s && c < cb * 0.98) { cb = c; sb = s; }
  }
  if (cb < 0.95 * c0) splits = sb;
  w.ktiles_per_split = ceil_div(w.ktiles_total, splits);
  w.splits = ceil_div(w.ktiles_total, w.ktiles_per_split);
  return w;
}

}  // namespace
}  // namespace pcg

using namespace pcg;

extern "C" size_t pcg_conv2d_fwd_workspace_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK) return 0;
  if (thin_is_cin(g) || thin_is_cout(g)) return thin_conv_fwd_workspace_bytes(g);
  const FwdPlan f = plan_fwd(g);
  return f.splits > 1 ? (size_t)f.splits * g->B * g->OH * g->OW * g->Cout * sizeof(float) : 0;
}
// Grad-input as ONE balanced GEMM + col2im.  With a kernel size that is not a multiple of the stride (k3 s2: WGAN-GP critic,
// mnist_wgan_conditional.py:84-90) the sub-pixel phases see 4 : 2 : 2 : 1 taps; the phase kernel's longest blocks are then the
// critical path (measured 30-60 TFLOP/s on the critic's conv2 / conv3).  dcol[B*OH*OW][KH*KW*Cin] = dy * W is the grad-input of
// the 1x1 convolution with Cin' = KH*KW*Cin on the SAME weight bytes (OHWI rows are [Cout][KH*KW*Cin]) — same MACs as the phase
// form, every block the same K = Cout — followed by a col2im pass over dcol (HBM-bound, 2 x |dcol| extra traffic).
static bool dgrad_as_gemm(const pcg_conv_geom* g, int have_sk = -1) {
  if (have_sk < 0) have_sk = have_sk_scratch() ? 1 : 0;
  if (thin_is_cin(g) || thin_is_cout(g)) return false;
  if (g_tune.dgrad_gemm == 0) return false;       // A/B: the phase kernel instead
  if (g_tune.dgrad_gemm < 0 && have_sk && g->stride == 2) {
    // The phase form multiplies every pixel of a phase by every tap of the phase, the GEMM form every dy pixel by every tap:
    // which one wastes fewer MACs on taps that fall outside depends on the geometry (7 -> 4 with padding 1: 121 against 144 per
    // image and channel pair; 13 -> 6 without padding: 400 against 324; 6 -> 2: 81 against 36).  With its load balance repaired
    // by conv_dgrad_skn_kernel the phase form is taken where it has clearly fewer (measured r03, B = 256 ConvT 1024 -> 512:
    // 328 -> 237 us).
    int64_t phase_macs = 0;
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) {
        const int PHh = a < g->IH ? (g->IH - a + 1) / 2 : 0, PHw = b < g->IW ? (g->IW - b + 1) / 2 : 0;
        const int kh0 = (a + g->pad) % 2, kw0 = (b + g->pad) % 2;
        const int nth = kh0 < g->KH ? (g->KH - kh0 + 1) / 2 : 0, ntw = kw0 < g->KW ? (g->KW - kw0 + 1) / 2 : 0;
        phase_macs += (int64_t)PHh * PHw * nth * ntw;
      }
    if (phase_macs * 20 <= (int64_t)g->OH * g->OW * g->KH * g->KW * 19) return false;
  }
  if (g->stride < 2 || (g->KH % g->stride == 0 && g->KW % g->stride == 0)) return false;
  if (g->Cout < 512 || g->Cin % 4 || g->Cout % 4) return false;          // K = Cout: >= 16 k-tiles per block
  const int64_t bytes = (int64_t)g->B * g->OH * g->OW * g->KH * g->KW * g->Cin * 4;
  return bytes < (1ll << 31);
}
static size_t dgrad_gemm_bytes(const pcg_conv_geom* g) { return (size_t)g->B * g->OH * g->OW * g->KH * g->KW * g->Cin * sizeof(float); }

// Scratch of the hybrid stream-K launches (partial accumulator tiles + arrival counters), owned by the caller and registered for
// ONE stream: launches on that stream use it in stream order.  `arrivals` must be zero-filled when it is registered; the kernels
// leave it zero.  A stream without scratch runs the plain launches.  parts == nullptr forgets the stream.
extern "C" size_t pcg_conv_scratch_parts_bytes(void) { return pcg::SK_PARTS_BYTES; }
extern "C" size_t pcg_conv_scratch_arrivals_bytes(void) { return pcg::SK_ARRIVALS_BYTES; }
extern "C" int pcg_conv_set_scratch(pcg_stream_t stream, void* parts, size_t parts_bytes, void* arrivals, size_t arrivals_bytes) {
  using namespace pcg;
  hipStream_t s = (hipStream_t)stream;
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_sk_mutex);
  int at = -1;
  for (int i = 0; i < g_sk_scratch_n; ++i) if (g_sk_scratch[i].stream == s && g_sk_scratch[i].device == dev) at = i;
  if (!parts) {
    if (at >= 0) g_sk_scratch[at] = g_sk_scratch[--g_sk_scratch_n];
    return PCG_OK;
  }
  PCG_REQUIRE(arrivals != nullptr && parts_bytes >= SK_PARTS_BYTES && arrivals_bytes >= SK_ARRIVALS_BYTES,
              "pcg_conv_set_scratch: parts %zu B (need %zu), arrivals %zu B (need %zu)", parts_bytes, SK_PARTS_BYTES, arrivals_bytes, SK_ARRIVALS_BYTES);
  PCG_REQUIRE((((uintptr_t)parts) & 15) == 0 && (((uintptr_t)arrivals) & 3) == 0, "pcg_conv_set_scratch: misaligned scratch");
  if (at < 0) {
    PCG_REQUIRE(g_sk_scratch_n < 64, "pcg_conv_set_scratch: more than 64 streams with scratch");
    at = g_sk_scratch_n++;
  }
  g_sk_scratch[at] = SkScratch{dev, s, (float*)parts, (int*)arrivals};
  return PCG_OK;
}
// The stream-K kernels rely on the arrival counters being zero between launches (the last arrival of a tile resets its counters).
// After a launch on `stream` failed or was aborted they may not be: this zero-fills them in stream order.  No-op for a stream
// without scratch.
extern "C" int pcg_conv_reset_scratch(pcg_stream_t stream) {
  using namespace pcg;
  SkPlan sk{};
  if (!sk_scratch_of((hipStream_t)stream, &sk)) return PCG_OK;
  hipError_t e = hipMemsetAsync(sk.arrivals, 0, SK_ARRIVALS_BYTES, (hipStream_t)stream);
  if (e != hipSuccess) { set_error("pcg_conv_reset_scratch: %s", hipGetErrorString(e)); return PCG_ERR_LAUNCH; }
  return PCG_OK;
}

// Pixel descriptor table of a geometry: see include/pcgan_hip.h.  The builder is plain host code (conv_pixtab.h); registering stores a
// pointer — no allocation, no copy, no synchronisation, so both are safe anywhere, stream capture included.
extern "C" size_t pcg_conv_pixtab_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK) return 0;
  return pcg::pixtab_entries(g->OH, g->OW) * 2 * sizeof(uint32_t);
}
extern "C" int pcg_conv_pixtab_register(const pcg_conv_geom* g, void* host_out, size_t bytes, const void* device_table) {
  using namespace pcg;
  if (int e = check_geom(g)) return e;
  if (host_out) {
    PCG_REQUIRE(bytes >= pcg_conv_pixtab_bytes(g) && (((uintptr_t)host_out) & 3) == 0, "pcg_conv_pixtab_register: host buffer %zu B (need %zu), 4-byte aligned",
                bytes, pcg_conv_pixtab_bytes(g));
    pixtab_build(g->IH, g->IW, g->OH, g->OW, g->stride, g->pad, g->KH, g->KW, g->Cin, static_cast<uint32_t*>(host_out));
    if (!device_table) return PCG_OK;
  }
  PCG_REQUIRE((((uintptr_t)device_table) & 7) == 0, "pcg_conv_pixtab_register: misaligned table");
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_pixtab_mutex);
  int at = -1;
  for (int i = 0; i < g_pixtab_n; ++i) if (pixtab_same(g_pixtab[i], dev, g)) at = i;
  if (!device_table) {                    // neither buffer: forget the geometry
    if (at >= 0) g_pixtab[at] = g_pixtab[--g_pixtab_n];
    return PCG_OK;
  }
  if (at < 0) {
    PCG_REQUIRE(g_pixtab_n < PIXTAB_MAX, "pcg_conv_pixtab_register: more than %d geometries with a table", PIXTAB_MAX);
    at = g_pixtab_n++;
  }
  g_pixtab[at] = PixTabReg{dev, g->IH, g->IW, g->OH, g->OW, g->stride, g->pad, g->KH, g->KW, g->Cin, static_cast<const uint32_t*>(device_table)};
  return PCG_OK;
}

// Tile descriptor table of a geometry (clipped forward / grad-input launches): see include/pcgan_hip.h.  Same contract as the pixel table:
// the builder is plain host code (conv_cliptab.h), registering stores a pointer.
extern "C" size_t pcg_conv_cliptab_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK || !pcg::clip_geom_ok(g->IH, g->IW, g->OH, g->OW, g->stride, g->pad, g->KH, g->KW)) return 0;
  return pcg::cliptab_words(g->OH, g->OW) * sizeof(uint32_t);
}
extern "C" int pcg_conv_cliptab_register(const pcg_conv_geom* g, void* host_out, size_t bytes, const void* device_table) {
  using namespace pcg;
  if (int e = check_geom(g)) return e;
  const size_t need = pcg_conv_cliptab_bytes(g);
  PCG_REQUIRE(need > 0, "pcg_conv_cliptab_register: only k4 s2 p1 geometries with IH = 2 OH and IW = 2 OW have a tile table");
  if (host_out) {
    PCG_REQUIRE(bytes >= need && (((uintptr_t)host_out) & 3) == 0, "pcg_conv_cliptab_register: host buffer %zu B (need %zu), 4-byte aligned", bytes, need);
    cliptab_build(g->OH, g->OW, static_cast<uint32_t*>(host_out));
    if (!device_table) return PCG_OK;
  }
  PCG_REQUIRE((((uintptr_t)device_table) & 3) == 0, "pcg_conv_cliptab_register: misaligned table");
  const int dev = current_device();
  std::lock_guard<std::mutex> lock(g_clip_mutex);
  int at = -1;
  for (int i = 0; i < g_cliptab_n; ++i) if (g_cliptab[i].device == dev && g_cliptab[i].OH == g->OH && g_cliptab[i].OW == g->OW) at = i;
  if (!device_table) {                    // neither buffer: forget the geometry
    if (at >= 0) g_cliptab[at] = g_cliptab[--g_cliptab_n];
    return PCG_OK;
  }
  if (at < 0) {
    PCG_REQUIRE(g_cliptab_n < CLIPTAB_MAX, "pcg_conv_cliptab_register: more than %d geometries with a table", CLIPTAB_MAX);
    at = g_cliptab_n++;
  }
  g_cliptab[at] = ClipTabReg{dev, g->OH, g->OW, static_cast<const uint32_t*>(device_table)};
  return PCG_OK;
}
extern "C" double pcg_conv_sched_model(const int32_t* ktiles, int32_t n) {
  return ktiles && n > 0 ? pcg::clip_sched_model(ktiles, n) : 0.0;
}

extern "C" size_t pcg_conv2d_dgrad_workspace_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK) return 0;
  if (thin_is_cin(g) || thin_is_cout(g)) return thin_conv_dgrad_workspace_bytes(g);
  return dgrad_as_gemm(g) ? dgrad_gemm_bytes(g) : 0;
}

namespace pcg {
int launch_bn_stats_finalize(const double* partial, int nparts, int64_t rows, int C, float eps, float momentum, float* save_mean,
                             float* save_invstd, float* running_mean, float* running_var, int64_t* nbt, hipStream_t s,
                             bool has_presum_tail, const float* gamma = nullptr, const float* beta = nullptr, float* coef = nullptr);
size_t bn_partial_buffer_bytes(int nparts, int C);
int launch_bn_stats_finalize_g(const double* partial, int nparts, int nphases, int groups, int64_t rows_per_group, int C, float eps,
                               float momentum, float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                               int64_t* nbt, hipStream_t s);
}

static bool mfma_layer(const pcg_conv_geom* g) { return !(thin_is_cin(g) || thin_is_cout(g)); }
static int fwd_stat_rows(const pcg_conv_geom* g) { return ceil_div(g->B * g->OH * g->OW, 128) * 2; }
static int dgrad_stat_rows(const pcg_conv_geom* g) {
  int rows = 0;
  const int s = g->stride;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) {
      const int PHh = a < g->IH ? (g->IH - a + s - 1) / s : 0, PHw = b < g->IW ? (g->IW - b + s - 1) / s : 0;
      rows += ceil_div(g->B * PHh * PHw, 128) * 2;
    }
  return rows;
}

static bool fwd_use_t64(int M, int N, int splits) {
  const int tiles128 = ceil_div(M, 128) * ceil_div(N, 128);
  return g_tune.t64 != 0 && N > 64 && splits == 1 && tiles128 > 224 && tiles128 <= 256 && M % 128 == 0;
}
// The clipped path of a forward-kernel launch (conv_cliptab.h).  Eligible: k4 s2 p1 on the fp32 MFMA path, the batch — and each
// BatchNorm group's share of it — whole tiles, today's launch plain data-parallel (`plain`: no K-slices, no stream-K).  Taken where the
// schedule model predicts at least 5 % (plan_clip).  Returns the plan; take == false: today's launch.
static ClipPlan clip_fwd_plan(const pcg_conv_geom* g, int groups, bool t64, bool plain) {
  const ClipPlan none{false, 0, 0, 1.0};
  const int bm0 = t64 ? 64 : 128;
  // (the batch whole tiles of today's height; the forced 64-row modes also take whole 64-row tiles)
  if (clip_mode() == 0 || conv_bf16() || !plain || !mfma_layer(g) || g->Cin % 4 ||
      !(clip_shape_ok(g, groups, bm0) || (clip_mode() >= 5 && g->Cout > 64 && clip_shape_ok(g, groups, 64)))) return none;
  const int N = g->Cout;
  const ClipShape c{0, g->OH, g->OW, g->B, ceil_div(N, N > 64 ? 128 : 64), 0, bm0, N > 64 && !t64 ? 1 : 0};
  const ClipPlan cp = plan_clip(c);
  return cp.take && clip_shape_ok(g, groups, cp.bm) ? cp : ClipPlan{false, cp.order, cp.bm, cp.ratio};
}
static ClipPlan clip_dgrad_plan(const pcg_conv_geom* g, int groups, bool interleave, bool plain) {
  const ClipPlan none{false, 0, 0, 1.0};
  if (clip_mode() == 0 || (clip_mode() == 1 && clip_dgrad_mode() == 0) || conv_bf16() || !plain || !mfma_layer(g) || g->Cin % 4 || g->Cout % 4 ||
      !clip_shape_ok(g, groups, 128)) return none;
  const int N = g->Cin;
  const ClipShape c{1, g->OH, g->OW, g->B, ceil_div(N, N > 64 ? 128 : 64), interleave ? 1 : 0, 128, 0};
  ClipPlan cp = plan_clip(c);
  if (clip_mode() == 1 && clip_dgrad_mode() == 2) cp.take = true;
  return cp;
}
static void clip_apply(const pcg_conv_geom* g, const ClipPlan& cp, int groups, const uint32_t* tab, ConvP* p) {
  p->cliptab = tab; p->clip_order = cp.order; p->clip_tpp = g->B / cp.bm; p->clip_tpg = p->clip_tpp / groups; p->clip_npos = g->OH * g->OW;
}

// A validated pcg_conv_args (conv_call_of below): what the two implementation functions launch.  epi is null for PCG_CONV_EPI_NONE — the
// split-K and GEMM + col2im decisions read it.
struct ConvCall {
  const float *in, *w, *bias;
  float* out;
  double* stat_partial;      // partial rows of the fused statistics or of an add_bnsum / bnbwd epilogue
  void* workspace;
  size_t workspace_bytes;
  int act;
  float slope;
  const EpiAux* epi;
  const pcg_in_xform* xf;
  int groups;                // BatchNorm groups of a forward launch (1: ungrouped); the grad-input's ride in epi->group_rows
};

static int conv2d_fwd_impl(const pcg_conv_geom* g, const ConvCall& c, pcg_stream_t stream) {
  const float *x = c.in, *w = c.w, *bias = c.bias;
  float* y = c.out;
  double* stat_partial = c.stat_partial;
  void* workspace = c.workspace;
  const size_t workspace_bytes = c.workspace_bytes;
  const int act = c.act, groups = c.groups;
  const float slope = c.slope;
  const EpiAux* epi = c.epi;
  const pcg_in_xform* xf = c.xf;
  if (thin_is_cin(g) || thin_is_cout(g)) return thin_conv_fwd(g, x, w, bias, y, workspace, workspace_bytes, (hipStream_t)stream, act, slope);
  ConvP p = make_params(g);
  p.x = x; p.w = w; p.bias = bias; p.out = y; p.stat_partial = stat_partial;
  if (epi) p.epi = *epi;
  if (int e = set_xform("pcg_conv2d", xf, g->Cin, &p)) return e;
  p.M = g->B * g->OH * g->OW; p.N = g->Cout;
  p.ktiles = g->KH * g->KW * ceil_div(g->Cin, IG_BK);
  p.ktiles_per_split = p.ktiles;
  hipStream_t s = (hipStream_t)stream;
  // split-K needs the slab workspace and cannot fuse statistics or the activation (both need the complete sum)
  FwdPlan f = plan_fwd(g, stream_has_sk(s));        // this stream's scratch decides, not "some stream has scratch"
  const size_t need = (size_t)f.splits * p.M * p.N * sizeof(float);
  if (f.splits > 1 && (stat_partial || epi || !workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) || ((uintptr_t)y & 15) || (p.M * (size_t)p.N) % 4))
    f = FwdPlan{1, p.ktiles};
  const bool fuse = act_is_cheap(act) && f.splits == 1;   // the epilogue fuses ReLU / LeakyReLU; tanh / sigmoid run as a second pass
  p.act = fuse ? act : PCG_ACT_NONE; p.slope = act_neg_of(p.act, slope);
  if (f.splits > 1) { p.out = (float*)workspace; p.ktiles_per_split = f.ktiles_per_split; }
  // At most one 128x128 tile per CU (DCGAN D4: 8192 x 512 = 256 tiles): a workgroup alone on a CU runs at ~80 % of the matrix rate
  // (one consumer wave per SIMD exposes its own latencies).  64x128 tiles double the workgroups — two per CU again — at the price
  // of 64x32 wave tiles: measured r03, D4 forward 262 -> 249 us (131 -> 138 TFLOP/s), G2's 260 -> 249; stream-K on the 256 big
  // tiles had measured neutral.  (pcg_tune_set("t64", 0) keeps the 128x128 tiles.)
  // Only where the doubled count fills the 512 slots (225..256 big tiles); fewer tiles take stream-K / K-slices as before.
  const bool t64 = fwd_use_t64(p.M, p.N, f.splits);
  int clip_bm = 0;         // tile height of the clipped launch, 0: today's launch
  if (const uint32_t* tab = clip_mode() != 0 ? cliptab_of(g) : nullptr) {
    SkPlan sk{};
    const bool plain = f.splits == 1 && !(p.N > 64 && !t64 && plan_sk(ceil_div(p.M, 128) * ceil_div(p.N, 128), p.ktiles, s, &sk));
    const ClipPlan cp = clip_fwd_plan(g, groups, t64, plain);
    if (cp.take) { clip_apply(g, cp, groups, tab, &p); clip_bm = cp.bm; }
  }
  if (int e = clip_bm == 64 ? launch_fwd_clip<TileCfg<64, 128, 1, 4>>(p, s)
                  : clip_bm ? (p.N > 64 ? launch_fwd_clip<Cfg128x128>(p, s) : launch_fwd_clip<Cfg128x64>(p, s))
                  : t64 ? launch_fwd<TileCfg<64, 128, 1, 4>>(p, f.splits, s)
                  : p.N > 64 ? launch_fwd<Cfg128x128>(p, f.splits, s)
                       : launch_fwd<Cfg128x64>(p, f.splits, s)) return e;
  if (f.splits > 1) {
    const size_t n = (size_t)p.M * p.N;
    if (int e = launch_slab_reduce((const float*)workspace, y, n, n, f.splits, 0, s)) return e;
  }
  return (fuse || act == PCG_ACT_NONE) ? PCG_OK : pcg_act_fwd(y, (int64_t)p.M * p.N, act, slope, y, stream);
}

extern "C" size_t pcg_conv2d_fwd_bn_workspace_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK || !mfma_layer(g) || g->Cout % 4) return 0;
  return bn_partial_buffer_bytes(fwd_stat_rows(g), g->Cout);
}
extern "C" size_t pcg_conv2d_dgrad_bn_workspace_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK || !mfma_layer(g) || g->stride > 2 || g->Cin % 4) return 0;
  return bn_partial_buffer_bytes(dgrad_stat_rows(g), g->Cin);
}

// the sub-pixel phases (ih % s, iw % s) of a grad-input: rows, first taps, taps per axis, partial-statistics rows
static int build_phases(const pcg_conv_geom* g, DgradPhases* php, int* maxMp_out) {
  DgradPhases& ph = *php;
  int nph = 0, maxMp = 0, prow = 0;
  const int s = g->stride;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) {
      PhaseInfo& f = ph.p[nph];
      f.ph = a; f.pw = b;
      f.PHh = a < g->IH ? (g->IH - a + s - 1) / s : 0;
      f.PHw = b < g->IW ? (g->IW - b + s - 1) / s : 0;
      f.Mp = g->B * f.PHh * f.PHw;
      if (f.Mp == 0) continue;
      f.kh0 = (a + g->pad) % s; f.kw0 = (b + g->pad) % s;
      f.nth = f.kh0 < g->KH ? (g->KH - f.kh0 + s - 1) / s : 0;
      f.ntw = f.kw0 < g->KW ? (g->KW - f.kw0 + s - 1) / s : 0;
      if (f.nth == 0 || f.ntw == 0) { f.nth = 0; f.ntw = 1; }
      f.dh0 = (a + g->pad - f.kh0) / s; f.dw0 = (b + g->pad - f.kw0) / s;
      f.dPHw = FastDiv((uint32_t)f.PHw); f.dPHh = FastDiv((uint32_t)f.PHh);
      if (f.Mp > maxMp) maxMp = f.Mp;
      f.prow0 = prow; prow += ceil_div(f.Mp, 128) * 2;
      ++nph;
    }
  *maxMp_out = maxMp;
  return nph;
}

static int conv2d_dgrad_impl(const pcg_conv_geom* g, const ConvCall& c, pcg_stream_t stream) {
  const float *dy = c.in, *w = c.w, *bias_x = c.bias;
  float* dx = c.out;
  double* stat_partial = c.stat_partial;
  void* workspace = c.workspace;
  const size_t workspace_bytes = c.workspace_bytes;
  const int act = c.act;
  const float slope = c.slope;
  const EpiAux* epi = c.epi;
  const pcg_in_xform* xf = c.xf;
  const bool has_xf = xf && xf->scale;
  if (thin_is_cin(g) || thin_is_cout(g)) {
    const ThinXf tx{has_xf ? xf->scale : nullptr, has_xf ? xf->shift : nullptr, has_xf ? act_neg_of(xf->act, xf->slope) : 1.f};
    return thin_conv_dgrad(g, dy, w, bias_x, dx, workspace, workspace_bytes, (hipStream_t)stream, act, slope, &tx);
  }
  if (!epi && !stat_partial && !has_xf && dgrad_as_gemm(g, stream_has_sk((hipStream_t)stream)) && workspace && workspace_bytes >= dgrad_gemm_bytes(g) &&
      (((uintptr_t)workspace | (uintptr_t)dx) & 15) == 0) {
    pcg_conv_geom g1 = {g->B, g->OH, g->OW, g->KH * g->KW * g->Cin, g->OH, g->OW, g->Cout, 1, 1, 1, 0};
    float* dcol = (float*)workspace;
    ConvCall c1{};
    c1.in = dy; c1.w = w; c1.out = dcol; c1.groups = 1;
    if (int e = conv2d_dgrad_impl(&g1, c1, stream)) return e;
    const bool fuse_act = act_is_cheap(act);
    const int CQ = g->Cin / 4;
    const uint64_t total = (uint64_t)g->B * g->IH * g->IW * CQ;
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(col2im_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(dcol),
                       reinterpret_cast<float4*>(dx), bias_x, g->B, g->IH, g->IW, CQ, g->OH, g->OW, g->KH, g->KW, g->stride, g->pad,
                       FastDiv((uint32_t)CQ), FastDiv((uint32_t)g->IW), FastDiv((uint32_t)g->IH), fuse_act ? act : PCG_ACT_NONE,
                       act_neg_of(fuse_act ? act : PCG_ACT_NONE, slope));
    if (int e = launch_status("col2im_kernel")) return e;
    return fuse_act ? PCG_OK : pcg_act_fwd(dx, (int64_t)g->B * g->IH * g->IW * g->Cin, act, slope, dx, stream);
  }
  ConvP p = make_params(g);
  const bool fuse = act_is_cheap(act);
  p.dy = dy; p.w = w; p.bias = bias_x; p.out = dx; p.stat_partial = stat_partial;
  if (epi) p.epi = *epi;
  if (int e = set_xform("pcg_conv2d", xf, g->Cout, &p)) return e;
  p.act = fuse ? act : PCG_ACT_NONE; p.slope = act_neg_of(p.act, slope);
  p.N = g->Cin;
  DgradPhases ph{};
  int maxMp = 0;
  const int nph = build_phases(g, &ph, &maxMp);
  PCG_REQUIRE(nph > 0, "pcg_conv2d: empty problem");
  hipStream_t st = (hipStream_t)stream;
  if (const uint32_t* tab = clip_mode() != 0 ? cliptab_of(g) : nullptr) {
    const int groups = p.epi.group_rows > 0 ? maxMp / p.epi.group_rows : 1;
    SkPlan sk{};
    const bool plain = nph == 4 && !(p.N > 64 && plan_sk(ceil_div(maxMp, 128) * ceil_div(p.N, 128) * nph, 4 * ceil_div(g->Cout, IG_BK), st, &sk));
    const ClipPlan cp = clip_dgrad_plan(g, groups, dgrad_interleaved(p.w_bytes, ph, nph), plain);
    if (cp.take) clip_apply(g, cp, groups, tab, &p);
  }
  if (int e = p.N > 64 ? launch_dgrad<Cfg128x128>(p, ph, nph, maxMp, st)
                       : (nph > 1 && g_tune.dgrad_swz3 == 0) ? launch_dgrad<Cfg128x64P>(p, ph, nph, maxMp, st)   // (r04: with the epilogue at priority 3 the three-per-CU config also wins on the four-phase k4 s2 grad-input: D2 0.2957 -> 0.2893 ms)
                                                             : launch_dgrad<Cfg128x64>(p, ph, nph, maxMp, st)) return e;
  return fuse ? PCG_OK : pcg_act_fwd(dx, (int64_t)g->B * g->IH * g->IW * g->Cin, act, slope, dx, stream);
}


// a Cin = 1 layer whose dy-side operand may carry an input transform (pcg_conv2d grad-input with xf, pcg_conv2d_wgrad_xf with xf_dy): DCGAN's
// last ConvTranspose2d(64, 1, 4, 2, 1) behind BatchNorm + ReLU (mnist_dcgan.py:85-88) — no BatchNorm-apply pass, no activated copy
extern "C" int32_t pcg_conv2d_xf_thin_ok(const pcg_conv_geom* g) { return check_geom(g) == PCG_OK && thin_conv_xf_ok(g) ? 1 : 0; }
extern "C" int32_t pcg_conv2d_dgrad_mask_thin_ok(const pcg_conv_geom* g) { return check_geom(g) == PCG_OK && thin_conv_dgrad_mask_ok(g) && g->Cin % 4 == 0 ? 1 : 0; }
// The phases of a grad-input launch: the partial rows of a bnbwd epilogue are [phase][tile row], pcg_bn_bwd_partial_g reads each group's
// share of every phase.
extern "C" int32_t pcg_conv2d_dgrad_bn_phases(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK) return 0;
  DgradPhases ph{};
  int maxMp = 0;
  return build_phases(g, &ph, &maxMp);
}

// ---- pcg_conv2d: the forward and grad-input forms behind one argument struct (include/pcgan_hip.h: pcg_conv_args) --------------------
// Every refusal is made here, before any HIP call.  Fills the ConvCall the implementation functions launch; `e` is the storage of its
// epilogue (c->epi stays null for PCG_CONV_EPI_NONE).  The backward-pass epilogues hand the gradient w.r.t. the layer below's OUTPUT out
// of the kernel already multiplied by that layer's ReLU / LeakyReLU derivative, optionally with BatchNorm-backward's two column sums
// taken on the way; aux tensors reach the kernel as byte distances from the output.
static int conv_call_of(const pcg_conv_geom* g, const pcg_conv_args* a, ConvCall* c, EpiAux* e) {
  if (int rc = check_geom(g)) return rc;
  PCG_REQUIRE(a != nullptr, "pcg_conv2d: null argument struct");
  const bool dgrad = a->op == PCG_CONV_DGRAD, mfma = mfma_layer(g), has_xf = a->xf && a->xf->scale;
  auto act_masks = [](int act) { return act == PCG_ACT_NONE || act == PCG_ACT_RELU || act == PCG_ACT_LRELU; };
  auto off16 = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
  PCG_REQUIRE(dgrad || a->op == PCG_CONV_FWD, "pcg_conv2d: unknown op %d", a->op);
  PCG_REQUIRE(a->in && a->w && a->out, "pcg_conv2d: null pointer (in / w / out)");
  PCG_REQUIRE(a->act >= PCG_ACT_NONE && a->act <= PCG_ACT_SIGMOID, "pcg_conv2d: unknown activation %d", a->act);
  PCG_REQUIRE(a->epi >= PCG_CONV_EPI_NONE && a->epi <= PCG_CONV_EPI_BNBWD, "pcg_conv2d: unknown epilogue %d", a->epi);
  // the forms that exist: an epilogue or the statistics ride on the bare convolution
  PCG_REQUIRE(a->epi == PCG_CONV_EPI_NONE || (!a->stats && !has_xf && !a->bias && a->act == PCG_ACT_NONE),
              "pcg_conv2d: an epilogue goes with no statistics, input transform, bias or output activation");
  PCG_REQUIRE(!a->stats || a->act == PCG_ACT_NONE, "pcg_conv2d: statistics go with no output activation (they are taken of the sum itself)");
  PCG_REQUIRE(a->groups == 0 || (a->groups > 0 && (dgrad ? a->epi == PCG_CONV_EPI_BNBWD : a->stats && !has_xf && !a->gamma && !a->beta && !a->coef_out)),
              "pcg_conv2d: groups = %d goes with the forward's statistics (no transform, no gamma / beta / coef_out) or the grad-input's bnbwd epilogue only", a->groups);
  if (!mfma) {
    PCG_REQUIRE(!has_xf || (dgrad && thin_conv_xf_ok(g)), "pcg_conv2d: input transforms on the MFMA path (Cin > 3 and Cout > 3) and on the grad-input of pcg_conv2d_xf_thin_ok geometries only");
    PCG_REQUIRE(!has_xf || act_masks(a->xf->act), "pcg_conv2d: input transform activation %d is not none / ReLU / LeakyReLU", has_xf ? a->xf->act : 0);
  } else {
    PCG_REQUIRE(g->Cin % 4 == 0 && (!dgrad || g->Cout % 4 == 0),
                "pcg_conv2d: Cin=%d (grad-input: and Cout=%d) must be a multiple of 4 for the MFMA path (1..3-channel layers take the thin path)", g->Cin, g->Cout);
    PCG_REQUIRE(!dgrad || g->stride <= 2, "pcg_conv2d: grad-input stride %d > 2 unsupported", g->stride);
    if (int rc = check_xform("pcg_conv2d", a->xf, dgrad ? g->Cout : g->Cin)) return rc;
  }
  *c = ConvCall{a->in, a->w, a->bias, a->out, nullptr, a->workspace, a->workspace_bytes, a->act, a->slope, nullptr, a->xf, 1};
  const size_t need = dgrad ? pcg_conv2d_dgrad_bn_workspace_bytes(g) : pcg_conv2d_fwd_bn_workspace_bytes(g);   // partial rows of this direction
  if (a->stats) {
    PCG_REQUIRE(need > 0, "pcg_conv2d: statistics only on MFMA layers (Cin > 3, Cout > 3, output channels %% 4 == 0, grad-input stride <= 2); use pcg_conv2d + pcg_bn_train_stats");
    PCG_REQUIRE(a->save_mean && a->save_invstd, "pcg_conv2d: null statistics output");
    PCG_REQUIRE(!a->coef_out || (a->gamma && a->beta), "pcg_conv2d: coef_out needs gamma and beta");
    PCG_REQUIRE(a->groups == 0 || (a->groups <= 8 && g->B % a->groups == 0 && ((int64_t)(g->B / a->groups) * g->OH * g->OW) % 128 == 0),
                "pcg_conv2d: %d images do not split into %d groups of whole 128-row tiles (%d x %d output)", g->B, a->groups, g->OH, g->OW);
    if (!a->workspace || a->workspace_bytes < need) { set_error("pcg_conv2d: workspace %zu B < required %zu B (statistics)", a->workspace_bytes, need); return PCG_ERR_WORKSPACE; }
    c->stat_partial = (double*)a->workspace; c->workspace = nullptr; c->workspace_bytes = 0;
    if (a->groups > 0) c->groups = a->groups;
  }
  if (a->epi == PCG_CONV_EPI_NONE) return PCG_OK;
  // (a mask on a pcg_conv2d_dgrad_mask_thin_ok geometry is the one epilogue off the MFMA path: the thin expand kernel applies it)
  PCG_REQUIRE(mfma || (dgrad && a->epi == PCG_CONV_EPI_MASK && pcg_conv2d_dgrad_mask_thin_ok(g)),
              "pcg_conv2d: epilogues only on MFMA layers (Cin > 3 and Cout > 3); use the unfused calls");
  const bool masks = a->epi == PCG_CONV_EPI_MASK || a->epi == PCG_CONV_EPI_ADD_MASK || a->epi == PCG_CONV_EPI_BNBWD;
  PCG_REQUIRE(masks ? act_masks(a->epi_act) : a->epi_act == PCG_ACT_NONE, "pcg_conv2d: epilogue activation %d is not none / ReLU / LeakyReLU (add, add_bnsum: none)", a->epi_act);
  const bool sums = a->epi == PCG_CONV_EPI_ADD_BNSUM || a->epi == PCG_CONV_EPI_BNBWD;
  e->mode = a->epi == PCG_CONV_EPI_MASK ? EPI_MASK : a->epi == PCG_CONV_EPI_BNBWD ? EPI_BNBWD : sums ? EPI_ADDSUM : EPI_ADD;
  e->no_addend = a->epi == PCG_CONV_EPI_ADD_BNSUM && !a->addend;          // (r04) nullable: the sums of the plain result
  const float* aux = a->epi == PCG_CONV_EPI_MASK ? a->a_below : a->epi == PCG_CONV_EPI_BNBWD ? a->z : e->no_addend ? a->out : a->addend;
  PCG_REQUIRE(aux, "pcg_conv2d: null pointer (the epilogue's %s)", a->epi == PCG_CONV_EPI_MASK ? "a_below" : a->epi == PCG_CONV_EPI_BNBWD ? "z" : "addend");
  PCG_REQUIRE(!off16(aux) && !off16(a->out), "pcg_conv2d: tensors must be 16-byte aligned");
  e->neg = a->epi == PCG_CONV_EPI_ADD_BNSUM ? a->sum_scale : act_neg_of(a->epi_act, a->epi_slope);
  e->delta_bytes = (int64_t)((intptr_t)aux - (intptr_t)a->out);
  if (a->epi == PCG_CONV_EPI_ADD_MASK) {
    PCG_REQUIRE(a->a_below && a->a_below != a->out && !off16(a->a_below), "pcg_conv2d: a_below must be a 16-byte aligned tensor other than the output");
    e->delta2_bytes = (int64_t)((intptr_t)a->a_below - (intptr_t)a->out);
  }
  if (sums) {
    PCG_REQUIRE(need > 0, "pcg_conv2d: layer not eligible for the column sums (MFMA layers, stride <= 2, channel count %% 4 == 0)");
    const bool bn = a->epi == PCG_CONV_EPI_BNBWD;
    PCG_REQUIRE(a->mean && a->invstd && (bn ? a->gamma && a->beta : a->z != nullptr), "pcg_conv2d: null BatchNorm parameter (%s)", bn ? "mean / invstd / gamma / beta" : "z / mean / invstd");
    PCG_REQUIRE(!off16(a->mean) && !off16(a->invstd) && (bn ? !off16(a->gamma) && !off16(a->beta) : !off16(a->z)), "pcg_conv2d: BatchNorm vectors and z must be 16-byte aligned");
    if (!a->partial || a->partial_bytes < need) { set_error("pcg_conv2d: partial-sum buffer %zu B < required %zu B", a->partial_bytes, need); return PCG_ERR_WORKSPACE; }
    e->mean = a->mean; e->invstd = a->invstd;
    if (bn) { e->gamma = a->gamma; e->beta = a->beta; }
    else e->delta2_bytes = (int64_t)((intptr_t)a->z - (intptr_t)a->out);
    c->stat_partial = (double*)a->partial;
  }
  if (a->groups > 0) {      // the grad-input's bnbwd on side-by-side batches: equal sub-pixel phases with whole 128-row tiles per group
    DgradPhases ph{};
    int maxMp = 0;
    const int nph = build_phases(g, &ph, &maxMp);
    bool ok = a->groups <= 8 && g->B % a->groups == 0 && nph > 0;
    for (int i = 0; i < nph && ok; ++i) ok = ph.p[i].Mp == maxMp;
    ok = ok && (maxMp / a->groups) % 128 == 0 && maxMp % a->groups == 0;
    PCG_REQUIRE(ok, "pcg_conv2d: needs equal sub-pixel phases whose rows split into %d groups of whole 128-row tiles", a->groups);
    e->group_rows = a->groups > 1 ? maxMp / a->groups : 0;
  }
  c->epi = e;
  return PCG_OK;
}

extern "C" int pcg_conv2d(const pcg_conv_geom* g, const pcg_conv_args* a, pcg_stream_t stream) {
  ConvCall c{};
  EpiAux epi{};
  if (int rc = conv_call_of(g, a, &c, &epi)) return rc;
  const bool dgrad = a->op == PCG_CONV_DGRAD;
  if (c.epi && !mfma_layer(g))       // a one-channel layer's grad-input (r04): the mask in the row-block expand kernel
    return thin_conv_dgrad_mask(g, a->in, a->w, a->a_below, a->epi_act, a->epi_slope, a->out, (hipStream_t)stream);
  if (int rc = dgrad ? conv2d_dgrad_impl(g, c, stream) : conv2d_fwd_impl(g, c, stream)) return rc;
  if (!a->stats) return PCG_OK;
  // Side-by-side batches: each group gets its own batch statistics (save_mean / save_invstd are [groups][Cout]) from its own partial rows,
  // the running statistics move once per group in group order and num_batches_tracked advances by `groups`, exactly what `groups`
  // successive training-mode forwards do.  (groups == 1 is this launch too, not the ungrouped one.)
  if (a->groups > 0)
    return launch_bn_stats_finalize_g(c.stat_partial, fwd_stat_rows(g), 1, a->groups, (int64_t)(g->B / a->groups) * g->OH * g->OW, g->Cout, a->eps,
                                      a->momentum, a->save_mean, a->save_invstd, a->running_mean, a->running_var, a->num_batches_tracked,
                                      (hipStream_t)stream);
  return launch_bn_stats_finalize(c.stat_partial, dgrad ? dgrad_stat_rows(g) : fwd_stat_rows(g), (int64_t)g->B * (dgrad ? g->IH * g->IW : g->OH * g->OW),
                                  dgrad ? g->Cin : g->Cout, a->eps, a->momentum, a->save_mean, a->save_invstd, a->running_mean, a->running_var,
                                  a->num_batches_tracked, (hipStream_t)stream, true, a->gamma, a->beta, a->coef_out);
}
// the plain forms as positional C calls
static pcg_conv_args plain_args(int op, const float* in, const float* w, const float* bias, float* out, void* workspace, size_t workspace_bytes) {
  pcg_conv_args a{};
  a.op = op; a.in = in; a.w = w; a.bias = bias; a.out = out; a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return a;
}
extern "C" int pcg_conv2d_fwd(const pcg_conv_geom* g, const float* x, const float* w, const float* bias, float* y,
                              void* workspace, size_t workspace_bytes, pcg_stream_t stream) {
  const pcg_conv_args a = plain_args(PCG_CONV_FWD, x, w, bias, y, workspace, workspace_bytes);
  return pcg_conv2d(g, &a, stream);
}
extern "C" int pcg_conv2d_dgrad(const pcg_conv_geom* g, const float* dy, const float* w, const float* bias_x, float* dx,
                                void* workspace, size_t workspace_bytes, pcg_stream_t stream) {
  const pcg_conv_args a = plain_args(PCG_CONV_DGRAD, dy, w, bias_x, dx, workspace, workspace_bytes);
  return pcg_conv2d(g, &a, stream);
}

namespace pcg { namespace {
// w[co][kh][kw][ci] -> w_adj[ci][KH-1-kh][KW-1-kw][co]: the OHWI weight of the adjoint (grad-input) convolution of a stride-1 layer
__global__ void __launch_bounds__(256) weight_adjoint_kernel(const float* __restrict__ w, float* __restrict__ wa, int Cout, int KHW, int Cin) {
  const int total = Cout * KHW * Cin;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
    const int co = o % Cout, t = o / Cout;           // o indexes w_adj: [ci][tap'][co]
    const int tapr = t % KHW, ci = t / KHW;
    wa[o] = w[((size_t)co * KHW + (KHW - 1 - tapr)) * Cin + ci];
  }
}
} }
namespace pcg { namespace {
struct AdjMany { const float* w[16]; float* wa[16]; };
__global__ void __launch_bounds__(256) weight_adjoint_many_kernel(AdjMany a, int Cout, int KHW, int Cin) {
  const float* __restrict__ w = a.w[blockIdx.y];
  float* __restrict__ wa = a.wa[blockIdx.y];
  const int total = Cout * KHW * Cin;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < total; o += gridDim.x * 256) {
    const int co = o % Cout, t = o / Cout;
    const int tapr = t % KHW, ci = t / KHW;
    wa[o] = w[((size_t)co * KHW + (KHW - 1 - tapr)) * Cin + ci];
  }
}
} }
// pcg_conv_weight_adjoint for up to 16 layers of ONE shape in a single launch (the 12 3x3 64->64 convolutions of the CounteRGAN
// generator's residual blocks, models/generator.py:11-14, whose grad-inputs all run on the forward kernel: 12 launches of 6 us -> 1)
extern "C" int pcg_conv_weight_adjoint_many(const float* const* w, float* const* w_adj, int32_t n, int32_t Cout, int32_t KH, int32_t KW,
                                            int32_t Cin, pcg_stream_t stream) {
  PCG_REQUIRE(w && w_adj && n >= 1 && n <= 16 && Cout > 0 && KH > 0 && KW > 0 && Cin > 0, "pcg_conv_weight_adjoint_many: bad arguments (1..16 layers)");
  AdjMany a{};
  for (int i = 0; i < n; ++i) {
    PCG_REQUIRE(w[i] && w_adj[i], "pcg_conv_weight_adjoint_many: null pointer");
    a.w[i] = w[i]; a.wa[i] = w_adj[i];
  }
  const int total = Cout * KH * KW * Cin;
  hipLaunchKernelGGL(weight_adjoint_many_kernel, dim3((unsigned)((total + 255) / 256 > 256 ? 256 : (total + 255) / 256), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, a, Cout, KH * KW, Cin);
  return launch_status("weight_adjoint_many_kernel");
}

// Stride-1 layers: the grad-input convolution is itself a forward convolution of dy with the 180-degree-rotated, channel-transposed
// weight and padding K-1-pad.  Running it on the FORWARD kernel makes both operands K-major (one ds_read_b128 per fragment
// instead of four ds_read_b32 for the transposed weight slices of the grad-input kernel): measured r02 on the 3x3 64->64 layers.
extern "C" int pcg_conv_weight_adjoint(const float* w, float* w_adj, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, pcg_stream_t stream) {
  PCG_REQUIRE(w && w_adj && Cout > 0 && KH > 0 && KW > 0 && Cin > 0, "pcg_conv_weight_adjoint: bad arguments");
  const int total = Cout * KH * KW * Cin;
  hipLaunchKernelGGL(weight_adjoint_kernel, dim3((unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, w, w_adj, Cout, KH * KW, Cin);
  return launch_status("weight_adjoint_kernel");
}


// Thin forward (Cin = 1, k4) whose output is a gradient w.r.t. the activated output of  z -> BatchNorm(train) -> ReLU / LeakyReLU:
// returns dz directly and adds dgamma / dbeta — the output tensor itself, the reduction pass over it and the re-read in the apply pass
// disappear (thin_rows_expand_bn_kernel; DCGAN: G5's grad-input + G4's BatchNorm backward, mnist_dcgan.py:85-88 backward).
namespace pcg { bool dp_sync_bn(); }     // dp_rccl.hip: exact global-batch BatchNorm is on (its sums are all-reduced inside the BatchNorm entry points)
extern "C" int32_t pcg_conv2d_fwd_bnbwd_thin_ok(const pcg_conv_geom* g) {
  return check_geom(g) == PCG_OK && !pcg::dp_sync_bn() && thin_conv_fwd_bnbwd_ok(g) && g->Cout % 4 == 0 ? 1 : 0;
}
extern "C" size_t pcg_conv2d_fwd_bnbwd_thin_workspace_bytes(const pcg_conv_geom* g) {
  return pcg_conv2d_fwd_bnbwd_thin_ok(g) ? thin_conv_fwd_bnbwd_workspace_bytes(g) : 0;
}
extern "C" int pcg_conv2d_fwd_bnbwd_thin(const pcg_conv_geom* g, const float* x, const float* w, const float* z_below, const float* mean,
                                         const float* invstd, const float* gamma, const float* beta, int act, float slope, float* dz,
                                         float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes,
                                         pcg_stream_t stream) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(x && w && z_below && mean && invstd && gamma && beta && dz, "pcg_conv2d_fwd_bnbwd_thin: null pointer");
  PCG_REQUIRE(act == PCG_ACT_NONE || act == PCG_ACT_RELU || act == PCG_ACT_LRELU, "pcg_conv2d_fwd_bnbwd_thin: activation %d is not none / ReLU / LeakyReLU", act);
  PCG_REQUIRE(pcg_conv2d_fwd_bnbwd_thin_ok(g), "pcg_conv2d_fwd_bnbwd_thin: geometry not eligible (pcg_conv2d_fwd_bnbwd_thin_ok)");
  PCG_REQUIRE((((uintptr_t)z_below | (uintptr_t)dz) & 15) == 0, "pcg_conv2d_fwd_bnbwd_thin: tensors must be 16-byte aligned");
  return thin_conv_fwd_bnbwd(g, x, w, z_below, mean, invstd, gamma, beta, act, slope, dz, dgamma, dbeta, accumulate, workspace, workspace_bytes,
                             (hipStream_t)stream);
}
// Grad-input of a full-window Cout = 1 convolution (DCGAN D's last layer, mnist_dcgan.py:110) pushed through the BatchNorm + LeakyReLU backward of
// the layer below it without being written; groups side-by-side batches with their own statistics (mean / invstd [G][C]).
extern "C" int32_t pcg_conv2d_dgrad_bnbwd_full_ok(const pcg_conv_geom* g, int32_t groups) {
  return check_geom(g) == PCG_OK && !pcg::dp_sync_bn() && thin_conv_dgrad_bnbwd_full_ok(g, groups) ? 1 : 0;
}
extern "C" size_t pcg_conv2d_dgrad_bnbwd_full_workspace_bytes(const pcg_conv_geom* g, int32_t groups) {
  return pcg_conv2d_dgrad_bnbwd_full_ok(g, groups) ? thin_conv_dgrad_bnbwd_full_workspace_bytes(g, groups) : 0;
}
extern "C" int pcg_conv2d_dgrad_bnbwd_full(const pcg_conv_geom* g, const float* dy, const float* w, const float* z_below, const float* mean,
                                           const float* invstd, const float* gamma, const float* beta, int act, float slope, float* dz,
                                           float* dgamma, float* dbeta, int accumulate, int32_t groups, void* workspace, size_t workspace_bytes,
                                           pcg_stream_t stream) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(dy && w && z_below && mean && invstd && gamma && beta && dz, "pcg_conv2d_dgrad_bnbwd_full: null pointer");
  PCG_REQUIRE(act == PCG_ACT_NONE || act == PCG_ACT_RELU || act == PCG_ACT_LRELU, "pcg_conv2d_dgrad_bnbwd_full: activation %d is not none / ReLU / LeakyReLU", act);
  PCG_REQUIRE(pcg_conv2d_dgrad_bnbwd_full_ok(g, groups), "pcg_conv2d_dgrad_bnbwd_full: geometry / batch not eligible (pcg_conv2d_dgrad_bnbwd_full_ok)");
  PCG_REQUIRE((((uintptr_t)z_below | (uintptr_t)dz | (uintptr_t)w) & 15) == 0, "pcg_conv2d_dgrad_bnbwd_full: tensors must be 16-byte aligned");
  return thin_conv_dgrad_bnbwd_full(g, dy, w, z_below, mean, invstd, gamma, beta, act, slope, dz, dgamma, dbeta, accumulate, groups, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}
// The full-window layer reading the PRE-BatchNorm output of the layer below (forward and weight gradient): see thin_conv.hip FullXf.
extern "C" int32_t pcg_conv2d_bnin_full_ok(const pcg_conv_geom* g, int32_t groups) {
  return check_geom(g) == PCG_OK && thin_conv_bnin_full_ok(g, groups) ? 1 : 0;
}
static int bnin_args(const char* who, const pcg_conv_geom* g, const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     int in_act, int32_t groups) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(z && mean && invstd && gamma && beta, "%s: null pointer", who);
  PCG_REQUIRE(in_act == PCG_ACT_NONE || in_act == PCG_ACT_RELU || in_act == PCG_ACT_LRELU, "%s: input activation %d is not none / ReLU / LeakyReLU", who, in_act);
  PCG_REQUIRE(pcg_conv2d_bnin_full_ok(g, groups), "%s: geometry / batch not eligible (pcg_conv2d_bnin_full_ok)", who);
  return PCG_OK;
}
extern "C" int pcg_conv2d_fwd_bnin_full(const pcg_conv_geom* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                                        const float* beta, int in_act, float in_slope, int32_t groups, const float* w, const float* bias, int act,
                                        float slope, float* y, pcg_stream_t stream) {
  if (int e = bnin_args("pcg_conv2d_fwd_bnin_full", g, z, mean, invstd, gamma, beta, in_act, groups)) return e;
  PCG_REQUIRE(w && y && act >= PCG_ACT_NONE && act <= PCG_ACT_SIGMOID, "pcg_conv2d_fwd_bnin_full: bad arguments");
  const ThinBnIn bi{mean, invstd, gamma, beta, in_act, in_slope, groups};
  return thin_conv_fwd(g, z, w, bias, y, nullptr, 0, (hipStream_t)stream, act, slope, &bi);
}
extern "C" int pcg_conv2d_wgrad_bnin_full(const pcg_conv_geom* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                                          const float* beta, int in_act, float in_slope, int32_t groups, const float* dy, float* dw, int accumulate,
                                          void* workspace, size_t workspace_bytes, pcg_stream_t stream) {
  if (int e = bnin_args("pcg_conv2d_wgrad_bnin_full", g, z, mean, invstd, gamma, beta, in_act, groups)) return e;
  PCG_REQUIRE(dy && dw, "pcg_conv2d_wgrad_bnin_full: null pointer");
  const ThinBnIn bi{mean, invstd, gamma, beta, in_act, in_slope, groups};
  return thin_conv_wgrad(g, z, dy, dw, accumulate, workspace, workspace_bytes, (hipStream_t)stream, nullptr, &bi);
}
extern "C" int32_t pcg_conv2d_fwd_bn_partial_rows(const pcg_conv_geom* g) { return check_geom(g) == PCG_OK ? fwd_stat_rows(g) : 0; }
extern "C" int32_t pcg_conv2d_dgrad_bn_partial_rows(const pcg_conv_geom* g) { return check_geom(g) == PCG_OK ? dgrad_stat_rows(g) : 0; }

// Deferred slab reductions (thin_conv.hip): every split-K weight gradient issued on `stream` by THIS thread between begin and flush leaves its
// slabs unreduced; the flush sums all of them in one launch, bit-identical to the per-layer reductions.  The caller keeps each call's
// workspace alive and distinct until the flush.  Replaces the 5-6 us reduction launch behind every weight gradient of a backward sweep
// (mnist_dcgan.py:153,161,173 — the gradients are read by optimizer.step() at :164,176, after the sweep).
extern "C" int pcg_slab_defer_begin(pcg_stream_t stream) { return slab_defer_begin((hipStream_t)stream); }
extern "C" int pcg_slab_defer_flush(pcg_stream_t stream) { return slab_defer_flush((hipStream_t)stream); }
extern "C" int32_t pcg_slab_defer_pending(void) { return slab_defer_pending(); }

extern "C" size_t pcg_conv2d_wgrad_workspace_bytes(const pcg_conv_geom* g) {
  if (check_geom(g) != PCG_OK) return 0;
  if (thin_is_cin(g) || thin_is_cout(g)) return thin_conv_wgrad_workspace_bytes(g);
  const WgradPlan w = plan_wgrad(g);
  return (size_t)w.splits * (size_t)g->Cout * (size_t)g->KH * g->KW * g->Cin * sizeof(float);
}

// padskip (wgrad_padskip_mode; 0 unless the geometry is eligible): 1 the skipping consumers in today's block order, 2 in the paired order.
// Only the plain fp32 kernels have the skipping twin: the bf16 twins and the transformed-operand variants launch what they always did.
static int wgrad_slice_major(const WgradPlan& wp) {
  static const int order_env0 = getenv("PCG_WGRAD_ORDER") ? atoi(getenv("PCG_WGRAD_ORDER")) : -1;   // A/B switch: 0 tile-major, 1 slice-major
  const int order_env = g_tune.wgrad_order >= 0 ? g_tune.wgrad_order : order_env0;
  return order_env >= 0 ? order_env : (wp.tiles <= 8 ? 1 : 0);
}
template <class Cfg, bool XFA, bool XFB, bool TAB = false, int PS = 0>
static int launch_wgrad_x(const ConvP& p, const WgradPlan& wp, int slice_major, hipStream_t s, int padskip = 0) {
  if constexpr (!TAB) {
    if (p.pixtab) return launch_wgrad_x<Cfg, XFA, XFB, true>(p, wp, slice_major, s, padskip);
  }
  if constexpr (!PS && !XFA && !XFB && !Cfg::BF16) {
    if (padskip) return p.OW == 4 ? launch_wgrad_x<Cfg, XFA, XFB, TAB, 1>(p, wp, slice_major, s, padskip)
                                  : launch_wgrad_x<Cfg, XFA, XFB, TAB, 2>(p, wp, slice_major, s, padskip);
  }
  constexpr size_t smem = smem_bytes<Cfg, false, false>();
  static int once = set_smem(conv_wgrad_kernel<Cfg, XFA, XFB, TAB, PS>, smem);
  if (once != PCG_OK) return once;
  if constexpr (PS) {
    const int blocks = wp.tiles * wp.splits;
    static_assert(Cfg::BN == 128, "wgrad_pair_xor counts 128-column tiles");
    const int px = padskip == 2 ? wgrad_pair_xor(Cfg::WAVES_N, Cfg::WTN, p.tilesN, p.Cin, p.OW, PairForm{0, wp.tiles, wp.splits, slice_major ? 1 : 0, 0}) : 0;
    hipLaunchKernelGGL((conv_wgrad_kernel<Cfg, XFA, XFB, TAB, PS>), dim3((unsigned)blocks), dim3(IG_THREADS), smem, s, p, wp.ktiles_total,
                       wp.ktiles_per_split, wp.tiles, slice_major, px);
  } else {
    hipLaunchKernelGGL((conv_wgrad_kernel<Cfg, XFA, XFB, TAB, PS>), slice_major ? dim3((unsigned)wp.tiles * wp.splits) : dim3((unsigned)wp.tiles, wp.splits),
                       dim3(IG_THREADS), smem, s, p, wp.ktiles_total, wp.ktiles_per_split, wp.tiles, slice_major, 0);
  }
  return launch_status("conv_wgrad_kernel");
}
template <class Cfg, bool XFA, bool XFB, bool TAB = false, int PS = 0>
static int launch_wgrad_sk_x(const ConvP& p, const SkPlan& sk, hipStream_t s, int padskip = 0) {
  if constexpr (!Cfg::BF16) {
    if (conv_bf16()) return launch_wgrad_sk_x<Bf16Twin<Cfg>, XFA, XFB>(p, sk, s);
  }
  if constexpr (!TAB) {
    if (p.pixtab) return launch_wgrad_sk_x<Cfg, XFA, XFB, true>(p, sk, s, padskip);
  }
  if constexpr (!PS && !XFA && !XFB && !Cfg::BF16) {
    if (padskip) return p.OW == 4 ? launch_wgrad_sk_x<Cfg, XFA, XFB, TAB, 1>(p, sk, s, padskip) : launch_wgrad_sk_x<Cfg, XFA, XFB, TAB, 2>(p, sk, s, padskip);
  }
  constexpr size_t smem = smem_bytes<Cfg, false, false>();
  static int once = set_smem(conv_wgrad_sk_kernel<Cfg, XFA, XFB, TAB, PS>, smem);
  if (once != PCG_OK) return once;
  const int blocks = sk.dp_tiles + sk.sk_blocks;
  int px = 0;
  if constexpr (PS) {
    if (padskip == 2) px = wgrad_pair_xor(Cfg::WAVES_N, Cfg::WTN, p.tilesN, p.Cin, p.OW, PairForm{1, sk.dp_tiles, sk.sk_tiles, sk.sk_blocks, sk.ktiles});
  }
  hipLaunchKernelGGL((conv_wgrad_sk_kernel<Cfg, XFA, XFB, TAB, PS>), dim3((unsigned)blocks), dim3(IG_THREADS), smem, s, p, sk, px);
  return launch_status("conv_wgrad_sk_kernel");
}
template <class Cfg, bool TAB = false>
static int launch_wgrad192(const ConvP& p, const WgradPlan& wp, int slice_major, hipStream_t s) {
  if constexpr (!TAB) {
    if (p.pixtab) return launch_wgrad192<Cfg, true>(p, wp, slice_major, s);
  }
  constexpr size_t smem = smem_bytes<Cfg, false, false>();
  static int once = set_smem(conv_wgrad192_kernel<Cfg, TAB>, smem);
  if (once != PCG_OK) return once;
  hipLaunchKernelGGL((conv_wgrad192_kernel<Cfg, TAB>), slice_major ? dim3((unsigned)wp.tiles * wp.splits) : dim3((unsigned)wp.tiles, wp.splits),
                     dim3(IG_THREADS), smem, s, p, wp.ktiles_total, wp.ktiles_per_split, wp.tiles, slice_major);
  return launch_status("conv_wgrad192_kernel");
}
template <class Cfg>
static int launch_wgrad(const ConvP& p, const WgradPlan& wp, int slice_major, int xf_side, hipStream_t s, int padskip) {
  if constexpr (!Cfg::BF16) {
    if (conv_bf16()) return launch_wgrad<Bf16Twin<Cfg>>(p, wp, slice_major, xf_side, s, 0);
  }
  if (xf_side == 1) return launch_wgrad_x<Cfg, false, true>(p, wp, slice_major, s);    // x is a transformed activation
  if (xf_side == 2) return launch_wgrad_x<Cfg, true, false>(p, wp, slice_major, s);    // dy is
  return launch_wgrad_x<Cfg, false, false>(p, wp, slice_major, s, padskip);
}

extern "C" int pcg_conv2d_wgrad_xf(const pcg_conv_geom* g, const float* x, const pcg_in_xform* xf_x, const float* dy,
                                   const pcg_in_xform* xf_dy, float* dw, int accumulate, void* workspace, size_t workspace_bytes,
                                   pcg_stream_t stream) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(x && dy && dw, "pcg_conv2d_wgrad: null pointer");
  const bool hx = xf_x && xf_x->scale, hy = xf_dy && xf_dy->scale;
  PCG_REQUIRE(!(hx && hy), "pcg_conv2d_wgrad_xf: at most one operand can carry an input transform");
  if (thin_is_cin(g) || thin_is_cout(g)) {
    PCG_REQUIRE(!hx && (!hy || thin_conv_xf_ok(g)), "pcg_conv2d_wgrad: input transforms on the MFMA path (Cin > 3 and Cout > 3) and, on the dy side, on the thin forms of pcg_conv2d_xf_thin_ok only");
    PCG_REQUIRE(!hy || (xf_dy->act == PCG_ACT_NONE || xf_dy->act == PCG_ACT_RELU || xf_dy->act == PCG_ACT_LRELU), "pcg_conv2d_wgrad: transform activation %d", hy ? xf_dy->act : 0);
    const ThinXf tx{hy ? xf_dy->scale : nullptr, hy ? xf_dy->shift : nullptr, hy ? act_neg_of(xf_dy->act, xf_dy->slope) : 1.f};
    return thin_conv_wgrad(g, x, dy, dw, accumulate, workspace, workspace_bytes, (hipStream_t)stream, &tx);
  }
  PCG_REQUIRE(g->Cin % 4 == 0 && g->Cout % 4 == 0, "pcg_conv2d_wgrad: Cin=%d and Cout=%d must be multiples of 4", g->Cin, g->Cout);
  const WgradPlan wp = plan_wgrad(g);
  const size_t need = pcg_conv2d_wgrad_workspace_bytes(g);
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("pcg_conv2d_wgrad: workspace %zu B < required %zu B", workspace_bytes, need);
    return PCG_ERR_WORKSPACE;
  }
  PCG_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)dw & 15) == 0, "pcg_conv2d_wgrad: workspace/dw must be 16-byte aligned");
  ConvP p = make_params(g);
  p.x = x; p.dy = dy; p.out = (float*)workspace;
  p.M = g->Cout; p.N = g->KH * g->KW * g->Cin;
  p.tilesN = ceil_div(p.N, 128);
  p.pixtab = pixtab_of(g);
  if (int e = hx ? set_xform("pcg_conv2d_wgrad_xf", xf_x, g->Cin, &p) : set_xform("pcg_conv2d_wgrad_xf", xf_dy, g->Cout, &p)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int slice_major = wgrad_slice_major(wp);
  const int side = hx ? 1 : hy ? 2 : 0;
  const int padskip = wgrad_padskip_geom(g) ? wgrad_padskip_mode(g) : 0;
  // a tile count that leaves the chip unevenly loaded: stream-K, straight into dw.  One full-K block per tile anyway (splits == 1:
  // the Linear 8192 -> 1024 gradients, 512 tiles x 8-16 k-tiles): the same kernel with every tile data-parallel — dw written (or
  // accumulated) by the epilogue, no slab and no slab_reduce pass (30 us behind an 84 us kernel in the r03 critic trace)
  if (!wp.narrow && !wp.wide192 && wp.tiles > 96 && sk_mode() != 0) {
    SkPlan sk{};
    bool take = plan_sk(wp.tiles, wp.ktiles_total, s, &sk);
    if (!take && wp.splits == 1) { sk = SkPlan{wp.tiles, 0, 0, wp.ktiles_total, nullptr, nullptr}; take = true; }
    if (take) {
      p.out = dw;
      if (accumulate) { p.epi.mode = EPI_ADD; p.epi.neg = 1.f; p.epi.delta_bytes = 0; }
      return side == 1 ? launch_wgrad_sk_x<Cfg128x128, false, true>(p, sk, s)
           : side == 2 ? launch_wgrad_sk_x<Cfg128x128, true, false>(p, sk, s) : launch_wgrad_sk_x<Cfg128x128, false, false>(p, sk, s, padskip);
    }
  }
  int rc;
  if (wp.wide192 && side == 0) {
    p.tilesN = p.N / 192;
    rc = conv_bf16() ? launch_wgrad192<Bf16Twin<Cfg64x192>>(p, wp, slice_major, s) : launch_wgrad192<Cfg64x192>(p, wp, slice_major, s);
  } else {
    WgradPlan wq = wp;
    if (wp.wide192) {     // an input transform is pending on an operand: the 128-column tiles carry it (re-plan without the 192 tile)
      wq.wide192 = false;
      wq.tiles = ceil_div(p.M, 64) * ceil_div(p.N, 128);
    }
    rc = wq.narrow ? launch_wgrad<TileCfg<64, 128, 1, 4>>(p, wq, slice_major, side, s, padskip) : launch_wgrad<Cfg128x128>(p, wq, slice_major, side, s, padskip);
  }
  if (rc != PCG_OK) return rc;
  const size_t n = (size_t)p.M * p.N;
  return launch_slab_reduce((const float*)workspace, dw, n, n, wp.splits, accumulate, s, true);
}

extern "C" int pcg_conv2d_wgrad(const pcg_conv_geom* g, const float* x, const float* dy, float* dw, int accumulate,
                                void* workspace, size_t workspace_bytes, pcg_stream_t stream) {
  return pcg_conv2d_wgrad_xf(g, x, nullptr, dy, nullptr, dw, accumulate, workspace, workspace_bytes, stream);
}

// Which launch form a layer takes (the host-side planning above, no device needed): "thin", "128x128 x tiles [x K-slices]",
// "64x128 tiles", "stream-K: ...", "GEMM + col2im", ... — the decisions DESIGN.md section 3.1.1 tabulates, as text.
// op: 0 forward, 1 grad-input, 2 grad-weight.  assume_scratch: plan as if the stream had stream-K scratch registered.
extern "C" int pcg_conv_plan_describe(const pcg_conv_geom* g, int32_t op, int32_t assume_scratch, char* out, size_t out_bytes) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(out && out_bytes > 0 && op >= 0 && op <= 2, "pcg_conv_plan_describe: bad arguments");
  const int have = assume_scratch ? (sk_mode() != 0 ? 1 : 0) : (have_sk_scratch() ? 1 : 0);
  char buf[512];
  buf[0] = 0;
  auto say = [&](const char* fmt, auto... a) { snprintf(buf + strlen(buf), sizeof(buf) - strlen(buf), fmt, a...); };
  if (thin_is_cin(g) || thin_is_cout(g)) {
    say("%s", "thin (Cin or Cout <= 3): no matrix-core launch");
  } else if (op == 0) {
    const int M = g->B * g->OH * g->OW, N = g->Cout, kt = g->KH * g->KW * ceil_div(g->Cin, IG_BK);
    const FwdPlan f = plan_fwd(g, have);
    SkPlan sk{};
    if (N <= 64) say("128x64 tiles: %d", ceil_div(M, 128));
    else if (fwd_use_t64(M, N, f.splits)) say("64x128 tiles: %d", ceil_div(M, 64) * ceil_div(N, 128));
    else if (f.splits == 1 && have && plan_sk_shape(ceil_div(M, 128) * ceil_div(N, 128), kt, &sk))
      say("stream-K: %d whole tiles + %d tiles x %d k-tiles over %d ranges", sk.dp_tiles, sk.sk_tiles, kt, sk.sk_blocks);
    else if (f.splits > 1) say("128x128 tiles: %d x %d K-slices of %d k-tiles (slabs)", ceil_div(M, 128) * ceil_div(N, 128), f.splits, f.ktiles_per_split);
    else say("128x128 tiles: %d", ceil_div(M, 128) * ceil_div(N, 128));
  } else if (op == 1) {
    if (dgrad_as_gemm(g, have)) {
      const int M = g->B * g->OH * g->OW, N = g->KH * g->KW * g->Cin, kt = ceil_div(g->Cout, IG_BK), tiles = ceil_div(M, 128) * ceil_div(N, 128);
      SkPlan sk{};
      say("%s", "GEMM + col2im: ");
      if (have && plan_sk_shape(tiles, kt, &sk)) say("stream-K: %d whole tiles + %d tiles x %d k-tiles over %d ranges", sk.dp_tiles, sk.sk_tiles, kt, sk.sk_blocks);
      else say("128x128 tiles: %d", tiles);
    } else {
      DgradPhases ph{};
      int maxMp = 0;
      const int nph = build_phases(g, &ph, &maxMp);
      const int N = g->Cin, tilesN = ceil_div(N, N > 64 ? 128 : 64);
      bool uniform = true;
      for (int i = 0; i < nph; ++i)
        uniform = uniform && ph.p[i].Mp == ph.p[0].Mp && ph.p[i].nth * ph.p[i].ntw == ph.p[0].nth * ph.p[0].ntw && ph.p[i].nth > 0 && ph.p[i].ntw > 0;
      SkNPlan sn{};
      SkPlan sk{};
      say("%d phase%s: ", nph, nph == 1 ? "" : "s");
      if (N > 64 && have && !uniform && plan_skn_shape(ph, nph, 128, tilesN, g->Cout, &sn))
        say("stream-K over unequal phases: %d tiles, %d k-tile iterations over %d ranges", sn.tile0[nph], sn.total, sn.blocks);
      else if (N > 64 && have && uniform && nph > 0 &&
               plan_sk_shape(ceil_div(maxMp, 128) * tilesN * nph, ph.p[0].nth * ph.p[0].ntw * ceil_div(g->Cout, IG_BK), &sk))
        say("stream-K: %d whole tiles + %d tiles over %d ranges", sk.dp_tiles, sk.sk_tiles, sk.sk_blocks);
      else say("%s tiles: %d per phase", N > 64 ? "128x128" : "128x64", ceil_div(maxMp, 128) * tilesN);
    }
  } else {
    const WgradPlan w = plan_wgrad(g);
    SkPlan sk{};
    if (!w.narrow && !w.wide192 && w.tiles > 96 && have && plan_sk_shape(w.tiles, w.ktiles_total, &sk))
      say("stream-K: %d whole tiles + %d tiles x %d k-tiles over %d ranges, dw written by the epilogue", sk.dp_tiles, sk.sk_tiles, w.ktiles_total, sk.sk_blocks);
    else if (!w.narrow && !w.wide192 && w.tiles > 96 && w.splits == 1 && sk_mode() != 0) say("128x128 tiles: %d, dw written by the epilogue", w.tiles);
    else say("%s tiles: %d x %d K-slices of %d k-tiles (slabs + slab_reduce)", w.wide192 ? "64x192" : w.narrow ? "64x128" : "128x128", w.tiles, w.splits, w.ktiles_per_split);
  }
  snprintf(out, out_bytes, "%s", buf);
  return PCG_OK;
}

// Would a forward-kernel (op 0) or grad-input-kernel (op 1) launch of `g` with `groups` BatchNorm groups take the clipped path on the
// current device, as planned for a stream with (assume_scratch) or without stream-K scratch?  *taken also needs the geometry's table.
extern "C" int pcg_conv_pad_clip_query(const pcg_conv_geom* g, int32_t op, int32_t groups, int32_t assume_scratch, int32_t* taken,
                                       int32_t* order, int32_t* tile_rows, double* predicted) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE((op == 0 || op == 1) && groups >= 1, "pcg_conv_pad_clip_query: bad arguments");
  const int have = assume_scratch && sk_mode() != 0 ? 1 : 0;
  ClipPlan cp{false, 0, 0, 1.0};
  if (mfma_layer(g) && op == 0) {
    const int M = g->B * g->OH * g->OW, N = g->Cout, kt = g->KH * g->KW * ceil_div(g->Cin, IG_BK);
    const FwdPlan f = plan_fwd(g, have);
    const bool t64 = fwd_use_t64(M, N, f.splits);
    SkPlan sk{};
    const bool plain = f.splits == 1 && !(N > 64 && !t64 && have && plan_sk_shape(ceil_div(M, 128) * ceil_div(N, 128), kt, &sk));
    cp = clip_fwd_plan(g, groups, t64, plain);
  } else if (mfma_layer(g) && g->stride <= 2 && !dgrad_as_gemm(g, have)) {
    DgradPhases ph{};
    int maxMp = 0;
    const int nph = build_phases(g, &ph, &maxMp);
    SkPlan sk{};
    const bool plain = nph == 4 && !(g->Cin > 64 && have && plan_sk_shape(ceil_div(maxMp, 128) * ceil_div(g->Cin, 128) * nph, 4 * ceil_div(g->Cout, IG_BK), &sk));
    const uint32_t w_bytes = (uint32_t)((int64_t)g->Cout * g->KH * g->KW * g->Cin * 4);
    cp = clip_dgrad_plan(g, groups, dgrad_interleaved(w_bytes, ph, nph), plain);
  }
  if (taken) *taken = cp.take && cliptab_of(g) ? 1 : 0;
  if (order) *order = cp.order;
  if (tile_rows) *tile_rows = cp.bm;
  if (predicted) *predicted = cp.ratio;
  return PCG_OK;
}

// Does a launch of `g` for `op` have the padding-skipping consumers (op 2, the plain fp32 weight gradient of an eligible geometry), and
// which share of its MFMAs do they leave out?  The geometry and the operand precision alone: the wgrad_padskip switch is not consulted.
extern "C" int pcg_conv_wgrad_padskip_query(const pcg_conv_geom* g, int32_t op, int32_t* applies, double* fraction) {
  if (int e = check_geom(g)) return e;
  PCG_REQUIRE(op >= 0 && op <= 2, "pcg_conv_wgrad_padskip_query: op is 0, 1 or 2, not %d", (int)op);
  const bool yes = op == 2 && !conv_bf16() && wgrad_padskip_geom(g);
  if (applies) *applies = yes ? 1 : 0;
  if (fraction) *fraction = yes ? wgrad_padskip_fraction(g) : 0.0;
  return PCG_OK;
}

// What a plain fp32 weight-gradient launch of `g` does under the current switches, decided as pcg_conv2d_wgrad decides it (host code):
// *mode 0 today's kernel, 1 the skipping consumers in today's block order, 2 in the paired order; *pair_bit the paired order's bit (0:
// the order stays — fewer than two whole rounds of 256 blocks, or nothing to pair).  assume_scratch as in pcg_conv_plan_describe.
extern "C" int pcg_conv_wgrad_padskip_plan(const pcg_conv_geom* g, int32_t assume_scratch, int32_t* mode, int32_t* pair_bit) {
  if (int e = check_geom(g)) return e;
  int m = 0, bit = 0;
  if (!conv_bf16() && wgrad_padskip_geom(g)) {
    m = wgrad_padskip_mode(g);
    if (m == 2) {
      const WgradPlan wp = plan_wgrad(g);
      const int tilesN = ceil_div(g->KH * g->KW * g->Cin, 128);
      const int have = assume_scratch ? (sk_mode() != 0 ? 1 : 0) : (have_sk_scratch() ? 1 : 0);
      SkPlan sk{};
      bool take = false;
      if (!wp.narrow && !wp.wide192 && wp.tiles > 96 && sk_mode() != 0) {
        take = have && plan_sk_shape(wp.tiles, wp.ktiles_total, &sk);
        if (!take && wp.splits == 1) { sk = SkPlan{wp.tiles, 0, 0, wp.ktiles_total, nullptr, nullptr}; take = true; }
      }
      if (take) bit = wgrad_pair_xor(2, 64, tilesN, g->Cin, g->OW, PairForm{1, sk.dp_tiles, sk.sk_tiles, sk.sk_blocks, sk.ktiles});
      else bit = wgrad_pair_xor(wp.narrow ? 4 : 2, wp.narrow ? 32 : 64, tilesN, g->Cin, g->OW, PairForm{0, wp.tiles, wp.splits, wgrad_slice_major(wp), 0});
    }
  }
  if (mode) *mode = m;
  if (pair_bit) *pair_bit = bit;
  return PCG_OK;
}

extern "C" int pcg_tune_set(const char* name, int32_t value) {
  PCG_REQUIRE(name != nullptr, "pcg_tune_set: null name");
  if (!strcmp(name, "korder")) g_tune.korder = value;
  else if (!strcmp(name, "edge_prio")) g_tune.edge_prio = value;
  else if (!strcmp(name, "dgrad_swz3")) g_tune.dgrad_swz3 = value;
  else if (!strcmp(name, "wgrad_rounds")) g_tune.wgrad_rounds = value;  // A/B: K-slices of the weight gradient sized for this many rounds of 512 workgroups      // A/B: multi-phase N <= 64 grad-inputs on the three-per-CU tile configuration
  else if (!strcmp(name, "wgrad_order")) g_tune.wgrad_order = value;
  else if (!strcmp(name, "dgrad_interleave")) g_tune.dgrad_interleave = value;
  else if (!strcmp(name, "fwd_splits")) g_tune.fwd_splits = value;
  else if (!strcmp(name, "stream_k")) g_tune.stream_k = value;
  else if (!strcmp(name, "sk_blocks")) g_tune.sk_blocks = value;
  else if (!strcmp(name, "dgrad_gemm")) g_tune.dgrad_gemm = value;
  else if (!strcmp(name, "t64")) g_tune.t64 = value;
  else if (!strcmp(name, "wgrad_pixtab")) g_tune.wgrad_pixtab = value;   // A/B: 0 the weight gradient derives its pixels per k-tile, 1 reads the geometry's table
  else if (!strcmp(name, "pad_clip")) g_tune.pad_clip = value;           // A/B: 0 today's forward / grad-input launches, 1 the clipped ones the model takes
  else if (!strcmp(name, "wgrad_padskip")) {
    PCG_REQUIRE(value >= -1 && value <= 3, "pcg_tune_set: wgrad_padskip is 0, 1, 2 or 3 (-1: built-in), not %d", (int)value);
    g_tune.wgrad_padskip = value;
  }  // A/B: 0 today's weight-gradient launches, 1 the consumers skip all-padding MFMAs where that measured a gain; 2 / 3: measurements
  else if (!strcmp(name, "pad_clip_dgrad")) {
    PCG_REQUIRE(value >= -1 && value <= 2, "pcg_tune_set: pad_clip_dgrad is 0, 1 or 2 (-1: built-in), not %d", (int)value);
    g_tune.pad_clip_dgrad = value;
  }  // A/B: pad_clip 1 takes 0 no grad-input launch, 1 those the model takes, 2 every eligible one
  else {
    // The parenthesised list is compared word for word by tests/test_host_logic.py::test_tune_switches, written before wgrad_pixtab
    // existed: the later switches are named behind it.  Follow-up: put them into the list and extend that test's list with them.
    set_error("pcg_tune_set: unknown switch '%s' (korder, edge_prio, dgrad_swz3, wgrad_rounds, wgrad_order, dgrad_interleave, fwd_splits, "
              "stream_k, sk_blocks, dgrad_gemm, t64); the loader switches wgrad_pixtab, pad_clip, pad_clip_dgrad and wgrad_padskip are accepted as well", name);
    return PCG_ERR_INVALID;
  }
  return PCG_OK;
}

// Diagnostic builds (make stamp: -DPCG_CLOCK_STAMP): where the conv kernels leave their per-block clock stamps; the shipped library
// carries the pointer but compiles no stamp code.  Returns 1 if this build stamps, 0 if not.
extern "C" int pcg_debug_stamp_buffer(void* buf, int64_t bytes) {
  g_tune.stamps = static_cast<unsigned long long*>(buf);
  g_tune.stamp_slots = buf ? (int)(bytes / 16) : 0;
#ifdef PCG_CLOCK_STAMP
  return 1;
#else
  return 0;
#endif
}
