// conv_cliptab.h — tile descriptor table of a k4 s2 p1 geometry and the schedule model that decides who reads it (host side, plain
// C++: no HIP call, usable without a GPU; the block -> tile map is shared with the kernels).
//
// Zero padding is out-of-range gathers that return zeros, but the k-tile is still staged and multiplied.  With the rows of a tile in
// (image, oh, ow) order no tap is padding for ALL rows of a tile; with the rows in (position, image) order — every row of a tile is the
// same output pixel (forward form) or the same pixel of a sub-pixel phase grid (grad-input form) of different images — the taps that
// fall outside are the same for the whole tile, and the tile iterates only the rectangle of taps that do not (conv_loaders.h, CLIP).
//
// Table of a geometry, 5 * npos words (npos = OH * OW; IH = 2 OH and IW = 2 OW, so every sub-pixel phase grid is OH x OW as well):
//   words [0, npos)                     forward form, one descriptor per output pixel
//   words [(1 + py) * npos, +npos)      grad-input form, phase py = 2 * (ih % 2) + (iw % 2), one descriptor per phase pixel
// Each section is sorted by the size of the tap rectangle, largest first, positions of one size in raster order.  Descriptor:
//   bits 0..15 position (row * OW + column)   16..19 first tap row   20..23 tap rows   24..27 first tap column   28..31 tap columns
// (forward: taps (kh, kw) of the 4 x 4 window; grad-input: taps (jh, jw) of the phase's 2 x 2).
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define PCG_CLIP_HD __host__ __device__ __forceinline__
#else
#define PCG_CLIP_HD inline
#endif

namespace pcg {

// order of a launch's M tiles over the sorted list of (position, image block) pairs
enum { CLIP_LONG_FIRST = 0, CLIP_SHORT_FIRST = 1, CLIP_PAIRS = 2 };

// Block b of a 1-D grid of tilesM * per blocks (per = interleaved phases * N tiles) -> N tile / phase slot `within` and the index of
// its M tile in the sorted list.  Blocks go round-robin over the 8 XCDs: the `per` blocks that share an M tile (the same activation
// rows) stay on one XCD and follow each other there, and dispatch order walks the list in steps of 8 tiles.  tilesM % 8 == 0.
// CLIP_PAIRS: the list from both ends, tile by tile — or, where the phases of a grad-input are rows of a 2-D grid (y = blockIdx.y,
// ygrid), every other phase backwards: a phase's long tiles then run beside the next phase's short ones.
PCG_CLIP_HD void clip_block_tile(uint32_t b, uint32_t per, uint32_t tilesM, int order, bool ygrid, uint32_t y, uint32_t& within, uint32_t& idx) {
  const uint32_t q = b >> 3, x = b & 7u, r = q / per;
  within = q - r * per;
  const uint32_t mt = r * 8u + x, back = tilesM - 1u - mt;
  idx = order == CLIP_LONG_FIRST ? mt : order == CLIP_SHORT_FIRST ? back : ygrid ? ((y & 1u) ? back : mt) : (mt & 1u) ? tilesM - 1u - (mt >> 1) : (mt >> 1);
}

inline bool clip_geom_ok(int IH, int IW, int OH, int OW, int stride, int pad, int KH, int KW) {
  return stride == 2 && pad == 1 && KH == 4 && KW == 4 && IH == 2 * OH && IW == 2 * OW && OH >= 1 && OW >= 1 && OH * OW < 65536;
}
inline size_t cliptab_words(int OH, int OW) { return (size_t)5 * OH * OW; }

inline uint32_t clip_desc(int pos, int h0, int nh, int w0, int nw) {
  return (uint32_t)pos | (uint32_t)h0 << 16 | (uint32_t)nh << 20 | (uint32_t)w0 << 24 | (uint32_t)nw << 28;
}
PCG_CLIP_HD int clip_desc_taps(uint32_t d) { return (int)((d >> 20) & 15u) * (int)(d >> 28); }

// out: cliptab_words(OH, OW) words.  The geometry is k4 s2 p1 with IH = 2 OH, IW = 2 OW (clip_geom_ok).
inline void cliptab_build(int OH, int OW, uint32_t* out) {
  const int npos = OH * OW, IH = 2 * OH, IW = 2 * OW;
  std::vector<uint32_t> d((size_t)npos);
  auto sorted_out = [&](uint32_t* dst) {
    std::stable_sort(d.begin(), d.end(), [](uint32_t a, uint32_t b) { return clip_desc_taps(a) > clip_desc_taps(b); });
    std::copy(d.begin(), d.end(), dst);
  };
  // [lo, hi) of the taps t in [0, n) with 0 <= base + sign * t < extent
  auto range = [](int base, int sign, int n, int extent, int& lo, int& cnt) {
    lo = n; cnt = 0;
    for (int t = 0; t < n; ++t) {
      const int v = base + sign * t;
      if (v >= 0 && v < extent) { if (cnt == 0) lo = t; ++cnt; }
    }
  };
  for (int oh = 0; oh < OH; ++oh)
    for (int ow = 0; ow < OW; ++ow) {
      int h0, nh, w0, nw;
      range(oh * 2 - 1, 1, 4, IH, h0, nh);       // input row of tap kh: oh * stride - pad + kh
      range(ow * 2 - 1, 1, 4, IW, w0, nw);
      d[(size_t)oh * OW + ow] = clip_desc(oh * OW + ow, h0, nh, w0, nw);
    }
  sorted_out(out);
  for (int py = 0; py < 4; ++py) {
    const int ph = py >> 1, pw = py & 1;
    const int kh0 = (ph + 1) % 2, kw0 = (pw + 1) % 2, dh0 = (ph + 1 - kh0) / 2, dw0 = (pw + 1 - kw0) / 2;   // build_phases
    for (int a = 0; a < OH; ++a)
      for (int c = 0; c < OW; ++c) {
        int h0, nh, w0, nw;
        range(a + dh0, -1, 2, OH, h0, nh);       // output row of tap jh: a + dh0 - jh
        range(c + dw0, -1, 2, OW, w0, nw);
        d[(size_t)a * OW + c] = clip_desc(a * OW + c, h0, nh, w0, nw);
      }
    sorted_out(out + (size_t)(1 + py) * npos);
  }
}

// ---- schedule model ------------------------------------------------------------------------------------------------------------
// 256 CUs with two workgroup slots each; slot s sits on CU s % 256.  Workgroups are dispatched in order: the first 512 fill the slots
// in slot order, every later one takes the slot that frees first (ties: lower CU, then lower slot).  A workgroup advances one k-tile
// per 3.5 us while the other slot of its CU is busy and per 2.2 us when it has the CU alone (plan_sk's constants).  len[i]: k-tiles
// of the i-th workgroup in dispatch order.  Returns the time at which the last one ends, in us.
inline double clip_sched_model(const int* len, int n) {
  constexpr int SLOTS = 512, CUS = 256;
  constexpr double SHARED = 3.5, ALONE = 2.2;
  double rem[SLOTS];
  bool busy[SLOTS];
  int next = 0;
  for (int s = 0; s < SLOTS; ++s) { busy[s] = next < n; rem[s] = busy[s] ? (double)len[next++] : 0.0; }
  double t = 0.0;
  int order[SLOTS];
  for (int c = 0; c < CUS; ++c) { order[2 * c] = c; order[2 * c + 1] = c + CUS; }   // (CU, slot) order
  for (;;) {
    double dt = -1.0;
    for (int s = 0; s < SLOTS; ++s)
      if (busy[s]) {
        const double d = rem[s] * (busy[s ^ CUS] ? SHARED : ALONE);
        if (dt < 0.0 || d < dt) dt = d;
      }
    if (dt < 0.0) return t;
    t += dt;
    bool freed[SLOTS];
    for (int s = 0; s < SLOTS; ++s) freed[s] = false;
    for (int s = 0; s < SLOTS; ++s)
      if (busy[s]) {
        rem[s] -= dt / (busy[s ^ CUS] ? SHARED : ALONE);
        freed[s] = rem[s] < 1e-9;
      }
    for (int s = 0; s < SLOTS; ++s) if (freed[s]) busy[s] = false;
    for (int i = 0; i < SLOTS; ++i) {
      const int s = order[i];
      if (freed[s] && next < n) { busy[s] = true; rem[s] = (double)len[next++]; }
    }
  }
}

}  // namespace pcg
