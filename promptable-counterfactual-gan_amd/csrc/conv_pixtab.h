// conv_pixtab.h — pixel descriptor table of a convolution geometry (host side, plain C++: no HIP call, usable without a GPU).
//
// The weight gradient contracts over output pixels: every k-tile brings 32 new pixels, and the x gather needs, per pixel, the byte
// offset of the input pixel under tap (0, 0) and which taps fall inside the input.  Both depend on (IH, IW, OH, OW, stride, pad,
// KH, KW, Cin) only — not on the batch, the data or the weights — so they are tabulated once per geometry and read by the loaders
// (conv_loaders.h, PixDesc8) instead of being re-derived with divisions, carries and bounds compares for every k-tile.
//
// Entry r = oh * OW + ow of ONE image, 8 bytes:
//   off   int32   ((oh*stride - pad) * IW + (ow*stride - pad)) * Cin * 4 — inside the image, negative for a padded border pixel
//   mask  uint32  bit kh*KW + kw set when input pixel (oh*stride - pad + kh, ow*stride - pad + kw) exists
// followed by PIXTAB_TAIL entries that continue into the next images: entry r >= OH*OW is entry r % (OH*OW) with (r / (OH*OW)) *
// IH*IW*Cin*4 added to its offset.  A wave gathers 8 consecutive pixels per k-tile; with the tail it reads their descriptors as ONE
// run of 8 entries starting at its first pixel's index, wherever the run crosses an image boundary.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pcg {

constexpr int PIXTAB_TAIL = 7;

inline size_t pixtab_entries(int OH, int OW) { return (size_t)OH * OW + PIXTAB_TAIL; }

// out: 2 * pixtab_entries(OH, OW) words, {off, mask} pairs.  KH * KW <= 32; the image is smaller than 2 GiB (check_geom).
inline void pixtab_build(int IH, int IW, int OH, int OW, int stride, int pad, int KH, int KW, int Cin, uint32_t* out) {
  const int64_t ohw = (int64_t)OH * OW, n = ohw + PIXTAB_TAIL;
  const int64_t img_bytes = (int64_t)IH * IW * Cin * 4;
  for (int64_t r = 0; r < n; ++r) {
    const int64_t img = r / ohw, rr = r - img * ohw;
    const int oh = (int)(rr / OW), ow = (int)(rr - (int64_t)oh * OW);
    const int ih0 = oh * stride - pad, iw0 = ow * stride - pad;
    uint32_t mask = 0;
    for (int kh = 0; kh < KH; ++kh)
      for (int kw = 0; kw < KW; ++kw)
        if (ih0 + kh >= 0 && ih0 + kh < IH && iw0 + kw >= 0 && iw0 + kw < IW) mask |= 1u << (kh * KW + kw);
    const int64_t off = img * img_bytes + ((int64_t)ih0 * IW + iw0) * Cin * 4;
    out[2 * r] = (uint32_t)off;      // 32-bit wrap-around like every offset of the gathers
    out[2 * r + 1] = mask;
  }
}

}  // namespace pcg
