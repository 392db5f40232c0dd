// thin_fast.inc — fast paths for a ONE-channel thin side with <= 16 taps and stride <= 2 (the DCGAN edge layers:
// D's first conv 1->64, G's last ConvTranspose 64->1, D's last conv 512->1).  Included inside thin_conv.hip's
// anonymous namespace (needs ThinP).  All tap gathers are branch-free raw buffer loads: an invalid tap (zero padding,
// wrong sub-pixel phase) gets the out-of-range offset and the hardware returns 0.
//
//   reduce  = tapdot (T[q][tap] = sum_c wide[q][c] * W[tap][c], every wide pixel read exactly once, 16 lanes per pixel,
//             butterfly reduce-scatter so lane t ends with tap t)  +  col2im (thin[P] = sum_tap T[map(P,tap)][tap])
//   expand  = one thread per (wide pixel, 16 channels): the 16 tap scalars are gathered once and reused for 16 outputs

typedef __amdgpu_buffer_rsrc_t thin_rsrc_t;
constexpr uint32_t THIN_OOB = 0x80000000u;

__device__ __forceinline__ thin_rsrc_t thin_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float thin_load1(thin_rsrc_t r, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

// pixel index on the "other" grid for tap (kh,kw) of iteration pixel (ph,pw), or -1 (the transposed map: strides 1 and 2 only)
__device__ __forceinline__ int tap_map_idx(const ThinP& p, int b, int ph, int pw, int kh, int kw) {
  int qh, qw;
  bool ok;
  if (!p.transposed) {
    qh = ph * p.stride - p.pad + kh;
    qw = pw * p.stride - p.pad + kw;
    ok = true;
  } else {
    const int th = ph + p.pad - kh, tw = pw + p.pad - kw;
    ok = (th | tw) >= 0 && (p.stride == 1 || ((th | tw) & 1) == 0);
    qh = p.stride == 1 ? th : th >> 1;
    qw = p.stride == 1 ? tw : tw >> 1;
  }
  ok = ok && (unsigned)qh < (unsigned)p.QH && (unsigned)qw < (unsigned)p.QW;
  return ok ? (b * p.QH + qh) * p.QW + qw : -1;
}

// ---- reduce, stage 1: T[pix][16] ---------------------------------------------------------------------------------
template <int NTAP>
__global__ void __launch_bounds__(256) thin_tapdot_kernel(ThinP p, float* __restrict__ T) {
  extern __shared__ __attribute__((aligned(16))) float Wl[];  // [NTAP][C]
  for (int i = threadIdx.x; i < NTAP * p.C; i += 256) {
    const int t = i / p.C, c = i - t * p.C;
    Wl[i] = p.w[(size_t)t * p.wsT + (size_t)c * p.wsC];
  }
  __syncthreads();
  const int CQ = p.C >> 2;
  const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const bool b3 = l16 & 8, b2 = l16 & 4, b1 = l16 & 2, b0 = l16 & 1;
  const float4* Wl4 = reinterpret_cast<const float4*>(Wl);
  for (uint32_t pix = blockIdx.x * 16u + grp; pix < (uint32_t)p.npix; pix += gridDim.x * 16u) {
    float acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    const float4* vp = reinterpret_cast<const float4*>(p.wide + (size_t)pix * p.C);
    for (int cq = l16; cq < CQ; cq += 16) {
      const float4 v = vp[cq];
#pragma unroll
      for (int t = 0; t < NTAP; ++t) {
        const float4 w4 = Wl4[t * CQ + cq];
        acc[t] = fmaf(v.x, w4.x, acc[t]); acc[t] = fmaf(v.y, w4.y, acc[t]);
        acc[t] = fmaf(v.z, w4.z, acc[t]); acc[t] = fmaf(v.w, w4.w, acc[t]);
      }
    }
    // butterfly reduce-scatter over the 16 lanes of the pixel: lane t ends with the full sum of tap t
    float r8[8], r4[4], r2[2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float send = b3 ? acc[j] : acc[j + 8], keep = b3 ? acc[j + 8] : acc[j];
      r8[j] = keep + __shfl_xor(send, 8);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float send = b2 ? r8[j] : r8[j + 4], keep = b2 ? r8[j + 4] : r8[j];
      r4[j] = keep + __shfl_xor(send, 4);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float send = b1 ? r4[j] : r4[j + 2], keep = b1 ? r4[j + 2] : r4[j];
      r2[j] = keep + __shfl_xor(send, 2);
    }
    const float send = b0 ? r2[0] : r2[1], keep = b0 ? r2[1] : r2[0];
    T[(size_t)pix * 16 + l16] = keep + __shfl_xor(send, 1);
  }
}

// ---- reduce, stage 1 for C = 64 on the matrix cores (r04) -----------------------------------------------------------------------
// Per 16 wide pixels the contraction is a 16 x 16 x 64 GEMM: sixteen v_mfma_f32_16x16x4_f32 whose D tile IS T's layout (lane l holds
// rows 4(l>>4)+i of column l&15), so the 15-shuffle reduce-scatter of thin_tapdot_kernel — most of that kernel's issue slots —
// disappears.  The FMA rate is the vector ALU's own (64 FLOP/clk/SIMD either way); what is saved is everything around the FMAs.
// The operand layout wants 16 DIFFERENT pixels on the lanes l&15 — loading them directly is 16 rows 256 B apart per quarter-wave (measured:
// 63 us against the shuffle kernel's 48), so each wave reads its 32 pixels with fully coalesced 16-byte loads and turns them through a
// private LDS tile (rows padded to 68 floats: the b128 writes and reads are both conflict-free; DS operations of one wave execute in
// order, so no barrier).  k-step (jj, e) of lane group h = l>>4 is channel 16jj + 4h + e; the filter operand is preloaded in that order.
// Two pixel groups per wave iteration: two independent accumulator chains (the instruction's dependent latency exceeds its issue interval).
// NB = 1: up to 16 outputs per pixel (one thin channel), T rows of 16; NB = 2: up to 32 outputs (2..3 thin channels x 9 taps, output
// tap*Cs + cs), T rows of 32 — the same A operand feeds both column blocks.
// NC > 1 (template MULTI): C = 64 * NC channels (WGAN-GP's last ConvTranspose2d(256, 1, 4, 2, 1), mnist_wgan_conditional.py:70) — the wave
// turns one 64-channel chunk at a time through its LDS tile, the accumulators run over the chunks, and the filter operand comes from an LDS
// image [tap][C + 4] (rows padded by 4 floats: the b128 reads of a quarter-wave fall on 64 different banks) instead of registers.
typedef float thin_f32x4 __attribute__((ext_vector_type(4)));
constexpr int TD64_LD = 68, TD64_MAX_C = 512;
template <int NB, bool MULTI>
__global__ void __launch_bounds__(256) thin_tapdot64_mfma_kernel(ThinP p, float* __restrict__ T) {
  __shared__ __attribute__((aligned(16))) float stage[4][32 * TD64_LD];
  extern __shared__ __attribute__((aligned(16))) float Wm[];     // MULTI only: [16][C + 4]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, h = lane >> 4;
  float* S = stage[wave];
  const int NO = p.KH * p.KW * p.Cs;
  const int NC = MULTI ? p.C >> 6 : 1, CQ = p.C >> 2, WLD = p.C + 4;
  float bw[NB][4][4];
  if constexpr (MULTI) {
    for (int i = threadIdx.x; i < 16 * p.C; i += 256) {
      const int t = i / p.C, c = i - t * p.C;
      Wm[t * WLD + c] = t < NO ? p.w[(size_t)t * p.wsT + (size_t)c * p.wsC] : 0.f;
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int o = 16 * nb + col, tap = o / p.Cs, cs = o - tap * p.Cs;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bw[nb][jj][e] = o < NO ? p.w[(size_t)cs * p.wsS + (size_t)tap * p.wsT + (size_t)(16 * jj + 4 * h + e) * p.wsC] : 0.f;
    }
  }
  const uint32_t npix = (uint32_t)p.npix, ngroups = (npix + 31u) / 32u;
  const float4* wide4 = reinterpret_cast<const float4*>(p.wide);
  // input transform (kernel-uniform): the wide operand is a PRE-BatchNorm tensor, read as act(z * scale[c] + shift[c]) — a lane's 16-byte
  // piece of a chunk is always channels 64 cb + 4 col .. + 3; the expression is the one every BatchNorm pass uses
  const bool has_xf = p.xf_scale != nullptr;
  float4 xsc = make_float4(1.f, 1.f, 1.f, 1.f), xsh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (has_xf && !MULTI) { xsc = *reinterpret_cast<const float4*>(p.xf_scale + 4 * col); xsh = *reinterpret_cast<const float4*>(p.xf_shift + 4 * col); }
  for (uint32_t grp = blockIdx.x * 4u + wave; grp < ngroups; grp += gridDim.x * 4u) {
    thin_f32x4 accA[NB], accB[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { accA[nb] = thin_f32x4{0.f, 0.f, 0.f, 0.f}; accB[nb] = thin_f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int cb = 0; cb < NC; ++cb) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {   // lane (h, col) reads 16-byte piece `col` of the chunk of pixel 4j + h of the group
        const uint32_t pix = grp * 32u + 4u * j + h;     // rows past the end repeat the last pixel; their results are not stored
        v[j] = wide4[(size_t)(pix < npix ? pix : npix - 1u) * CQ + 16 * cb + col];
      }
      if (has_xf) {
        if constexpr (MULTI) {
          xsc = *reinterpret_cast<const float4*>(p.xf_scale + 64 * cb + 4 * col); xsh = *reinterpret_cast<const float4*>(p.xf_shift + 64 * cb + 4 * col);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[j].x = act_neg_scale(fmaf(v[j].x, xsc.x, xsh.x), p.xf_neg); v[j].y = act_neg_scale(fmaf(v[j].y, xsc.y, xsh.y), p.xf_neg);
          v[j].z = act_neg_scale(fmaf(v[j].z, xsc.z, xsh.z), p.xf_neg); v[j].w = act_neg_scale(fmaf(v[j].w, xsc.w, xsh.w), p.xf_neg);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<float4*>(S + (4 * j + h) * TD64_LD + 4 * col) = v[j];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float4 qa = *reinterpret_cast<const float4*>(S + col * TD64_LD + 16 * jj + 4 * h);
        const float4 qb = *reinterpret_cast<const float4*>(S + (col + 16) * TD64_LD + 16 * jj + 4 * h);
        if constexpr (MULTI) {
          const float4 wq = *reinterpret_cast<const float4*>(Wm + col * WLD + 64 * cb + 16 * jj + 4 * h);
          bw[0][jj][0] = wq.x; bw[0][jj][1] = wq.y; bw[0][jj][2] = wq.z; bw[0][jj][3] = wq.w;
        }
#define PCG_TD64_STEP(E, C)                                                                      \
        _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) {                                       \
          accA[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.C, bw[nb][jj][E], accA[nb], 0, 0, 0); \
          accB[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qb.C, bw[nb][jj][E], accB[nb], 0, 0, 0); \
        }
        PCG_TD64_STEP(0, x) PCG_TD64_STEP(1, y) PCG_TD64_STEP(2, z) PCG_TD64_STEP(3, w)
#undef PCG_TD64_STEP
      }
    }
    // T is TAP-major (r04): plane o = 16 nb + col holds output o of every wide pixel — this lane's four pixels 4 h .. 4 h + 3 are four
    // consecutive floats of it (one 16-byte store), and the col2im gathers behind read consecutive addresses for consecutive pixels
    // (the pixel-major rows cost them one cache line per lane: 21 us for 2 M outputs)
    const uint32_t r0 = grp * 32u + 4u * h;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int o = 16 * nb + col;
      if (o >= NO) continue;
      float* plane = T + (size_t)o * npix;
      if ((npix & 3u) == 0u) {          // (kernel-uniform) the planes are 16-byte aligned
        if (r0 < npix) *reinterpret_cast<float4*>(plane + r0) = make_float4(accA[nb][0], accA[nb][1], accA[nb][2], accA[nb][3]);
        if (r0 + 16u < npix) *reinterpret_cast<float4*>(plane + r0 + 16u) = make_float4(accB[nb][0], accB[nb][1], accB[nb][2], accB[nb][3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (r0 + i < npix) plane[r0 + i] = accA[nb][i];
          if (r0 + 16u + i < npix) plane[r0 + 16u + i] = accB[nb][i];
        }
      }
    }
  }
}

// ---- reduce, stage 2: thin[P] = bias + sum_tap T[map(P,tap)][tap]  (iteration grid = thin grid, other = wide grid) ----
// t_off(q, o): byte offset of output o of wide pixel q in T — pixel-major rows of `row` floats (the vector tap-dot kernels) or tap-major
// planes of `plane` floats (the matrix-core ones: plane != 0)
__device__ __forceinline__ uint32_t t_off(int q, int o, uint32_t plane, int row) {
  return plane ? ((uint32_t)o * plane + (uint32_t)q) * 4u : (uint32_t)(q * row + o) * 4u;
}
__global__ void __launch_bounds__(256) thin_col2im_kernel(ThinP p, const float* __restrict__ T, uint32_t t_bytes, uint32_t plane) {
  const thin_rsrc_t rs = thin_rsrc(T, t_bytes);
  const float bv = p.bias ? p.bias[0] : 0.f;
  for (uint32_t P = blockIdx.x * 256u + threadIdx.x; P < (uint32_t)p.npix; P += gridDim.x * 256u) {
    uint32_t t, pw, b, ph;
    p.dIW.divmod(P, t, pw);
    p.dIH.divmod(t, b, ph);
    float acc = bv;
    if (p.transposed && p.stride == 2 && p.KH == 4 && p.KW == 4) {
      // sub-pixel phases: only the taps of the pixel's parity land on the other grid — 4 loads instead of 16, the 12 skipped ones
      // were zeros (same sum, bit for bit)
      const int kh0 = ((int)ph + p.pad) & 1, kw0 = ((int)pw + p.pad) & 1;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int kh = kh0 + 2 * a, kw = kw0 + 2 * c;
          const int q = tap_map_idx(p, (int)b, (int)ph, (int)pw, kh, kw);
          acc += thin_load1(rs, q >= 0 ? t_off(q, kh * 4 + kw, plane, 16) : THIN_OOB);
        }
    } else {
      for (int kh = 0; kh < p.KH; ++kh)
#pragma unroll 4
        for (int kw = 0; kw < p.KW; ++kw) {
          const int q = tap_map_idx(p, (int)b, (int)ph, (int)pw, kh, kw);
          acc += thin_load1(rs, q >= 0 ? t_off(q, kh * p.KW + kw, plane, 16) : THIN_OOB);
        }
    }
    p.out[P] = act_apply(acc, p.act, p.slope);
  }
}

// the sub-pixel map (transposed, k4 s2) with four neighbouring outputs per thread and one 16-byte store: a quarter of the waves
// of the kernel above for the same 4 loads per output (one output per thread is dispatch-bound: 19 us for 2 M outputs)
__global__ void __launch_bounds__(256) thin_col2im_s2k4_kernel(ThinP p, const float* __restrict__ T, uint32_t t_bytes, uint32_t plane) {
  const thin_rsrc_t rs = thin_rsrc(T, t_bytes);
  const float bv = p.bias ? p.bias[0] : 0.f;
  const uint32_t n4 = (uint32_t)p.npix >> 2;
  for (uint32_t P4 = blockIdx.x * 256u + threadIdx.x; P4 < n4; P4 += gridDim.x * 256u) {
    const uint32_t P = P4 << 2;
    uint32_t t, pw0, b, ph;
    p.dIW.divmod(P, t, pw0);
    p.dIH.divmod(t, b, ph);
    const int kh0 = ((int)ph + p.pad) & 1;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int pw = (int)pw0 + j, kw0 = (pw + p.pad) & 1;
      float acc = bv;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int kh = kh0 + 2 * a, kw = kw0 + 2 * c;
          const int q = tap_map_idx(p, (int)b, (int)ph, pw, kh, kw);
          acc += thin_load1(rs, q >= 0 ? t_off(q, kh * 4 + kw, plane, 16) : THIN_OOB);
        }
      o[j] = act_apply(acc, p.act, p.slope);
    }
    *reinterpret_cast<float4*>(p.out + P) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- reduce with 2..3 thin channels (counteRGAN conv_in 3->64 and critic entry 2->64 grad-inputs): the same two stages with
// NTC = taps*Cs <= 32 dot products per wide pixel (row stride 32 in T); lane t of a pixel's 16 ends with outputs 2t and 2t+1 ----------
template <int NTC>
__global__ void __launch_bounds__(256) thin_tapdot32_kernel(ThinP p, float* __restrict__ T) {
  static_assert(NTC > 16 && NTC <= 32, "thin_tapdot32_kernel: 17..32 outputs per pixel");
  extern __shared__ __attribute__((aligned(16))) float Wl[];  // [NTC][C], row (tap*Cs + cs)
  stage_weights(p, Wl);
  const int CQ = p.C >> 2;
  const int l16 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const bool b3 = l16 & 8, b2 = l16 & 4, b1 = l16 & 2, b0 = l16 & 1;
  const float4* Wl4 = reinterpret_cast<const float4*>(Wl);
  for (uint32_t pix = blockIdx.x * 16u + grp; pix < (uint32_t)p.npix; pix += gridDim.x * 16u) {
    float acc[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) acc[t] = 0.f;
    const float4* vp = reinterpret_cast<const float4*>(p.wide + (size_t)pix * p.C);
    for (int cq = l16; cq < CQ; cq += 16) {
      const float4 v = vp[cq];
#pragma unroll
      for (int t = 0; t < NTC; ++t) {
        const float4 w4 = Wl4[t * CQ + cq];
        acc[t] = fmaf(v.x, w4.x, acc[t]); acc[t] = fmaf(v.y, w4.y, acc[t]);
        acc[t] = fmaf(v.z, w4.z, acc[t]); acc[t] = fmaf(v.w, w4.w, acc[t]);
      }
    }
    float r16[16], r8[8], r4[4], r2[2];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float send = b3 ? acc[j] : acc[j + 16], keep = b3 ? acc[j + 16] : acc[j];
      r16[j] = keep + __shfl_xor(send, 8);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float send = b2 ? r16[j] : r16[j + 8], keep = b2 ? r16[j + 8] : r16[j];
      r8[j] = keep + __shfl_xor(send, 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float send = b1 ? r8[j] : r8[j + 4], keep = b1 ? r8[j + 4] : r8[j];
      r4[j] = keep + __shfl_xor(send, 2);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float send = b0 ? r4[j] : r4[j + 2], keep = b0 ? r4[j + 2] : r4[j];
      r2[j] = keep + __shfl_xor(send, 1);
    }
    // lane holds outputs j + 2*b0 + 4*b1 + 8*b2 + 16*b3 (j = 0, 1)
    const int o0 = 2 * (int)b0 + 4 * (int)b1 + 8 * (int)b2 + 16 * (int)b3;
    *reinterpret_cast<float2*>(T + (size_t)pix * 32 + o0) = make_float2(r2[0], r2[1]);
  }
}

__global__ void __launch_bounds__(256) thin_col2im32_kernel(ThinP p, const float* __restrict__ T, uint32_t t_bytes, uint32_t plane) {
  const thin_rsrc_t rs = thin_rsrc(T, t_bytes);
  const uint32_t total = (uint32_t)p.npix * (uint32_t)p.Cs;
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const uint32_t P = idx / (uint32_t)p.Cs, cs = idx - P * (uint32_t)p.Cs;
    uint32_t t, pw, b, ph;
    p.dIW.divmod(P, t, pw);
    p.dIH.divmod(t, b, ph);
    float acc = p.bias ? p.bias[cs] : 0.f;
    for (int kh = 0; kh < p.KH; ++kh)
      for (int kw = 0; kw < p.KW; ++kw) {
        const int q = tap_map_idx(p, (int)b, (int)ph, (int)pw, kh, kw);
        acc += thin_load1(rs, q >= 0 ? t_off(q, (kh * p.KW + kw) * p.Cs + (int)cs, plane, 32) : THIN_OOB);
      }
    p.out[idx] = act_apply(acc, p.act, p.slope);
  }
}

// ---- expand: wide[P][16g .. 16g+15] = bias + sum_tap thin[map(P,tap)] * W[tap][c] ------------------------------------
template <int KH, int KW>
__global__ void __launch_bounds__(256) thin_expand16_kernel(ThinP p, uint32_t thin_bytes) {
  constexpr int NT = KH * KW;
  extern __shared__ __attribute__((aligned(16))) float Wl[];  // [NT][C]
  for (int i = threadIdx.x; i < NT * p.C; i += 256) {
    const int t = i / p.C, c = i - t * p.C;
    Wl[i] = p.w[(size_t)t * p.wsT + (size_t)c * p.wsC];
  }
  __syncthreads();
  const thin_rsrc_t rs = thin_rsrc(p.thin, thin_bytes);
  const int G = p.C >> 4, CQ = p.C >> 2;
  const uint32_t total = (uint32_t)p.npix * (uint32_t)G;
  const float4* Wl4 = reinterpret_cast<const float4*>(Wl);
  const float4* bias4 = reinterpret_cast<const float4*>(p.bias);
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    uint32_t pix, g, t, pw, b, ph;
    p.dCQ.divmod(idx, pix, g);  // dCQ prepared as FastDiv(C/16) for this kernel
    p.dIW.divmod(pix, t, pw);
    p.dIH.divmod(t, b, ph);
    float sv[NT];
#pragma unroll
    for (int kh = 0; kh < KH; ++kh)
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) {
        const int q = tap_map_idx(p, (int)b, (int)ph, (int)pw, kh, kw);
        sv[kh * KW + kw] = thin_load1(rs, q >= 0 ? (uint32_t)(q * 4) : THIN_OOB);
      }
    float4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = p.bias ? bias4[g * 4 + e] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int tp = 0; tp < NT; ++tp)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float4 w4 = Wl4[tp * CQ + g * 4 + e];
        acc[e].x = fmaf(sv[tp], w4.x, acc[e].x); acc[e].y = fmaf(sv[tp], w4.y, acc[e].y);
        acc[e].z = fmaf(sv[tp], w4.z, acc[e].z); acc[e].w = fmaf(sv[tp], w4.w, acc[e].w);
      }
    float4* o = reinterpret_cast<float4*>(p.out + (size_t)pix * p.C) + g * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (p.act != PCG_ACT_NONE) {   // ReLU / LeakyReLU only on the wide side: neg = 0 / slope
        acc[e].x = act_neg_scale(acc[e].x, p.slope); acc[e].y = act_neg_scale(acc[e].y, p.slope);
        acc[e].z = act_neg_scale(acc[e].z, p.slope); acc[e].w = act_neg_scale(acc[e].w, p.slope);
      }
      o[e] = acc[e];
    }
  }
}
