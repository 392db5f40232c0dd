/*
 * pcgan_hip.h — C ABI of libpcgan_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * Generator/Discriminator training step of flash4242/Promptable-Counterfactual-GAN.
 *
 * The reference has no FFI of its own: every FLOP of its hot path is a torch.nn / torch.optim call
 * (SURVEY.md §8b).  Each entry point below therefore cites the reference call site whose ATen
 * operator it replaces; the Python shim (promptable-counterfactual-gan_amd/) binds them with ctypes
 * and hands over `tensor.data_ptr()` of PyTorch-ROCm tensors.
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch types; no exceptions.  Every function returns PCG_OK (0)
 *    or a negative pcg_status; pcg_last_error() gives the text for the calling thread.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises, nothing
 *    allocates: every buffer, including workspaces, is owned by the caller and only borrowed until
 *    the enqueued work has run.  All launches are hipGraph-capturable.
 *  - Activations are fp32 NHWC  [B][H][W][C]  (PyTorch: torch.channels_last tensors of shape [B,C,H,W]).
 *    Conv2d weights are fp32 OHWI [Cout][KH][KW][Cin] (PyTorch: channels_last tensor [Cout,Cin,KH,KW]);
 *    ConvTranspose2d weights [Cin][KH][KW][Cout] (channels_last tensor [Cin,Cout,KH,KW]) — which is
 *    the OHWI weight of the adjoint convolution, so one geometry struct serves both layer kinds:
 *        Conv2d           forward = pcg_conv2d_fwd,   grad-input = pcg_conv2d_dgrad, grad-weight = pcg_conv2d_wgrad
 *        ConvTranspose2d  forward = pcg_conv2d_dgrad, grad-input = pcg_conv2d_fwd,   grad-weight = pcg_conv2d_wgrad
 *    (for the transposed layer, `x` of the geometry is the layer's OUTPUT side and `y` its INPUT side).
 *  - Labels / class indices are int64 (torch.long), as in the reference.
 */
#ifndef PCGAN_HIP_H
#define PCGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pcg_stream_t; /* hipStream_t */

typedef enum pcg_status {
  PCG_OK = 0,
  PCG_ERR_INVALID = -1,     /* bad argument / unsupported shape */
  PCG_ERR_WORKSPACE = -2,   /* workspace too small */
  PCG_ERR_LAUNCH = -3,      /* HIP launch error */
  PCG_ERR_UNSUPPORTED = -4
} pcg_status;

typedef enum pcg_act {
  PCG_ACT_NONE = 0,
  PCG_ACT_RELU = 1,
  PCG_ACT_LRELU = 2,   /* slope given separately */
  PCG_ACT_TANH = 3,
  PCG_ACT_SIGMOID = 4
} pcg_act;

/* y[b,oh,ow,co] = bias[co] + sum_{kh,kw,ci} x[b, oh*stride-pad+kh, ow*stride-pad+kw, ci] * w[co,kh,kw,ci] */
typedef struct pcg_conv_geom {
  int32_t B;
  int32_t IH, IW, Cin;   /* x: [B][IH][IW][Cin]  */
  int32_t OH, OW, Cout;  /* y: [B][OH][OW][Cout] */
  int32_t KH, KW, stride, pad;
} pcg_conv_geom;

/* ---- library ------------------------------------------------------------------------------- */
int pcg_abi_version(void);
/* sizeof of an argument struct of this header by its typedef name (0: unknown name) — a binding checks its own layout against it */
size_t pcg_abi_struct_bytes(const char* name);
const char* pcg_last_error(void);
/* "gfx950" — the only code object in the library */
const char* pcg_target_arch(void);

/* ---- convolution family (MFMA f32 implicit GEMM; thin Cin==1 / Cout==1 layers on the vector ALU) -
 * replaces nn.Conv2d / nn.ConvTranspose2d forward + autograd:
 *   dconv_gan/mnist/mnist_dcgan.py:76-88 (G ConvT stack), :100-111 (D Conv stack);
 *   conditional_counteRGAN/mnist/models/generator.py:11-14,39,49-50; models/discriminator.py:14-24;
 *   models/classifier.py:7-12.                                                                    */
/* Optional scratch for fwd / dgrad: 0 for MFMA layers; for a layer whose reduced side has ONE channel (Cout==1 fwd,
 * Cin==1 dgrad) it buys the two-stage "tap dot + col2im" path that reads the wide tensor exactly once.  Passing
 * workspace == NULL is always valid (a slower single-kernel path is used).                                        */
size_t pcg_conv2d_fwd_workspace_bytes(const pcg_conv_geom* g);
size_t pcg_conv2d_dgrad_workspace_bytes(const pcg_conv_geom* g);
/* Operand precision of the matrix-core (implicit-GEMM) convolutions, per calling thread (default PCG_PREC_F32).  PCG_PREC_BF16: the two
 * GEMM operands are rounded once to bf16 (round-to-nearest-even, after any input transform) and the products summed in fp32 — tensors,
 * workspaces and epilogues stay fp32, and every geometry the fp32 path accepts runs in bf16.  The thin (Cin or Cout <= 3) layers and all
 * other kernels ignore it.  Each pcg_conv2d_* call reads the calling thread's setting when it enqueues its launches (a HIP-graph capture
 * records it).  set: PCG_ERR_INVALID for any other value; get: the calling thread's setting.                                          */
typedef enum pcg_precision { PCG_PREC_F32 = 0, PCG_PREC_BF16 = 1 } pcg_precision;
int pcg_conv_precision_set(int32_t precision);
int32_t pcg_conv_precision_get(void);
/* The plain forms as positional calls (pcg_conv2d below with nothing but the operands and the workspace set). */
int pcg_conv2d_fwd(const pcg_conv_geom* g, const float* x, const float* w, const float* bias /*nullable*/,
                   float* y, void* workspace /*nullable*/, size_t workspace_bytes, pcg_stream_t stream);
int pcg_conv2d_dgrad(const pcg_conv_geom* g, const float* dy, const float* w, const float* bias_x /*nullable: added per Cin channel (ConvTranspose2d bias)*/,
                     float* dx, void* workspace /*nullable*/, size_t workspace_bytes, pcg_stream_t stream);
size_t pcg_conv2d_wgrad_workspace_bytes(const pcg_conv_geom* g);
/* Deferred slab reductions (r04).  A split-K weight gradient ends with a small launch that sums its K-slice slabs into dw; in a backward
 * sweep nothing reads dw before the sweep ends (optimizer.step(), mnist_dcgan.py:164,176; the gradient exchange).  Between
 * pcg_slab_defer_begin(stream) and pcg_slab_defer_flush(stream) the pcg_conv2d_wgrad* calls of THIS thread on `stream` leave their slabs
 * unreduced and the flush sums all of them in ONE launch — bit-identical to the per-call reductions (same order per element).  The
 * caller must give every deferred call its own workspace and keep it until the flush; two sums into the same dw stay in call order.
 * No nesting.  pcg_slab_defer_pending(): recorded entries, -1 when not deferring.                                                  */
int pcg_slab_defer_begin(pcg_stream_t stream);
int pcg_slab_defer_flush(pcg_stream_t stream);
int32_t pcg_slab_defer_pending(void);
/* dw[co,kh,kw,ci] (+)= sum_{b,oh,ow} dy[b,oh,ow,co] * x[b,oh*s-p+kh,ow*s-p+kw,ci];  accumulate!=0 adds into dw
 * (the reference accumulates .grad over two backward() calls: mnist_dcgan.py:153,161).             */
int pcg_conv2d_wgrad(const pcg_conv_geom* g, const float* x, const float* dy, float* dw, int accumulate,
                     void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* Partial-row buffers of the fused BatchNorm statistics (pcg_conv_args.stats) and of the add_bnsum / bnbwd epilogues
 * (0 = layer not eligible: use the separate calls).                                                                     */
size_t pcg_conv2d_fwd_bn_workspace_bytes(const pcg_conv_geom* g);
size_t pcg_conv2d_dgrad_bn_workspace_bytes(const pcg_conv_geom* g);
/* ---- input transforms: BatchNorm + ReLU / LeakyReLU of the PRODUCING layer applied inside the consumer's gather ------------------
 * In `Conv -> BatchNorm(train) -> LeakyReLU -> Conv` (mnist_dcgan.py:102-110, G: :76-87) the activated tensor a = act(bn(z)) is
 * only ever read by the next convolution (forward, and again by that layer's weight gradient).  With a transform the consumer
 * reads the pre-BatchNorm tensor z itself and evaluates act(z*scale[c] + shift[c]) between the gather and the LDS write, so the
 * separate BatchNorm-apply pass and the activated copy of every such activation disappear.  scale / shift are the folded
 * BatchNorm (scale = gamma*invstd, shift = beta - mean*scale — exactly the expression pcg_bn_apply_act evaluates, so results are
 * bit-identical to the unfused sequence); zero padding stays zero.  MFMA layers only (Cin > 3, Cout > 3, channel counts % 4 == 0).
 * pcg_conv_args.xf puts one on the input operand of a forward or grad-input launch; pcg_conv2d_wgrad_xf takes one on x (Conv2d) or on
 * dy (ConvTranspose2d, whose forward input sits on the dy side of the adjoint geometry) — at most one of the two. */
typedef struct pcg_in_xform {
  const float* scale;   /* [C], 16-byte aligned; NULL: no transform */
  const float* shift;   /* [C] */
  int32_t act;          /* PCG_ACT_NONE / PCG_ACT_RELU / PCG_ACT_LRELU */
  float slope;
} pcg_in_xform;
int pcg_conv2d_wgrad_xf(const pcg_conv_geom* g, const float* x, const pcg_in_xform* xf_x, const float* dy, const pcg_in_xform* xf_dy,
                        float* dw, int accumulate, void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* Thin layers that take an input transform (r04): a Cin = 1 geometry with Cout = 64 and <= 16 taps — DCGAN's last ConvTranspose2d(64, 1, 4, 2, 1)
 * (mnist_dcgan.py:88), whose input is BatchNorm2d + ReLU of the layer before (:86-87).  A grad-input pcg_conv2d with xf (its forward) and
 * pcg_conv2d_wgrad_xf with xf_dy (its weight gradient) then read the PRE-BatchNorm tensor: the BatchNorm-apply pass and the activated
 * copy of that activation disappear (both kernels are HBM-bound: the transform is free).  Needs the workspace of
 * pcg_conv2d_dgrad_workspace_bytes / pcg_conv2d_wgrad_workspace_bytes.                                                              */
int32_t pcg_conv2d_xf_thin_ok(const pcg_conv_geom* g);
/* One-channel layers whose grad-input takes the row-block form (k3 / k4, Cout <= 3, Cin a power-of-two multiple of 4) also take the
 * mask epilogue (r04): it is applied in the thin expand kernel (CounteRGAN conv_out, models/generator.py:50). */
int32_t pcg_conv2d_dgrad_mask_thin_ok(const pcg_conv_geom* g);

/* ---- pcg_conv2d: every form of the forward and the grad-input convolution -------------------------------------------------------
 * One launch = one pcg_conv_args.  A zero-filled struct with op, in, w and out set is the plain convolution; every other member
 * switches one thing on.  Three families exist, and pcg_conv2d refuses every mixture of them before any HIP call:
 *   - the convolution with its bias, output activation and input transform (act, slope, bias, xf);
 *   - the same without activation + the training-mode BatchNorm statistics of its output (stats; bias and xf allowed);
 *   - the bare convolution with a backward-pass epilogue (epi; no bias, activation, transform or statistics).
 * A ConvTranspose2d layer runs the other direction (header comment): its forward is PCG_CONV_DGRAD, its grad-input PCG_CONV_FWD, so
 * every epilogue exists in both directions.  A stride-1 Conv2d's grad-input may also run as a FORWARD convolution of dy with the adjoint
 * weight — pcg_conv_weight_adjoint: w[co][kh][kw][ci] -> w_adj[ci][KH-1-kh][KW-1-kw][co], geometry {B, OH, OW, Cout -> IH, IW, Cin,
 * pad' = K-1-pad} — which makes both GEMM operands K-major.                                                                        */
typedef enum pcg_conv_op { PCG_CONV_FWD = 0, PCG_CONV_DGRAD = 1 } pcg_conv_op;
/* Backward-pass epilogues (MFMA layers).  In autograd's sweep through `Conv -> [BatchNorm] -> ReLU/LeakyReLU -> Conv` (D:
 * mnist_dcgan.py:100-110, G: :76-87) the gradient w.r.t. a layer's OUTPUT a = act(..) is produced by the grad-input kernel of the
 * layer above; an epilogue applies the lower layer's activation derivative (epi_act: none / ReLU / LeakyReLU, epi_slope) or a skip
 * connection's add while that tile is still in registers.  out = conv(in, w) in the launch's direction, then:                      */
typedef enum pcg_conv_epi {
  PCG_CONV_EPI_NONE = 0,
  /* out *= act'(a_below)   (a_below = the post-activation output of the layer below, out's shape) — replaces the pcg_act_bwd pass of a
   * Conv + LeakyReLU layer without BatchNorm (mnist_dcgan.py:100-101).  Also on pcg_conv2d_dgrad_mask_thin_ok geometries.          */
  PCG_CONV_EPI_MASK = 1,
  /* out += addend   (addend may be out itself: in-place accumulation) — the skip connection of a residual block in the backward
   * sweep (`x + 0.1*out`, conditional_counteRGAN/mnist/models/generator.py:20): no separate add pass.                               */
  PCG_CONV_EPI_ADD = 2,
  /* out = (out + addend) * act'(a_below) — the add followed by pcg_act_bwd in ONE epilogue: the last skip-add of a residual chain
   * arriving at the entry convolution's LeakyReLU (models/generator.py:76 backward).  a_below: the activated output, not out itself. */
  PCG_CONV_EPI_ADD_MASK = 3,
  /* The add + the BatchNorm-backward column sums of the SUM for the next BatchNorm down the skip chain (`x + 0.1*bn2(conv2(...))`,
   * models/generator.py:18-20: the gradient arriving at block i-1's bn2 is the sum block i's backward just formed): the partial rows
   * get sum(sum_scale*out) and sum(sum_scale*out*xhat) with xhat from z / mean / invstd of that BatchNorm (z = its pre-normalisation
   * output z_next); out itself is stored unscaled.  Finish with pcg_bn_bwd_partial_db(dm = out, dm_scale = sum_scale).
   * addend == NULL (r04): the plain result with the sums — the head of the chain, conv_mid's grad-input above the last block's bn2
   * (generator.py:49,78).                                                                                                           */
  PCG_CONV_EPI_ADD_BNSUM = 4,
  /* out *= act'(bn(z)) with the mask recomputed from the pre-BatchNorm output z (= z_below) of the layer below as
   * fma(z, gamma*invstd, beta - mean*gamma*invstd) > 0, and the per-channel sums of out and out*xhat written as partial rows — the
   * reduction pass of BatchNorm's backward disappears; finish with pcg_bn_bwd_partial.                                              */
  PCG_CONV_EPI_BNBWD = 5
} pcg_conv_epi;
typedef struct pcg_conv_args {
  const float* in;              /* forward: x [B][IH][IW][Cin]; grad-input: dy [B][OH][OW][Cout] */
  const float* w;               /* OHWI */
  const float* bias;            /* nullable; grad-input: added per Cin channel (ConvTranspose2d bias) */
  float* out;                   /* forward: y; grad-input: dx */
  const pcg_in_xform* xf;       /* nullable: input transform on `in` (MFMA layers; the grad-input of pcg_conv2d_xf_thin_ok geometries) */
  /* the epilogue's tensors — each epilogue reads the ones its enumerator names, all 16-byte aligned as `out` must then be */
  const float* addend;
  const float* a_below;
  const float* z;               /* add_bnsum: z_next; bnbwd: z_below */
  const float* mean;            /* add_bnsum, bnbwd: statistics of that BatchNorm, [C] ([groups][C] with groups) */
  const float* invstd;
  const float* gamma;           /* bnbwd: required.  stats: optional, with beta, for coef_out */
  const float* beta;
  void* partial;                /* add_bnsum, bnbwd: fp64 partial rows [pcg_conv2d_*_bn_partial_rows][2][C], the buffer of */
  size_t partial_bytes;         /*   pcg_conv2d_{fwd,dgrad}_bn_workspace_bytes of the launch's direction                   */
  /* Fused statistics (stats != 0; MFMA layers only): the per-channel sum / sum of squares are taken from the accumulator tile in the
   * conv epilogue (no extra pass over out), partial rows are finalised in a fixed order.  Same outputs as the plain launch followed
   * by pcg_bn_train_stats.  `workspace` is then the buffer of pcg_conv2d_{fwd,dgrad}_bn_workspace_bytes and is required.          */
  float* save_mean;             /* [C]; [groups][C] with groups */
  float* save_invstd;
  float* running_mean;          /* nullable */
  float* running_var;           /* nullable */
  int64_t* num_batches_tracked; /* nullable: += 1 (+= groups) */
  float* coef_out;              /* nullable [2][C]: the folded scale / shift of THIS layer's BatchNorm (gamma, beta required), written by
                                   the statistics finalize — ready to be the next consumer's transform */
  /* Optional scratch (pcg_conv2d_{fwd,dgrad}_workspace_bytes; NULL is always valid: a slower path is used); the statistics' buffer */
  void* workspace;
  size_t workspace_bytes;
  int32_t op;                   /* pcg_conv_op */
  /* The activation that follows the layer fused into the output write — out = act(conv(in) + bias): Conv2d + LeakyReLU
   * (mnist_dcgan.py:100-101, counteRGAN models/discriminator.py:17-24, generator.py:36-37,50), Conv2d + ReLU (models/classifier.py:7-12),
   * Conv2d + Sigmoid (mnist_dcgan.py:110-111), ConvTranspose2d + Tanh (mnist_dcgan.py:88-89, mnist_wgan_conditional.py:70-71).
   * The backward needs only out (pcg_act_bwd).                                                                                   */
  int32_t act;                  /* pcg_act */
  float slope;
  int32_t epi;                  /* pcg_conv_epi */
  int32_t epi_act;              /* mask, add_mask, bnbwd: the layer below's activation (none / ReLU / LeakyReLU); add, add_bnsum: none */
  float epi_slope;
  float sum_scale;              /* add_bnsum */
  int32_t stats;
  float eps, momentum;          /* stats */
  /* 0: one batch.  >= 1 (at most 8): `groups` batches of B / groups images side by side (grouped batches, below) — the forward with
   * stats (no transform, no coef_out; (B / groups) * OH * OW a multiple of 128) and the grad-input with bnbwd (equal sub-pixel phases
   * — pcg_conv2d_dgrad_bn_phases of them — whose rows split into whole 128-row tiles per group; the partial rows keep the ungrouped
   * layout [phase][tile row]).  groups = 1 runs the grouped finalize on one group, not the ungrouped one.                          */
  int32_t groups;
} pcg_conv_args;
int pcg_conv2d(const pcg_conv_geom* g, const pcg_conv_args* a, pcg_stream_t stream);
int pcg_conv_weight_adjoint(const float* w, float* w_adj, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, pcg_stream_t stream);
/* The same for n <= 16 layers of one shape in ONE launch (host arrays of device pointers). */
int pcg_conv_weight_adjoint_many(const float* const* w, float* const* w_adj, int32_t n, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                                 pcg_stream_t stream);
int32_t pcg_conv2d_fwd_bn_partial_rows(const pcg_conv_geom* g);
int32_t pcg_conv2d_dgrad_bn_partial_rows(const pcg_conv_geom* g);
/* db[c] (+)= sum_rows dy[row][c]   (bias gradient of Conv2d / Linear; rows = B*OH*OW)             */
size_t pcg_colsum_workspace_bytes(int64_t rows, int32_t C);
int pcg_colsum(const float* dy, int64_t rows, int32_t C, float* db, int accumulate,
               void* workspace, size_t workspace_bytes, pcg_stream_t stream);

/* ---- BatchNorm (training mode) + activation --------------------------------------------------
 * replaces nn.BatchNorm2d(train) + nn.ReLU / nn.LeakyReLU(0.2): mnist_dcgan.py:77-87,103-110;
 * models/generator.py:12-15,18-20 (counteRGAN _ResBlock).  [torch] semantics: normalise with the
 * biased batch variance, eps inside the sqrt, running_var updated with the unbiased variance,
 * running = (1-momentum)*running + momentum*batch.                                                 */
size_t pcg_bn_workspace_bytes(int64_t rows, int32_t C);
/* stats over rows = B*H*W of x[rows][C]: writes save_mean[C], save_invstd[C]; updates running_* if non-null */
int pcg_bn_train_stats(const float* x, int64_t rows, int32_t C, float eps, float momentum,
                       float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                       int64_t* num_batches_tracked /*nullable: += 1*/,
                       void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* the same + the folded scale / shift [2][C] of y = x*scale + shift (gamma, beta required when coef_out != NULL) */
int pcg_bn_train_stats_coef(const float* x, int64_t rows, int32_t C, float eps, float momentum,
                            float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                            int64_t* num_batches_tracked, const float* gamma, const float* beta, float* coef_out,
                            void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* y = act( (x-mean)*invstd*gamma + beta ).  var_eps < 0: `invstd_or_var` holds invstd (training: save_invstd);
 * var_eps >= 0: it holds a variance and invstd = rsqrt(var + var_eps) (eval mode: running_var, eps).   */
int pcg_bn_apply_act(const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd_or_var,
                     float var_eps, const float* gamma, const float* beta, int act, float slope,
                     const float* residual /*nullable*/, float alpha /* y = residual + alpha*act(bn(x)) :
                     counteRGAN _ResBlock `x + 0.1*out`, models/generator.py:20; plain BN: NULL, 1 */,
                     float* y, pcg_stream_t stream);
/* backward of y = act(bn(x)):  given dy (grad wrt y), x (pre-BN), y (post-activation: the sign mask)
 *   dgamma (+)= sum dz*xhat ; dbeta (+)= sum dz ; dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)),
 *   dz = dy*act'(.)     ([torch] LeakyReLU/ReLU sub-gradient at 0 is the negative-side one: uses y>0) */
int pcg_bn_act_bwd(const float* dy, const float* x, const float* y /*nullable when act==NONE*/, int64_t rows, int32_t C,
                   const float* mean, const float* invstd, const float* gamma,
                   int act, float slope, float dy_scale /* dz = dy_scale*dy*act'(.) : the alpha of the forward */,
                   float* dx, float* dgamma, float* dbeta, int accumulate,
                   void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* The same without reading y: for ReLU / LeakyReLU the mask act'(y) is the sign of the BatchNorm output, recomputed from x with the
 * forward's own expression fma(x, gamma*invstd, beta - mean*gamma*invstd) — two HBM reads of the activation less per layer. */
int pcg_bn_act_bwd_premask(const float* dy, const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, int act, float slope, float dy_scale, float* dx, float* dgamma,
                           float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, pcg_stream_t stream);

/* BatchNorm backward from the partial sums a pcg_conv2d_*_bnbwd call left behind: dm = dy*act'(.) (already masked), partial =
 * fp64 [nparts][2][C] (sum dm, sum dm*xhat: every per-channel sum of the BatchNorm family is accumulated in double, as the
 * reference's CPU path does — [torch] at::acc_type<float, false>) in the opaque, 8-byte-aligned buffer of
 * pcg_conv2d_*_bn_workspace_bytes (its tail is scratch for the two-level
 * finalize used when there are >= 4096 partial rows).  Fixed-order fp64 finalize (dgamma, dbeta as in pcg_bn_act_bwd) + the elementwise pass
 * dx = gamma*invstd*(dm - mean(dm) - xhat*mean(dm*xhat)).  workspace: pcg_bn_bwd_partial_workspace_bytes(C). */
size_t pcg_bn_bwd_partial_workspace_bytes(int32_t C);
int pcg_bn_bwd_partial(const float* dm, const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd,
                       const float* gamma, const void* partial, int32_t nparts, float* dx, float* dgamma, float* dbeta,
                       int accumulate, void* workspace, size_t workspace_bytes, pcg_stream_t stream);

/* The same two backward calls, additionally returning the column sums of the dx they write: dcol[c] (+)= sum_rows dx[row][c] — the
 * bias gradient of the convolution in front of this BatchNorm (models/generator.py:11-14: Conv2d(bias=True) -> BatchNorm2d; the sum is
 * analytically zero, the reference computes its rounding residue, so it is computed) taken while dx streams out of the apply pass
 * instead of by a separate pcg_colsum pass over it (fp64 per thread, fixed-order block sums, fixed-order finalize).
 * y == NULL with ReLU / LeakyReLU and beta given: the mask is recomputed (as pcg_bn_act_bwd_premask). */
size_t pcg_bn_db_workspace_bytes(int64_t rows, int32_t C);
int pcg_bn_act_bwd_db(const float* dy, const float* x, const float* y /*nullable*/, int64_t rows, int32_t C, const float* mean,
                      const float* invstd, const float* gamma, const float* beta /*nullable*/, int act, float slope, float dy_scale,
                      float* dx, float* dgamma, float* dbeta, int accumulate, float* dcol, int accumulate_col, void* workspace,
                      size_t workspace_bytes, pcg_stream_t stream);
size_t pcg_bn_bwd_partial_db_workspace_bytes(int32_t C);
/* dm_scale: the partial sums already include this factor, the apply pass multiplies dm by it (1: plain) — the 0.1 of a residual
 * branch whose incoming gradient is the unscaled skip-path sum (PCG_CONV_EPI_ADD_BNSUM).  dcol may be NULL. */
int pcg_bn_bwd_partial_db(const float* dm, const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd,
                          const float* gamma, const void* partial, int32_t nparts, float dm_scale, float* dx, float* dgamma,
                          float* dbeta, int accumulate, float* dcol /*nullable*/, int accumulate_col, void* workspace,
                          size_t workspace_bytes, pcg_stream_t stream);

/* ---- grouped batches (r04): the discriminator's real and fake passes as ONE pass --------------------------------------------
 * mnist_dcgan.py:151-161 runs netD twice per D step — on the real batch and on fake.detach() — and adds the two backward passes
 * into .grad before optimizerD.step() (:164).  Neither pass depends on the other, so both run as one tensor of `groups` (= 2)
 * batches side by side along the batch axis: one convolution launch per layer and direction over 2B images, one weight-gradient
 * launch whose sum over pixels covers both batches (the .grad accumulation of :153,161).  BatchNorm keeps the reference's
 * semantics: every group has its OWN batch statistics (save_mean / save_invstd / the backward's two means are [groups][C], taken
 * from the group's own 64-row partial sums in the fixed order of the ungrouped finalize), the running statistics are updated
 * once per group in group order, num_batches_tracked advances by `groups`; dgamma / dbeta are the groups' sums added in group
 * order.  Against two separate passes the results differ only where a sum's ORDER differs: the weight gradients (one K-loop over
 * 2B images instead of two added results) — a few ulp, stated in tests/test_hip_groups.py.  Constraints: C / 4 a power of two
 * <= 256, (B / groups) * OH * OW a multiple of 128, equal sub-pixel phases; not available in the exact-BatchNorm data-parallel
 * mode.  Callers fall back to separate passes otherwise (pcgan_amd.nn.SequentialConvNet.supports_groups).                      */
/* y = act(bn_g(x)) with group g's statistics on group g's rows (training mode only: mean / invstd are save_mean / save_invstd) */
int pcg_bn_apply_act_g(const float* x, int64_t rows, int32_t C, const float* mean /*[groups][C]*/, const float* invstd /*[groups][C]*/,
                       const float* gamma, const float* beta, int act, float slope, float* y, int32_t groups, pcg_stream_t stream);
/* the sub-pixel phases of a grad-input launch (pcg_conv_args.groups with the bnbwd epilogue; pcg_bn_bwd_partial_g's nphases) */
int32_t pcg_conv2d_dgrad_bn_phases(const pcg_conv_geom* g);
/* pcg_bn_bwd_partial on `groups` side-by-side batches (partial rows from a grouped bnbwd grad-input; nphases = the phases of that launch) */
size_t pcg_bn_bwd_partial_g_workspace_bytes(int32_t C, int32_t groups);
int pcg_bn_bwd_partial_g(const float* dm, const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd,
                         const float* gamma, const void* partial, int32_t nparts, int32_t nphases, float* dx, float* dgamma,
                         float* dbeta, int accumulate, int32_t groups, void* workspace, size_t workspace_bytes, pcg_stream_t stream);
/* pcg_bn_act_bwd_premask on `groups` side-by-side batches (BatchNorm + ReLU / LeakyReLU backward behind a thin layer: one column
 * reduction per group, one grouped finalize, one grouped apply)                                                               */
size_t pcg_bn_act_bwd_g_workspace_bytes(int64_t rows, int32_t C, int32_t groups);
int pcg_bn_act_bwd_premask_g(const float* dy, const float* x, int64_t rows, int32_t C, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, int act, float slope, float* dx, float* dgamma, float* dbeta,
                             int accumulate, int32_t groups, void* workspace, size_t workspace_bytes, pcg_stream_t stream);

/* Thin forward fused with the BatchNorm backward of the layer below (r04).  A ConvTranspose2d with ONE output channel (DCGAN's G5,
 * mnist_dcgan.py:88) hands its grad-input — a forward convolution of the image gradient with Cin = 1 — to BatchNorm2d + ReLU
 * (:86-87).  The chain wrote that gradient (134 MB at batch 512), reduced it against z, and read both again; it costs 16 FMAs per
 * element to recompute, so here it never reaches memory: pass 1 leaves the two column sums, the usual finalize follows, pass 2
 * writes dz.  dgamma / dbeta as in pcg_bn_act_bwd.  Only k4, Cin = 1 geometries the row-block form covers (..._ok).               */
int32_t pcg_conv2d_fwd_bnbwd_thin_ok(const pcg_conv_geom* g);
size_t pcg_conv2d_fwd_bnbwd_thin_workspace_bytes(const pcg_conv_geom* g);
int pcg_conv2d_fwd_bnbwd_thin(const pcg_conv_geom* g, const float* x, const float* w, const float* z_below, const float* mean,
                              const float* invstd, const float* gamma, const float* beta, int act, float slope, float* dz,
                              float* dgamma /*nullable*/, float* dbeta /*nullable*/, int accumulate, void* workspace,
                              size_t workspace_bytes, pcg_stream_t stream);
/* The same idea for a FULL-WINDOW Cout = 1 convolution above a BatchNorm layer (r04): DCGAN D's last conv, Conv2d(512, 1, 4, 1, 0) on
 * a 4x4 map (mnist_dcgan.py:110), whose grad-input dy[b] * w[hw][c] is ONE multiply per element; the layer below is Conv -> BatchNorm2d
 * -> LeakyReLU (:107-109).  Instead of  outer product (write d) -> column sums (read d, z) -> apply (read d, z; write dz)  the sums
 * pass reads z only and the apply pass reads z and writes dz.  `groups` side-by-side batches of B / groups samples with their own
 * statistics (mean / invstd [G][C]; the paired D step, section "grouped batches"); dgamma / dbeta: the groups' sums in group order.
 * Eligibility (..._ok): Cout = 1, window = input map, KH*KW a divisor of 256, (Cin/4) a multiple of 256/(KH*KW), B / groups a
 * multiple of 16; not in the exact-BatchNorm data-parallel mode.                                                                */
int32_t pcg_conv2d_dgrad_bnbwd_full_ok(const pcg_conv_geom* g, int32_t groups);
size_t pcg_conv2d_dgrad_bnbwd_full_workspace_bytes(const pcg_conv_geom* g, int32_t groups);
int pcg_conv2d_dgrad_bnbwd_full(const pcg_conv_geom* g, const float* dy, const float* w, const float* z_below, const float* mean,
                                const float* invstd, const float* gamma, const float* beta, int act, float slope, float* dz,
                                float* dgamma /*nullable*/, float* dbeta /*nullable*/, int accumulate, int32_t groups, void* workspace,
                                size_t workspace_bytes, pcg_stream_t stream);

/* ... and its INPUT never needs the BatchNorm-apply pass (r04): the same full-window layer's forward and weight gradient read the
 * pre-BatchNorm output z of the layer below and evaluate act(bn(z)) in their loads, with that layer's batch statistics (mean / invstd
 * [groups][Cin], group = sample / (B / groups)) and the one bn_fold expression every BatchNorm pass uses — the values
 * pcg_bn_apply_act would have written.  Workspace of the weight gradient: pcg_conv2d_wgrad_workspace_bytes.
 * Eligibility: Cout = 1, window = input map, 256 % (Cin / 4) == 0, B / groups a multiple of 16.                                     */
int32_t pcg_conv2d_bnin_full_ok(const pcg_conv_geom* g, int32_t groups);
int pcg_conv2d_fwd_bnin_full(const pcg_conv_geom* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                             const float* beta, int in_act, float in_slope, int32_t groups, const float* w, const float* bias /*nullable*/,
                             int act, float slope, float* y, pcg_stream_t stream);
int pcg_conv2d_wgrad_bnin_full(const pcg_conv_geom* g, const float* z, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, int in_act, float in_slope, int32_t groups, const float* dy, float* dw, int accumulate,
                               void* workspace, size_t workspace_bytes, pcg_stream_t stream);

/* ---- pointwise activations (layers without BatchNorm) ----------------------------------------
 * nn.LeakyReLU after D's first conv (mnist_dcgan.py:101), nn.Tanh (:89), nn.Sigmoid (:112).        */
int pcg_act_fwd(const float* x, int64_t n, int act, float slope, float* y, pcg_stream_t stream);
/* dx = dy * act'(.) expressed through the OUTPUT y (relu/lrelu: y>0; tanh: 1-y^2; sigmoid: y(1-y)) */
int pcg_act_bwd(const float* dy, const float* y, int64_t n, int act, float slope, float* dx, pcg_stream_t stream);

/* ---- losses ----------------------------------------------------------------------------------
 * nn.BCELoss (mean): mnist_dcgan.py:125,152,160,172  ([torch]: log clamped at -100; backward
 * (p-t)/max(p(1-p),1e-12)/n).  loss is one float on the device; dp may be null (forward only).     */
int pcg_bce_fwd_bwd(const float* p, const float* target /*nullable → target_const*/, float target_const,
                    int64_t n, float grad_scale, const float* grad_out_dev /*nullable: one float, multiplies dp*/,
                    float* loss /*nullable*/, float* dp /*nullable*/, pcg_stream_t stream);
/* Two nn.BCELoss (mean) over the two halves of p in ONE launch: the discriminator's real and fake outputs side by side
 * (mnist_dcgan.py:152,160) and errD = errD_real + errD_fake (:163).  loss3 = {BCE(p[:n], target0), BCE(p[n:], target1), their fp32
 * sum}; the first two carry the bits pcg_bce_fwd_bwd gives on each half.  Backward: g0 / g1 / g2 = one-element device cotangents of
 * the three outputs (nullable: 0; all null: 1); dp[h*n + i] = (g_h + g2) / n * dBCE/dp.                                          */
int pcg_bce_pair(const float* p, int64_t n_half, float target0, float target1, const float* g0_dev /*nullable*/,
                 const float* g1_dev /*nullable*/, const float* g2_dev /*nullable*/, float* loss3 /*nullable*/, float* dp /*nullable*/,
                 pcg_stream_t stream);
/* nn.BCEWithLogitsLoss (mean): conditional_counteRGAN/mnist/trainer.py:79,106-107,117              */
int pcg_bce_logits_fwd_bwd(const float* z, float target_const, int64_t n, float grad_scale,
                           const float* grad_out_dev /*nullable*/, float* loss /*nullable*/, float* dz /*nullable*/,
                           pcg_stream_t stream);

/* ---- optimizer -------------------------------------------------------------------------------
 * torch.optim.Adam over one flat fp32 parameter buffer: mnist_dcgan.py:126-127,164,175;
 * mnist/trainer.py:77-78,112,123.  [torch] non-amsgrad, eps outside the sqrt of the bias-corrected
 * second moment: p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).  `step` is the 1-based step count.   */
/* Hyper-parameters are double, as in Python: 1-beta1, 1-beta2 and the bias corrections are formed in double and
 * rounded to fp32 once (that is what torch does). */
int pcg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled_wd,
                  int64_t step, pcg_stream_t stream);

/* hipGraph-capturable form: the step count lives on the device (*step_counter_dev is incremented by the
 * call) and the bias corrections are computed there in fp64, inside the update kernel itself: its last block to
 * finish stores the new count and the corrections of the next step.  hyper_scratch2_dev is 48 bytes (8-byte aligned)
 * the caller zero-initialises ONCE and then leaves alone. */
int pcg_adam_step_capturable(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                             double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled_wd,
                             int64_t* step_counter_dev, float* hyper_scratch2_dev, pcg_stream_t stream);

/* ---- CounteRGAN step: non-convolution pieces (conditional_counteRGAN/mnist) -------------------------
 * nn.Embedding(num_classes, H*W) lookup + torch.cat along channels (models/generator.py:73-74,
 * models/discriminator.py:35-36): out[b][p] = (x[b][p], table[idx[b]][p] [, mask[b][p]]) — exact copies.
 * bwd: dtable[k][p] (+)= sum_{b: idx[b]==k, ascending b} dinp[b][p][1];  dx[b][p] = dinp[b][p][0] (nullable).   */
int pcg_embed_concat_fwd(const float* x, const int64_t* idx, const float* table, const float* mask /*C==3*/,
                         float* out, int32_t B, int32_t HW, int32_t C, int32_t K, pcg_stream_t stream);
int pcg_embed_concat_bwd(const float* dinp, const int64_t* idx, float* dtable /*nullable*/, float* dx /*nullable*/,
                         int32_t B, int32_t HW, int32_t C, int32_t K, int accumulate, pcg_stream_t stream);
/* r04: the table gradient alone from channel `ch` of a [B][HW][C] gradient, and the [rows] column `ch` of a [rows][C] tensor — together
 * they let conv_in's grad-input be computed for its label-map channel only (the image and mask channels' gradients are read by nobody). */
int pcg_embed_table_grad(const float* dinp, const int64_t* idx, float* dtable, int32_t B, int32_t HW, int32_t C, int32_t ch, int32_t K,
                         int accumulate, pcg_stream_t stream);
int pcg_gather_channel(const float* src, float* dst, int32_t rows, int32_t C, int32_t ch, pcg_stream_t stream);
/* out = a*x + b*y (y nullable): residual-path gradient sums */
int pcg_axpby(float* out, float a, const float* x, float b, const float* y, int64_t n, pcg_stream_t stream);
/* raw = scale*c ; masked = raw*mask (generator.py:80-82);  bwd: dc = scale*(d_raw + d_masked*mask) */
int pcg_scale_mask_fwd(const float* c, const float* mask, float scale, float* raw, float* masked, int64_t n, pcg_stream_t stream);
int pcg_scale_mask_bwd(const float* d_raw /*nullable*/, const float* d_masked /*nullable*/, const float* mask, float scale,
                       float* dc, int64_t n, pcg_stream_t stream);
/* x_cf = clamp(x + r, lo, hi) (trainer.py:97); bwd: dr = dy on lo <= x+r <= hi, else 0 ([torch] clamp) */
int pcg_clamp_add_fwd(const float* x, const float* r, float lo, float hi, float* y, int64_t n, pcg_stream_t stream);
int pcg_clamp_add_bwd(const float* dy, const float* x, const float* r, float lo, float hi, float* dr, int64_t n, pcg_stream_t stream);
/* out[0] = mean |a*w|, w = m, 1-m (one_minus_m) or 1 (m NULL): trainer.py:99,119; bwd da (+)= g*sign(a*w)*w/n */
size_t pcg_abs_mean_workspace_bytes(void);
int pcg_abs_mean_fwd(const float* a, const float* m, int one_minus_m, int64_t n, float* out, void* workspace,
                     size_t workspace_bytes, pcg_stream_t stream);
int pcg_abs_mean_bwd(const float* a, const float* m, int one_minus_m, int64_t n, const float* grad_out_dev /*nullable*/,
                     float grad_scale, float* da, int accumulate, pcg_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) (discriminator.py:26): y[b][c] = mean over the HW pixels of x[b][p][c] */
int pcg_avgpool_fwd(const float* x, float* y, int32_t B, int32_t HW, int32_t C, pcg_stream_t stream);
int pcg_avgpool_bwd(const float* dy, float* dx, int32_t B, int32_t HW, int32_t C, pcg_stream_t stream);
/* nn.CrossEntropyLoss (mean) on logits [B][K] with int64 targets: trainer.py:80,118 */
int pcg_cross_entropy_fwd_bwd(const float* logits, const int64_t* target, int32_t B, int32_t K, float grad_scale,
                              const float* grad_out_dev /*nullable*/, float* loss /*nullable*/, float* dlogits /*nullable*/,
                              pcg_stream_t stream);

/* ---- device-side batch synthesis (counter-based Philox-4x32-10; deterministic in (seed, offset)) ---------------
 * Replaces the per-iteration host draws of the training loops: build_mask (trainer.py:45-72: per sample choose
 * `num_selected` of the (H/patch)x(W/patch) patches, nearest-upsample to HxW), torch.randint targets (trainer.py:94;
 * `exclude` != NULL applies house_sales trainer.py:248-249's rule: draw k uniformly over [low, high) and map a collision
 * k == exclude[i] to low + (k - low + 1) % (high - low), i.e. the next class gets probability 2/K, the others 1/K) and
 * torch.randn latent noise (mnist_dcgan.py:156).  Streams differ from torch's generators by design. */
int pcg_patch_mask(float* out /*[B][H][W]*/, int32_t B, int32_t H, int32_t W, int32_t patch_size, int32_t num_selected,
                   uint64_t seed, uint64_t offset, pcg_stream_t stream);
int pcg_randint(int64_t* out, int64_t n, int32_t low, int32_t high /*exclusive*/, const int64_t* exclude /*nullable*/,
                uint64_t seed, uint64_t offset, pcg_stream_t stream);
int pcg_randn(float* out, int64_t n, float mean, float std, uint64_t seed, uint64_t offset, pcg_stream_t stream);
/* Gumbel(0,1) noise  -log(-log(u))  — the draw inside F.gumbel_softmax (models/generator.py:90 of house_sales_kc_usa) */
int pcg_rand_gumbel(float* out, int64_t n, uint64_t seed, uint64_t offset, pcg_stream_t stream);
/* Bernoulli(1/2) feature mask [B][D] with the listed columns forced to 0 — house_sales_kc_usa/trainer.py:253-255 */
int pcg_feature_mask(float* out, int32_t B, int32_t D, const int32_t* zero_cols /*device, nullable*/, int32_t n_zero_cols,
                     uint64_t seed, uint64_t offset, pcg_stream_t stream);

/* ---- helpers ---------------------------------------------------------------------------------- */
int pcg_fill(float* p, int64_t n, float value, pcg_stream_t stream);
/* x[r][c] += bias[c] in place — the bias of a ConvTranspose2d that is run as one plain GEMM (a 1x1 input: all KH*KW output
 * positions of a channel share the bias; mnist_dcgan.py:76, mnist_wgan_conditional.py:61) */
int pcg_add_bias_rows(float* x, int64_t rows, int32_t C, const float* bias, pcg_stream_t stream);
/* out[0] (+)= sum p[i]^2   (grad_norm diagnostic: mnist/trainer.py:41-42) */
int pcg_sumsq(const float* p, int64_t n, float* out, int accumulate, pcg_stream_t stream);
/* out[0] = sum over segments s of || flat[seg[2s] .. seg[2s] + seg[2s+1]) ||_2 — the grad_norm diagnostic of
 * house_sales_kc_usa/trainer.py:182-183 (a SUM of per-parameter norms) in one launch over the net's flat gradient buffer;
 * seg_dev: int64 [nseg][2] = (offset, numel) of every parameter, on the device. */
int pcg_norm_sum(const float* flat, const int64_t* seg_dev, int32_t nseg, float* out, pcg_stream_t stream);

/* ---- tabular CounteRGAN (conditional_counteRGAN/house_sales_kc_usa), SURVEY.md section 8a row a15 -------------------
 * All operands are dense row-major fp32 [rows][features]; the layer widths (38, 32, 21, 17, 10, 9, 30, 6, 2, 5, 13, 1)
 * are too small and too ragged for the MFMA tiles, so these are bounds-checked VALU kernels.
 *
 * pcg_gemm: C[M][N] (+)= opA[M][K] . opB[K][N] (+ bias[N]); opA = A or A^T, opB = B or B^T (ld* = row stride of the
 * stored matrix).  nn.Linear forward  y = x W^T + b  -> (0,1, B,out,in, x, W, y, bias)
 *                  input gradient     dx = dy W       -> (0,0, B,in,out, dy, W, dx)
 *                  weight gradient    dW += dy^T x    -> (1,0, out,in,B, dy, x, dW, accumulate=1)
 * replaces the nn.Linear calls of models/generator.py:11-12,22-25,47,54-60, models/discriminator.py:9-15 and
 * models/nn_classifier.py:8-27. */
int pcg_gemm(int transA, int transB, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
             float* C, int32_t ldc, const float* bias, int accumulate, pcg_stream_t stream);
/* pcg_gemm with the layer's ReLU / LeakyReLU fused into the output write (Linear + LeakyReLU: discriminator.py:9-14, nn_classifier.py:8-25) */
int pcg_gemm_act(int transA, int transB, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb,
                 float* C, int32_t ldc, const float* bias, int accumulate, int act, float slope, pcg_stream_t stream);
/* nn.Linear weight + bias gradient in one launch, reducing over the batch with a deterministic split over row slabs:
 * dW[O][I] (+)= dy^T x, db[O] (+)= column sums of dy (db nullable).  dy / x may be column slices (ld = row stride).
 * tickets: caller-owned int32[pcg_linear_wgrad_ticket_count()], zero before first use; the kernel leaves it zero. */
size_t pcg_linear_wgrad_workspace_bytes(int32_t B, int32_t O, int32_t I);
int32_t pcg_linear_wgrad_ticket_count(void);
int pcg_linear_wgrad(const float* dy, int32_t ldy, const float* x, int32_t ldx, int32_t B, int32_t O, int32_t I, float* dW, float* db,
                     int accumulate_w, int accumulate_b, void* workspace, size_t workspace_bytes, int32_t* tickets, pcg_stream_t stream);
/* The same for up to 40 LAYERS that reduce over the SAME B rows, in one launch on the matrix cores — the 29 Linear layers of the
 * tabular generator's backward.  The library cuts every layer into 32x32 output tiles (at most 64 per call) and the rows into
 * slabs; tile_x / tile_y are reserved (0).  tickets: int32[>= 64], zero before first use, left zero.
 * pcg_linear_wgrad_grouped_slabs: partial results per layer the workspace holds. */
typedef struct pcg_wgrad_item {
  const float* dy; const float* x; float* dW; float* db /*nullable*/;
  int32_t ldy, ldx, O, I, accumulate_w, accumulate_b, tile_x, tile_y;
} pcg_wgrad_item;
int32_t pcg_linear_wgrad_grouped_slabs(int32_t B);
size_t pcg_linear_wgrad_grouped_workspace_bytes(int32_t B, const pcg_wgrad_item* items, int32_t n_items);
int pcg_linear_wgrad_grouped(const pcg_wgrad_item* items, int32_t n_items, int32_t B, void* workspace, size_t workspace_bytes,
                             int32_t* tickets, pcg_stream_t stream);
/* F.one_hot(idx, K).float() — trainer.py:250,290 */
int pcg_onehot(const int64_t* idx, int32_t B, int32_t K, float* out, pcg_stream_t stream);
/* torch.cat([a, b], dim=1) and its backward — generator.py:73-74, discriminator.py:19 */
int pcg_concat_cols(const float* a, int32_t ca, const float* b, int32_t cb, int32_t rows, float* out, pcg_stream_t stream);
int pcg_split_cols(const float* d, int32_t ca, int32_t cb, int32_t rows, float* da /*nullable*/, float* db /*nullable*/,
                   pcg_stream_t stream);
/* FiLM modulation y = gamma*h + beta — generator.py:13-16; backward gives dgamma = dy*h, dh = dy*gamma (dbeta = dy) */
int pcg_film_fwd(const float* gamma, const float* h, const float* beta, float* y, int64_t n, pcg_stream_t stream);
int pcg_film_bwd(const float* dy, const float* gamma, const float* h, float* dgamma, float* dh, int64_t n, pcg_stream_t stream);
/* F.gumbel_softmax(logits, tau, hard=False) over S heads packed side by side in T columns (seg_offsets[S+1], device
 * int32), with the Gumbel(0,1) noise supplied — generator.py:86-90.  y = softmax((logits + noise)/tau) per head;
 * y_hard (nullable) = one-hot of the per-head argmax of y: the forward value of hard=True (eval_utils.py:77), whose
 * straight-through backward is the soft one below. */
int pcg_gumbel_softmax_fwd(const float* logits, const float* noise, const int32_t* seg_offsets, int32_t S, int32_t T, int32_t B,
                           float tau, float* y, float* y_hard /*nullable*/, pcg_stream_t stream);
int pcg_gumbel_softmax_bwd(const float* dy, const float* y, const int32_t* seg_offsets, int32_t S, int32_t T, int32_t B, float tau,
                           float* dlogits, pcg_stream_t stream);
/* residual_full — trainer.py:266-279: column cont_idx[i] = cont[:, i]; categorical column cat_idx[s] =
 * samples[:, head s] . norm_vals[head s] - x[:, cat_idx[s]].  ncont + S must equal D. */
int pcg_assemble_residual_fwd(const float* cont, int32_t ncont, const int32_t* cont_idx, const float* samples,
                              const int32_t* seg_offsets, int32_t S, int32_t T, const int32_t* cat_idx, const float* norm_vals,
                              const float* x, int32_t D, int32_t B, float* residual, pcg_stream_t stream);
int pcg_assemble_residual_bwd(const float* dres, int32_t ncont, const int32_t* cont_idx, const int32_t* seg_offsets, int32_t S,
                              int32_t T, const int32_t* cat_idx, const float* norm_vals, int32_t D, int32_t B, float* dcont,
                              float* dsamples, pcg_stream_t stream);
/* tensor.mean() (Wasserstein critic losses, trainer.py:292,299) and its backward dx = grad_out * grad_scale / n */
size_t pcg_mean_workspace_bytes(void);
int pcg_mean_fwd(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, pcg_stream_t stream);
int pcg_mean_bwd(const float* grad_out_dev /*nullable = 1*/, float grad_scale, int64_t n, float* dx, pcg_stream_t stream);
/* torch.nn.utils.spectral_norm (n_power_iterations = 1) — discriminator.py:9-15.  Forward: when power_iteration != 0
 * (training mode) v <- normalize(W^T u), u <- normalize(W v) in place, then sigma = u.(W v), w_bar = W / sigma.
 * u_used / v_used (nullable): copies of the vectors this forward used — what torch's `u.clone()` keeps for backward,
 * since a later forward overwrites u and v.  Backward (u, v constants): dW (+)= (dw_bar - <dw_bar, w_bar> u v^T) / sigma.
 * Dimensions up to 256. */
int pcg_spectral_norm_fwd(const float* w_orig, int32_t out_features, int32_t in_features, float* u, float* v, float eps,
                          int power_iteration, float* w_bar, float* sigma, float* u_used, float* v_used, pcg_stream_t stream);
/* All (up to 8) spectral-norm layers of a net in one launch.  Every array member is a HOST array of device pointers / ints.
 * Forward: `reps` successive calls of every layer (each one power iteration from the previous call's u, v, as the module's forward
 * does: D(real) then D(fake)); reps > 1 needs power_iteration.  The output arrays hold reps * n entries, call-major (call r of layer
 * l: r * n + l).  At most 8 layers x calls. */
typedef struct pcg_sn_fwd_batch {
  int32_t n, reps, power_iteration;
  float eps;
  const float* const* w_orig;                          /* [n] */
  const int32_t* out_features; const int32_t* in_features;   /* [n] */
  float* const* u; float* const* v;                    /* [n], updated in place when power_iteration != 0 */
  float* const* w_bar; float* const* sigma;            /* [n * reps] */
  float* const* u_used; float* const* v_used;          /* [n * reps], entries nullable */
} pcg_sn_fwd_batch;
/* Backward of `passes` calls of the same n layers, applied one after the other into the same dw_orig[l] (the first writes or
 * accumulates as accumulate[l] says, the others add — what chained launches compute); per-call arrays hold passes * n entries,
 * pass-major.  Then, where db_dst[l] is given, db_dst[l] += db_src[l] over out_features[l] values (the bias gradient of a later pass,
 * reduced into its own buffer because one grouped weight-gradient launch cannot order two writers of the same vector). */
typedef struct pcg_sn_bwd_batch {
  int32_t n, passes;
  const float* const* dw_bar; const float* const* w_bar;     /* [n * passes] */
  const int32_t* out_features; const int32_t* in_features;   /* [n] */
  const float* const* u; const float* const* v; const float* const* sigma;   /* [n * passes] */
  float* const* dw_orig;                               /* [n] */
  const int32_t* accumulate;                           /* [n] */
  float* const* db_dst;                                /* nullable; [n], entries nullable */
  const float* const* db_src;                          /* nullable; [n], needed where db_dst[l] is given */
} pcg_sn_bwd_batch;
int pcg_spectral_norm_fwd_batched(const pcg_sn_fwd_batch* batch, pcg_stream_t stream);
int pcg_spectral_norm_bwd_batched(const pcg_sn_bwd_batch* batch, pcg_stream_t stream);
int pcg_spectral_norm_bwd(const float* dw_bar, const float* w_bar, int32_t out_features, int32_t in_features, const float* u,
                          const float* v, const float* sigma, float* dw_orig, int accumulate, pcg_stream_t stream);

/* ---- conditional WGAN-GP (conditional_gan/mnist/mnist_wgan_conditional.py), SURVEY.md section 8a row a14 -----------------
 * nn.InstanceNorm2d(C, affine=True) (:88,91,94) on an NHWC activation [B][HW][C]: statistics per (sample, channel) over HW,
 * biased variance, eps inside the square root; `act` fuses the LeakyReLU(0.2) that follows (:89,92,95). */
int pcg_instnorm_fwd(const float* x, int32_t B, int32_t HW, int32_t C, const float* gamma, const float* beta, float eps, int act,
                     float slope, float* y, float* mean /*[B*C]*/, float* invstd /*[B*C]*/, pcg_stream_t stream);
/* backward: dx (nullable); per-sample partial sums dgamma_partial / dbeta_partial [B][C] (nullable; reduce over B with pcg_colsum) */
int pcg_instnorm_bwd(const float* dy, const float* x, int32_t B, int32_t HW, int32_t C, const float* mean, const float* invstd,
                     const float* gamma, float* dx, float* dgamma_partial, float* dbeta_partial, pcg_stream_t stream);
/* the same with the stage's neighbours folded in (one launch for what autograd runs as LeakyReLU backward, InstanceNorm backward, an
 * add and the conv bias gradient's reduction, :88-95): act_y (nullable) = the LeakyReLU OUTPUT, dy is multiplied by lrelu'(.) first
 * (dn_out, nullable, keeps that masked gradient for the double backward); addend (nullable) is added to the stored dx;
 * dxsum_partial (nullable) [B][C] = sum over HW of the stored dx (the conv bias gradient's per-sample partial).                  */
int pcg_instnorm_bwd_fused(const float* dy, const float* act_y, float neg_slope, const float* x, int32_t B, int32_t HW, int32_t C,
                           const float* mean, const float* invstd, const float* gamma, float* dn_out, const float* addend, float* dx,
                           float* dgamma_partial, float* dbeta_partial, float* dxsum_partial, pcg_stream_t stream);
/* sums over the rows of up to three [rows][C] partial arrays (the three above) in one launch; acc_k: dst_k += instead of =        */
int pcg_rowsum3(int32_t n, const float* src0, float* dst0, int acc0, const float* src1, float* dst1, int acc1, const float* src2,
                float* dst2, int acc2, int32_t rows, int32_t C, pcg_stream_t stream);
/* backward of pcg_instnorm_bwd — what autograd.grad(..., create_graph=True) + critic_loss.backward() (:149,154) need: with r
 * the cotangent on dx, returns the cotangents reaching dy (ddy), x (ez) and gamma (per-sample partials); any may be NULL. */
int pcg_instnorm_bwd_bwd(const float* r, const float* dy, const float* x, int32_t B, int32_t HW, int32_t C, const float* mean,
                         const float* invstd, const float* gamma, float* ddy, float* ez, float* dgamma_partial, pcg_stream_t stream);
/* ... with the cotangent ddy continuing through the stage's LeakyReLU (act_y = its output; nullable) in the same launch          */
int pcg_instnorm_bwd_bwd_act(const float* r, const float* dy, const float* x, int32_t B, int32_t HW, int32_t C, const float* mean,
                             const float* invstd, const float* gamma, const float* act_y, float neg_slope, float* ddy, float* ez,
                             float* dgamma_partial, pcg_stream_t stream);
/* nn.Flatten of an NCHW tensor (:96) from the NHWC activation, flat[b][c*HW + p] = act[b][p][c]; inverse != 0: the other way */
int pcg_nhwc_to_nchw_flat(const float* src, float* dst, int32_t B, int32_t HW, int32_t C, int inverse, pcg_stream_t stream);
/* x3 = [real | fake | alpha*real + (1-alpha)*fake] (3B samples): the input of the batched critic pass in one launch (r04) */
int pcg_interpolate_stack(const float* alpha, const float* real, const float* fake, float* x3, int32_t B, int32_t per_sample,
                          pcg_stream_t stream);
/* interpolates = alpha*real + (1-alpha)*fake, alpha per sample (:147) */
int pcg_interpolate(const float* alpha, const float* real, const float* fake, float* out, int32_t B, int32_t per_sample,
                    pcg_stream_t stream);
/* gradient penalty lambda * mean_b (||g_b||_2 - 1)^2 (:150): forward keeps the per-sample norms for the backward,
 * dg = grad_out * 2*lambda/B * (||g_b|| - 1) * g_b / ||g_b|| */
int pcg_gradient_penalty_fwd(const float* grads, int32_t B, int32_t per_sample, float lambda, float* norms /*[B]*/, float* penalty /*[1]*/,
                             pcg_stream_t stream);
int pcg_gradient_penalty_bwd(const float* grads, const float* norms, const float* grad_out_dev /*nullable = 1*/, int32_t B,
                             int32_t per_sample, float lambda, float* dgrads, pcg_stream_t stream);
/* torch.rand: uniform [0, 1) — the interpolation coefficients alpha (:146) */
int pcg_rand_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, pcg_stream_t stream);

/* ---- counterfactual evaluation -----------------------------------------------------------------
 * out[0] = class-flip rate = mean_b [argmax logits_cf[b] == target[b]];
 * out[1] = prediction gain = mean_b (softmax(logits_cf[b])[target[b]] - q_b) with q_b = softmax(logits_ref[b])[target[b]]
 * (house_sales_kc_usa/eval_utils.py:246-258) or, when logits_ref is NULL, softmax(logits_cf[b])[other[b]]
 * (mnist/eval_utils.py:61-64).  Actionability (mean |residual|) is pcg_abs_mean_fwd. */
int pcg_cf_metrics(const float* logits_cf, const float* logits_ref /*nullable*/, const int64_t* target, const int64_t* other /*nullable*/,
                   int32_t B, int32_t K, float* out /*[2]*/, pcg_stream_t stream);

/* ---- classifier pre-training -----------------------------------------------------------------
 * nn.CrossEntropyLoss(weight=class_weight), mean reduction = weighted sum / sum of the weights of the targets
 * (house_sales_kc_usa/trainer.py:55-57) */
int pcg_cross_entropy_weighted_fwd_bwd(const float* logits, const int64_t* target, const float* class_weight, int32_t B, int32_t K,
                                       float grad_scale, const float* grad_out_dev /*nullable*/, float* loss /*nullable*/,
                                       float* dlogits /*nullable*/, pcg_stream_t stream);
/* nn.Dropout / nn.Dropout2d in training mode, forward and backward (same map): y = x * mask * scale, scale = 1/(1-p).
 * Dropout: inner = 1, mask has n entries; Dropout2d on an NHWC activation [B][HW][C]: inner = HW, mask is [B][C]
 * (mnist/models/classifier.py:13,19; house_sales_kc_usa/models/nn_classifier.py:11,16,22).  The 0/1 mask is an input:
 * pcg_rand_bernoulli draws it on the device (keep probability 1-p); parity runs pass the reference's draws. */
int pcg_dropout_apply(const float* x, const float* mask, int64_t n, int32_t inner, int32_t C, float scale, float* y, pcg_stream_t stream);
int pcg_rand_bernoulli(float* out, int64_t n, float keep_prob, uint64_t seed, uint64_t offset, pcg_stream_t stream);

/* ---- input pipeline -------------------------------------------------------------------------
 * transforms.Resize -> ToTensor -> Normalize (dconv_gan/mnist/mnist_dcgan.py:42-46) for a batch of 8-bit one-channel images:
 * Pillow's separable fixed-point bilinear resize (bounds[2*i] = first source index, bounds[2*i+1] = taps, coefficients with 22
 * fractional bits, ksize per output coordinate — built by the host as Pillow's precompute_coeffs does), rounding to uint8
 * after each pass, then float32 v/255 and (t - mean)/std.  dst: [N][OH][OW] float32 (= [N,1,OH,OW]). */
int pcg_resize8_normalize(const uint8_t* src, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, const int32_t* x_bounds,
                          const int32_t* x_coeffs, int32_t x_ksize, const int32_t* y_bounds, const int32_t* y_coeffs, int32_t y_ksize,
                          float mean, float stdv, float* dst, pcg_stream_t stream);

/* ---- fused tabular generator (house_sales_kc_usa/models/generator.py:38-92) -------------------------------------------------
 * The whole ResidualGenerator forward (fc_in, 5 x [fc1, BatchNorm1d, FiLM, ReLU, fc2, BatchNorm1d, FiLM, residual add], the
 * continuous head and the packed Gumbel-softmax heads) as 11 launches and its backward (down to the pre-activation gradients
 * every Linear's weight gradient needs) as 11 launches: one thread per batch row, kernels cut at the BatchNorm statistics.
 * Built for hidden width 32 and 5 blocks (the reference's configuration, config.py:15-17); all buffers are the caller's.
 * Offsets are element offsets into ONE flat fp32 parameter buffer (and the gradient buffer of the same layout). */
#define PCG_HOUSE_ROWS_PER_BLOCK 64
typedef struct pcg_house_g_desc {
  int32_t fc_in_w, fc_in_b;
  int32_t fc1_w[5], fc1_b[5], bn1_g[5], bn1_b[5], fc2_w[5], fc2_b[5], bn2_g[5], bn2_b[5];
  int32_t film_gamma_w[5], film_gamma_b[5], film_beta_w[5], film_beta_b[5];
  int32_t cont_w, cont_b;
  int32_t head_w[8], head_b[8], seg[9];      /* categorical heads and their packed column offsets (seg[nheads] = T) */
  int32_t nheads, ncont, D, NC;              /* D = input_dim, NC = num_classes */
  int32_t hidden, nblocks;                   /* must be 32 and 5 */
} pcg_house_g_desc;

typedef struct pcg_house_g_fwd_args {
  const float* params;
  const float *x, *onehot, *mask, *noise;    /* [B][D], [B][NC], [B][D], Gumbel noise [B][T] */
  float* inp;                                /* out [B][D+NC+D]: (x, onehot, mask) — the cond operand of later weight gradients */
  float *H, *Z1, *Z2;                        /* out [6][B][32], [5][B][32], [5][B][32]: block inputs and pre-BatchNorm activations */
  float* P;                                  /* scratch [10][ceil(B/64)][2][32] partial statistics */
  float* SM;                                 /* out [10][2][32] saved mean / invstd (layer order bn1_0, bn2_0, bn1_1, ...) */
  float* running_mean[10]; float* running_var[10]; int64_t* num_batches_tracked[10];   /* nullable: BatchNorm buffers to update */
  float *cont, *logits, *soft, *hard;        /* out [B][ncont], [B][T], [B][T], nullable [B][T] one-hot of the soft arg-max */
  int32_t B;
  float eps, momentum, tau, res_scale;
} pcg_house_g_fwd_args;

typedef struct pcg_house_g_bwd_args {
  const float* params; float* grads;         /* BatchNorm gamma / beta gradients are written into `grads` (accumulate flag) */
  const float *onehot, *mask;
  const float *H, *Z1, *Z2, *SM, *soft;      /* from the forward */
  const float *d_cont, *d_logits, *d_samples;/* nullable cotangents of the three outputs */
  float *DH, *DZ1, *DZ2, *A1;                /* out [5][B][32] each: block-top gradients, pre-BN gradients (weight-gradient operands), ReLU outputs */
  float* DN1;                                /* scratch [B][32] */
  float *DG, *DB;                            /* out [5][B][32]: gradients at the FiLM gamma / beta Linear outputs */
  float* DZIN;                               /* out [B][32]: gradient at fc_in's output */
  float *DL, *DC;                            /* out [B][T], [B][ncont]: gradients at the head outputs */
  float* Q;                                  /* scratch [9 * ceil(B/64) + ceil(B/16)][2][32]: per-block partial sums of the ten BatchNorm backwards
                                                (64-row blocks; the last bn2's come from the 16-row head kernel) */
  int32_t B, accumulate;
  float tau, res_scale;
} pcg_house_g_bwd_args;

int pcg_house_g_fwd(const pcg_house_g_desc* desc, const pcg_house_g_fwd_args* args, pcg_stream_t stream);
int pcg_house_g_bwd(const pcg_house_g_desc* desc, const pcg_house_g_bwd_args* args, pcg_stream_t stream);

/* Loss composition on the device: total = sum_i w_i * term_i for up to 8 one-element loss tensors, e.g.
 * G_loss = G_adv + lambda_cls*G_cls + lambda_reg*G_reg + lambda_mask*mask_pen (house_sales_kc_usa/trainer.py:307-312); the backward
 * hands every term its w_i * grad_out.  One launch each instead of a dozen scalar tensor-op kernels. */
int pcg_weighted_sum_fwd(int32_t n, const float* const* terms, const float* weights, float* out, pcg_stream_t stream);
int pcg_weighted_sum_bwd(int32_t n, const float* weights, const float* grad_out_dev /*nullable = 1*/, float* const* grads /*entries nullable*/,
                         pcg_stream_t stream);

/* The tabular spectral-norm critic (house_sales_kc_usa/models/discriminator.py:5-20) as one forward and one backward launch, one
 * thread per row, for n_pass (1 or 2) independent passes per launch — D(real) and D(fake) of the critic step (trainer.py:290-291)
 * share the module but not the spectral-norm weights (two successive power iterations).  Every per-pass member is a HOST array of
 * n_pass device pointers; w_bar has n_pass * 4 entries (pass-major): the four layers' normalised weights (from
 * pcg_spectral_norm_fwd_batched); bias[4].  Forward writes the concatenated input a0 [B][21] and the post-LeakyReLU activations
 * a1 [B][32], a2 [B][64], a3 [B][128]; backward writes the pre-activation gradients d3, d2, d1 (the dy operands of the weight
 * gradients; layer 4's is dout itself) and, where dx[q] != NULL, the gradient of the first D input columns.  Built for input_dim +
 * num_classes = 21, hidden width 32. */
typedef struct pcg_house_critic_fwd_args {
  int32_t n_pass, B, D, NC;
  float slope;
  const float* const* x; const float* const* onehot;
  const float* const* w_bar; const float* const* bias;
  float* const* a0; float* const* a1; float* const* a2; float* const* a3; float* const* out;
} pcg_house_critic_fwd_args;
typedef struct pcg_house_critic_bwd_args {
  int32_t n_pass, B, D;
  float slope;
  const float* const* dout; const float* const* w_bar;
  const float* const* a1; const float* const* a2; const float* const* a3;
  float* const* d3; float* const* d2; float* const* d1;
  float* const* dx;                                    /* [n_pass], entries nullable */
} pcg_house_critic_bwd_args;
int pcg_house_critic_fwd(const pcg_house_critic_fwd_args* args, pcg_stream_t stream);
int pcg_house_critic_bwd(const pcg_house_critic_bwd_args* args, pcg_stream_t stream);

/* "Riders": two launches of the tabular step that do not depend on each other issued as ONE launch whose blocks split between the
 * two kernel bodies (a HIP graph with parallel branches is launched node by node by the host; one launch is not).  Same bodies, same
 * bits as the separate calls.  At the ABI a rider is an optional (nullable) argument struct of the launch that carries it:
 *   pcg_house_residual_fwd   + a training-mode pcg_sn_fwd_batch: the critic step's power iterations only need the critic's weights
 *                              (trainer.py:266-287 beside models/discriminator.py:9-16)
 *   pcg_house_residual_bwd   + pcg_house_loss_args (+ pcg_house_diag_args): the logged scalars do not feed the backward
 *                              (trainer.py:314 beside :292, :307-312)
 *   pcg_house_classifier_fwd + pcg_sn_bwd_batch, and
 *   pcg_house_classifier_bwd + a training-mode pcg_sn_fwd_batch: the frozen classifier's term (trainer.py:301-302) does not depend on
 *                              the critic update (:290-295), so its two launches carry the critic's spectral-norm work that is on
 *                              the chain at the same time
 *
 * The frozen tabular classifier of the counterfactual loss (house_sales_kc_usa/models/nn_classifier.py:4-32 in eval mode, each
 * BatchNorm1d folded into the following Linear by the caller: Linear 17->256, 256->256, 256->128, 128->64 + LeakyReLU(0.1), Linear
 * 64->4) as one launch each way on the matrix cores, 16 rows per block, activations in LDS between layers.
 *   forward:  w_kmajor[l], l = 0..3: the folded weight TRANSPOSED, [K_l][N_l] row-major, layer 0 zero-padded to K = 20;
 *             w_kmajor[4]: the last layer as stored [4][64]; bias[l]; writes the post-activation outputs a1 [B][256], a2 [B][256],
 *             a3 [B][128], a4 [B][64] (the backward's masks) and logits [B][4].
 *             ce_target != NULL (only with a rider): the forward also evaluates the cross-entropy of its logits against ce_target
 *             (trainer.py:302) — per row the term lse - z[target] into ce_row_loss[B] and ce_grad_scale / B * (softmax - onehot)
 *             into ce_dlogits[B][4] (16-byte aligned), the expressions of pcg_cross_entropy_fwd_bwd; pcg_house_residual_bwd with
 *             pcg_house_loss_args(ce_row_loss, n_ce = B) then forms the mean in that kernel's summation order (out6[5], and uses it
 *             for G_loss instead of *g_cls): the same bits as the separate cross-entropy launch.
 *   backward: w_stored[l]: the folded weights as stored [N_l][K_l]; dx [B][17] = d(logits . dlogits)/dx.  (trainer.py:301-302;
 *             the parameters are frozen, main.py:27-30: no weight gradients.) */
typedef struct pcg_house_cls_fwd_args {
  const float* x;
  int32_t B;
  const float* const* w_kmajor; const float* const* bias;    /* HOST arrays of 5 device pointers */
  float* a1; float* a2; float* a3; float* a4; float* logits;
  const int64_t* ce_target;                            /* nullable: no cross-entropy tail */
  float ce_grad_scale;
  float* ce_dlogits; float* ce_row_loss;               /* needed with ce_target */
} pcg_house_cls_fwd_args;
typedef struct pcg_house_cls_bwd_args {
  const float* dlogits;
  int32_t B;
  const float* const* w_stored;                        /* HOST array of 5 device pointers */
  const float* a1; const float* a2; const float* a3; const float* a4;
  float* dx;
} pcg_house_cls_bwd_args;
int pcg_house_classifier_fwd(const pcg_house_cls_fwd_args* args, const pcg_sn_bwd_batch* rider /*nullable*/, pcg_stream_t stream);
int pcg_house_classifier_bwd(const pcg_house_cls_bwd_args* args, const pcg_sn_fwd_batch* rider /*nullable*/, pcg_stream_t stream);

/* Prompted counterfactual queries and evaluation of the trained tabular CounteRGAN in ONE launch (csrc/house_cf_eval.hip):
 * house_sales_kc_usa/eval_utils.py:25-181 (build_counterfactuals), :185-289 (compute_metrics_per_target: every target class, every
 * loader batch), :351-434 (analyze_class_pair_sensitivity) and gradio_app.py:144-169 (this row, that class, only these features).
 * Both nets in eval mode (BatchNorm: the running statistics, 1 / sqrtf(var + eps)), so rows are independent; nothing of the nets is
 * written.  Built for the descriptor's D = 17, NC = 4, hidden = 32, nblocks = 5, seg[nheads] <= 96, ncont + nheads = 17, and the
 * classifier image of pcg_house_classifier_fwd (c_w_kmajor / c_bias).  One work item is (target slot t, row i):
 *   generator   cond = [onehot(target), mask]; h = relu(fc_in([x, cond])); five blocks; cont = res_scale * fc_cont(h); the packed
 *               head logits; per head the hard Gumbel-softmax sample by pcg_gumbel_softmax_fwd's rule on (logit + noise) / tau
 *   residual    column f: cont (col_src[f] = its index >= 0) or norm_vals[seg[s] + chosen[s]] - x[f] (col_src[f] = -(s + 1));
 *               masked = residual * mask; x_cf_raw = x + masked (two roundings); x_cf = clamp(x_cf_raw, 0, 1)
 *   classifier  logits_x = C(x), logits_cf = C(clamp_cls ? x_cf : x_cf_raw)  (eval_utils.py:245 classifies the raw sum,
 *               gradio_app.py:163-169 the clamped one); gain = softmax(logits_cf)[target] - softmax(logits_x)[target]; pred = the
 *               first maximum
 * Forms:  sweep    target NULL: slots t = 0..T-1 are the target classes (1 <= T <= 4), every row
 *         per row  target [N] (int64, values in [0, 4)), T = 1
 * mask: [17] broadcast (mask_rows = 0) or [N][17] (mask_rows = 1).  noise [T][N][seg[nheads]]: always an input.
 * `group` is the loader's batch size: rows are cut into 16-row tiles that never straddle a group; tiles_per_group =
 * ceil(min(group, N) / 16), n_tiles = ceil(N / group) * tiles_per_group, tile q holds rows of group q / tiles_per_group (possibly
 * none).  One workgroup per tile runs all T slots.  Every per-row output is optional (NULL: not written); leading dimensions [T][N]
 * (logits_x, pred_x: [N]).  tile_sums [T][n_tiles][4], optional: over the tile's rows with y NULL or y[i] != target
 * (eval_utils.py:226) their count, the count with pred_cf == target, the sum of gain and the sum of |masked| over the 17 columns.
 * class_sums [T][n_tiles][4][17] with class_counts [T][n_tiles][4] (together, optional, need y): per source class y the sum of
 * |masked| per feature and the row count.  Fixed summation order (ascending row, ascending feature), no atomics: bitwise repeatable. */
typedef struct pcg_house_cf_eval_args {
  int64_t N; int32_t T, group, clamp_cls, mask_rows;
  const float* g_flat; int32_t nG;                     /* the generator's flat parameter buffer and its element count             */
  const float* bn_mean[10]; const float* bn_var[10];   /* running statistics, layer order bn1_0, bn2_0, bn1_1, ...                */
  float bn_eps, tau, res_scale;
  int32_t col_src[17];
  const float* norm_vals;                              /* [seg[nheads]] normalised category values, head order                    */
  const float* const* c_w_kmajor; const float* const* c_bias;   /* HOST arrays of 5 device pointers (pcg_house_cls_fwd_args)      */
  const float* x; const int64_t* y;                    /* [N][17]; [N] or NULL                                                    */
  const int64_t* target; const float* mask; const float* noise;
  float* cont; float* logits; int32_t* chosen;         /* [T][N][ncont], [T][N][seg[nheads]], [T][N][nheads]                      */
  float* masked; float* x_cf; float* x_cf_raw;         /* [T][N][17]                                                              */
  float* logits_cf; float* logits_x;                   /* [T][N][4]; [N][4]                                                       */
  int64_t* pred_cf; int64_t* pred_x;                   /* [T][N]; [N]                                                             */
  float* gain;                                         /* [T][N]                                                                  */
  float* tile_sums; float* class_sums; float* class_counts;
} pcg_house_cf_eval_args;
int pcg_house_cf_eval(const pcg_house_g_desc* desc, const pcg_house_cf_eval_args* args, pcg_stream_t stream);

/* Prompted queries and per-target evaluation of the MNIST CounteRGAN (csrc/mnist_cf_eval.hip): what surrounds the
 * generator's and the classifier's convolutions when ONE pass carries every (target class, row) query of a loader batch.
 * A query is q = t * B + b (target-major) for B rows and T targets per row:
 *   sweep    target NULL, T <= K: query (t, b) asks for target class t
 *   per row  target [B] (int64, values in [0, K)), T = 1
 * Every launch works on a window [q0, q0 + nq) of the T * B queries so that the host can chunk; per-QUERY inputs and outputs
 * (out, c, x_cf, raw, masked, sums, logits_cf, tail_sums, pred ... flip) are indexed by q - q0, per-ROW ones (x, y_true, target,
 * logits_orig) by b.  x is never replicated T times, neither is the mask: mask_mode says which row of `mask` a query reads.
 * fp32, no atomics, every sum in one fixed order (two calls give the same bits). */
enum { PCG_MASK_SHARED = 0,      /* mask [HW]        one mask for every query                                                  */
       PCG_MASK_PER_ROW = 1,     /* mask [B][HW]     query (t, b) reads row b                                                  */
       PCG_MASK_PER_QUERY = 2 }; /* mask [T*B][HW]   query q reads row q (NOT window-relative)                                  */

/* eval_utils.py:247-256 create_mask_from_indices / gradio_app.py:234-240 make_mask_from_patch_list: bit p of bits[m] set = patch
 * p = (i, j) = divmod(p, W / ps) of mask m is modifiable: mask[m][i*ps .. (i+1)*ps)[j*ps .. (j+1)*ps) = 1, everything else 0 (the
 * pixels outside the (H/ps)*ps x (W/ps)*ps grid included).  Needs (H/ps) * (W/ps) <= 64. */
typedef struct pcg_patch_mask_bits_args {
  const uint64_t* bits;   /* [n]        */
  float* mask;            /* [n][H][W]  */
  int32_t n, H, W, ps;
} pcg_patch_mask_bits_args;
int pcg_patch_mask_bits(const pcg_patch_mask_bits_args* args, pcg_stream_t stream);

/* generator.py:73-74 `torch.cat([x, embed(target).view(B,1,H,W), mask], 1)` for the window's queries, NHWC:
 * out[q - q0][p] = (x[b][p], table[target(q)][p], mask[row(q)][p]) — pcg_embed_concat_fwd with the broadcast done by indexing. */
typedef struct pcg_mnist_cf_entry_args {
  const float* x;          /* [B][HW]                              */
  const float* table;      /* [K][HW]  the label embedding         */
  const float* mask;       /* see mask_mode                        */
  const int64_t* target;   /* NULL (sweep) or [B]                  */
  float* out;              /* [nq][HW][3]                          */
  int32_t B, T, HW, K, mask_mode, q0, nq;
} pcg_mnist_cf_entry_args;
int pcg_mnist_cf_entry(const pcg_mnist_cf_entry_args* args, pcg_stream_t stream);

/* generator.py:80,82 + eval_utils.py:57,66,325,330 from conv_out's result c: raw = scale * c, masked = raw * m,
 * x_cf = clamp(x[b] + masked, -1, 1), each product and sum rounded on its own as the reference's tensor expressions are.  x_cf is
 * always written (rows of HW floats: the classifier's input), raw and masked only when given.  sums[q - q0] =
 * { sum |x_cf - x|, sum |raw * m|, sum |raw * (1 - m)| } over the HW pixels: the numerators of actionability,
 * Residual_L1_norm_in_allowed_patches and mask_penalty_pre.  One wave per query, 16-byte loads (HW % 4 == 0, 16-byte aligned
 * pointers), the wave's partial sums combined by a fixed butterfly. */
typedef struct pcg_mnist_cf_tail_args {
  const float* c;          /* [nq][HW]                             */
  const float* x;          /* [B][HW]                              */
  const float* mask;       /* see mask_mode                        */
  float* x_cf;             /* [nq][HW]                             */
  float* raw; float* masked;   /* [nq][HW] or NULL                 */
  float* sums;             /* [nq][3]                              */
  float scale;
  int32_t B, T, HW, mask_mode, q0, nq;
} pcg_mnist_cf_tail_args;
int pcg_mnist_cf_tail(const pcg_mnist_cf_tail_args* args, pcg_stream_t stream);

/* eval_utils.py:58-64 (evaluate_counterfactuals) and :305-321 (compute_masked_metrics) from the classifier's logits (rows of ld >= K
 * floats, K <= 16 read): max-subtracted softmax; pred = the first maximum (torch.argmax), conf = its probability; p_target =
 * p_cf[target(q)], p_true = p_cf[y_true[b]], p_orig_true = softmax(logits_orig[b])[y_true[b]] (0 without logits_orig), flip =
 * (pred == target).  Every per-query output is optional.  group_sums [T][ceil(B / group_rows)][8], optional: for group (t, j), j =
 * b / group_rows the loader batch, over its rows inside the window in ascending b, by one workgroup:
 *   { sum flip, max flip, sum (p_target - p_true)  [:63-64, both from the counterfactual's softmax],
 *     sum (p_target - p_orig_true)  [:314-316; 0 without logits_orig], the three sums of pcg_mnist_cf_tail (0 without tail_sums), count }
 * Without y_true both gains are 0.  A ragged last batch has its own count. */
#define PCG_MNIST_CF_GROUP_SUMS 8
typedef struct pcg_mnist_cf_score_args {
  const float* logits_cf;     /* [nq][ld]                          */
  const float* logits_orig;   /* [B][ld] or NULL                   */
  const int64_t* target;      /* NULL (sweep) or [B]               */
  const int64_t* y_true;      /* [B] or NULL                       */
  const float* tail_sums;     /* [nq][3] or NULL                   */
  int64_t* pred; float* conf; float* p_target; float* p_true; float* p_orig_true; float* flip;   /* [nq] or NULL */
  float* group_sums;
  int32_t B, T, K, ld, group_rows, q0, nq;
} pcg_mnist_cf_score_args;
int pcg_mnist_cf_score(const pcg_mnist_cf_score_args* args, pcg_stream_t stream);

/* The scalars the tabular trainer logs per step (house_sales_kc_usa/trainer.py:292, :299, :307-312, :318-330) in one launch:
 * out5 = { D_loss = mean(d_fake) - mean(d_real), G_loss = -mean(d_fake_g) + lambda_cls*g_cls + w_reg*am + lambda_mask*pen,
 *          g_adv = -mean(d_fake_g), g_reg = w_reg_log*am, mean(d_fake_g) } — the same reduction trees and fma chains as
 * pcg_mean_fwd + pcg_weighted_sum_fwd (bit-identical values), n <= 16384 critic outputs. */
int pcg_house_losses(const float* d_real, const float* d_fake, const float* d_fake_g, int64_t n, const float* g_cls, const float* am,
                     const float* pen, float lambda_cls, float w_reg, float lambda_mask, float w_reg_log, float* out5, pcg_stream_t stream);

/* The residual block of the tabular step (house_sales_kc_usa/trainer.py:266-287, :305) in one launch each way.
 * Forward: residual_full (as pcg_assemble_residual_fwd), masked = residual_full * mask, x_cf = x + masked, and the penalties
 * pen = mean|residual_full * (1 - mask)|, am = mean|masked| — bit-identical to pcg_assemble_residual_fwd + pcg_scale_mask_fwd +
 * pcg_axpby + 2 x pcg_abs_mean_fwd (same element arithmetic, same partition and trees of the sums).  col_src (HOST int32[D]):
 * >= 0 the index of a continuous column in cont, -(s + 1) categorical head s.  partial512: 512 floats of scratch; ticket: one
 * int32, zero before first use, left zero.
 * Backward: the gradient of  lambda_mask * pen + w_reg * am + <gx_a + gx_b, x_cf>  with respect to (cont, samples) — w_pen =
 * lambda_mask, w_am = lambda_reg * D as the trainer weighs them; gx_a, gx_b: the two addends of dLoss/dx_cf (critic, classifier).
 * Bit-identical to the chain pcg_axpby, pcg_weighted_sum_bwd, 2 x pcg_abs_mean_bwd, pcg_axpby, pcg_scale_mask_bwd, add,
 * pcg_assemble_residual_bwd. */
typedef struct pcg_house_res_fwd_args {
  const float* cont; int32_t ncont;
  const float* samples; const int32_t* seg_dev; int32_t T;
  const float* norm; const float* x; const float* mask;
  const int32_t* col_src;                              /* HOST int32[D] */
  int32_t D, B;
  float* res; float* masked; float* x_cf; float* partial512; int32_t* ticket; float* pen_out; float* am_out;
} pcg_house_res_fwd_args;
typedef struct pcg_house_res_bwd_args {
  const float* res; const float* masked; const float* mask; const float* gx_a; const float* gx_b;
  float w_pen, w_am;
  int32_t ncont; const int32_t* cont_idx_dev; const int32_t* seg_dev; int32_t S, T;
  const int32_t* cat_idx_dev; const float* norm;
  int32_t D, B;
  float* dcont; float* dsamples;
} pcg_house_res_bwd_args;
/* the operands of pcg_house_losses as a rider of the backward: n <= 16384 critic outputs; out6 = the five scalars + g_cls.
 * ce_row_loss != NULL: the [n_ce] row terms the classifier forward's cross-entropy tail left (g_cls may then be NULL). */
typedef struct pcg_house_loss_args {
  const float* d_real; const float* d_fake; const float* d_fake_g; int32_t n;
  const float* g_cls;                                  /* nullable with ce_row_loss */
  const float* am; const float* pen;
  float lambda_cls, w_reg, lambda_mask, w_reg_log;
  const float* ce_row_loss;                            /* nullable */
  int32_t n_ce;
  float* out6;
} pcg_house_loss_args;
/* The four per-iteration diagnostics of house_sales_kc_usa/trainer.py:318-343 in one single-block launch (pcg_house_diag) or as a
 * rider block of pcg_house_residual_bwd:
 *   out4 = { pred_gain, sparsity (|masked residual| > eps), reg_loss_l2, class_flip_rate }
 * logits_orig: the frozen classifier's logits of the ORIGINAL rows (it does not change during GAN training: evaluated once for the
 * training set), gathered through src_rows (nullable: row b).  acc (nullable, double[8]): epoch accumulators —
 * acc[2..5] += out4 (as a rider the launch also adds D_loss, G_loss and the iteration count to acc[0], acc[1], acc[6]),
 * read once per epoch instead of six .item() calls per iteration (trainer.py:327-353). */
typedef struct pcg_house_diag_args {
  const float* logits_cf; const float* logits_orig;
  const int64_t* src_rows;                             /* nullable */
  const int64_t* target_y; const float* masked;
  int32_t B, nc, D;
  float eps;
  float* out4;
  double* acc;                                         /* nullable */
} pcg_house_diag_args;
/* rider (nullable): the critic step's training-mode power iterations (see "Riders" above) */
int pcg_house_residual_fwd(const pcg_house_res_fwd_args* args, const pcg_sn_fwd_batch* rider /*nullable*/, pcg_stream_t stream);
/* losses (nullable): the logged scalars ride in the launch; diag (nullable, only with losses): the diagnostics too (one more block) */
int pcg_house_residual_bwd(const pcg_house_res_bwd_args* args, const pcg_house_loss_args* losses /*nullable*/,
                           const pcg_house_diag_args* diag /*nullable*/, pcg_stream_t stream);
int pcg_house_diag(const pcg_house_diag_args* args, pcg_stream_t stream);
/* The three per-iteration draws of the tabular trainer in one launch — target class != y (trainer.py:248-249, as pcg_randint with
 * exclude), feature mask (:253-255, as pcg_feature_mask), Gumbel noise [B][T] (generator.py:90, as pcg_rand_gumbel) — each from its
 * own counter offset: the values the three separate calls produce.  onehot_target / onehot_y (nullable, [B][num_classes]): the float
 * one-hot rows of the drawn targets and of y (trainer.py:250, :290), written by the same launch. */
int pcg_house_draws(int64_t* target_y, int32_t B, int32_t num_classes, const int64_t* y, uint64_t offset_target, float* mask, int32_t D,
                    const int32_t* zero_cols, int32_t n_zero_cols, uint64_t offset_mask, float* noise, int32_t T, uint64_t offset_noise,
                    uint64_t seed, float* onehot_target, float* onehot_y, pcg_stream_t stream);
/* The same launch with the Philox offsets taken from a DEVICE counter: counter[0] = the running offset (the three draws take
 * consecutive ranges of (B+3)/4, (B*D+3)/4, (B*T+3)/4 counter values from it, as the host-side bookkeeping of the call above hands
 * them out), counter[1] = a ticket (zero before first use, left zero); the launch advances counter[0] itself.  Captured in a HIP
 * graph it draws fresh numbers on every replay — the values successive pcg_house_draws calls would produce. */
int pcg_house_draws_counter(int64_t* target_y, int32_t B, int32_t num_classes, const int64_t* y, float* mask, int32_t D,
                            const int32_t* zero_cols, int32_t n_zero_cols, float* noise, int32_t T, uint64_t seed, float* onehot_target,
                            float* onehot_y, uint64_t* counter, pcg_stream_t stream);
/* pcg_house_draws_counter + the BATCH: the training set X [n_rows][D] / Y [n_rows] and the epoch's permutation perm [n_perm] are
 * resident in HBM; the launch copies rows perm[cursor .. cursor+B) into x_out / y_out (the static inputs of the captured step),
 * writes the source rows to src_out (nullable) and draws target / mask / noise / one-hot rows for them.  counter: uint64[4] =
 * [Philox offset, ticket, row cursor, unused]; the launch advances offset and cursor (+= B) itself, so a replayed graph walks
 * through the epoch with no host-side copy — DataLoader(shuffle=True, drop_last=True) of house_sales_kc_usa/trainer.py:198. */
int pcg_house_batch_draws_counter(int64_t* target_y, int32_t B, int32_t num_classes, const float* X, const int64_t* Y,
                                  const int64_t* perm, int64_t n_perm, int64_t n_rows, float* x_out, int64_t* y_out,
                                  int64_t* src_out /*nullable*/, float* mask, int32_t D, const int32_t* zero_cols, int32_t n_zero_cols,
                                  float* noise, int32_t T, uint64_t seed, float* onehot_target /*nullable*/, float* onehot_y /*nullable*/,
                                  uint64_t* counter, pcg_stream_t stream);

/* ---- classifier pre-training of the tabular pipeline as a replayed step (house_sales_kc_usa/trainer.py:18-180) ----------------------
 * pcg_house_clf_batch: the batch and the forward's three Dropout masks (models/nn_classifier.py:11,16,22) in one launch.  Rows
 * perm[cursor .. cursor+B) of the resident X [n_rows][D] / Y [n_rows] go to x_out [B][D] / y_out [B]; m0 [B][w0], m1 [B][w1], m2 [B][w2]
 * are 0/1 with P(1) = keep0 / keep1 / keep2: exactly what three pcg_rand_bernoulli calls write at offset, offset + (B*w0+3)/4,
 * offset + (B*w0+3)/4 + (B*w1+3)/4.  Refused: cursor + B > n_perm.
 * pcg_house_clf_batch_counter: the same launch with offset and cursor read from a DEVICE counter uint64[4] = [Philox offset, ticket
 * (zero before first use, left zero), row cursor, unused], which the launch advances itself (offset by the three spans, cursor by B):
 * captured in a HIP graph, every replay takes the next rows and the next numbers.  The caller keeps cursor + B <= n_perm (the kernel
 * clamps its reads, it cannot report). */
int pcg_house_clf_batch(const float* X, const int64_t* Y, const int64_t* perm, int64_t n_perm, int64_t n_rows, float* x_out, int64_t* y_out,
                        int32_t B, int32_t D, float* m0, int32_t w0, float keep0, float* m1, int32_t w1, float keep1, float* m2, int32_t w2,
                        float keep2, uint64_t seed, uint64_t offset, int64_t cursor, pcg_stream_t stream);
int pcg_house_clf_batch_counter(const float* X, const int64_t* Y, const int64_t* perm, int64_t n_perm, int64_t n_rows, float* x_out,
                                int64_t* y_out, int32_t B, int32_t D, float* m0, int32_t w0, float keep0, float* m1, int32_t w1, float keep1,
                                float* m2, int32_t w2, float keep2, uint64_t seed, uint64_t* counter, pcg_stream_t stream);
/* The weighted cross-entropy head with its bookkeeping, one launch, one workgroup, fixed summation order.  For each run of `seg`
 * consecutive rows of logits [B][K] (the last run may be shorter; seg >= B: one run) L_s = sum_r w[y_r] nll_r / sum_r w[y_r] -- the
 * value (bit for bit) of pcg_cross_entropy_weighted_fwd_bwd on those rows -- and adds to the device tally double[3]:
 *   tally[0] += sum_s L_s n_s   (trainer.py:89 running_loss += loss.item() * n; :110 over the validation loader's batches)
 *   tally[1] += rows whose argmax equals the target (first maximum: a tie counts for the lower index)
 *   tally[2] += B
 * dlogits (nullable; needs seg >= B, refused otherwise): the gradient of that single mean, as pcg_cross_entropy_weighted_fwd_bwd
 * writes it with grad_scale 1.  dbias (nullable, [K], needs dlogits): the column sums of dlogits, the bias gradient of the Linear that
 * made the logits.  seg_loss (nullable, one float per segment): the L_s themselves. */
int pcg_ce_weighted_tally(const float* logits, const int64_t* target, const float* class_weight, int32_t B, int32_t K, int32_t seg,
                          double* tally /*[3], accumulated*/, float* dlogits /*nullable*/, float* dbias /*nullable*/,
                          float* seg_loss /*nullable*/, pcg_stream_t stream);

/* ---- classifier pre-training of the MNIST CounteRGAN as a replayed step (conditional_counteRGAN/mnist/trainer.py:8-39) ----------------
 * All fp32, fixed summation order, no atomics on floats; every entry may be captured into a HIP graph.
 * pcg_mnist_clf_batch(_counter): pcg_house_clf_batch(_counter) with TWO masks (models/classifier.py:14 Dropout2d [B][128], :20 Dropout
 * [B][256]): rows perm[cursor .. cursor+B) of X [n_rows][D] / Y [n_rows] into x_out [B][D] / y_out [B]; m0 [B][w0], m1 [B][w1] hold what
 * two pcg_rand_bernoulli calls write at offset and offset + (B*w0+3)/4.  Same counter layout, same clamping, same refusals. */
int pcg_mnist_clf_batch(const float* X, const int64_t* Y, const int64_t* perm, int64_t n_perm, int64_t n_rows, float* x_out, int64_t* y_out,
                        int32_t B, int32_t D, float* m0, int32_t w0, float keep0, float* m1, int32_t w1, float keep1, uint64_t seed,
                        uint64_t offset, int64_t cursor, pcg_stream_t stream);
int pcg_mnist_clf_batch_counter(const float* X, const int64_t* Y, const int64_t* perm, int64_t n_perm, int64_t n_rows, float* x_out,
                                int64_t* y_out, int32_t B, int32_t D, float* m0, int32_t w0, float keep0, float* m1, int32_t w1, float keep1,
                                uint64_t seed, uint64_t* counter, pcg_stream_t stream);
/* nn.Dropout2d + nn.Flatten of the NCHW tensor (models/classifier.py:14,17) from the NHWC activation a [R][HW][C] in one launch:
 * out[b][c*HW + p] = a[b][p][c] * mask[b][c] * scale -- bit for bit pcg_dropout_apply(inner = HW) followed by pcg_nhwc_to_nchw_flat. */
int pcg_drop2d_flatten_fwd(const float* a, const float* mask /*[R][C]*/, float scale, int32_t R, int32_t HW, int32_t C, float* out,
                           pcg_stream_t stream);
/* Its backward with the derivative of the activation whose output y [R][HW][C] was saved (classifier.py:13):
 * out[b][p][c] = dflat[b][c*HW + p] * mask[b][c] * scale * act'(y[b][p][c]) -- bit for bit pcg_nhwc_to_nchw_flat(inverse),
 * pcg_dropout_apply, pcg_act_bwd. */
int pcg_drop2d_flatten_bwd(const float* dflat, const float* mask, float scale, const float* y, int act, float slope, int32_t R, int32_t HW,
                           int32_t C, float* out, pcg_stream_t stream);
/* Everything above fc1's output (classifier.py:19-21, trainer.py:10,19-20) in one launch of one workgroup; R <= 128, I == 256, K <= 16.
 * h [R][I] is fc1's post-ReLU output, m1 [R][I] the Dropout mask.  logits [R][K] = (h * m1 * scale) W2^T + b2; loss [1] the mean
 * cross-entropy; tally double[3] += (loss * R, rows whose argmax is the label -- first maximum, as pcg_ce_weighted_tally --, R);
 * dW2 [K][I], db2 [K]; dh [R][I] = (dlogits W2) * m1 * scale * [h > 0] with dlogits = (softmax - onehot) / R; db1 [I] its column sums. */
int pcg_mnist_clf_head(const float* h, const float* m1, float scale, const float* W2, const float* b2, const int64_t* y, int32_t R, int32_t I,
                       int32_t K, float* logits, float* loss, double* tally /*[3], accumulated*/, float* dW2, float* db2, float* dh, float* db1,
                       pcg_stream_t stream);

/* A barrier of the ranks on the library's own communicator (a 4-byte all-reduce in stream order; synchronise `stream` afterwards):
 * bench.py brackets its timed region with it, so that region uses ONE communicator — the one that carries the gradient exchange.
 * pcg_dp_rccl_version: ncclGetVersion of the RCCL the library bound (22105 = 2.21.5; 0 = unknown).                              */
int pcg_dp_barrier(pcg_stream_t stream);
int32_t pcg_dp_rccl_version(void);

/* ---- data-parallel exchange (RCCL over xGMI) --------------------------------------------------------------------------------
 * The reference is single-process (mnist_dcgan.py:140-175, mnist/trainer.py:89-123); data-parallel replicas add ONE exchange per
 * optimizer step: the average of the net's flat fp32 gradient bucket.  The library owns the RCCL communicator (bound at run time,
 * no link-time dependency), a side HIP stream and the ordering events.  Bootstrap: rank 0 makes an id (pcg_dp_unique_id), the
 * host layer ships the 128 bytes to the other ranks by any means (the Python layer: torch.distributed's store), every rank calls
 * pcg_dp_init on ITS GPU (the current HIP device).  None of these calls may be captured in a HIP graph: the step is captured as
 * graph segments cut at the exchange points (nn.GraphedStep).
 *   pcg_dp_allreduce          buf <- mean over ranks, in stream order on `stream`
 *   pcg_dp_allreduce_begin    the same on the library's side stream, after everything queued on producer_stream so far;
 *                             `slot` (0..7) names the reduction
 *   pcg_dp_side_stream        that stream: the caller may queue work behind the reduction (Adam), then pcg_dp_record(slot)
 *   pcg_dp_allreduce_wait     consumer_stream waits on the GPU for slot (the reduction and whatever pcg_dp_record covered)
 *   pcg_dp_allreduce_sum_f64  sum of doubles in stream order (exact-BatchNorm statistic sums, 2*C values per layer)
 *   pcg_dp_broadcast          bytes from rank `root` (initial weights, BatchNorm buffers)
 *   pcg_dp_sync_batchnorm     exact global-batch BatchNorm (SURVEY.md §8e option ii; the reference's BatchNorm spans the whole batch,
 *                             mnist_dcgan.py:77-87): while enabled, every BatchNorm-family entry point (pcg_bn_train_stats*,
 *                             pcg_conv2d_*_bn*, pcg_bn_act_bwd*, pcg_bn_bwd_partial) sums its per-channel partial rows locally in
 *                             the usual fixed order, all-reduces the 2*C fp64 sums (sum x, sum x^2 | sum dy, sum dy*xhat) over the
 *                             ranks in stream order, and finalises with rows*world rows — N ranks x B/N images compute what one
 *                             process computes on B (equal shards assumed).  dgamma / dbeta stay local sums (they are averaged with
 *                             the gradient bucket).  These calls then contain an RCCL collective: do not capture them in a graph. */
#define PCG_DP_UNIQUE_ID_BYTES 128
int pcg_dp_unique_id(void* id_out /*[PCG_DP_UNIQUE_ID_BYTES]*/);
int pcg_dp_init(const void* id /*[PCG_DP_UNIQUE_ID_BYTES]*/, int32_t rank, int32_t world);
int32_t pcg_dp_world(void);   /* 0 before pcg_dp_init */
int32_t pcg_dp_rank(void);
pcg_stream_t pcg_dp_side_stream(void);
int pcg_dp_allreduce(float* buf, int64_t n, pcg_stream_t stream);
int pcg_dp_allreduce_begin(float* buf, int64_t n, int32_t slot, pcg_stream_t producer_stream);
int pcg_dp_record(int32_t slot);
int pcg_dp_allreduce_wait(int32_t slot, pcg_stream_t consumer_stream);
int pcg_dp_allreduce_sum_f64(double* buf, int64_t n, pcg_stream_t stream);
int pcg_dp_broadcast(void* buf, int64_t nbytes, int32_t root, pcg_stream_t stream);
int pcg_dp_sync_batchnorm(int32_t enable);
int pcg_dp_shutdown(void);

/* ---- tuning switches (diagnostics): A/B of launch-planning choices inside ONE process, e.g. scripts/conv_microbench.py --ab.
 *   "korder"            order of the k-tiles of the forward / grad-input kernels: 0 (tap, channel chunk), 1 L2-friendly (default)
 *   "wgrad_order"       weight-gradient block order: 0 tile-major, 1 slice-major, -1 built-in rule
 *   "dgrad_interleave"  sub-pixel phases of a grad-input tile neighbours in launch order: 0 / 1, -1 built-in rule
 *   "stream_k"          hybrid stream-K launches: 0 off, 1 where the launch plan's model gains > 10 % (default), 2 wherever valid
 *   "sk_blocks"         number of stream-K workgroups (512 / 256 / 128 / 64), -1 built-in choice
 *   "dgrad_gemm"        grad-input of a kernel size that is not a multiple of the stride: 0 sub-pixel-phase kernel, 1 one GEMM +
 *                       col2im, -1 whichever has fewer multiply-adds for the geometry (built-in)
 *   "t64"               forward launches with at most 256 tiles of 128x128: 64x128 tiles instead (default 1), 0 keeps 128x128
 *   "fwd_splits"        forward K-slices
 *   "wgrad_pixtab"      weight-gradient x gather: 1 pixels from the geometry's registered descriptor table (default), 0 derived per
 *                       k-tile (the environment variable PCG_WGRAD_PIXTAB=0 does the same for a whole process)
 *   "pad_clip"          k4 s2 p1 forward / grad-input launches: 0 today's kernels, 1 position-major tiles that skip their all-padding
 *                       taps where the schedule model predicts >= 5 % (pcg_conv_pad_clip_query); 2 / 3 / 4 (measurements) every
 *                       eligible launch, tiles long first / short first / in pairs.  PCG_PAD_CLIP=v for a whole process.
 *   "pad_clip_dgrad"    what "pad_clip" 1 does with grad-input launches: 1 (default) those the schedule model predicts no loss for,
 *                       its measured unit cost included, from one round of 512 workgroups up; 0 none (forward-kernel launches
 *                       only); 2 (measurements) every eligible one; other values are refused.  PCG_PAD_CLIP_DGRAD=v for a whole process.
 *   "wgrad_padskip"     fp32 weight gradients of k4 s2 p1 layers (pcg_conv_wgrad_padskip_query): 0 today's launches; 1 the consumer
 *                       waves leave out the MFMAs whose x operand is all padding — same products otherwise, in the same order, so
 *                       the result is bit-identical for finite dy (a non-finite dy at a padded position gives NaN under 0 and is
 *                       ignored under 1), with the blocks ordered so that a skipping tile shares its CU with a full one, for the
 *                       layer classes that measured a gain (OW = 4 and 8; default); 2 / 3 (measurements) every eligible launch, in
 *                       that paired order / in today's order; other values are refused.  PCG_WGRAD_PADSKIP=v for a whole process (a value
 *                       outside 0 .. 3 there means the default).
 * value -1 restores the built-in choice.  Results stay correct under every setting (the order of a sum changes, not its terms). */
int pcg_tune_set(const char* name, int32_t value);

/* ---- scratch of the hybrid stream-K launches (conv_igemm.hip: conv_fwd_sk_kernel / conv_dgrad_sk_kernel) --------------------------
 * A forward / grad-input launch whose tile count is not a multiple of the chip's 512 workgroup slots gives its remainder tiles to
 * workgroups that each take an equal share of those tiles' K loop; they exchange partial accumulator tiles through `parts` and
 * count arrivals per tile in `arrivals`.  Both buffers are the caller's, registered for ONE stream (launches on that stream use
 * them in stream order; two graphs that bake the same scratch must not replay concurrently).  `arrivals` must be zero when it is
 * registered; the kernels leave it zero.  A stream without scratch runs the plain launches (same results up to the order of the
 * K sum).  parts == NULL forgets the stream.  The reference has no counterpart: ATen picks its conv algorithm inside
 * torch.nn.functional.conv2d (mnist_wgan_conditional.py:61-70,87-95).                                                          */
/* Which launch form a convolution takes, as text ("128x128 tiles: 512", "64x128 tiles: 512", "stream-K: 512 whole tiles + 352 tiles x
 * 72 k-tiles over 512 ranges", "GEMM + col2im: ...", "4 phases: stream-K over unequal phases: ..."): the host-side launch planning,
 * no device needed.  op: 0 forward, 1 grad-input, 2 grad-weight; assume_scratch != 0: plan as if the stream had stream-K scratch. */
int pcg_conv_plan_describe(const pcg_conv_geom* g, int32_t op, int32_t assume_scratch, char* out, size_t out_bytes);
/* Which route a non-convolution launch takes, as text — the host-side switches of csrc/tabular.hip, cf_ops.hip and pointwise.hip,
 * evaluated by the predicates the launchers themselves call; no device needed.  args holds n_args integers:
 *   PCG_PLAN_GEMM_ACT, PCG_PLAN_GEMM  (transA, transB, M, N, K)   "rowdot<4>: 129 blocks" | "skinny: 33 blocks, two columns per thread,
 *                                      62784 bytes of LDS" | "64x64 tiles: 1 x 8" (grid x, y).  pcg_gemm has no skinny launch.
 *   PCG_PLAN_LINEAR_WGRAD             (B, O, I)                   "64x64 tiles: 1, slabs: 2 of 64 rows"
 *   PCG_PLAN_LINEAR_WGRAD_GROUPED     (B)                         "blocks per tile: 2, rows per wave: 64"
 *   PCG_PLAN_MEAN, PCG_PLAN_ABS_MEAN  (n)                         "one block of 1024" | "64 partials + finish" (256 for abs_mean)
 *   PCG_PLAN_CROSS_ENTROPY            (B, K, logits 16-byte aligned, dlogits absent or 16-byte aligned)
 *                                                                 "256 threads, float4 rows" | "1024 threads, no float4 rows" | ...
 *   PCG_PLAN_EMBED_CONCAT_BWD         (B, has_dtable, has_dx)     "batch-split table gradient + copy" | "batch-split table gradient" |
 *                                                                 "one pass"
 *   PCG_PLAN_ACT                      (n, every pointer 16-byte aligned)   pcg_act_fwd / pcg_act_bwd:
 *                                                                 "float4 lanes: 8192 blocks of 256: 2 passes" | "scalar lanes: ..."
 *   PCG_PLAN_ELEMENTWISE              (family, n work items)      the grid-stride launch of one thread per item, "4096 blocks of 256:
 *                                      2 passes"; family: PCG_PLAN_EW_TABULAR (tabular.hip), PCG_PLAN_EW_CF_OPS (cf_ops.hip),
 *                                      PCG_PLAN_EW_POINTWISE (pcg_add_bias_rows), PCG_PLAN_EW_GATHER_CHANNEL (pcg_gather_channel)
 *   PCG_PLAN_ADAM                     (n, every pointer 16-byte aligned, capturable)   pcg_adam_step (capturable 0) /
 *                                      pcg_adam_step_capturable (1, at most 256 blocks: PCG_ADAM_TICK_BLOCKS, at least 1, for the
 *                                      float4 lanes): "float4 lanes: 256 blocks of 256: 2 passes, tail of 3" (the 1..3 elements behind
 *                                      the 16-byte lanes, on block 0) | "scalar lanes: 256 blocks of 256: 3 passes"
 * The normalisation layer (csrc/batchnorm.hip, instnorm.hip, spectral_norm_body.h); "aligned": every tensor pointer of the call is
 * 16-byte aligned:
 *   PCG_PLAN_BN_COLREDUCE             (rows, C, aligned)          the column reduction of pcg_bn_train_stats / pcg_bn_act_bwd* / pcg_colsum:
 *                                                                 "float4: 8 x 32 threads, 2 channel passes, 8 blocks of 128 rows" |
 *                                                                 "scalar: ..." (threads: channel groups x row lanes)
 *   PCG_PLAN_BN_APPLY                 (pass, rows, C, aligned)    pass 0 pcg_bn_apply_act, 1 the apply of pcg_bn_act_bwd* / pcg_bn_bwd_partial,
 *                                                                 2 the same with fused column sums (dcol):
 *                                                                 "fast<2>: 500 blocks, temporal stores, thread 0: 0 main trips + tail of 1"
 *                                                                 (<loads in flight>; "non-temporal stores"; the trips of the grid-stride
 *                                                                 loop as thread 0 walks it) | "float4 lanes: 9 blocks of 256: 1 pass" |
 *                                                                 "scalar lanes: ..."; reads PCG_BN_DEPTH / PCG_BN_NT / PCG_BN_BLOCKS
 *   PCG_PLAN_BN_FINALIZE              (nparts)                    the finalize over nparts partial rows: "256 threads, 1 eight-deep trip" |
 *                                                                 "1024 threads, 0 eight-deep trips" | "presum: 228 chunks of 9 rows, 256
 *                                                                 threads, 1 eight-deep trip" (the two-level form of pcg_bn_bwd_partial* and
 *                                                                 the conv epilogues' statistics; trips of slice 0 through the batched loop)
 *   PCG_PLAN_INSTNORM                 (pass, B, HW, C, aligned)   pass 0 pcg_instnorm_fwd, 1 pcg_instnorm_bwd*, 2 pcg_instnorm_bwd_bwd*:
 *                                                                 "reg<6>: 32 channels x 32 lanes, grid 2 x 2" | "stream<4>: ..." |
 *                                                                 "stream<1>: ..." (channels per block x position-lanes, grid B x blocks)
 *   PCG_PLAN_SPECTRAL_NORM            (pass, O, I)                pass 0 forward: "LDS image: 12192 of 12288 floats, row stride 127" |
 *                                                                 "global memory: 12384 floats exceed 12288, row stride 129"; pass 1
 *                                                                 backward (pcg_spectral_norm_bwd*): "one burst: 8192 of 8192 elements" |
 *                                                                 "loops: 8320 elements exceed 8192"  */
enum { PCG_PLAN_GEMM_ACT = 0, PCG_PLAN_GEMM = 1, PCG_PLAN_LINEAR_WGRAD = 2, PCG_PLAN_LINEAR_WGRAD_GROUPED = 3, PCG_PLAN_MEAN = 4,
       PCG_PLAN_ABS_MEAN = 5, PCG_PLAN_CROSS_ENTROPY = 6, PCG_PLAN_EMBED_CONCAT_BWD = 7, PCG_PLAN_ACT = 8, PCG_PLAN_ELEMENTWISE = 9,
       PCG_PLAN_BN_COLREDUCE = 10, PCG_PLAN_BN_APPLY = 11, PCG_PLAN_BN_FINALIZE = 12, PCG_PLAN_INSTNORM = 13, PCG_PLAN_SPECTRAL_NORM = 14,
       PCG_PLAN_ADAM = 15 };
enum { PCG_PLAN_EW_TABULAR = 0, PCG_PLAN_EW_CF_OPS = 1, PCG_PLAN_EW_POINTWISE = 2, PCG_PLAN_EW_GATHER_CHANNEL = 3 };
int pcg_launch_plan_describe(int32_t op, const int64_t* args, int32_t n_args, char* out, size_t out_bytes);
size_t pcg_conv_scratch_parts_bytes(void);
size_t pcg_conv_scratch_arrivals_bytes(void);
int pcg_conv_set_scratch(pcg_stream_t stream, void* parts, size_t parts_bytes, void* arrivals, size_t arrivals_bytes);
/* Zero-fill the arrival counters of `stream`'s scratch in stream order — after a launch on that stream failed or was aborted (the
 * kernels leave the counters zero only when every range of a launch ran).  The registry is keyed by (current device, stream): the
 * default stream has the same handle on every device.  No-op for a stream without scratch.                                      */
int pcg_conv_reset_scratch(pcg_stream_t stream);
/* ---- pixel descriptor table of a convolution geometry (csrc/conv_pixtab.h) ------------------------------------------------------------
 * The weight gradient contracts over output pixels; where the x gather of pixel (oh, ow) starts and which taps fall inside the input
 * depends on (IH, IW, OH, OW, stride, pad, KH, KW, Cin) only — not on B, Cout, the data or the weights.  The table holds, per output
 * pixel of ONE image, {int32 byte offset of input pixel (oh*stride - pad, ow*stride - pad) inside the image (may be negative), uint32
 * mask with bit kh*KW + kw set for every tap inside the input}, followed by 7 entries that continue into the next images (a wave reads
 * the descriptors of 8 consecutive pixels as one run).  pcg_conv_pixtab_bytes: size of the table.  pcg_conv_pixtab_register:
 *   host_out != NULL      fill host_out (`bytes` >= the size) on the host — plain C++, no device needed;
 *   device_table != NULL  remember device_table as THE table of this geometry on the current device: the caller has copied the
 *                         built table there, owns the memory and keeps it alive and unchanged while it is registered;
 *   both NULL             forget the geometry.
 * No allocation, copy or synchronisation happens inside.  Weight-gradient launches of a registered geometry read their pixels from
 * the table (pcg_tune_set("wgrad_pixtab", 0) keeps the loaders that derive them per k-tile); a geometry without a table runs those
 * loaders.  Results are bit-identical either way.  The reference has no counterpart (ATen's conv backward, mnist_dcgan.py:153-173). */
size_t pcg_conv_pixtab_bytes(const pcg_conv_geom* g);
int pcg_conv_pixtab_register(const pcg_conv_geom* g, void* host_out, size_t bytes, const void* device_table);
/* ---- tile descriptor table of a k4 s2 p1 geometry (csrc/conv_cliptab.h) -------------------------------------------------------------
 * Zero padding is gathered as zeros and multiplied like any other tap.  A tile whose rows are ONE output pixel (forward form) or ONE
 * pixel of a sub-pixel phase grid (grad-input form) of different images has the same padded taps in every row and can leave them
 * out.  The table holds, for the forward form and each of the four grad-input phases, one 32-bit descriptor per position — position,
 * first valid tap and tap count per axis — sorted by tap count, largest first; it depends on (OH, OW) only (IH = 2 OH, IW = 2 OW).
 * pcg_conv_cliptab_bytes: its size, 0 for a geometry that has none.  pcg_conv_cliptab_register: the contract of
 * pcg_conv_pixtab_register (host_out: build on the host; device_table: remember the caller's device copy; both NULL: forget).
 * An eligible launch — fp32 MFMA path, batch and each BatchNorm group's share of it whole tiles, no K-slices, no stream-K — of a
 * registered geometry takes the clipped kernels where the schedule model predicts at least 5 % (forward kernel) or no loss (grad-input
 * kernel, launches of at least 512 workgroups; pcg_tune_set("pad_clip_dgrad", 0): none) — pcg_tune_set("pad_clip", 0): never.
 * Convolution outputs are bit-identical; fused BatchNorm sums regroup their fp64 partial rows.
 * pcg_conv_sched_model: the model — time in us at which the last of n workgroups ends that are dispatched in order onto 256 CUs x 2
 * slots and run ktiles[i] k-tiles each, at 3.5 us per k-tile beside a busy neighbour slot and 2.2 us alone.
 * pcg_conv_pad_clip_query: what a launch of `g` would do.  op 0: forward kernel, 1: grad-input kernel; groups: BatchNorm groups along
 * the batch; assume_scratch: plan as for a stream with stream-K scratch.  *taken 1: the clipped path (also needs the table on the
 * current device); *order 0 long tiles first, 1 short first, 2 pairs; *tile_rows 128 / 64; *predicted: model time, clipped / today's
 * (1.0 for a launch that is not eligible).  Outputs may be NULL.                                                                  */
size_t pcg_conv_cliptab_bytes(const pcg_conv_geom* g);
int pcg_conv_cliptab_register(const pcg_conv_geom* g, void* host_out, size_t bytes, const void* device_table);
double pcg_conv_sched_model(const int32_t* ktiles, int32_t n);
int pcg_conv_pad_clip_query(const pcg_conv_geom* g, int32_t op, int32_t groups, int32_t assume_scratch, int32_t* taken, int32_t* order,
                            int32_t* tile_rows, double* predicted);
/* The padding skip of the weight gradients (pcg_tune_set "wgrad_padskip"): plain host code, no device.  *applies 1 for op 2 (grad-weight)
 * in fp32 operand precision on a k4 s2 p1 geometry with IH = 2 OH, IW = 2 OW, OH and OW powers of two >= 4 and Cin a multiple of 64, else
 * 0 (ops 0 and 1, the bf16 mode and every other geometry launch what they always did); *fraction: the share of the launch's MFMAs left
 * out — 1/8 for OW = 4 (one MFMA in four for the taps kw = 0 and 3), 1 / (2 OH) for OW >= 8 (one k-group in OH for kh = 0 and 3) —
 * or 0.  The switch itself is not consulted.  Outputs may be NULL.                                                                 */
int pcg_conv_wgrad_padskip_query(const pcg_conv_geom* g, int32_t op, int32_t* applies, double* fraction);
/* What a plain fp32 weight-gradient launch of `g` does under the current switches, decided as pcg_conv2d_wgrad decides it (host code,
 * no device): *mode 0 today's kernel, 1 the skipping consumers in today's block order, 2 in the paired order; *pair_bit: the bit m of
 * the paired order (blocks b of every odd round of 256 work as block b ^ m), 0 where the order stays as it is.  assume_scratch as in
 * pcg_conv_plan_describe.  Outputs may be NULL.                                                                                  */
int pcg_conv_wgrad_padskip_plan(const pcg_conv_geom* g, int32_t assume_scratch, int32_t* mode, int32_t* pair_bit);
/* Diagnostic builds only (`make -C csrc stamp`, -DPCG_CLOCK_STAMP): every conv kernel block leaves {shader-clock ticks, 100 MHz
 * ticks} of its main loop at buf[2*block], buf[2*block+1] (uint64) — the clock the chip holds inside the kernel.  Returns 1 when
 * this build stamps, 0 for the shipped library (which compiles no stamp code).  buf = NULL turns it off.                        */
int pcg_debug_stamp_buffer(void* buf, int64_t bytes);

/* ---- moons CounteRGAN (conditional_counteRGAN/moons): whole training iterations in one launch, one workgroup ------------------
 * The three nets — ResidualGenerator (models/generator.py:4-24: Linear-BN1d-ReLU x3, Linear), the spectral-norm Discriminator
 * (models/discriminator.py:6-22: four SN Linears, LeakyReLU 0.2) and the frozen NNClassifier (models/nn_classifier.py:3-15) — at
 * input_dim 2, 3 classes, hidden 32 or 64 (classifier hidden 32), batch 2..512.  Parameters live in the modules' flat buffers; the
 * offsets (floats) of every tensor inside them are in the descriptor:
 *   g_off: net.0.weight/bias, net.1.weight/bias, net.3.*, net.4.*, net.6.*, net.7.*, net.9.weight/bias      (14)
 *   d_off: net.{0,2,4,6}.weight_orig, then net.{0,2,4,6}.bias                                             (8)
 *   c_off: net.{0,2,4}.weight/bias                                                                       (6)
 * Adam runs over the first nG_adam / nD_adam floats of the flat buffers (the optimizer's one segment), with the arithmetic of
 * pcg_adam_step_capturable (betas, eps, lr; weight decay 0) and its device step counter, advanced by one per iteration.   */
typedef struct pcg_moons_cf_desc {
  int32_t hidden, clf_hidden, B, N;        /* hidden 32 | 64, clf_hidden 32, batch 2..512, training rows            */
  int32_t nG, nD, nC, nG_adam, nD_adam;    /* flat lengths (floats) and the Adam spans                             */
  int32_t g_off[14], d_off[8], c_off[6];
  double lr_G, lr_D, beta1, beta2, adam_eps;
  float bn_eps, bn_momentum, sn_eps, slope;
  float lambda_cls, lambda_l1, lambda_l2, lambda_mask;
} pcg_moons_cf_desc;

/* State of one model (every pointer per model, so that several models can later be strided one per workgroup). */
typedef struct pcg_moons_cf_train_args {
  const float* X; const int64_t* Y;        /* the training set in HBM: [N][2], [N]                                 */
  const int64_t* rows;                     /* [n_steps][B] row indices into X / Y (the DataLoader's order)          */
  const int64_t* target_y;                 /* [n_steps][B] trainer.py:64-65                                         */
  const float* mask;                       /* [n_steps][B][2] trainer.py:69                                         */
  float* g_flat; float* d_flat; const float* c_flat;
  float* g_exp_avg; float* g_exp_avg_sq; int64_t* g_step;
  float* d_exp_avg; float* d_exp_avg_sq; int64_t* d_step;
  float* bn_mean[3]; float* bn_var[3]; int64_t* bn_nbt[3];
  float* sn_u[4]; float* sn_v[4];
  float* logs;                             /* [n_steps][9]: D_loss, G_loss, mean sigmoid(D_real), mean sigmoid(D_fake),
                                              g_adv, g_cls, reg_l1, reg_l2, mask_pen (trainer.py:101-113)               */
  float* scratch; size_t scratch_bytes;    /* activations that do not fit in LDS (pcg_moons_cf_scratch_bytes)       */
} pcg_moons_cf_train_args;

/* Bytes of global activation scratch a train / forward launch with this descriptor needs (0: the train step keeps them in LDS). */
size_t pcg_moons_cf_scratch_bytes(const pcg_moons_cf_desc* desc, int32_t forward);
/* n_steps consecutive iterations of train_countergan's batch loop (trainer.py:58-113) in ONE launch of one workgroup: batch gather,
 * G forward in training mode (BatchNorm batch statistics, running statistics updated, momentum, unbiased variance, +1 batch),
 * critic step (D(real), D(fake) with one power iteration each, D_loss = -mean D_real + mean D_fake, backward through both passes and
 * through sigma, Adam D), generator step (a third power iteration, frozen classifier, G_loss with the four regularisers, backward
 * to G, Adam G), the nine logged scalars.  Weights, moments and buffers are read once and written once per launch.          */
int pcg_moons_cf_train_steps(const pcg_moons_cf_desc* desc, const pcg_moons_cf_train_args* args, int32_t n_steps, pcg_stream_t stream);

/* Forward of one net, one workgroup: which = 0 generator (models/generator.py:20-24; out0 = raw_residual, out1 = masked_residual;
 * train: batch statistics and running-statistics update, else running statistics), 1 critic (discriminator.py:20-22; train: one
 * power iteration that updates u / v, else sigma from the stored u / v; out0 [B][1]), 2 classifier (nn_classifier.py:14-15;
 * out0 = logits [B][3]).  onehot [B][3] for 0 and 1, mask [B][2] for 0.  params = the net's flat buffer.                  */
typedef struct pcg_moons_cf_fwd_args {
  int32_t which, train, B;
  const float* x; const float* onehot; const float* mask;
  float* params;
  float* bn_mean[3]; float* bn_var[3]; int64_t* bn_nbt[3];
  float* sn_u[4]; float* sn_v[4];
  float* out0; float* out1;
  float* scratch; size_t scratch_bytes;
} pcg_moons_cf_fwd_args;
int pcg_moons_cf_forward(const pcg_moons_cf_desc* desc, const pcg_moons_cf_fwd_args* args, pcg_stream_t stream);

/* Counterfactual queries and evaluation of the trained moons CounteRGAN in ONE launch over many workgroups (csrc/moons_cf_eval.hip):
 * eval_utils.py:29-106 (compute_metrics_per_target: every mask, every target class, every loader batch), :114-124 / :196-206 (the
 * decision grid) and gradio_app.py:79-95 (one point, one target, one mask).  Both nets in eval mode (BatchNorm: the running
 * statistics), so rows are independent; nothing of the nets is written.  Of the descriptor hidden, clf_hidden, nG, nC, g_off, c_off
 * and bn_eps are read (B is not).  One work item is (mask slot m, target slot t, row i):
 *   h = [x_i, onehot(t), mask]; raw = G(h); masked = raw * mask; x_cf = x_i + masked (no clamp, eval_utils.py:79);
 *   logits_cf = C(x_cf), logits_x = C(x_i); gain = softmax(logits_cf)[t] - softmax(logits_x)[t]; pred = argmax (first maximum).
 * Forms:  sweep    masks [M][2], targets 0..T-1 (T <= 3), every row: grid = ceil(N / group) x T x M workgroups
 *         per row  target [N] (int64, values in [0, 3)) and row_mask [N][2]; masks NULL, M = T = 1
 *         classifier only  g_flat NULL: logits_x / pred_x of N rows (M = T = 1, every other output NULL)
 * `group` is the loader's batch_size (eval_utils.py:40), 1 <= group <= 2^24: one workgroup owns the rows [g group, (g+1) group).
 * Every per-row output is optional (NULL: not written).  sums [M][T][n_groups][4], n_groups = ceil(N / group), optional: over the
 * group's included rows — y NULL or y[i] != t (eval_utils.py:57) — their count, the count with pred_cf == t, the sum of gain and
 * the sum of |masked| over both features; fixed summation order, no atomics: bitwise repeatable.                              */
typedef struct pcg_moons_cf_eval_args {
  int64_t N; int32_t M, T, group;
  const float* x; const int64_t* y;        /* [N][2]; [N] or NULL                                                    */
  const float* masks;                      /* sweep: [M][2]                                                          */
  const int64_t* target; const float* row_mask;   /* per row: [N], [N][2]                                             */
  const float* g_flat; const float* c_flat;
  const float* bn_mean[3]; const float* bn_var[3];
  float* raw; float* masked; float* x_cf;  /* [M][T][N][2]                                                           */
  float* logits_cf; float* logits_x;       /* [M][T][N][3]; [N][3]                                                   */
  int64_t* pred_cf; int64_t* pred_x;       /* [M][T][N]; [N]                                                         */
  float* gain;                             /* [M][T][N]                                                              */
  float* sums;                             /* [M][T][n_groups][4]                                                    */
} pcg_moons_cf_eval_args;
int pcg_moons_cf_eval(const pcg_moons_cf_desc* desc, const pcg_moons_cf_eval_args* args, pcg_stream_t stream);

/* ---- whole-batch dense layers: nn.Linear (+ nn.BatchNorm1d) (+ activation) for at most 128 rows (csrc/dense_rows.hip) ----------
 * The MLP GAN of simple_gan/mnist/mnist_gan.py (Generator :44-59, Discriminator :70-77) at batch 64: every operand is dense row-major
 * fp32, activations [R][features], weights [out][in] as nn.Linear stores them, 1 <= R <= 128.  One workgroup owns ALL rows of 16
 * output columns, so BatchNorm1d's batch statistics are complete inside it: no partials, no finalize launch, no second pass.
 * fp32 on v_mfma_f32_16x16x4_f32, fixed summation order (bitwise repeatable).  No workspace.  Refused with PCG_ERR_INVALID and a
 * pcg_last_error text: R outside 1..128, R < 2 with training-mode BatchNorm (forward or backward), in_features % 4 != 0 in the
 * forward, x / W not 16-byte aligned in the forward, an unknown activation.
 *
 *   pcg_dense_rows_fwd    y[R][O] = act(BN(x[R][I] W^T + bias))            replaces nn.Linear + nn.BatchNorm1d(O, 0.8) + nn.LeakyReLU /
 *                         nn.Tanh / nn.Sigmoid (mnist_gan.py:46-58,71-76).  bn NULL: no BatchNorm.  bn->training: normalise with the batch
 *                         mean and biased variance, write save_mean / save_invstd [O] and (nullable) xhat [R][O] for the backward, update
 *                         running_mean / running_var (momentum, unbiased variance; nullable) and num_batches_tracked (int64, nullable) in
 *                         the same launch.  Evaluation mode normalises with the running statistics.  bias nullable.
 *   pcg_dense_rows_dgrad  g = (dz[R][O] W) * act'(y_below), then, with bn, the BatchNorm backward of the layer below:
 *                         dbeta (+)= sum_r g, dgamma (+)= sum_r g xhat, dx = gamma invstd (g - mean_r g - xhat mean_r(g xhat)); without
 *                         bn dx = g; below_act PCG_ACT_NONE and bn NULL: plain dx = dz W (the image gradient, mnist_gan.py:126 through D).
 *                         act' is taken from the layer's OUTPUT y_below[R][I] (LeakyReLU: its sign).
 *   pcg_dense_rows_wgrad  dW[O][I] (+)= dz^T x, db[O] (+)= column sums of dz (db nullable); one workgroup per 64x64 tile of dW reduces
 *                         over all rows: no slab split, no tickets.  Writes straight into the flat gradient buffer (mnist_gan.py:126,133). */
typedef struct {
  const float* gamma;            /* [O] */
  const float* beta;             /* [O] */
  float* running_mean;           /* [O]; training: nullable */
  float* running_var;            /* [O]; training: nullable */
  int64_t* num_batches_tracked;  /* one element; nullable */
  float* save_mean;              /* [O], written in training mode */
  float* save_invstd;            /* [O], written in training mode */
  float* xhat;                   /* [R][O] normalised pre-activation, nullable */
  float eps;                     /* the reference passes 0.8 (mnist_gan.py:48 puts it in the eps slot) */
  float momentum;
  int32_t training;
} pcg_dense_bn;
typedef struct {
  const float* xhat;    /* [R][I] as the forward saved it */
  const float* gamma;   /* [I] */
  const float* invstd;  /* [I] */
  float* dgamma;        /* [I] */
  float* dbeta;         /* [I] */
  int32_t accumulate;   /* add to dgamma / dbeta instead of overwriting */
} pcg_dense_bn_bwd;
int pcg_dense_rows_fwd(const float* x, const float* W, const float* bias /*nullable*/, int32_t R, int32_t I, int32_t O,
                       const pcg_dense_bn* bn /*nullable*/, int act, float slope, float* y, pcg_stream_t stream);
int pcg_dense_rows_dgrad(const float* dz, const float* W, int32_t R, int32_t O, int32_t I, int below_act, float below_slope,
                         const float* y_below /*nullable with PCG_ACT_NONE*/, const pcg_dense_bn_bwd* bn /*nullable*/, float* dx,
                         pcg_stream_t stream);
int pcg_dense_rows_wgrad(const float* dz, const float* x, int32_t R, int32_t O, int32_t I, float* dW, float* db /*nullable*/,
                         int accumulate, pcg_stream_t stream);
/* The post-activation stage Linear -> activation -> BatchNorm1d (batch statistics) -> Dropout of the tabular classifier in training mode
 * (house_sales_kc_usa/models/nn_classifier.py:8-25), same workgroup shape and summation order as the two kernels above; training mode
 * only (evaluation folds the BatchNorm into the next Linear).  2 <= R <= 128; act: PCG_ACT_NONE or PCG_ACT_LRELU; anything else, or a
 * null a / save_mean / save_invstd (forward), a / mean / invstd / gamma / dgamma / dbeta (backward), is refused with PCG_ERR_INVALID.
 *   pcg_dense_rows_fwd_post    a = act(x W^T + bias) is written to a[R][O], the ONLY saved activation; mean and biased variance of a per
 *                              column -> save_mean / save_invstd, running statistics (momentum, unbiased variance; nullable) and
 *                              num_batches_tracked (nullable) as pcg_dense_rows_fwd updates them; xhat = (a - mean) invstd;
 *                              y = (gamma xhat + beta) * mask * scale with mask[R][O] of 0/1 (nullable: no Dropout), scale = 1/(1-p).
 *                              in_features % 4 != 0 or unaligned x / W rows (the first layer's 17 columns) take guarded scalar operand
 *                              loads; aligned shapes the 16-byte loads.
 *   pcg_dense_rows_dgrad_post  g = dz[R][O] W[O][I], then the backward of the stage below: dn = g * mask * scale; xhat recomputed from
 *                              (a, mean, invstd) with the forward's expression; dbeta (+)= sum_r dn, dgamma (+)= sum_r dn xhat;
 *                              da = gamma invstd (dn - dbeta/R - xhat dgamma/R); dx = da * act'(a), act' from the sign of a;
 *                              db[I] (nullable) (+)= sum_r dx, the bias gradient of the stage's Linear: the columns are complete here.
 * The weight gradients are pcg_dense_rows_wgrad (x = the stage's input, dz = the dx written here; db NULL when taken here: its own
 * bias sum is a loop over the rows by one thread per column, three quarters of that launch at 128 rows). */
int pcg_dense_rows_fwd_post(const float* x, const float* W, const float* bias /*nullable*/, int32_t R, int32_t I, int32_t O, int act,
                            float slope, const float* gamma, const float* beta, float* running_mean /*nullable*/,
                            float* running_var /*nullable*/, int64_t* num_batches_tracked /*nullable*/, float eps, float momentum,
                            const float* mask /*nullable*/, float scale, float* a, float* save_mean, float* save_invstd, float* y,
                            pcg_stream_t stream);
int pcg_dense_rows_dgrad_post(const float* dz, const float* W, int32_t R, int32_t O, int32_t I, const float* mask /*nullable*/, float scale,
                              const float* a, const float* mean, const float* invstd, const float* gamma, int act, float slope,
                              float* dgamma, float* dbeta, float* db /*nullable*/, int accumulate, float* dx, pcg_stream_t stream);

/* ---- moons GAN and conditional GAN: whole training iterations in one launch, one workgroup (csrc/moons_gan.hip) ----------------
 * simple_gan/moons/make_moons_gan.py (build_generator :33-38, build_discriminator :40-46, the batch loop :61-88) and
 * conditional_gan/moons/make_moons_cgan.py (Generator :35-46, Discriminator :48-60, the batch loop :90-129) are one family:
 *   G: Linear(z_dim + label_dim -> hidden), ReLU, Linear(hidden -> 2)           on cat[z, onehot]
 *   D: Linear(2 + label_dim -> hidden), ReLU, Linear(hidden -> 1), Sigmoid      on cat[x, onehot]
 * with label_dim 0 for the simple GAN.  hidden 32 | 64 | 128, z_dim a multiple of 4 in [4, 64], label_dim 0 | 2, batch 1..256;
 * anything else is refused with PCG_ERR_INVALID.  Parameters live in the modules' flat buffers:
 *   g_off: first Linear weight [hidden][z_dim + label_dim], bias, second Linear weight [2][hidden], bias          (floats, in this order)
 *   d_off: first Linear weight [hidden][2 + label_dim], bias, second Linear weight [1][hidden], bias
 * Adam as in pcg_moons_cf_desc: pcg_adam_step_capturable's arithmetic over the first n*_adam floats, weight decay 0, the device step
 * counters advanced by one per iteration.                                                                                       */
typedef struct pcg_moons_gan_desc {
  int32_t hidden, z_dim, label_dim, B, N;  /* B, N: batch and training rows (train only)                           */
  int32_t nG, nD, nG_adam, nD_adam;        /* flat lengths (floats) and the Adam spans                             */
  int32_t g_off[4], d_off[4];
  double lr_G, lr_D, beta1, beta2, adam_eps;
} pcg_moons_gan_desc;

typedef struct pcg_moons_gan_train_args {
  const float* X; const int64_t* Y;        /* the training set in HBM: [N][2], [N] (Y: label_dim > 0 only)          */
  const int64_t* rows;                     /* [n_steps][B] rows of X / Y: the real batch of every iteration.  The caller checks the
                                              range; the kernel clamps an index into [0, N) rather than read outside X.          */
  const float* z;                          /* [n_steps][2][B][z_dim]: the D step's draw (:63 / :97), then the G step's (:78 / :116) */
  const int64_t* labels;                   /* [n_steps][2][B] fake labels (cgan :98, :117); label_dim > 0 only       */
  float* g_flat; float* d_flat;
  float* g_exp_avg; float* g_exp_avg_sq; int64_t* g_step;
  float* d_exp_avg; float* d_exp_avg_sq; int64_t* d_step;
  float* logs;                             /* [n_steps][2]: loss_D, loss_G                                          */
  float* scratch; size_t scratch_bytes;    /* activations that do not fit in LDS (pcg_moons_gan_scratch_bytes), 16-byte aligned */
} pcg_moons_gan_train_args;

/* Bytes of global activation scratch a train launch with this descriptor needs (0: everything stays in LDS, as at 50 x 128). */
size_t pcg_moons_gan_scratch_bytes(const pcg_moons_gan_desc* desc);
/* n_steps consecutive iterations of the batch loop (make_moons_gan.py:62-87, make_moons_cgan.py:91-129) in ONE launch of one
 * workgroup.  D step: fake = G(z_d), loss_D = -mean(log D(real) + log(1 - D(fake))), D's gradients only (what flows into G there is
 * discarded by the reference: zero_grad :85 / detach :105), Adam D.  G step: fake = G(z_g), loss_G = -mean(log D(fake)) with the
 * updated D, backward through D into G, Adam G.  Both losses and their gradients are formed from D's logit a (-log D =
 * softplus(-a), -log(1 - D) = softplus(a)): equal to the reference's expression in exact arithmetic and finite where its bare log
 * of a saturated sigmoid is inf.  fp32, fixed summation order: n steps in one launch are bit-identical to n launches of one.
 * Weights and moments are read once and written once per launch.                                                                */
int pcg_moons_gan_train_steps(const pcg_moons_gan_desc* desc, const pcg_moons_gan_train_args* args, int32_t n_steps, pcg_stream_t stream);

/* Forward of one net over R rows, a grid over blocks of 64 rows: which = 0 generator (make_moons_gan.py:112, make_moons_cgan.py:44-46,
 * :155; x = z [R][z_dim], 16-byte aligned, out [R][2]), 1 discriminator (:66-68 / :58-60; x [R][2], out [R][1], probabilities).
 * onehot [R][label_dim] floats (label_dim > 0 only).  params: the net's flat buffer.                                             */
typedef struct pcg_moons_gan_fwd_args {
  int32_t which; int64_t R;
  const float* x; const float* onehot; const float* params;
  float* out;
} pcg_moons_gan_fwd_args;
int pcg_moons_gan_forward(const pcg_moons_gan_desc* desc, const pcg_moons_gan_fwd_args* args, pcg_stream_t stream);

/* ---- moons CounteRGAN: the classifier fit in one launch, one workgroup (csrc/moons_clf.hip) --------------------------------------
 * conditional_counteRGAN/moons/trainer.py:13-29 (train_classifier) and main.py:14-40 (get_classifier) fit
 * NNClassifier = Linear(2 -> 32), ReLU, Linear(32 -> 32), ReLU, Linear(32 -> 3) with full-batch Adam steps of the mean cross-entropy
 * over the N training rows (trainer.py:22-25).  hidden 32 and 1 <= N <= 4096 only; anything else is refused with PCG_ERR_INVALID and
 * pcg_last_error() names the field.  Parameters live in the module's flat buffer of nC floats:
 *   c_off: net.0.weight [32][2], net.0.bias, net.2.weight [32][32], net.2.bias, net.4.weight [3][32], net.4.bias   (floats, in this
 *          order, each a multiple of 4, not overlapping)
 * Adam as in pcg_moons_cf_desc: pcg_adam_step_capturable's arithmetic over the first nC_adam floats, weight decay 0, the device step
 * counter advanced by one per iteration.                                                                                        */
typedef struct pcg_moons_clf_fit_desc {
  int32_t hidden, N, nC, nC_adam;          /* 32; rows 1..4096; flat length; Adam span (floats)           */
  int32_t c_off[6];                        /* net.{0,2,4}.weight/bias offsets (floats) in the flat buffer */
  double lr, beta1, beta2, adam_eps;
} pcg_moons_clf_fit_desc;
typedef struct pcg_moons_clf_fit_args {
  const float* X; const int64_t* Y;        /* [N][2], [N] in HBM (labels 0..2: the caller checks)                            */
  float* c_flat; float* exp_avg; float* exp_avg_sq; int64_t* step;
  float* losses;                           /* [n_steps]: the loss before the update of each iteration (trainer.py:23)        */
  int32_t* correct;                        /* optional [1]: rows with argmax(logits) == Y under the final weights             */
  float* scratch; size_t scratch_bytes;    /* pcg_moons_clf_fit_scratch_bytes of them, 16-byte aligned (may be NULL with 0)  */
} pcg_moons_clf_fit_args;
/* Bytes of global scratch a launch with this descriptor needs.  0 for every valid descriptor: the rows are walked in chunks whose
 * activations live in LDS.  (0 for an invalid one as well; pcg_moons_clf_fit refuses it.)                                        */
size_t pcg_moons_clf_fit_scratch_bytes(const pcg_moons_clf_fit_desc* desc);
/* n_steps consecutive iterations of trainer.py:22-25 in ONE launch of one workgroup: forward of all N rows, loss = mean
 * cross-entropy (log-softmax with the row maximum subtracted), d logits = (softmax - onehot) / N, backward through both ReLUs, the
 * six gradient tensors, Adam, step counter + 1.  fp32, every sum in an order fixed by N alone: n steps in one launch are
 * bit-identical to any split into several launches.  Weights and moments are read once and written once per launch.  With
 * `correct` the launch ends with one more forward under the final weights (ties of the argmax go to the lower index).          */
int pcg_moons_clf_fit(const pcg_moons_clf_fit_desc* desc, const pcg_moons_clf_fit_args* args, int32_t n_steps, pcg_stream_t stream);

/* ---- calibration (diagnostics; not on the step's path) -----------------------------------------------------------------------
 * What THIS box's fp32 matrix pipe and HBM sustain right now — bench.py prints it next to the step (`calib`) so that a run on a
 * slower-clocked box can be told from a slower kernel (the reference has nothing comparable: it publishes no performance numbers,
 * BASELINE.md §2 "re-derive from the box").
 *   pcg_calib_mfma   `rounds` blocks per CU of 4 waves, each issuing iters*16 back-to-back v_mfma_f32_32x32x2_f32 on four
 *                    independent accumulators.  workspace: [2048 floats of operands — caller-initialised, any finite values]
 *                    [blocks*256 floats sink][blocks*2 uint64: shader-clock ticks, 100 MHz reference ticks of the block's loop].
 *                    *flop_out = FLOP of the launch; *stamps_out = device address of the stamps.  Time it with events on `stream`.
 *   pcg_calib_copy   dst <- src (16 bytes per lane, grid-stride): 2*nbytes of HBM traffic.                                       */
int32_t pcg_calib_mfma_blocks(int32_t rounds);
size_t pcg_calib_mfma_workspace_bytes(int32_t rounds);
int pcg_calib_mfma(int32_t iters, int32_t rounds, void* workspace, size_t workspace_bytes, double* flop_out /*nullable*/,
                   uint64_t** stamps_out /*nullable*/, pcg_stream_t stream);
int pcg_calib_copy(const void* src, void* dst, int64_t nbytes, pcg_stream_t stream);

/* ---- ReLU + MaxPool2d(2) of the max-pool MNIST classifier (conditional_counteRGAN/mnist/modules/classifier.py:9-13) --------------------
 * fp32, NHWC [B][H][W][C] with C % 4 == 0 (any other C is refused), 2x2 windows, stride 2, floor mode: Hp = H / 2, Wp = W / 2.
 * Streaming kernels (maxpool.hip): one thread owns four channels of one pooled pixel; no LDS, no atomics, grid-stride; every entry may
 * be captured into a HIP graph.
 * pcg_relu_maxpool2_fwd replaces nn.ReLU + nn.MaxPool2d(2) (modules/classifier.py:9-10 and :12-13): z is the convolution's output, raw
 * or already through ReLU (the kernel applies ReLU itself; a NaN survives it).  p [B][Hp][Wp][C] = max over the window of relu(z);
 * idx [B][Hp][Wp][C] (uint8, dh * 2 + dw) = the position torch.nn.functional.max_pool2d(..., return_indices=True) picks: row-major scan,
 * a later cell wins only if strictly greater or NaN, so ties (the all-zero window of a dead ReLU patch too) keep the first cell. */
int pcg_relu_maxpool2_fwd(const float* z, float* p, uint8_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, pcg_stream_t stream);
/* The backward of the same two layers (modules/classifier.py:9-10, :12-13) in one pass: dz [B][H][W][C], the gradient with respect to the
 * convolution's RAW output.  The chosen cell of each window gets dp where p > 0 (p > 0 is that cell's ReLU mask, so z is not read; a NaN
 * p counts as live, as in torch) and 0 elsewhere; the other three cells, and the row / column an odd H / W leaves outside every
 * window, get 0.  Every element of dz is stored exactly once: no pre-zeroing, no atomics, deterministic. */
int pcg_relu_maxpool2_bwd(const float* dp, const float* p, const uint8_t* idx, float* dz, int32_t B, int32_t H, int32_t W, int32_t C,
                          pcg_stream_t stream);

/* ---- the launches around the convolutions of the additive-delta MNIST CounteRGAN (conditional_counteRGAN/mnist/gan_train.py:117-144
 * on modules/generator.py and modules/discriminator.py; csrc/delta_gan.hip) ---------------------------------
 * All fp32, gfx950 only, every sum in a fixed order, no floating-point atomics; every entry takes a stream and may be captured into a
 * HIP graph.  Every entry validates its arguments before it touches HIP: PCG_ERR_INVALID and a pcg_last_error text otherwise.
 * Rows are images of HW pixels; an NHWC tensor of C channels holds pixel p of row b at [b][p][c].                                      */
#define PCG_DELTA_GAN_BUILD 0     /* pcg_delta_gan_entry: build g_in and d_in                                                          */
#define PCG_DELTA_GAN_REGATHER 1  /* pcg_delta_gan_entry: rewrite channel 1 of d_in rows B..2B only                                    */
#define PCG_LOGIT_HEAD_D 0        /* pcg_logit_head_fwd: rows 0..R/2 labelled 1, the rest 0; loss = mean(real) + mean(fake)            */
#define PCG_LOGIT_HEAD_G 1        /* pcg_logit_head_fwd: every row labelled 1; loss = mean                                             */
#define PCG_DELTA_GAN_CHUNK 1024  /* elements per partial sum of pcg_delta_gan_tail_fwd                                                */

/* The 2-channel inputs of both nets in one launch (generator.py:19-20 at gan_train.py:122,133; discriminator.py:21-22 at :123-124):
 *   g_in [B][HW][2]  = (x, table_g[target])
 *   d_in [2B][HW][2]: rows 0..B = (x, table_d[y]); rows B..2B get channel 1 = table_d[target] (their channel 0 is x_cf, written by
 *                     pcg_delta_gan_tail_fwd).
 * Pure copies: the bits pcg_embed_concat_fwd writes.  mode PCG_DELTA_GAN_REGATHER writes nothing but channel 1 of d_in rows B..2B
 * (the label map of D's pass in the G step, :134, from the table Adam(D) has just updated, :130); x, y, table_g, g_in may be null then.
 * labels_2b (nullable, [2B]) receives (y, target): the index of D's embedding-table gradient.  head_w / head_w_packed (nullable, both
 * or neither; [head_P * head_C]) : head_w_packed[p * head_C + c] = head_w[c * head_P + p], the (h,w,c) image of a Linear weight row
 * whose columns nn.Flatten orders (c,h,w) (discriminator.py:15-16), refreshed by the same launch in either mode.
 * y and target are device pointers.  y_host / target_host (nullable) are host copies of the same labels: where given, a label outside
 * 0..K-1 is refused before any launch.  Without them a label is clamped into the table, as pcg_embed_concat_fwd clamps it.           */
typedef struct pcg_delta_gan_entry_args {
  const float* x;              /* [B][HW]                                                      */
  const int64_t* y;            /* [B], device                                                  */
  const int64_t* target;       /* [B], device                                                  */
  const int64_t* y_host;       /* nullable: host copy of y, range-checked                      */
  const int64_t* target_host;  /* nullable: host copy of target, range-checked                 */
  const float* table_g;        /* [K][HW]                                                      */
  const float* table_d;        /* [K][HW]                                                      */
  float* g_in;                 /* [B][HW][2]                                                   */
  float* d_in;                 /* [2B][HW][2]                                                  */
  int64_t* labels_2b;          /* nullable: [2B] = (y, target)                                 */
  const float* head_w;         /* nullable: [head_C * head_P], columns (c, p)                  */
  float* head_w_packed;        /* nullable: [head_P * head_C], columns (p, c)                  */
  int32_t B, HW, K, mode, head_C, head_P;
} pcg_delta_gan_entry_args;
int pcg_delta_gan_entry(const pcg_delta_gan_entry_args* args, pcg_stream_t stream);

/* What follows G's last, one-channel convolution (generator.py:22 at gan_train.py:133, the input of :134-135, and :139):
 *   x_cf[b][p] = x[b][p] + delta[b][p]                   (the classifier's input)
 *   d_in[B + b][p][0] = the same value                   (channel 0 of D's rows B..2B; d_in is the [2B][HW][2] tensor of the entry)
 *   loss_reg[0] = mean |delta|
 * The mean's order is fixed by the data alone: the n = B * HW elements are cut into chunks of PCG_DELTA_GAN_CHUNK, a chunk's sum is
 * one 256-thread tree over four-element thread sums, and the last workgroup to arrive adds the chunk sums in index order (thread t
 * takes chunks t, t + 256, ... in float64, then a tree).  grid (0: one workgroup per chunk, at most 1024) changes no bit.
 * workspace: pcg_delta_gan_tail_workspace_bytes(B, HW) bytes, 16-byte aligned, whose first 16 bytes are zero at the first call; the
 * entry leaves them zero.  HW % 4 == 0; x, delta, x_cf 16-byte aligned, d_in 8-byte aligned.                                          */
typedef struct pcg_delta_gan_tail_fwd_args {
  const float* x;       /* [B][HW] */
  const float* delta;   /* [B][HW] */
  float* x_cf;          /* [B][HW] */
  float* d_in;          /* [2B][HW][2] */
  float* loss_reg;      /* [1] */
  void* workspace;
  size_t workspace_bytes;
  int32_t B, HW, grid;
} pcg_delta_gan_tail_fwd_args;
size_t pcg_delta_gan_tail_workspace_bytes(int32_t B, int32_t HW);
int pcg_delta_gan_tail_fwd(const pcg_delta_gan_tail_fwd_args* args, pcg_stream_t stream);

/* nn.Flatten + nn.Linear(F -> 1) (discriminator.py:15-16) + nn.BCEWithLogitsLoss (gan_train.py:127 in mode PCG_LOGIT_HEAD_D, :137 in
 * mode PCG_LOGIT_HEAD_G) and the loss's gradient, in one launch.  a [R][F]: D's last activation, NHWC, through its LeakyReLU; w [F]:
 * the weight row with its columns packed (h,w,c) (pcg_delta_gan_entry's head_w_packed); bias [1].
 *   logits[r] = a[r] . w + bias      one workgroup per row: thread t folds the 16-byte groups t, t + 256, ... with fmaf, then a tree
 *   loss[0]   = mode D: mean over rows 0..R/2 of l(z, 1) + mean over rows R/2..R of l(z, 0); mode G: mean over all rows of l(z, 1),
 *               l(z, t) = (1 - t) z + max(-z, 0) + log(exp(-max(-z, 0)) + exp(-z - max(-z, 0)))  -- pcg_bce_logits_fwd_bwd's element
 *   dlogit[r] = (1 / rows of the mean) * (sigmoid(z) - t)                                        -- pcg_bce_logits_fwd_bwd's element
 *   db[0]     = sum over r of dlogit[r]   (thread t takes rows t, t + 256, ... in order, then a tree)
 * The last workgroup to arrive forms loss, dlogit and db.  workspace: 16 bytes, 4-byte aligned, zero at the first call, left zero.
 * R >= 1, even in mode D; F % 4 == 0; a and w 16-byte aligned.                                                                         */
typedef struct pcg_logit_head_fwd_args {
  const float* a;       /* [R][F] */
  const float* w;       /* [F], packed (h,w,c) */
  const float* bias;    /* [1] */
  float* logits;        /* [R] */
  float* loss;          /* [1] */
  float* dlogit;        /* [R] */
  float* db;            /* [1] */
  void* workspace;      /* 16 bytes */
  int32_t R, F, mode;
} pcg_logit_head_fwd_args;
int pcg_logit_head_fwd(const pcg_logit_head_fwd_args* args, pcg_stream_t stream);

/* The backward of the same head down to conv3's pre-activation (gan_train.py:129 / :143 through discriminator.py:14-16), one pass over a:
 *   da[r][f] = (dlogit[r] * w[f]) * (a[r][f] > 0 ? 1 : slope)     the grad-input with the LeakyReLU derivative already applied
 *   dw[f]    = sum over r of dlogit[r] * a[r][f]                   (nullable: mode G passes NULL and dw is not touched)
 * dw's rows are taken in index order: the R rows are cut into 16 contiguous groups of ceil(R / 16), a group is folded row by row with
 * fmaf, and the group sums are added in group order.  dw_C, dw_P (both 0: dw[f] is stored at f): column f = p * dw_C + c is stored at
 * dw[c * dw_P + p], the (c,h,w) order of the Linear weight's own gradient; dw_C * dw_P == F then.
 * F % 4 == 0; a, w, da 16-byte aligned.                                                                                                */
typedef struct pcg_logit_head_bwd_args {
  const float* a;        /* [R][F] */
  const float* w;        /* [F], packed (h,w,c) */
  const float* dlogit;   /* [R] */
  float* da;             /* [R][F] */
  float* dw;             /* nullable: [F] */
  float slope;
  int32_t R, F, dw_C, dw_P;
} pcg_logit_head_bwd_args;
int pcg_logit_head_bwd(const pcg_logit_head_bwd_args* args, pcg_stream_t stream);

/* The gradient of loss_G (gan_train.py:141-143) with respect to delta in one launch:
 *   d_delta[b][p] = dD[(b * HW + p) * dD_stride] + lambda_cls * dC[b][p] + reg_scale * sign(delta[b][p])
 * added in exactly that order, every product and sum rounded on its own (no contraction).  dD: channel 0 of D's grad-input (dD_stride
 * 2), or the one-channel grad-input (dD_stride 1); dC: the classifier's input gradient; reg_scale = lambda_reg / (B * HW), the
 * caller's rounding; sign(0) = 0, as the backward of torch.abs has it.                                                                 */
typedef struct pcg_delta_gan_tail_bwd_args {
  const float* dD;
  const float* dC;       /* [B][HW] */
  const float* delta;    /* [B][HW] */
  float* d_delta;        /* [B][HW] */
  float lambda_cls, reg_scale;
  int32_t B, HW, dD_stride;
} pcg_delta_gan_tail_bwd_args;
int pcg_delta_gan_tail_bwd(const pcg_delta_gan_tail_bwd_args* args, pcg_stream_t stream);

/* ---- the prompted half of the additive-delta MNIST CounteRGAN (conditional_counteRGAN/mnist/gan_train_copy.py on
 * modules/generator.py; csrc/delta_cf_eval.hip) ------------------------------------------------------------------
 * All fp32, gfx950 only, no floating-point atomics, every sum in an order fixed by the shapes alone; every entry takes a stream and may
 * be captured into a HIP graph.  Every entry validates its arguments before it touches HIP: PCG_ERR_INVALID and a pcg_last_error text
 * otherwise.  A query is q = t * B + b (target slot t of T, row b of B), as in pcg_mnist_cf_entry; entry and tail work on the window
 * [q0, q0 + nq) of the T * B queries and index their per-query tensors relative to q0.  The classifier's logits of x_cf are scored by
 * pcg_mnist_cf_score as it is: pcg_delta_cf_tail's sums are its tail_sums.                                                              */

/* The generator's 2-channel input for a window of queries (modules/generator.py:19-20 at gan_train_copy.py:165):
 *   out[q - q0][p] = (x[b][p], table[target(q)][p])
 * target NULL: the sweep, target(q) = t, T <= K.  target [B] (device): target(q) = target[b], and T must be 1.  The broadcast of x over
 * the T targets is done by indexing.  Pure copies: at T = 1, q0 = 0 the bits are pcg_delta_gan_entry's g_in.  A device label outside
 * 0..K-1 is clamped into the table, as pcg_embed_concat_fwd clamps it; target_host (nullable) is a host copy of target: where given, a
 * label outside 0..K-1 is refused before any launch.  HW % 4 == 0; out is written 8 bytes at a time.                                   */
typedef struct pcg_delta_cf_entry_args {
  const float* x;              /* [B][HW]                                          */
  const float* table;          /* [K][HW]                                          */
  const int64_t* target;       /* nullable: [B], device                            */
  const int64_t* target_host;  /* nullable: host copy of target, range-checked     */
  float* out;                  /* [nq][HW][2]                                      */
  int32_t B, T, HW, K, q0, nq;
} pcg_delta_cf_entry_args;
int pcg_delta_cf_entry(const pcg_delta_cf_entry_args* args, pcg_stream_t stream);

/* What follows G's last convolution for a window of queries (gan_train_copy.py:165-166):
 *   x_cf[q - q0][p] = clamp(x[b][p] + delta[q - q0][p], -1, 1)     the sum is rounded first, then clamped; a NaN stays a NaN
 *   sums[q - q0]    = { sum |x_cf - x|, sum |delta|, sum (x_cf - x)^2 } over the HW pixels
 * One wave per query: lane l folds the 16-byte groups l, l + 64, ... element by element, every term rounded on its own, then a fixed
 * xor butterfly adds the 64 lane sums.  All three sums are continuous in the inputs.  HW % 4 == 0; delta, x, x_cf 16-byte aligned.     */
typedef struct pcg_delta_cf_tail_args {
  const float* delta;   /* [nq][HW] */
  const float* x;       /* [B][HW]  */
  float* x_cf;          /* [nq][HW] */
  float* sums;          /* [nq][3]  */
  int32_t B, T, HW, q0, nq;
} pcg_delta_cf_tail_args;
int pcg_delta_cf_tail(const pcg_delta_cf_tail_args* args, pcg_stream_t stream);

/* The iteration's one random class (gan_train_copy.py:119-120: torch.randint(0, 10, (1,)), torch.full_like(y_true, .)): ONE class, the
 * value pcg_randint(out, 1, 0, K, NULL, seed, offset) writes to out[0], written to all B rows of target.  counter NULL: the Philox
 * offset is the by-value argument.  counter (device, uint64[2], 8-byte aligned): the offset is counter[0] and the launch advances
 * counter[0] by 1, the (1 + 3) / 4 counter values a one-element pcg_randint spans; counter[1] is not touched.  One workgroup: every
 * thread reads the counter, a barrier, one thread writes the increment -- a captured launch draws the next class of the stream on every
 * replay.                                                                                                                              */
typedef struct pcg_delta_gan_target_draw_args {
  int64_t* target;      /* [B], device             */
  uint64_t* counter;    /* nullable: device [2]    */
  uint64_t seed, offset;
  int32_t B, K;
} pcg_delta_gan_target_draw_args;
int pcg_delta_gan_target_draw(const pcg_delta_gan_target_draw_args* args, pcg_stream_t stream);

/* ---- the head and the losses of the full-resolution MNIST CounteRGAN (conditional_counteRGAN/mnist/countergan2.py:76-93, :188, :198;
 * csrc/prob_head.hip) ----------------------------------------------------------------------------------------
 * All fp32, gfx950 only, every sum in an order fixed by the data and the arguments, no floating-point atomics, no grid barrier; every
 * entry takes a stream and may be captured into a HIP graph.  Every entry validates its arguments before it touches HIP:
 * PCG_ERR_INVALID (PCG_ERR_WORKSPACE for a workspace too small) and a pcg_last_error text otherwise.                                   */
#define PCG_PROB_HEAD_D 0          /* rows 0..R/2 are D(real), rows R/2..R are D(fake): countergan2.py:188                             */
#define PCG_PROB_HEAD_G 1          /* every row is D(fake) of the generator's step: countergan2.py:198                                 */
#define PCG_PROB_HEAD_MAX_SLABS 16

/* nn.Flatten + nn.Linear(F -> 1) + nn.Sigmoid (countergan2.py:85-87 at :186-187 and :195), the log-eps loss of :188 (mode D) or :198
 * (mode G), the loss's gradient with respect to the logit and the bias gradient, in one launch.  a [R][F]: D's last activation, NHWC,
 * through its LeakyReLU; w [F]: the weight row packed (h,w,c) by pcg_delta_gan_entry; bias [1].  With half = R/2 (mode D) or R (mode G):
 *   logits[r] = a[r] . w + bias
 *   prob[r]   = d = 1 / (1 + exp(-logit))                    pcg_act_fwd's PCG_ACT_SIGMOID expression: the same bits for the same logit
 *   loss[0]   = mode D: -(1/half) * sum_b [ log(d_b + eps) + log((1 - d_{half+b}) + eps) ]       the fake term left to right, as :188
 *               mode G: -(1/R) * sum_b log(d_b + eps)
 *   dlogit[r] = real rows (all rows in mode G): -(1/half) * d (1 - d) / (d + eps);  fake rows: +(1/half) * d (1 - d) / ((1 - d) + eps)
 *   db[0]     = sum over r of dlogit[r]
 * One workgroup of 256 threads per (row, slab): the F/4 16-byte groups of a row are cut into `slabs` contiguous slabs of
 * ceil((F/4) / slabs) groups (a slab past the end is empty and contributes +0); thread t folds groups t, t + 256, ... of its slab with
 * fmaf, then a 256-wide tree.  The last workgroup to arrive finishes: thread t takes rows t, t + 256, ...: logit = ((p_0 + p_1) + ...)
 * + bias over the slab partials in slab order, then d, dlogit; the loss terms are summed in the order of pcg_log_eps_loss_fwd_bwd, db
 * over rows t, t + 256, ... in order, each then a tree.  With slabs = 1 the logits are pcg_logit_head_fwd's bit for bit.
 * slabs: 1..16, or 0 for the library's choice: 2 for R <= 128, 1 above.  That is what scripts/bench_countergan2.py showed at
 * F = 50176: at R = 128 two slabs beat one in every round (14.5 against 15.7 us), at R = 256 no count beat
 * one, and 4 or 8 slabs lost at both; other row counts were not measured and fall on the side of the nearer measured one.  workspace: pcg_prob_head_workspace_bytes(R, slabs) bytes (0 for an R or a slab
 * count the entry refuses), 4-byte aligned, all zero at the first call and left all zero.  R >= 1, even in mode D; F % 4 == 0; a and w
 * 16-byte aligned; 0 < eps < 1.  The backward of this head is pcg_logit_head_bwd with dlogit as it stands.                             */
typedef struct pcg_prob_head_fwd_args {
  const float* a;       /* [R][F] */
  const float* w;       /* [F], packed (h,w,c) */
  const float* bias;    /* [1] */
  float* logits;        /* [R] */
  float* prob;          /* [R] */
  float* loss;          /* [1] */
  float* dlogit;        /* [R] */
  float* db;            /* [1] */
  void* workspace;
  size_t workspace_bytes;
  float eps;
  int32_t R, F, mode, slabs;
} pcg_prob_head_fwd_args;
size_t pcg_prob_head_workspace_bytes(int32_t R, int32_t slabs);
int pcg_prob_head_fwd(const pcg_prob_head_fwd_args* args, pcg_stream_t stream);

/* The same loss on given probabilities p [R] (countergan2.py:188 in mode PCG_PROB_HEAD_D, :198 in mode PCG_PROB_HEAD_G), for the op
 * chain that ends in pcg_act_fwd's sigmoid.  loss [1] (nullable); dp [R] (nullable, out of place) = d loss / d p, before the sigmoid:
 * real rows -(1/half) / (p + eps), fake rows +(1/half) / ((1 - p) + eps), times grad_out[0] where grad_out (nullable, device) is given.
 * One workgroup; thread t takes b = t, t + 256, ... below half, the term of b in mode D being log(p_b + eps) + log((1 - p_{half+b}) +
 * eps), then a 256-wide tree: the order of pcg_prob_head_fwd, so fed that entry's prob it returns that entry's loss bit for bit.       */
typedef struct pcg_log_eps_loss_args {
  const float* p;          /* [R] */
  const float* grad_out;   /* nullable: [1], device */
  float* loss;             /* nullable: [1] */
  float* dp;               /* nullable: [R] */
  float eps;
  int32_t R, mode;
} pcg_log_eps_loss_args;
int pcg_log_eps_loss_fwd_bwd(const pcg_log_eps_loss_args* args, pcg_stream_t stream);

/* ---- the numbers and pixels of the MNIST CounteRGAN's report figures (conditional_counteRGAN/mnist/eval_utils.py:113-201, gr.py and
 * gradio_app.py:346-441, :498-568; csrc/cf_report.hip) ---------------------------------------------------------
 * All fp32, gfx950 only; every entry takes a stream, may be captured into a HIP graph and validates its arguments before it touches HIP:
 * PCG_ERR_INVALID and a pcg_last_error text otherwise.  The only atomics are integer maxima, so no result depends on an order.        */
#define PCG_CLASS_PICK_FIRST 0    /* the first row of every class (eval_utils.py:146-147)                                              */
#define PCG_CLASS_PICK_BEST 1     /* the row the classifier is most confident about, the lowest such row on a tie (:142-144)           */
#define PCG_CLASS_PICK_KMAX 64    /* classes a pick keeps per workgroup                                                                */
#define PCG_CF_PANELS_GRID 0
#define PCG_CF_PANELS_PANELS 1

/* One source row per class over a data set walked in chunks (replaces the per-row loop of eval_utils.py:139-149: one batch-1 classifier
 * forward and one host read per row).  A call folds the n rows [row0, row0 + n) of one chunk into state (uint64 [K], 8-byte aligned,
 * zeroed by the caller before the first chunk):
 *   key(row) = (uint64(hi) << 32) | (0xFFFFFFFF - row)          state[labels[row]] = max(state[labels[row]], key(row))
 *   mode BEST:  hi = the bits of conf = softmax(logits[row][0..K))[labels[row]], fp32, max-subtracted: the arithmetic (and the device
 *               function, csrc/softmax_label.h) of pcg_mnist_cf_score's own-label probabilities.  conf >= 0, and non-negative floats
 *               order as their bit patterns, so the maximum key is the highest confidence and, among equal confidences, the lowest row:
 *               the strict `conf > best_conf[idx]` scan of :143 in data-set order.  A row whose conf is not finite is skipped (a NaN
 *               never wins that `>` either).
 *   mode FIRST: hi = 1 and logits is not read (it may be null): the lowest row of the class, the early exit of :146-149.
 * A row whose label is outside [0, K) is skipped.  logits [n][kp] (kp >= K, a multiple of 4: the layout of the padded classifier
 * logits), labels [n] int64, both indexed from the chunk's first row.  K <= PCG_CLASS_PICK_KMAX; row0 + n <= 2^32 - 1 (a larger row does
 * not fit the key and is refused).  One thread per row; a workgroup keeps K keys in LDS (64-bit LDS maxima) and then issues at most K
 * global 64-bit atomicMax.  A maximum does not depend on the order of its operands: the state after all chunks is the same for ANY order
 * of chunks, workgroups and threads, bit for bit.                                                                                       */
int pcg_class_pick(const float* logits /*nullable in mode FIRST*/, const int64_t* labels, uint64_t* state, int32_t n, int32_t kp, int32_t K,
                   int64_t row0, int32_t mode, pcg_stream_t stream);

/* Decodes the state of pcg_class_pick (the `samples` / `best_conf` lists of eval_utils.py:136-137 after the loop): rows [K] int64 = the
 * picked row of each class, -1 where the state word is 0 (no row of that class); conf [K] = its confidence (0 in mode FIRST and for an
 * absent class).  X [N][HW] (nullable, with sources): the data set resident on the device; sources [K][HW] = X[rows[k]] (zeros for an
 * absent class or a row >= N, which is never read).                                                                                     */
int pcg_class_pick_gather(const uint64_t* state, const float* X /*nullable*/, int64_t* rows, float* conf, float* sources /*nullable*/,
                          int32_t K, int64_t N, int32_t HW, int32_t mode, pcg_stream_t stream);

/* The pixels of the figures.  Every operation is a single fp32 rounding (cf_report.hip compiles its kernels under
 * `#pragma clang fp contract(off)`: a multiply is never fused with the add that follows it): the output is bit-identical to the same
 * expressions in NumPy fp32.
 * mode PCG_CF_PANELS_GRID (eval_utils.py:167-195): x = sources [n][HW] (n = K source classes), x_cf [T][n][HW] (the [target][row] layout
 *   of the one-pass sweep), both in [-1, 1].  out (nullable) [n*H][T*W] float: cell (r, c) = (x_cf[c][r] + 1) / 2 (:190), the diagonal
 *   r == c = (sources[r] + 1) / 2 (:175).  out_u8 (nullable) the same image as uint8, min(255, max(0, floor(v * 255 + 0.5))): the
 *   convention of torchvision's save_image (countergan2.py:222).  mask, mask_mode, vmax are not read.
 * mode PCG_CF_PANELS_PANELS (gr.py:370-372, :399, :533-535): x, x_cf [n][HW] in [-1, 1]; mask [HW] (PCG_MASK_SHARED) or [n][HW]
 *   (PCG_MASK_PER_ROW).  out [n][4][H][W] = xv = (x + 1) / 2, cv = (x_cf + 1) / 2, |cv - xv| (from the two rounded values), mask.
 *   vmax [1]: zeroed by the caller; the launch raises it to the maximum of the third panel with an atomicMax on the float's bits (the
 *   values are >= 0).  T and out_u8 are not read.                                                                                      */
int pcg_cf_panels(int32_t mode, const float* x, const float* x_cf, const float* mask /*nullable in grid mode*/, int32_t mask_mode, float* out,
                  uint8_t* out_u8 /*nullable*/, float* vmax /*nullable in grid mode*/, int32_t n, int32_t T, int32_t H, int32_t W,
                  pcg_stream_t stream);

/* ---- the normalised image sheets of the trainers: torchvision's make_grid and the pixels of save_image on CPU fp32 tensors, as called
 * at dconv_gan/mnist/mnist_dcgan.py:190 (padding 2) and :222 (padding 5), simple_gan/mnist/mnist_gan.py:141 (nrow 5),
 * conditional_counteRGAN/mnist/gan_train.py:161-163 and countergan2.py:222-224 (nrow 4; the delta as deltas * 0.5 + 0.5),
 * conditional_gan/mnist/mnist_wgan_conditional.py:123-125 and :181-182 (csrc/image_sheet.hip) ------------------
 * All fp32, gfx950 only; both entries take a stream, may be captured into one HIP graph and validate their arguments before they touch
 * HIP.  Every pixel operation is a single fp32 rounding (no contraction), the division is a true fp32 division.  Pixels of a NaN input
 * are unspecified; a NaN cannot fault.                                                                                                   */

/* Bytes of the workspace of pcg_image_range: a ticket and one (min, max) pair per workgroup.  The caller zeroes it ONCE, when it is
 * allocated; every launch leaves the ticket zero, so nothing is reset between calls.  One launch at a time per workspace.              */
size_t pcg_image_range_workspace_bytes(void);

/* range[0] = min, range[1] = max of pre_scale * x[i] + pre_shift over the n floats of x (the product and the sum are two roundings;
 * pre_scale 1 and pre_shift 0 read x as it is): the global minimum and maximum make_grid(normalize=True) takes when no value_range is
 * given.  x 4-byte aligned: 16-byte loads from the first 16-byte boundary on, scalar ends.  Reduced as floats per wave (shuffles), per
 * workgroup (LDS) and, by the workgroup that takes the last ticket, over the workgroups' pairs; a minimum does not depend on the order
 * of its operands, so the result is the same bits for any order of workgroups.  n <= 2^31 - 1; range 4-byte, workspace 16-byte aligned. */
int pcg_image_range(const float* x, int64_t n, float pre_scale, float pre_shift, float* range, void* workspace, size_t workspace_bytes,
                    pcg_stream_t stream);

/* make_grid(x [N][C][H][W], nrow, padding, normalize, value_range, pad_value) and the uint8 pixels of save_image in one launch.
 *   every element first becomes e = pre_scale * x + pre_shift (two roundings; (1, 0): x as it is);
 *   normalize: e = (min(max(e, lo), hi) - lo) / d.  range != null: lo = range[0], hi = range[1] are read on the DEVICE (what
 *     pcg_image_range left there) and d = float(max(double(hi) - double(lo), 1e-5)) is formed there; range == null: the host gives
 *     lo, hi and d (a value_range; d > 0, lo <= hi);
 *   C == 1: the channel three times (C' = 3);
 *   N == 1: the grid is the image, [C'][H][W]; else xmaps = min(nrow, N), ymaps = ceil(N / xmaps), the grid is
 *     [C'][ymaps * (H + padding) + padding][xmaps * (W + padding) + padding], image k at row (k / xmaps) * (H + padding) + padding and
 *     column (k % xmaps) * (W + padding) + padding, every other pixel pad_value (the unused cells of the last row too).
 * grid (nullable): the float grid.  u8 (nullable): uint8(min(255, max(0, floor(g * 255 + 0.5)))) laid out [Hg][Wg][3], or [Hg][Wg]
 * with gray != 0 (C == 1 only).  At least one of the two.  One thread per pixel of the grid plane.
 * Refused: C outside {1, 3}; N, H, W or nrow < 1; padding < 0; N * C * H * W or 3 * Hg * Wg above 2^31 - 1; a range pointer that is not
 * 4-byte aligned.                                                                                                                       */
typedef struct pcg_image_sheet_args {
  const float* x;          /* [N][C][H][W] */
  const float* range;      /* nullable: [2] on the device, read when normalize != 0 */
  float* grid;             /* nullable: [3][Hg][Wg] */
  uint8_t* u8;             /* nullable: [Hg][Wg][3] or, gray, [Hg][Wg] */
  float lo, hi, d;         /* read when normalize != 0 and range == null */
  float pad_value, pre_scale, pre_shift;
  int32_t N, C, H, W, nrow, padding, normalize, gray;
} pcg_image_sheet_args;
int pcg_image_sheet(const pcg_image_sheet_args* args, pcg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PCGAN_HIP_H */
