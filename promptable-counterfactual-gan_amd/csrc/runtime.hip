// runtime.hip — library-level entry points: ABI version, target, thread-local error text.
#include "pcg_common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace pcg {
namespace {
thread_local char g_err[512] = "";
thread_local int32_t g_conv_prec = PCG_PREC_F32;
}

bool conv_bf16() { return g_conv_prec == PCG_PREC_BF16; }

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return PCG_OK;
  set_error("%s: launch failed: %s", what, hipGetErrorString(e));
  return PCG_ERR_LAUNCH;
}
}  // namespace pcg

// ABI history.  v7: the forward and grad-input convolutions take one argument struct: pcg_conv2d(geom, pcg_conv_args) replaces the twenty
//   positional entries pcg_conv2d_{fwd,dgrad}_{act,xf,bn,bn_xf,mask,add,add_mask,add_bnsum,bnbwd} and the grouped _fwd_bn_g / _dgrad_bnbwd_g;
//   pcg_conv2d_fwd / pcg_conv2d_dgrad stay as positional conveniences.
//   v6: the tabular step's launches take argument structs, a rider is an optional struct pointer (eighteen entry points
//   became nine: pcg_spectral_norm_{fwd,bwd}_batched, pcg_house_critic_{fwd,bwd}, pcg_house_classifier_{fwd,bwd},
//   pcg_house_residual_{fwd,bwd}, pcg_house_diag); + pcg_abi_struct_bytes.  v6, additive: + pcg_house_cf_eval;
//   + pcg_patch_mask_bits, pcg_mnist_cf_entry, pcg_mnist_cf_tail, pcg_mnist_cf_score (csrc/mnist_cf_eval.hip);
//   + pcg_moons_clf_fit, pcg_moons_clf_fit_scratch_bytes (csrc/moons_clf.hip).
//   + pcg_launch_plan_describe (csrc/tabular.hip: the routes of the non-convolution launches as text, host logic).
//   + pcg_delta_gan_entry, pcg_delta_gan_tail_fwd (+ _workspace_bytes), pcg_logit_head_fwd, pcg_logit_head_bwd, pcg_delta_gan_tail_bwd
//     (csrc/delta_gan.hip).
//   + pcg_delta_cf_entry, pcg_delta_cf_tail, pcg_delta_gan_target_draw (csrc/delta_cf_eval.hip).
//   + pcg_prob_head_fwd (+ _workspace_bytes), pcg_log_eps_loss_fwd_bwd (csrc/prob_head.hip).
//   + pcg_class_pick, pcg_class_pick_gather, pcg_cf_panels (csrc/cf_report.hip).
//   + pcg_image_range (+ _workspace_bytes), pcg_image_sheet (csrc/image_sheet.hip).
// v5, additive: + pcg_conv_precision_set / _get (thread-local bf16-operand mode of the implicit-GEMM convolutions).
// v5 (r04): + grouped batches (the grouped forward-statistics and bnbwd grad-input entries, part of pcg_conv2d since v7; pcg_bn_apply_act_g, pcg_conv2d_dgrad_bn_phases,
//   pcg_bn_bwd_partial_g(+_workspace_bytes), pcg_bn_act_bwd_premask_g(+pcg_bn_act_bwd_g_workspace_bytes), pcg_bce_pair),
//   pcg_conv2d_fwd_bnbwd_thin(+_ok, +_workspace_bytes), pcg_conv_weight_adjoint_many, pcg_conv_reset_scratch, pcg_dp_barrier,
//   pcg_dp_rccl_version; the stream-K scratch registry is keyed by (device, stream).
// v4 (r03): + pcg_calib_*, pcg_conv_set_scratch / pcg_conv_scratch_*_bytes, pcg_tune_set, pcg_conv_plan_describe, pcg_debug_stamp_buffer,
//   pcg_instnorm_bwd_fused / _bwd_bwd_act, pcg_rowsum3, pcg_norm_sum, pcg_house_diag, pcg_house_batch_draws_counter, the fused
//   critic-stage entry points.  v3 (r02): pcg_adam_step_capturable scratch is 48 bytes; pcg_linear_wgrad_grouped takes whole layers;
//   + the pcg_house_* / spectral-norm reps / seq entry points.  v2 (r02): + pcg_conv2d_*_xf, pcg_bn_train_stats_coef, pcg_dp_*;
//   pcg_bn_bwd_partial takes fp64 partial rows.
extern "C" int pcg_abi_version(void) { return 7; }
extern "C" size_t pcg_abi_struct_bytes(const char* name) {
#define PCG_STRUCT(T) {#T, sizeof(T)}
  static const struct { const char* name; size_t bytes; } table[] = {
      PCG_STRUCT(pcg_conv_geom), PCG_STRUCT(pcg_conv_args), PCG_STRUCT(pcg_in_xform), PCG_STRUCT(pcg_wgrad_item), PCG_STRUCT(pcg_sn_fwd_batch), PCG_STRUCT(pcg_sn_bwd_batch),
      PCG_STRUCT(pcg_house_g_desc), PCG_STRUCT(pcg_house_g_fwd_args), PCG_STRUCT(pcg_house_g_bwd_args), PCG_STRUCT(pcg_house_critic_fwd_args),
      PCG_STRUCT(pcg_house_critic_bwd_args), PCG_STRUCT(pcg_house_cls_fwd_args), PCG_STRUCT(pcg_house_cls_bwd_args),
      PCG_STRUCT(pcg_house_res_fwd_args), PCG_STRUCT(pcg_house_res_bwd_args), PCG_STRUCT(pcg_house_loss_args), PCG_STRUCT(pcg_house_diag_args),
      PCG_STRUCT(pcg_moons_cf_desc), PCG_STRUCT(pcg_moons_cf_train_args), PCG_STRUCT(pcg_moons_cf_fwd_args), PCG_STRUCT(pcg_moons_cf_eval_args),
      PCG_STRUCT(pcg_house_cf_eval_args), PCG_STRUCT(pcg_patch_mask_bits_args), PCG_STRUCT(pcg_mnist_cf_entry_args),
      PCG_STRUCT(pcg_mnist_cf_tail_args), PCG_STRUCT(pcg_mnist_cf_score_args),
      PCG_STRUCT(pcg_dense_bn), PCG_STRUCT(pcg_dense_bn_bwd), PCG_STRUCT(pcg_moons_gan_desc), PCG_STRUCT(pcg_moons_gan_train_args),
      PCG_STRUCT(pcg_moons_gan_fwd_args), PCG_STRUCT(pcg_moons_clf_fit_desc), PCG_STRUCT(pcg_moons_clf_fit_args),
      PCG_STRUCT(pcg_delta_gan_entry_args), PCG_STRUCT(pcg_delta_gan_tail_fwd_args), PCG_STRUCT(pcg_logit_head_fwd_args),
      PCG_STRUCT(pcg_logit_head_bwd_args), PCG_STRUCT(pcg_delta_gan_tail_bwd_args), PCG_STRUCT(pcg_delta_cf_entry_args),
      PCG_STRUCT(pcg_delta_cf_tail_args), PCG_STRUCT(pcg_delta_gan_target_draw_args), PCG_STRUCT(pcg_prob_head_fwd_args),
      PCG_STRUCT(pcg_log_eps_loss_args), PCG_STRUCT(pcg_image_sheet_args)};
#undef PCG_STRUCT
  if (name)
    for (const auto& t : table)
      if (!strcmp(t.name, name)) return t.bytes;
  return 0;
}
extern "C" const char* pcg_last_error(void) { return pcg::g_err; }
extern "C" const char* pcg_target_arch(void) { return "gfx950"; }
extern "C" int pcg_conv_precision_set(int32_t precision) {
  PCG_REQUIRE(precision == PCG_PREC_F32 || precision == PCG_PREC_BF16, "pcg_conv_precision_set: unknown precision %d (0 fp32, 1 bf16)", precision);
  pcg::g_conv_prec = precision;
  return PCG_OK;
}
extern "C" int32_t pcg_conv_precision_get(void) { return pcg::g_conv_prec; }
