"""ctypes binding of libpcgan_hip.so (the C ABI declared in include/pcgan_hip.h).

There is no CPU fallback: if the library is missing or a call fails, this module raises.  `import torch`
happens first on purpose — PyTorch-ROCm ships its own libamdhip64.so.7, and the dynamic linker must
resolve our library's HIP runtime to that already-loaded copy so that streams and device pointers are
shared with PyTorch.
"""
import ctypes
import os

import torch  # noqa: F401  (loads the HIP runtime this process will use)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCG_LIB") or os.path.join(_HERE, "libpcgan_hip.so")  # PCG_LIB: A/B builds of the same ABI

PCG_OK = 0
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
# pcg_launch_plan_describe: ops and element-wise families (include/pcgan_hip.h)
(PLAN_GEMM_ACT, PLAN_GEMM, PLAN_LINEAR_WGRAD, PLAN_LINEAR_WGRAD_GROUPED, PLAN_MEAN, PLAN_ABS_MEAN, PLAN_CROSS_ENTROPY,
 PLAN_EMBED_CONCAT_BWD, PLAN_ACT, PLAN_ELEMENTWISE, PLAN_BN_COLREDUCE, PLAN_BN_APPLY, PLAN_BN_FINALIZE, PLAN_INSTNORM,
 PLAN_SPECTRAL_NORM, PLAN_ADAM) = range(16)
PLAN_EW_TABULAR, PLAN_EW_CF_OPS, PLAN_EW_POINTWISE, PLAN_EW_GATHER_CHANNEL = range(4)


class PcgError(RuntimeError):
    pass


class ConvGeom(ctypes.Structure):
    """pcg_conv_geom (include/pcgan_hip.h)."""

    _fields_ = [(n, ctypes.c_int32) for n in ("B", "IH", "IW", "Cin", "OH", "OW", "Cout", "KH", "KW", "stride", "pad")]

    def key(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


_I, _P = ctypes.c_int32, ctypes.c_void_p


class HouseGDesc(ctypes.Structure):
    """pcg_house_g_desc (include/pcgan_hip.h)."""
    _fields_ = ([("fc_in_w", _I), ("fc_in_b", _I)] +
                [(n, _I * 5) for n in ("fc1_w", "fc1_b", "bn1_g", "bn1_b", "fc2_w", "fc2_b", "bn2_g", "bn2_b",
                                       "film_gamma_w", "film_gamma_b", "film_beta_w", "film_beta_b")] +
                [("cont_w", _I), ("cont_b", _I), ("head_w", _I * 8), ("head_b", _I * 8), ("seg", _I * 9)] +
                [(n, _I) for n in ("nheads", "ncont", "D", "NC", "hidden", "nblocks")])


class WgradItem(ctypes.Structure):
    """pcg_wgrad_item."""
    _fields_ = [("dy", _P), ("x", _P), ("dW", _P), ("db", _P)] + [(n, _I) for n in ("ldy", "ldx", "O", "I", "accumulate_w", "accumulate_b",
                                                                                      "tile_x", "tile_y")]


class HouseGFwdArgs(ctypes.Structure):
    """pcg_house_g_fwd_args."""
    _fields_ = ([(n, _P) for n in ("params", "x", "onehot", "mask", "noise", "inp", "H", "Z1", "Z2", "P", "SM")] +
                [("running_mean", _P * 10), ("running_var", _P * 10), ("num_batches_tracked", _P * 10)] +
                [(n, _P) for n in ("cont", "logits", "soft", "hard")] + [("B", ctypes.c_int32)] +
                [(n, ctypes.c_float) for n in ("eps", "momentum", "tau", "res_scale")])


class HouseGBwdArgs(ctypes.Structure):
    """pcg_house_g_bwd_args."""
    _fields_ = ([(n, _P) for n in ("params", "grads", "onehot", "mask", "H", "Z1", "Z2", "SM", "soft", "d_cont", "d_logits", "d_samples",
                                   "DH", "DZ1", "DZ2", "A1", "DN1", "DG", "DB", "DZIN", "DL", "DC", "Q")] +
                [("B", ctypes.c_int32), ("accumulate", ctypes.c_int32), ("tau", ctypes.c_float), ("res_scale", ctypes.c_float)])


class InXform(ctypes.Structure):
    """pcg_in_xform."""
    _fields_ = [("scale", _P), ("shift", _P), ("act", _I), ("slope", ctypes.c_float)]


class ConvArgs(ctypes.Structure):
    """pcg_conv_args: one forward / grad-input convolution launch (pcg_conv2d)."""
    _fields_ = ([(n, _P) for n in ("in_", "w", "bias", "out", "xf", "addend", "a_below", "z", "mean", "invstd", "gamma", "beta", "partial")] +
                [("partial_bytes", ctypes.c_size_t)] +
                [(n, _P) for n in ("save_mean", "save_invstd", "running_mean", "running_var", "num_batches_tracked", "coef_out", "workspace")] +
                [("workspace_bytes", ctypes.c_size_t), ("op", _I), ("act", _I), ("slope", ctypes.c_float), ("epi", _I), ("epi_act", _I),
                 ("epi_slope", ctypes.c_float), ("sum_scale", ctypes.c_float), ("stats", _I), ("eps", ctypes.c_float),
                 ("momentum", ctypes.c_float), ("groups", _I)])


CONV_FWD, CONV_DGRAD = 0, 1                                                          # pcg_conv_op
CONV_EPIS = ("none", "mask", "add", "add_mask", "add_bnsum", "bnbwd")                # pcg_conv_epi, by value


class MoonsCfDesc(ctypes.Structure):
    """pcg_moons_cf_desc (include/pcgan_hip.h)."""
    _fields_ = ([(n, _I) for n in ("hidden", "clf_hidden", "B", "N", "nG", "nD", "nC", "nG_adam", "nD_adam")] +
                [("g_off", _I * 14), ("d_off", _I * 8), ("c_off", _I * 6)] +
                [(n, ctypes.c_double) for n in ("lr_G", "lr_D", "beta1", "beta2", "adam_eps")] +
                [(n, ctypes.c_float) for n in ("bn_eps", "bn_momentum", "sn_eps", "slope", "lambda_cls", "lambda_l1", "lambda_l2",
                                               "lambda_mask")])


class MoonsCfTrainArgs(ctypes.Structure):
    """pcg_moons_cf_train_args."""
    _fields_ = ([(n, _P) for n in ("X", "Y", "rows", "target_y", "mask", "g_flat", "d_flat", "c_flat", "g_exp_avg", "g_exp_avg_sq", "g_step",
                                   "d_exp_avg", "d_exp_avg_sq", "d_step")] +
                [("bn_mean", _P * 3), ("bn_var", _P * 3), ("bn_nbt", _P * 3), ("sn_u", _P * 4), ("sn_v", _P * 4)] +
                [("logs", _P), ("scratch", _P), ("scratch_bytes", ctypes.c_size_t)])


class MoonsCfFwdArgs(ctypes.Structure):
    """pcg_moons_cf_fwd_args."""
    _fields_ = ([(n, _I) for n in ("which", "train", "B")] + [(n, _P) for n in ("x", "onehot", "mask", "params")] +
                [("bn_mean", _P * 3), ("bn_var", _P * 3), ("bn_nbt", _P * 3), ("sn_u", _P * 4), ("sn_v", _P * 4)] +
                [("out0", _P), ("out1", _P), ("scratch", _P), ("scratch_bytes", ctypes.c_size_t)])


class MoonsCfEvalArgs(ctypes.Structure):
    """pcg_moons_cf_eval_args."""
    _fields_ = ([("N", ctypes.c_int64), ("M", _I), ("T", _I), ("group", _I)] +
                [(n, _P) for n in ("x", "y", "masks", "target", "row_mask", "g_flat", "c_flat")] + [("bn_mean", _P * 3), ("bn_var", _P * 3)] +
                [(n, _P) for n in ("raw", "masked", "x_cf", "logits_cf", "logits_x", "pred_cf", "pred_x", "gain", "sums")])


class HouseCfEvalArgs(ctypes.Structure):
    """pcg_house_cf_eval_args."""
    _fields_ = ([("N", ctypes.c_int64)] + [(n, _I) for n in ("T", "group", "clamp_cls", "mask_rows")] + [("g_flat", _P), ("nG", _I)] +
                [("bn_mean", _P * 10), ("bn_var", _P * 10)] + [(n, ctypes.c_float) for n in ("bn_eps", "tau", "res_scale")] +
                [("col_src", _I * 17), ("norm_vals", _P), ("c_w_kmajor", ctypes.POINTER(ctypes.c_void_p)), ("c_bias", ctypes.POINTER(ctypes.c_void_p))] +
                [(n, _P) for n in ("x", "y", "target", "mask", "noise", "cont", "logits", "chosen", "masked", "x_cf", "x_cf_raw", "logits_cf",
                                   "logits_x", "pred_cf", "pred_x", "gain", "tile_sums", "class_sums", "class_counts")])


class PatchMaskBitsArgs(ctypes.Structure):
    """pcg_patch_mask_bits_args."""
    _fields_ = [("bits", _P), ("mask", _P)] + [(n, _I) for n in ("n", "H", "W", "ps")]


class MnistCfEntryArgs(ctypes.Structure):
    """pcg_mnist_cf_entry_args."""
    _fields_ = [(n, _P) for n in ("x", "table", "mask", "target", "out")] + [(n, _I) for n in ("B", "T", "HW", "K", "mask_mode", "q0", "nq")]


class MnistCfTailArgs(ctypes.Structure):
    """pcg_mnist_cf_tail_args."""
    _fields_ = ([(n, _P) for n in ("c", "x", "mask", "x_cf", "raw", "masked", "sums")] + [("scale", ctypes.c_float)] +
                [(n, _I) for n in ("B", "T", "HW", "mask_mode", "q0", "nq")])


class MnistCfScoreArgs(ctypes.Structure):
    """pcg_mnist_cf_score_args."""
    _fields_ = ([(n, _P) for n in ("logits_cf", "logits_orig", "target", "y_true", "tail_sums", "pred", "conf", "p_target", "p_true",
                                   "p_orig_true", "flip", "group_sums")] + [(n, _I) for n in ("B", "T", "K", "ld", "group_rows", "q0", "nq")])


MASK_SHARED, MASK_PER_ROW, MASK_PER_QUERY = 0, 1, 2      # PCG_MASK_* (include/pcgan_hip.h)
MNIST_CF_GROUP_SUMS = 8                                  # PCG_MNIST_CF_GROUP_SUMS


class MoonsGanDesc(ctypes.Structure):
    """pcg_moons_gan_desc."""
    _fields_ = ([(n, _I) for n in ("hidden", "z_dim", "label_dim", "B", "N", "nG", "nD", "nG_adam", "nD_adam")] +
                [("g_off", _I * 4), ("d_off", _I * 4)] + [(n, ctypes.c_double) for n in ("lr_G", "lr_D", "beta1", "beta2", "adam_eps")])


class MoonsGanTrainArgs(ctypes.Structure):
    """pcg_moons_gan_train_args."""
    _fields_ = ([(n, _P) for n in ("X", "Y", "rows", "z", "labels", "g_flat", "d_flat", "g_exp_avg", "g_exp_avg_sq", "g_step",
                                   "d_exp_avg", "d_exp_avg_sq", "d_step", "logs", "scratch")] + [("scratch_bytes", ctypes.c_size_t)])


class MoonsGanFwdArgs(ctypes.Structure):
    """pcg_moons_gan_fwd_args."""
    _fields_ = [("which", _I), ("R", ctypes.c_int64)] + [(n, _P) for n in ("x", "onehot", "params", "out")]


class MoonsClfFitDesc(ctypes.Structure):
    """pcg_moons_clf_fit_desc."""
    _fields_ = ([(n, _I) for n in ("hidden", "N", "nC", "nC_adam")] + [("c_off", _I * 6)] +
                [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "adam_eps")])


class MoonsClfFitArgs(ctypes.Structure):
    """pcg_moons_clf_fit_args."""
    _fields_ = ([(n, _P) for n in ("X", "Y", "c_flat", "exp_avg", "exp_avg_sq", "step", "losses", "correct", "scratch")] +
                [("scratch_bytes", ctypes.c_size_t)])


class DenseBn(ctypes.Structure):
    """pcg_dense_bn."""
    _fields_ = ([(n, _P) for n in ("gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "save_mean", "save_invstd", "xhat")] +
                [("eps", ctypes.c_float), ("momentum", ctypes.c_float), ("training", _I)])


class DenseBnBwd(ctypes.Structure):
    """pcg_dense_bn_bwd."""
    _fields_ = [(n, _P) for n in ("xhat", "gamma", "invstd", "dgamma", "dbeta")] + [("accumulate", _I)]


_PP, _PI, _F = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.c_float
# In the structs below _PP / _PI members are HOST arrays (of device pointers / of ints): assign the ctypes array object itself, not its
# address — the struct then keeps the array alive for as long as it lives.


class SnFwdBatch(ctypes.Structure):
    """pcg_sn_fwd_batch."""
    _fields_ = ([("n", _I), ("reps", _I), ("power_iteration", _I), ("eps", _F), ("w_orig", _PP), ("out_features", _PI), ("in_features", _PI)] +
                [(n, _PP) for n in ("u", "v", "w_bar", "sigma", "u_used", "v_used")])


class SnBwdBatch(ctypes.Structure):
    """pcg_sn_bwd_batch."""
    _fields_ = [("n", _I), ("passes", _I), ("dw_bar", _PP), ("w_bar", _PP), ("out_features", _PI), ("in_features", _PI), ("u", _PP), ("v", _PP),
                ("sigma", _PP), ("dw_orig", _PP), ("accumulate", _PI), ("db_dst", _PP), ("db_src", _PP)]


class HouseCriticFwdArgs(ctypes.Structure):
    """pcg_house_critic_fwd_args."""
    _fields_ = ([(n, _I) for n in ("n_pass", "B", "D", "NC")] + [("slope", _F)] +
                [(n, _PP) for n in ("x", "onehot", "w_bar", "bias", "a0", "a1", "a2", "a3", "out")])


class HouseCriticBwdArgs(ctypes.Structure):
    """pcg_house_critic_bwd_args."""
    _fields_ = ([(n, _I) for n in ("n_pass", "B", "D")] + [("slope", _F)] +
                [(n, _PP) for n in ("dout", "w_bar", "a1", "a2", "a3", "d3", "d2", "d1", "dx")])


class HouseClsFwdArgs(ctypes.Structure):
    """pcg_house_cls_fwd_args."""
    _fields_ = ([("x", _P), ("B", _I), ("w_kmajor", _PP), ("bias", _PP)] + [(n, _P) for n in ("a1", "a2", "a3", "a4", "logits", "ce_target")] +
                [("ce_grad_scale", _F), ("ce_dlogits", _P), ("ce_row_loss", _P)])


class HouseClsBwdArgs(ctypes.Structure):
    """pcg_house_cls_bwd_args."""
    _fields_ = [("dlogits", _P), ("B", _I), ("w_stored", _PP)] + [(n, _P) for n in ("a1", "a2", "a3", "a4", "dx")]


class HouseResFwdArgs(ctypes.Structure):
    """pcg_house_res_fwd_args."""
    _fields_ = ([("cont", _P), ("ncont", _I), ("samples", _P), ("seg_dev", _P), ("T", _I), ("norm", _P), ("x", _P), ("mask", _P), ("col_src", _PI),
                 ("D", _I), ("B", _I)] + [(n, _P) for n in ("res", "masked", "x_cf", "partial512", "ticket", "pen_out", "am_out")])


class HouseResBwdArgs(ctypes.Structure):
    """pcg_house_res_bwd_args."""
    _fields_ = ([(n, _P) for n in ("res", "masked", "mask", "gx_a", "gx_b")] + [("w_pen", _F), ("w_am", _F), ("ncont", _I), ("cont_idx_dev", _P),
                ("seg_dev", _P), ("S", _I), ("T", _I), ("cat_idx_dev", _P), ("norm", _P), ("D", _I), ("B", _I), ("dcont", _P), ("dsamples", _P)])


class HouseLossArgs(ctypes.Structure):
    """pcg_house_loss_args."""
    _fields_ = ([("d_real", _P), ("d_fake", _P), ("d_fake_g", _P), ("n", _I), ("g_cls", _P), ("am", _P), ("pen", _P)] +
                [(n, _F) for n in ("lambda_cls", "w_reg", "lambda_mask", "w_reg_log")] + [("ce_row_loss", _P), ("n_ce", _I), ("out6", _P)])


class HouseDiagArgs(ctypes.Structure):
    """pcg_house_diag_args."""
    _fields_ = ([(n, _P) for n in ("logits_cf", "logits_orig", "src_rows", "target_y", "masked")] + [("B", _I), ("nc", _I), ("D", _I), ("eps", _F),
                ("out4", _P), ("acc", _P)])


class DeltaGanEntryArgs(ctypes.Structure):
    """pcg_delta_gan_entry_args."""
    _fields_ = ([(n, _P) for n in ("x", "y", "target", "y_host", "target_host", "table_g", "table_d", "g_in", "d_in", "labels_2b", "head_w",
                                   "head_w_packed")] + [(n, _I) for n in ("B", "HW", "K", "mode", "head_C", "head_P")])


class DeltaGanTailFwdArgs(ctypes.Structure):
    """pcg_delta_gan_tail_fwd_args."""
    _fields_ = ([(n, _P) for n in ("x", "delta", "x_cf", "d_in", "loss_reg", "workspace")] + [("workspace_bytes", ctypes.c_size_t)] +
                [(n, _I) for n in ("B", "HW", "grid")])


class LogitHeadFwdArgs(ctypes.Structure):
    """pcg_logit_head_fwd_args."""
    _fields_ = [(n, _P) for n in ("a", "w", "bias", "logits", "loss", "dlogit", "db", "workspace")] + [(n, _I) for n in ("R", "F", "mode")]


class LogitHeadBwdArgs(ctypes.Structure):
    """pcg_logit_head_bwd_args."""
    _fields_ = [(n, _P) for n in ("a", "w", "dlogit", "da", "dw")] + [("slope", _F)] + [(n, _I) for n in ("R", "F", "dw_C", "dw_P")]


class DeltaGanTailBwdArgs(ctypes.Structure):
    """pcg_delta_gan_tail_bwd_args."""
    _fields_ = ([(n, _P) for n in ("dD", "dC", "delta", "d_delta")] + [("lambda_cls", _F), ("reg_scale", _F)] +
                [(n, _I) for n in ("B", "HW", "dD_stride")])


class DeltaCfEntryArgs(ctypes.Structure):
    """pcg_delta_cf_entry_args."""
    _fields_ = [(n, _P) for n in ("x", "table", "target", "target_host", "out")] + [(n, _I) for n in ("B", "T", "HW", "K", "q0", "nq")]


class DeltaCfTailArgs(ctypes.Structure):
    """pcg_delta_cf_tail_args."""
    _fields_ = [(n, _P) for n in ("delta", "x", "x_cf", "sums")] + [(n, _I) for n in ("B", "T", "HW", "q0", "nq")]


class DeltaGanTargetDrawArgs(ctypes.Structure):
    """pcg_delta_gan_target_draw_args."""
    _fields_ = [("target", _P), ("counter", _P), ("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("B", _I), ("K", _I)]


class ProbHeadFwdArgs(ctypes.Structure):
    """pcg_prob_head_fwd_args."""
    _fields_ = ([(n, _P) for n in ("a", "w", "bias", "logits", "prob", "loss", "dlogit", "db", "workspace")] +
                [("workspace_bytes", ctypes.c_size_t), ("eps", _F)] + [(n, _I) for n in ("R", "F", "mode", "slabs")])


class LogEpsLossArgs(ctypes.Structure):
    """pcg_log_eps_loss_args."""
    _fields_ = [(n, _P) for n in ("p", "grad_out", "loss", "dp")] + [("eps", _F), ("R", _I), ("mode", _I)]


class ImageSheetArgs(ctypes.Structure):
    """pcg_image_sheet_args."""
    _fields_ = ([(n, _P) for n in ("x", "range", "grid", "u8")] + [(n, _F) for n in ("lo", "hi", "d", "pad_value", "pre_scale", "pre_shift")] +
                [(n, _I) for n in ("N", "C", "H", "W", "nrow", "padding", "normalize", "gray")])


DELTA_GAN_BUILD, DELTA_GAN_REGATHER = 0, 1              # PCG_DELTA_GAN_* (include/pcgan_hip.h)
LOGIT_HEAD_D, LOGIT_HEAD_G = 0, 1                        # PCG_LOGIT_HEAD_*
DELTA_GAN_CHUNK = 1024                                   # PCG_DELTA_GAN_CHUNK
PROB_HEAD_D, PROB_HEAD_G = 0, 1                          # PCG_PROB_HEAD_*
PROB_HEAD_MAX_SLABS = 16                                 # PCG_PROB_HEAD_MAX_SLABS
CLASS_PICK_FIRST, CLASS_PICK_BEST = 0, 1                 # PCG_CLASS_PICK_*
CLASS_PICK_KMAX = 64                                     # PCG_CLASS_PICK_KMAX
CF_PANELS_GRID, CF_PANELS_PANELS = 0, 1                  # PCG_CF_PANELS_*

# typedef name in include/pcgan_hip.h -> its class here (pcg_abi_struct_bytes checks the sizes: tests/test_house_abi_host.py)
STRUCTS = {"pcg_conv_geom": ConvGeom, "pcg_conv_args": ConvArgs, "pcg_in_xform": InXform, "pcg_wgrad_item": WgradItem, "pcg_sn_fwd_batch": SnFwdBatch,
           "pcg_sn_bwd_batch": SnBwdBatch, "pcg_house_g_desc": HouseGDesc, "pcg_house_g_fwd_args": HouseGFwdArgs,
           "pcg_house_g_bwd_args": HouseGBwdArgs, "pcg_house_critic_fwd_args": HouseCriticFwdArgs,
           "pcg_house_critic_bwd_args": HouseCriticBwdArgs, "pcg_house_cls_fwd_args": HouseClsFwdArgs, "pcg_house_cls_bwd_args": HouseClsBwdArgs,
           "pcg_house_res_fwd_args": HouseResFwdArgs, "pcg_house_res_bwd_args": HouseResBwdArgs, "pcg_house_loss_args": HouseLossArgs,
           "pcg_house_diag_args": HouseDiagArgs, "pcg_moons_cf_desc": MoonsCfDesc, "pcg_moons_cf_train_args": MoonsCfTrainArgs,
           "pcg_moons_cf_fwd_args": MoonsCfFwdArgs, "pcg_moons_cf_eval_args": MoonsCfEvalArgs,
           "pcg_house_cf_eval_args": HouseCfEvalArgs, "pcg_patch_mask_bits_args": PatchMaskBitsArgs,
           "pcg_mnist_cf_entry_args": MnistCfEntryArgs, "pcg_mnist_cf_tail_args": MnistCfTailArgs,
           "pcg_mnist_cf_score_args": MnistCfScoreArgs, "pcg_dense_bn": DenseBn,
           "pcg_dense_bn_bwd": DenseBnBwd, "pcg_moons_gan_desc": MoonsGanDesc, "pcg_moons_gan_train_args": MoonsGanTrainArgs,
           "pcg_moons_gan_fwd_args": MoonsGanFwdArgs, "pcg_moons_clf_fit_desc": MoonsClfFitDesc,
           "pcg_moons_clf_fit_args": MoonsClfFitArgs, "pcg_delta_gan_entry_args": DeltaGanEntryArgs,
           "pcg_delta_gan_tail_fwd_args": DeltaGanTailFwdArgs, "pcg_logit_head_fwd_args": LogitHeadFwdArgs,
           "pcg_logit_head_bwd_args": LogitHeadBwdArgs, "pcg_delta_gan_tail_bwd_args": DeltaGanTailBwdArgs,
           "pcg_delta_cf_entry_args": DeltaCfEntryArgs, "pcg_delta_cf_tail_args": DeltaCfTailArgs,
           "pcg_delta_gan_target_draw_args": DeltaGanTargetDrawArgs, "pcg_prob_head_fwd_args": ProbHeadFwdArgs,
           "pcg_log_eps_loss_args": LogEpsLossArgs, "pcg_image_sheet_args": ImageSheetArgs}

_c = ctypes
_vp, _f, _i, _i64, _sz = _c.c_void_p, _c.c_float, _c.c_int, _c.c_int64, _c.c_size_t
_d = _c.c_double
_i32 = _c.c_int32
_gp = _c.POINTER(ConvGeom)
_xp = _c.POINTER(InXform)

# name -> (restype, argtypes); every symbol include/pcgan_hip.h declares
PROTOTYPES = {
    "pcg_abi_version": (_i, []),
    "pcg_abi_struct_bytes": (_sz, [_c.c_char_p]),
    "pcg_last_error": (_c.c_char_p, []),
    "pcg_target_arch": (_c.c_char_p, []),
    "pcg_tune_set": (_i, [_c.c_char_p, _i32]),
    "pcg_debug_stamp_buffer": (_i, [_vp, _i64]),
    "pcg_conv_plan_describe": (_i, [_c.POINTER(ConvGeom), _i32, _i32, _c.c_char_p, _sz]),
    "pcg_launch_plan_describe": (_i, [_i32, _c.POINTER(_i64), _i32, _c.c_char_p, _sz]),
    "pcg_conv_scratch_parts_bytes": (_sz, []),
    "pcg_conv_scratch_arrivals_bytes": (_sz, []),
    "pcg_conv_set_scratch": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "pcg_conv_reset_scratch": (_i, [_vp]),
    "pcg_conv_pixtab_bytes": (_sz, [_gp]),
    "pcg_conv_pixtab_register": (_i, [_gp, _vp, _sz, _vp]),
    "pcg_conv_cliptab_bytes": (_sz, [_gp]),
    "pcg_conv_cliptab_register": (_i, [_gp, _vp, _sz, _vp]),
    "pcg_conv_sched_model": (_d, [_vp, _i32]),
    "pcg_conv_pad_clip_query": (_i, [_gp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "pcg_conv_wgrad_padskip_query": (_i, [_gp, _i32, _vp, _vp]),
    "pcg_conv_wgrad_padskip_plan": (_i, [_gp, _i32, _vp, _vp]),
    "pcg_bn_apply_act_g": (_i, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i, _f, _vp, _i32, _vp]),
    "pcg_conv2d_dgrad_bn_phases": (_i32, [_gp]),
    "pcg_bn_bwd_partial_g_workspace_bytes": (_sz, [_i32, _i32]),
    "pcg_bn_bwd_partial_g": (_i, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i, _i32, _vp, _sz, _vp]),
    "pcg_bn_act_bwd_g_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "pcg_bn_act_bwd_premask_g": (_i, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i32, _vp, _sz, _vp]),
    "pcg_bce_pair": (_i, [_vp, _i64, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcg_conv2d_fwd_bnbwd_thin_ok": (_i32, [_gp]),
    "pcg_conv2d_fwd_bnbwd_thin_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d_fwd_bnbwd_thin": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_conv2d_bnin_full_ok": (_i32, [_gp, _i32]),
    "pcg_conv2d_fwd_bnin_full": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i32, _vp, _vp, _i, _f, _vp, _vp]),
    "pcg_conv2d_wgrad_bnin_full": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _i, _f, _i32, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_conv_precision_set": (_i, [_i32]),
    "pcg_conv_precision_get": (_i32, []),
    "pcg_slab_defer_begin": (_i, [_vp]),
    "pcg_slab_defer_flush": (_i, [_vp]),
    "pcg_slab_defer_pending": (_i32, []),
    "pcg_conv2d_dgrad_bnbwd_full_ok": (_i32, [_gp, _i32]),
    "pcg_conv2d_dgrad_bnbwd_full_workspace_bytes": (_sz, [_gp, _i32]),
    "pcg_conv2d_dgrad_bnbwd_full": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i32, _vp, _sz, _vp]),
    "pcg_calib_mfma_blocks": (_i32, [_i32]),
    "pcg_calib_mfma_workspace_bytes": (_sz, [_i32]),
    "pcg_calib_mfma": (_i, [_i32, _i32, _vp, _sz, _c.POINTER(_d), _c.POINTER(_c.c_uint64), _vp]),
    "pcg_calib_copy": (_i, [_vp, _vp, _i64, _vp]),
    "pcg_conv2d_fwd_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d_dgrad_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d": (_i, [_gp, _c.POINTER(ConvArgs), _vp]),
    "pcg_conv2d_fwd": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pcg_conv2d_dgrad": (_i, [_gp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pcg_conv2d_fwd_bn_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d_dgrad_bn_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d_dgrad_mask_thin_ok": (_i32, [_gp]),
    "pcg_conv2d_xf_thin_ok": (_i32, [_gp]),
    "pcg_conv2d_fwd_bn_partial_rows": (_c.c_int32, [_gp]),
    "pcg_conv2d_dgrad_bn_partial_rows": (_c.c_int32, [_gp]),
    "pcg_bn_bwd_partial_workspace_bytes": (_sz, [_c.c_int32]),
    "pcg_bn_bwd_partial": (_i, [_vp, _vp, _i64, _c.c_int32, _vp, _vp, _vp, _vp, _c.c_int32, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_conv2d_wgrad_xf": (_i, [_gp, _vp, _xp, _vp, _xp, _vp, _i, _vp, _sz, _vp]),
    "pcg_bn_train_stats_coef": (_i, [_vp, _i64, _c.c_int32, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pcg_bn_db_workspace_bytes": (_sz, [_i64, _c.c_int32]),
    "pcg_bn_act_bwd_db": (_i, [_vp, _vp, _vp, _i64, _c.c_int32, _vp, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "pcg_bn_bwd_partial_db_workspace_bytes": (_sz, [_c.c_int32]),
    "pcg_bn_bwd_partial_db": (_i, [_vp, _vp, _i64, _c.c_int32, _vp, _vp, _vp, _vp, _c.c_int32, _f, _vp, _vp, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "pcg_conv_weight_adjoint": (_i, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pcg_conv_weight_adjoint_many": (_i, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "pcg_house_losses": (_i, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _vp]),
    "pcg_dp_unique_id": (_i, [_vp]),
    "pcg_dp_init": (_i, [_vp, _i32, _i32]),
    "pcg_dp_world": (_i32, []),
    "pcg_dp_rank": (_i32, []),
    "pcg_dp_side_stream": (_vp, []),
    "pcg_dp_allreduce": (_i, [_vp, _i64, _vp]),
    "pcg_dp_allreduce_begin": (_i, [_vp, _i64, _i32, _vp]),
    "pcg_dp_record": (_i, [_i32]),
    "pcg_dp_allreduce_wait": (_i, [_i32, _vp]),
    "pcg_dp_allreduce_sum_f64": (_i, [_vp, _i64, _vp]),
    "pcg_dp_broadcast": (_i, [_vp, _i64, _i32, _vp]),
    "pcg_dp_sync_batchnorm": (_i, [_i32]),
    "pcg_dp_barrier": (_i, [_vp]),
    "pcg_dp_rccl_version": (_i32, []),
    "pcg_dp_shutdown": (_i, []),
    "pcg_conv2d_wgrad_workspace_bytes": (_sz, [_gp]),
    "pcg_conv2d_wgrad": (_i, [_gp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_colsum_workspace_bytes": (_sz, [_i64, _c.c_int32]),
    "pcg_colsum": (_i, [_vp, _i64, _c.c_int32, _vp, _i, _vp, _sz, _vp]),
    "pcg_bn_workspace_bytes": (_sz, [_i64, _c.c_int32]),
    "pcg_bn_train_stats": (_i, [_vp, _i64, _c.c_int32, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "pcg_bn_apply_act": (_i, [_vp, _i64, _c.c_int32, _vp, _vp, _f, _vp, _vp, _i, _f, _vp, _f, _vp, _vp]),
    "pcg_bn_act_bwd": (_i, [_vp, _vp, _vp, _i64, _c.c_int32, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_bn_act_bwd_premask": (_i, [_vp, _vp, _i64, _c.c_int32, _vp, _vp, _vp, _vp, _i, _f, _f, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "pcg_embed_concat_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _vp]),
    "pcg_embed_concat_bwd": (_i, [_vp, _vp, _vp, _vp, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _i, _vp]),
    "pcg_embed_table_grad": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i, _vp]),
    "pcg_gather_channel": (_i, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "pcg_axpby": (_i, [_vp, _f, _vp, _f, _vp, _i64, _vp]),
    "pcg_scale_mask_fwd": (_i, [_vp, _vp, _f, _vp, _vp, _i64, _vp]),
    "pcg_scale_mask_bwd": (_i, [_vp, _vp, _vp, _f, _vp, _i64, _vp]),
    "pcg_clamp_add_fwd": (_i, [_vp, _vp, _f, _f, _vp, _i64, _vp]),
    "pcg_clamp_add_bwd": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i64, _vp]),
    "pcg_abs_mean_workspace_bytes": (_sz, []),
    "pcg_abs_mean_fwd": (_i, [_vp, _vp, _i, _i64, _vp, _vp, _sz, _vp]),
    "pcg_abs_mean_bwd": (_i, [_vp, _vp, _i, _i64, _vp, _f, _vp, _i, _vp]),
    "pcg_avgpool_fwd": (_i, [_vp, _vp, _c.c_int32, _c.c_int32, _c.c_int32, _vp]),
    "pcg_avgpool_bwd": (_i, [_vp, _vp, _c.c_int32, _c.c_int32, _c.c_int32, _vp]),
    "pcg_cross_entropy_fwd_bwd": (_i, [_vp, _vp, _c.c_int32, _c.c_int32, _f, _vp, _vp, _vp, _vp]),
    "pcg_act_fwd": (_i, [_vp, _i64, _i, _f, _vp, _vp]),
    "pcg_act_bwd": (_i, [_vp, _vp, _i64, _i, _f, _vp, _vp]),
    "pcg_bce_fwd_bwd": (_i, [_vp, _vp, _f, _i64, _f, _vp, _vp, _vp, _vp]),
    "pcg_bce_logits_fwd_bwd": (_i, [_vp, _f, _i64, _f, _vp, _vp, _vp, _vp]),
    "pcg_adam_step": (_i, [_vp, _vp, _vp, _vp, _i64, _d, _d, _d, _d, _d, _i, _i64, _vp]),
    "pcg_adam_step_capturable": (_i, [_vp, _vp, _vp, _vp, _i64, _d, _d, _d, _d, _d, _i, _vp, _vp, _vp]),
    "pcg_patch_mask": (_i, [_vp, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_int32, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_randint": (_i, [_vp, _i64, _c.c_int32, _c.c_int32, _vp, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_randn": (_i, [_vp, _i64, _f, _f, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_fill": (_i, [_vp, _i64, _f, _vp]),
    "pcg_add_bias_rows": (_i, [_vp, _i64, _i32, _vp, _vp]),
    "pcg_sumsq": (_i, [_vp, _i64, _vp, _i, _vp]),
    "pcg_norm_sum": (_i, [_vp, _vp, _i32, _vp, _vp]),
    "pcg_instnorm_fwd": (_i, [_vp, _i32, _i32, _i32, _vp, _vp, _f, _i, _f, _vp, _vp, _vp, _vp]),
    "pcg_instnorm_bwd": (_i, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcg_instnorm_bwd_bwd": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcg_instnorm_bwd_fused": (_i, [_vp, _vp, _f, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcg_instnorm_bwd_bwd_act": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "pcg_rowsum3": (_i, [_i32, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i32, _i32, _vp]),
    "pcg_nhwc_to_nchw_flat": (_i, [_vp, _vp, _i32, _i32, _i32, _i, _vp]),
    "pcg_interpolate": (_i, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "pcg_interpolate_stack": (_i, [_vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "pcg_gradient_penalty_fwd": (_i, [_vp, _i32, _i32, _f, _vp, _vp, _vp]),
    "pcg_gradient_penalty_bwd": (_i, [_vp, _vp, _vp, _i32, _i32, _f, _vp, _vp]),
    "pcg_rand_uniform": (_i, [_vp, _i64, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_cross_entropy_weighted_fwd_bwd": (_i, [_vp, _vp, _vp, _i32, _i32, _f, _vp, _vp, _vp, _vp]),
    "pcg_dropout_apply": (_i, [_vp, _vp, _i64, _i32, _i32, _f, _vp, _vp]),
    "pcg_rand_bernoulli": (_i, [_vp, _i64, _f, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_resize8_normalize": (_i, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _f, _f, _vp, _vp]),
    "pcg_house_g_fwd": (_i, [_c.POINTER(HouseGDesc), _c.POINTER(HouseGFwdArgs), _vp]),
    "pcg_house_g_bwd": (_i, [_c.POINTER(HouseGDesc), _c.POINTER(HouseGBwdArgs), _vp]),
    "pcg_weighted_sum_fwd": (_i, [_i32, _vp, _vp, _vp, _vp]),
    "pcg_weighted_sum_bwd": (_i, [_i32, _vp, _vp, _vp, _vp]),
    "pcg_cf_metrics": (_i, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "pcg_gemm": (_i, [_i, _i, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i, _vp]),
    "pcg_linear_wgrad_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "pcg_linear_wgrad_ticket_count": (_i32, []),
    "pcg_linear_wgrad": (_i, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i, _i, _vp, _sz, _vp, _vp]),
    "pcg_spectral_norm_fwd_batched": (_i, [_c.POINTER(SnFwdBatch), _vp]),
    "pcg_spectral_norm_bwd_batched": (_i, [_c.POINTER(SnBwdBatch), _vp]),
    "pcg_house_critic_fwd": (_i, [_c.POINTER(HouseCriticFwdArgs), _vp]),
    "pcg_house_critic_bwd": (_i, [_c.POINTER(HouseCriticBwdArgs), _vp]),
    "pcg_house_classifier_fwd": (_i, [_c.POINTER(HouseClsFwdArgs), _c.POINTER(SnBwdBatch), _vp]),
    "pcg_house_classifier_bwd": (_i, [_c.POINTER(HouseClsBwdArgs), _c.POINTER(SnFwdBatch), _vp]),
    "pcg_house_cf_eval": (_i, [_c.POINTER(HouseGDesc), _c.POINTER(HouseCfEvalArgs), _vp]),
    "pcg_patch_mask_bits": (_i, [_c.POINTER(PatchMaskBitsArgs), _vp]),
    "pcg_mnist_cf_entry": (_i, [_c.POINTER(MnistCfEntryArgs), _vp]),
    "pcg_mnist_cf_tail": (_i, [_c.POINTER(MnistCfTailArgs), _vp]),
    "pcg_mnist_cf_score": (_i, [_c.POINTER(MnistCfScoreArgs), _vp]),
    "pcg_house_residual_fwd": (_i, [_c.POINTER(HouseResFwdArgs), _c.POINTER(SnFwdBatch), _vp]),
    "pcg_house_residual_bwd": (_i, [_c.POINTER(HouseResBwdArgs), _c.POINTER(HouseLossArgs), _c.POINTER(HouseDiagArgs), _vp]),
    "pcg_house_diag": (_i, [_c.POINTER(HouseDiagArgs), _vp]),
    "pcg_house_draws": (_i, [_vp, _i32, _i32, _vp, _c.c_uint64, _vp, _i32, _vp, _i32, _c.c_uint64, _vp, _i32, _c.c_uint64, _c.c_uint64, _vp, _vp, _vp]),
    "pcg_house_draws_counter": (_i, [_vp, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _c.c_uint64, _vp, _vp, _vp, _vp]),
    "pcg_house_batch_draws_counter": (_i, [_vp, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _c.c_uint64,
                                           _vp, _vp, _vp, _vp]),
    "pcg_linear_wgrad_grouped_slabs": (_i32, [_i32]),
    "pcg_linear_wgrad_grouped_workspace_bytes": (_sz, [_i32, _c.POINTER(WgradItem), _i32]),
    "pcg_linear_wgrad_grouped": (_i, [_c.POINTER(WgradItem), _i32, _i32, _vp, _sz, _vp, _vp]),
    "pcg_gemm_act": (_i, [_i, _i, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i, _i, _f, _vp]),
    "pcg_onehot": (_i, [_vp, _i32, _i32, _vp, _vp]),
    "pcg_concat_cols": (_i, [_vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "pcg_split_cols": (_i, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "pcg_film_fwd": (_i, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "pcg_film_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "pcg_gumbel_softmax_fwd": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _f, _vp, _vp, _vp]),
    "pcg_rand_gumbel": (_i, [_vp, _i64, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_feature_mask": (_i, [_vp, _i32, _i32, _vp, _i32, _c.c_uint64, _c.c_uint64, _vp]),
    "pcg_gumbel_softmax_bwd": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _f, _vp, _vp]),
    "pcg_assemble_residual_fwd": (_i, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "pcg_assemble_residual_bwd": (_i, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "pcg_mean_workspace_bytes": (_sz, []),
    "pcg_mean_fwd": (_i, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "pcg_mean_bwd": (_i, [_vp, _f, _i64, _vp, _vp]),
    "pcg_moons_cf_scratch_bytes": (_sz, [_c.POINTER(MoonsCfDesc), _i32]),
    "pcg_moons_cf_train_steps": (_i, [_c.POINTER(MoonsCfDesc), _c.POINTER(MoonsCfTrainArgs), _i32, _vp]),
    "pcg_moons_cf_forward": (_i, [_c.POINTER(MoonsCfDesc), _c.POINTER(MoonsCfFwdArgs), _vp]),
    "pcg_moons_cf_eval": (_i, [_c.POINTER(MoonsCfDesc), _c.POINTER(MoonsCfEvalArgs), _vp]),
    "pcg_moons_gan_scratch_bytes": (_sz, [_c.POINTER(MoonsGanDesc)]),
    "pcg_moons_gan_train_steps": (_i, [_c.POINTER(MoonsGanDesc), _c.POINTER(MoonsGanTrainArgs), _i32, _vp]),
    "pcg_moons_gan_forward": (_i, [_c.POINTER(MoonsGanDesc), _c.POINTER(MoonsGanFwdArgs), _vp]),
    "pcg_moons_clf_fit_scratch_bytes": (_sz, [_c.POINTER(MoonsClfFitDesc)]),
    "pcg_moons_clf_fit": (_i, [_c.POINTER(MoonsClfFitDesc), _c.POINTER(MoonsClfFitArgs), _i32, _vp]),
    "pcg_dense_rows_fwd": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _c.POINTER(DenseBn), _i, _f, _vp, _vp]),
    "pcg_dense_rows_dgrad": (_i, [_vp, _vp, _i32, _i32, _i32, _i, _f, _vp, _c.POINTER(DenseBnBwd), _vp, _vp]),
    "pcg_dense_rows_wgrad": (_i, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i, _vp]),
    "pcg_dense_rows_fwd_post": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _i, _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "pcg_dense_rows_dgrad_post": (_i, [_vp, _vp, _i32, _i32, _i32, _vp, _f, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _vp, _vp]),
    "pcg_ce_weighted_tally": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pcg_house_clf_batch": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _f, _vp, _i32, _f, _vp, _i32, _f, _c.c_uint64,
                                 _c.c_uint64, _i64, _vp]),
    "pcg_house_clf_batch_counter": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _f, _vp, _i32, _f, _vp, _i32, _f, _c.c_uint64,
                                         _vp, _vp]),
    "pcg_mnist_clf_batch": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _f, _vp, _i32, _f, _c.c_uint64, _c.c_uint64, _i64,
                                 _vp]),
    "pcg_mnist_clf_batch_counter": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _f, _vp, _i32, _f, _c.c_uint64, _vp, _vp]),
    "pcg_drop2d_flatten_fwd": (_i, [_vp, _vp, _f, _i32, _i32, _i32, _vp, _vp]),
    "pcg_drop2d_flatten_bwd": (_i, [_vp, _vp, _f, _vp, _i, _f, _i32, _i32, _i32, _vp, _vp]),
    "pcg_relu_maxpool2_fwd": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pcg_relu_maxpool2_bwd": (_i, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pcg_mnist_clf_head": (_i, [_vp, _vp, _f, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcg_delta_gan_entry": (_i, [_c.POINTER(DeltaGanEntryArgs), _vp]),
    "pcg_delta_gan_tail_workspace_bytes": (_sz, [_i32, _i32]),
    "pcg_delta_gan_tail_fwd": (_i, [_c.POINTER(DeltaGanTailFwdArgs), _vp]),
    "pcg_logit_head_fwd": (_i, [_c.POINTER(LogitHeadFwdArgs), _vp]),
    "pcg_logit_head_bwd": (_i, [_c.POINTER(LogitHeadBwdArgs), _vp]),
    "pcg_delta_gan_tail_bwd": (_i, [_c.POINTER(DeltaGanTailBwdArgs), _vp]),
    "pcg_delta_cf_entry": (_i, [_c.POINTER(DeltaCfEntryArgs), _vp]),
    "pcg_delta_cf_tail": (_i, [_c.POINTER(DeltaCfTailArgs), _vp]),
    "pcg_delta_gan_target_draw": (_i, [_c.POINTER(DeltaGanTargetDrawArgs), _vp]),
    "pcg_prob_head_workspace_bytes": (_sz, [_i32, _i32]),
    "pcg_prob_head_fwd": (_i, [_c.POINTER(ProbHeadFwdArgs), _vp]),
    "pcg_log_eps_loss_fwd_bwd": (_i, [_c.POINTER(LogEpsLossArgs), _vp]),
    "pcg_class_pick": (_i, [_vp, _vp, _vp, _i32, _i32, _i32, _i64, _i32, _vp]),
    "pcg_class_pick_gather": (_i, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp]),
    "pcg_cf_panels": (_i, [_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "pcg_image_range_workspace_bytes": (_sz, []),
    "pcg_image_range": (_i, [_vp, _i64, _f, _f, _vp, _vp, _sz, _vp]),
    "pcg_image_sheet": (_i, [_c.POINTER(ImageSheetArgs), _vp]),
    "pcg_spectral_norm_fwd": (_i, [_vp, _i32, _i32, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "pcg_spectral_norm_bwd": (_i, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i, _vp]),
}

_lib = None


def load():
    """Load the library (once) and attach prototypes.  Raises PcgError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PcgError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {os.path.join(_HERE, 'csrc')}` — there is no CPU/PyTorch fallback path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_TRACE = os.environ.get("PCG_TRACE_OPS")     # diagnostic: a file; every library call is followed by a device synchronise and logged there


def check(rc, what=""):
    if rc != PCG_OK:
        msg = load().pcg_last_error().decode("utf-8", "replace")
        raise PcgError(f"{what or 'libpcgan_hip'} failed (status {rc}): {msg}")
    if _TRACE:      # (a faulting kernel is then the call AFTER the last line of the file)
        with open(_TRACE, "a") as f:
            f.write(f"{what} issued\n")
        torch.cuda.synchronize()
        with open(_TRACE, "a") as f:
            f.write(f"{what} done\n")
