"""Short names of the library's kernels for profile summaries and resource tables (no torch, no GPU).

The implicit-GEMM conv kernels are templates over TileCfg<BM, BN, WAVES_M, WAVES_N[, SWZ, MINW, PF, BF16]>
(promptable-counterfactual-gan_amd/csrc/igemm_core.h); their demangled names are long and differ only in those arguments.
short_kernel_name() prints the tile as BMxBN, "/swz3" for the three-workgroups-per-CU configuration (MINW = 6: swizzled unpadded
LDS images in fp32) and ",bf16" for a bf16-operand twin, which keeps its fp32 configuration's launch bounds and so its name."""
import re

_TILE_CFG = re.compile(r"pcg::TileCfg<(\d+), (\d+), \d+, \d+(?:, (?:true|false), (\d+), \d+(?:, (true|false))?)?>")


def _tile(m):
    bm, bn, minw, bf16 = m.groups()
    return f"{bm}x{bn}" + ("/swz3" if minw and int(minw) >= 6 else "") + (",bf16" if bf16 == "true" else "")


def short_kernel_name(name):
    """'void pcg::(anonymous namespace)::conv_fwd_kernel<pcg::TileCfg<128, 64, 2, 2, true, 6, 1, false>, true>(pcg::ConvP)'
    -> 'conv_fwd_kernel<128x64/swz3, true>'"""
    name = name.replace("pcg::(anonymous namespace)::", "").replace("void ", "")
    return _TILE_CFG.sub(_tile, name).replace(" >", ">").split("(")[0]
