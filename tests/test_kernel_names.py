"""CPU: scripts/kernel_names.short_kernel_name on literal demangled kernel names of both operand precisions."""
from scripts.kernel_names import short_kernel_name

NS = "void pcg::(anonymous namespace)::"
CASES = {
    NS + "conv_fwd_kernel<pcg::TileCfg<128, 128, 2, 2, false, 4, 2, false>, false>(pcg::ConvP)": "conv_fwd_kernel<128x128, false>",
    NS + "conv_fwd_kernel<pcg::TileCfg<128, 128, 2, 2, false, 4, 2, true>, false>(pcg::ConvP)": "conv_fwd_kernel<128x128,bf16, false>",
    NS + "conv_fwd_kernel<pcg::TileCfg<128, 64, 2, 2, true, 6, 1, false>, true>(pcg::ConvP)": "conv_fwd_kernel<128x64/swz3, true>",
    NS + "conv_fwd_kernel<pcg::TileCfg<128, 64, 2, 2, false, 6, 1, true>, true>(pcg::ConvP)": "conv_fwd_kernel<128x64/swz3,bf16, true>",
    NS + "conv_dgrad_kernel<pcg::TileCfg<128, 64, 2, 2, false, 4, 2, false>, false>(pcg::ConvP, pcg::DgradPhases)":
        "conv_dgrad_kernel<128x64, false>",
    NS + "conv_dgrad_kernel<pcg::TileCfg<128, 64, 2, 2, false, 4, 2, true>, false>(pcg::ConvP, pcg::DgradPhases)":
        "conv_dgrad_kernel<128x64,bf16, false>",
    NS + "conv_fwd_kernel<pcg::TileCfg<64, 128, 1, 4, false, 4, 2, true>, true>(pcg::ConvP)": "conv_fwd_kernel<64x128,bf16, true>",
    NS + "conv_wgrad192_kernel<pcg::TileCfg<64, 192, 2, 2, false, 4, 2, false> >(pcg::ConvP, int, int, int, int)":
        "conv_wgrad192_kernel<64x192>",
    NS + "conv_wgrad_sk_kernel<pcg::TileCfg<128, 128, 2, 2, false, 4, 2, true>, false, true>(pcg::ConvP, pcg::SkPlan)":
        "conv_wgrad_sk_kernel<128x128,bf16, false, true>",
    # older traces spell the tile with its first four arguments only
    NS + "conv_fwd_kernel<pcg::TileCfg<128, 128, 2, 2>, false>(pcg::ConvP)": "conv_fwd_kernel<128x128, false>",
    # kernels without a tile configuration keep their name
    NS + "col2im_kernel(HIP_vector_type<float, 4u> const*, HIP_vector_type<float, 4u>*, float const*, int)": "col2im_kernel",
    "pcg::adam_kernel(float*, float const*, int)": "pcg::adam_kernel",
}


def test_short_kernel_names():
    for name, short in CASES.items():
        assert short_kernel_name(name) == short, name


def test_precisions_and_configs_stay_apart():
    assert len(set(map(short_kernel_name, CASES))) == len(CASES) - 1      # only the old 4-argument spelling repeats a name
