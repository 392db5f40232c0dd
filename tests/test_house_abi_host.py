"""CPU: the struct-based ABI of the tabular step (include/pcgan_hip.h: pcg_sn_*_batch, pcg_house_*_args).  The layouts of the ctypes
classes against the library's own sizeof, and the refusals the entry points make before any HIP call — no device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null "device pointer": every call below is refused before anything could read it


def _header_structs():
    text = open(os.path.join(ROOT, "include", "pcgan_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(re.findall(r"typedef\s+struct\b[^{;]*\{[^}]*\}\s*(pcg_[a-z0-9_]+)\s*;", text))


def test_every_struct_of_the_header_has_the_size_its_ctypes_class_has():
    """Sizes only: a missing, extra or wrongly typed member shows, two swapped members of one type do not — the member ORDER of a
    ctypes class is checked against the header by reading, and by the GPU tests that launch through it."""
    from pcgan_amd import _lib
    lib = _lib.load()
    names = _header_structs()
    assert len(names) >= 25 and "pcg_sn_fwd_batch" in names and "pcg_dense_bn" in names and "pcg_conv_geom" in names
    assert sorted(_lib.STRUCTS) == names
    for name in names:
        assert lib.pcg_abi_struct_bytes(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0, name
    assert lib.pcg_abi_struct_bytes(b"pcg_no_such_struct") == 0 and lib.pcg_abi_struct_bytes(None) == 0


def _refused(lib, rc, entry):
    from pcgan_amd import _lib
    msg = lib.pcg_last_error().decode()
    assert rc != _lib.PCG_OK and msg.startswith(entry + ":"), (entry, rc, msg)
    return msg


def _ptrs(n, value=FAKE):
    return (ctypes.c_void_p * n)(*[value] * n)


def _sn_fwd(_lib, n, reps, power_iteration=1):
    i32 = (ctypes.c_int32 * n)(*[8] * n)
    return _lib.SnFwdBatch(n=n, reps=reps, power_iteration=power_iteration, eps=1e-12, w_orig=_ptrs(n), out_features=i32, in_features=i32,
                           u=_ptrs(n), v=_ptrs(n), w_bar=_ptrs(n * reps), sigma=_ptrs(n * reps), u_used=_ptrs(n * reps), v_used=_ptrs(n * reps))


def _sn_bwd(_lib, n, passes):
    i32 = (ctypes.c_int32 * n)(*[8] * n)
    return _lib.SnBwdBatch(n=n, passes=passes, dw_bar=_ptrs(n * passes), w_bar=_ptrs(n * passes), out_features=i32, in_features=i32,
                           u=_ptrs(n * passes), v=_ptrs(n * passes), sigma=_ptrs(n * passes), dw_orig=_ptrs(n), accumulate=i32)


def _fill(struct, **scalars):
    """Every pointer member = FAKE, every other member 1 unless given: an argument struct that passes the null checks."""
    for name, typ in struct._fields_:
        if name in scalars:
            setattr(struct, name, scalars[name])
        elif typ is ctypes.c_void_p:
            setattr(struct, name, FAKE)
        elif typ in (ctypes.c_int32, ctypes.c_float):
            setattr(struct, name, 1)
    return struct


def test_null_argument_struct_refused_by_each_of_the_nine_entries():
    from pcgan_amd import _lib
    lib = _lib.load()
    for entry, nargs in (("pcg_spectral_norm_fwd_batched", 1), ("pcg_spectral_norm_bwd_batched", 1), ("pcg_house_critic_fwd", 1),
                         ("pcg_house_critic_bwd", 1), ("pcg_house_classifier_fwd", 2), ("pcg_house_classifier_bwd", 2),
                         ("pcg_house_residual_fwd", 2), ("pcg_house_residual_bwd", 3), ("pcg_house_diag", 1)):
        assert "null argument struct" in _refused(lib, getattr(lib, entry)(*([None] * nargs), None), entry)


def test_spectral_norm_batch_limits_refused():
    from pcgan_amd import _lib
    lib = _lib.load()
    assert "at most 8" in _refused(lib, lib.pcg_spectral_norm_fwd_batched(_sn_fwd(_lib, 3, 3), None), "pcg_spectral_norm_fwd_batched")
    assert "training mode" in _refused(lib, lib.pcg_spectral_norm_fwd_batched(_sn_fwd(_lib, 2, 2, power_iteration=0), None),
                                       "pcg_spectral_norm_fwd_batched")
    assert "at most 8" in _refused(lib, lib.pcg_spectral_norm_bwd_batched(_sn_bwd(_lib, 3, 3), None), "pcg_spectral_norm_bwd_batched")
    # the same limits hold for a batch that rides in another launch
    cls_bwd = _fill(_lib.HouseClsBwdArgs(), w_stored=_ptrs(5))
    assert "at most 8" in _refused(lib, lib.pcg_house_classifier_bwd(cls_bwd, _sn_fwd(_lib, 3, 3), None), "pcg_spectral_norm_fwd_batched")


def test_critic_pass_count_refused():
    from pcgan_amd import _lib
    lib = _lib.load()
    arr = {n: _ptrs(3) for n in ("x", "onehot", "bias", "a0", "a1", "a2", "a3", "out", "dout", "d3", "d2", "d1", "dx")}
    f = _lib.HouseCriticFwdArgs(n_pass=3, B=5, D=17, NC=4, slope=0.2, w_bar=_ptrs(12),
                                **{k: arr[k] for k in ("x", "onehot", "bias", "a0", "a1", "a2", "a3", "out")})
    assert "1 or 2 passes" in _refused(lib, lib.pcg_house_critic_fwd(f, None), "pcg_house_critic_fwd")
    b = _lib.HouseCriticBwdArgs(n_pass=3, B=5, D=17, slope=0.2, w_bar=_ptrs(12), **{k: arr[k] for k in ("dout", "a1", "a2", "a3", "d3", "d2", "d1", "dx")})
    assert "1 or 2 passes" in _refused(lib, lib.pcg_house_critic_bwd(b, None), "pcg_house_critic_bwd")


def test_cross_entropy_tail_refusals():
    from pcgan_amd import _lib
    lib = _lib.load()
    c = _fill(_lib.HouseClsFwdArgs(), B=5, w_kmajor=_ptrs(5), bias=_ptrs(5))
    assert "needs a rider" in _refused(lib, lib.pcg_house_classifier_fwd(c, None, None), "pcg_house_classifier_fwd")
    c.ce_dlogits = FAKE + 4                                                                   # off 16-byte alignment
    assert "16-byte aligned" in _refused(lib, lib.pcg_house_classifier_fwd(c, _sn_bwd(_lib, 4, 2), None), "pcg_house_classifier_fwd")


def test_residual_backward_rider_refusals():
    from pcgan_amd import _lib
    lib = _lib.load()
    r = _fill(_lib.HouseResBwdArgs(), B=20000, D=17)
    d = _fill(_lib.HouseDiagArgs(), B=20000, nc=4, D=17)
    assert "ride with the logged scalars" in _refused(lib, lib.pcg_house_residual_bwd(r, None, d, None), "pcg_house_residual_bwd")
    lo = _fill(_lib.HouseLossArgs(), n=16385)
    assert "at most 16384 rows" in _refused(lib, lib.pcg_house_residual_bwd(r, lo, None, None), "pcg_house_residual_bwd")
    assert "at most 16384 rows" in _refused(lib, lib.pcg_house_residual_bwd(r, lo, d, None), "pcg_house_residual_bwd")


@pytest.mark.parametrize("overlap", ["critic", "both", 2, None, ""])
def test_graphed_step_refuses_unknown_overlap_values(overlap):
    """Before anything touches a device: the nets and the normalisation table are never looked at."""
    from pcgan_amd import PcgError, house as H
    with pytest.raises(PcgError, match="overlap must be"):
        H.GraphedTrainStep(None, None, None, None, None, None, 128, overlap=overlap)


def _g_desc(_lib, widths, ncont, **over):
    d = _lib.HouseGDesc(nheads=len(widths), ncont=ncont, D=17, NC=4, hidden=32, nblocks=5)
    for s, w in enumerate(widths):
        d.seg[s + 1] = d.seg[s] + w
    for k, v in over.items():
        setattr(d, k, v)
    return d


# descriptors pcg_house_g_fwd and pcg_house_g_bwd refuse before any launch (csrc/house_fused.hip: desc_ok), and a word of the message
BAD_G_DESCS = [
    ("nheads = 0", [], 10, "nheads = 0"),                      # T = 0: tile_walk would divide by it
    ("ncont = 0", [9, 30], 0, "ncont = 0"),                    # never run by the fused kernels: the module takes the op chain
    ("9 heads", [2] * 8, 1, "nheads = 9"),                     # (made 9 below: seg has 9 entries)
    ("a 33-wide head", [33, 5], 4, "1 .. 32 columns wide"),
    ("an empty head", [5, 0, 5], 4, "1 .. 32 columns wide"),
    ("T = 97", [32, 32, 32, 1], 1, "T = 97"),
    ("T + ncont = 97", [32, 32, 31], 2, "T + ncont = 97"),
    ("ncont = 33", [9], 33, "ncont = 33"),
]


@pytest.mark.parametrize("what,widths,ncont,word", BAD_G_DESCS, ids=[b[0] for b in BAD_G_DESCS])
def test_generator_descriptor_refused_by_forward_and_backward(what, widths, ncont, word):
    """Every pointer is a fake non-null address and B = 5: a call that got past the descriptor checks would launch on them."""
    from pcgan_amd import _lib
    lib = _lib.load()
    d = _g_desc(_lib, widths, ncont)
    if what == "9 heads":
        d.nheads = 9
    f = _fill(_lib.HouseGFwdArgs(), B=5, running_mean=_ptrs(10), running_var=_ptrs(10), num_batches_tracked=_ptrs(10))
    b = _fill(_lib.HouseGBwdArgs(), B=5, accumulate=0)
    for entry, args in (("pcg_house_g_fwd", f), ("pcg_house_g_bwd", b)):
        assert word in _refused(lib, getattr(lib, entry)(d, args, None), entry), (what, entry)


def test_generator_descriptor_fixed_dimensions_refused_by_forward_and_backward():
    from pcgan_amd import _lib
    lib = _lib.load()
    f = _fill(_lib.HouseGFwdArgs(), B=5, running_mean=_ptrs(10), running_var=_ptrs(10), num_batches_tracked=_ptrs(10))
    b = _fill(_lib.HouseGBwdArgs(), B=5, accumulate=0)
    for over, word in ((dict(hidden=64), "hidden width 32"), (dict(nblocks=4), "5 residual blocks"), (dict(D=16), "input_dim 17"),
                       (dict(NC=3), "4 classes")):
        d = _g_desc(_lib, [9, 30, 6, 2, 5, 5, 13], 10, **over)
        for entry, args in (("pcg_house_g_fwd", f), ("pcg_house_g_bwd", b)):
            assert word in _refused(lib, getattr(lib, entry)(d, args, None), entry), (over, entry)
    # and the null-buffer check behind them still answers for a descriptor that passes
    d = _g_desc(_lib, [9, 30, 6, 2, 5, 5, 13], 10)
    f.soft = None
    b.Q = None
    assert "null buffer" in _refused(lib, lib.pcg_house_g_fwd(d, f, None), "pcg_house_g_fwd")
    assert "null buffer" in _refused(lib, lib.pcg_house_g_bwd(d, b, None), "pcg_house_g_bwd")


@pytest.mark.parametrize("cont,cats", [([], {0: 9, 1: 30}), (list(range(17)), {})], ids=["no continuous column", "no categorical head"])
def test_generator_without_heads_or_continuous_columns_takes_the_chain(cont, cats):
    """Neither _fused_ok nor _eval_dims_ok may send T = 0 or ncont = 0 to the fused kernels; the house configuration still goes."""
    from pcgan_amd import house as H
    G = H.ResidualGenerator(17, 32, 4, cont, cats)
    G.train()
    assert not G._fused_ok() and not G._eval_dims_ok()
    G = H.ResidualGenerator(17, 32, 4, H.CONFIG["continuous_idx"], H.CONFIG["categorical_info"])
    G.train()
    assert G._fused_ok() and G._eval_dims_ok()
