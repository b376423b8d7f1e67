"""mlp_activation_func without a GPU: the mapping module -> (kind, param), the refusals, the argument checks of every entry that takes an
activation (fake pointers, in the style of test_backward_tier_host.py), the shimmed oracle, and the kink condition of the backward cases."""
import ctypes as C
import math

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import _lib as L
from swin_unet_image_fusion_amd import modules as M
from tests import activation_cases as A
from tests.activation_oracle import shimmed

P = 4096   # a fake device pointer: every call here stops before a launch


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_every_case_maps_to_its_kind_and_parameter(case):
    kind, param = M._activation_of(case.make())
    assert kind == case.kind and param == pytest.approx(case.param, abs=0.0)
    act = M._act(case.make())
    assert (act.kind, act.param) == (case.kind, C.c_float(case.param).value)


def test_inplace_is_ignored_and_alpha_one_is_the_default_kind():
    assert M._activation_of(nn.ELU(inplace=True)) == M._activation_of(nn.ELU(alpha=1.0, inplace=False)) == (L.ACT_ELU1, 0.0)
    assert M._activation_of(nn.ReLU(inplace=True)) == (L.ACT_RELU, 0.0)
    assert M._activation_of(nn.LeakyReLU(0.2, inplace=True)) == (L.ACT_LEAKY_RELU, 0.2)
    assert M._activation_of(nn.SiLU(inplace=True)) == (L.ACT_SILU, 0.0)
    assert L.Activation().kind == L.ACT_ELU1 == 0                      # a zero-initialised descriptor is today's ELU(alpha = 1)
    assert L.BlockDesc(L.AttnDesc(8, 2, 4, 4, 4, 0), 32, 0, L.PREC_FAST).act.kind == 0 and L.BlockDesc(L.AttnDesc(), 1, 0, 0, 0).act.kind == 0
    assert L.ModelDesc().act.kind == 0


@pytest.mark.parametrize("bad", [nn.PReLU(), nn.Tanh(), nn.ELU(float("nan")), nn.LeakyReLU(float("inf")), nn.Identity()], ids=lambda m: type(m).__name__)
def test_other_modules_are_refused_with_the_supported_list(bad):
    with pytest.raises(NotImplementedError) as e:
        M._activation_of(bad)
    for name in ("nn.ELU", "nn.ReLU", "nn.LeakyReLU", "nn.GELU", "nn.SiLU"):
        assert name in str(e.value)


def test_version_is_unchanged_and_every_sibling_is_bound():
    lib = L.lib()
    assert lib.swf_version() == 1
    siblings = [n for n in L.SIGNATURES if n.endswith("_act")]
    assert len(siblings) == 15
    for n in siblings:
        assert L.SIGNATURES[n][1] == [C.POINTER(L.Activation)] + L.SIGNATURES[n[:-4]][1]


GOOD, UNKNOWN, NAN = L.Activation(L.ACT_GELU, 0.0), L.Activation(7, 0.0), L.Activation(L.ACT_LEAKY_RELU, float("nan"))


def _lin():
    return L.Linear(P, P)


def _stream_params():
    return L.BlockStreamParams(L.Norm(P, P), L.AttnParams(_lin(), _lin(), _lin(), _lin(), P), L.Norm(P, P), _lin(), _lin())


def _head():
    return L.HeadParams(*([P] * 8))


def _entries():
    """name -> (call(act, first), workspace-taking?): `first` replaces the first pointer argument (NULL probe)."""
    lib = L.lib()
    f1, f2, pp, sp, hp, nrm = _lin(), _lin(), L.PatchParams(_lin(), L.Norm(P, P)), _stream_params(), _head(), L.Norm(P, P)
    g = L.Linear(P, P)
    ref = lambda a: C.byref(a) if a is not None else None
    return {
        "swf_mlp_fwd_act": lambda a, x=P: lib.swf_mlp_fwd_act(ref(a), L.PREC_FP32, C.byref(sp), None, x, None, P, None, 64, 8, 32, None, 0, None),
        "swf_mlp_fwd_drop_act": lambda a, x=P: lib.swf_mlp_fwd_drop_act(ref(a), C.byref(f1), C.byref(f2), x, P, 64, 8, 32,
                                                                        C.byref(L.Dropout(1, 0.0, 0.0, 0.1)), 0, None, 0, None),
        "swf_mlp_bwd_opt_act": lambda a, x=P: lib.swf_mlp_bwd_opt_act(ref(a), C.byref(f1), C.byref(f2), x, P, P, C.byref(g), C.byref(g), 64, 8, 32, None, 0,
                                                                      None, None, None, 0, None),
        "swf_patch_merge_fwd_act": lambda a, x=P: lib.swf_patch_merge_fwd_act(ref(a), C.byref(pp), x, P, 1, 8, 8, 8, 16, 2, 2, 1, 1, None, 0, None),
        "swf_patch_unmerge_fwd_act": lambda a, x=P: lib.swf_patch_unmerge_fwd_act(ref(a), C.byref(pp), x, None, P, 1, 4, 4, 4, 4, 16, 8, 2, 2, 8, 8, None, 0,
                                                                                  None),
        "swf_patch_merge_fwd_prec_act": lambda a, x=P: lib.swf_patch_merge_fwd_prec_act(ref(a), L.PREC_FAST, C.byref(pp), C.byref(pp), x, P, P, P, 2, 8, 8, 8, 16,
                                                                                        2, 2, 4, 4, None, None, None, None, 0, None),
        "swf_patch_unmerge_fwd_prec_act": lambda a, x=P: lib.swf_patch_unmerge_fwd_prec_act(ref(a), L.PREC_FAST, C.byref(pp), C.byref(pp), x, P, None, None, P, P,
                                                                                            2, 8, 8, 5, 7, 16, 8, 2, 2, 9, 14, None, None, None, None, 0, None),
        "swf_patch_layer_bwd_opt_act": lambda a, x=P: lib.swf_patch_layer_bwd_opt_act(ref(a), C.byref(pp), x, P, P, C.byref(pp), 1, 8, 8, 8, 16, 2, 2, 1, None,
                                                                                      None, None, 0, None),
        "swf_final_head_fwd_act": lambda a, x=P: lib.swf_final_head_fwd_act(ref(a), C.byref(hp), x, P, P, 1, 8, 8, 3, None, 0, None),
        "swf_linear_fwd_prec_act": lambda a, x=P: lib.swf_linear_fwd_prec_act(ref(a), C.byref(f1), L.PREC_FAST, x, None, P, 64, 512, 8, 1, None, 0, None),
    }


@pytest.mark.parametrize("name", [
    "swf_mlp_fwd_act", "swf_mlp_fwd_drop_act", "swf_mlp_bwd_opt_act", "swf_patch_merge_fwd_act", "swf_patch_unmerge_fwd_act",
    "swf_patch_merge_fwd_prec_act", "swf_patch_unmerge_fwd_prec_act", "swf_patch_layer_bwd_opt_act", "swf_final_head_fwd_act",
    "swf_linear_fwd_prec_act"])
def test_workspace_entries_check_null_then_activation_then_workspace(name):
    call = _entries()[name]
    assert call(GOOD, None) == L.ERR_NULL
    assert call(UNKNOWN) == L.ERR_UNSUPPORTED and call(NAN) == L.ERR_UNSUPPORTED          # with no workspace at all: refused before it is looked at
    assert call(L.Activation(-1, 0.0)) == L.ERR_UNSUPPORTED
    assert call(GOOD) == L.ERR_WORKSPACE and call(None) == L.ERR_WORKSPACE and call(L.Activation()) == L.ERR_WORKSPACE
    assert call(L.Activation(L.ACT_RELU, float("nan"))) == L.ERR_WORKSPACE                # a parameter no kind reads is ignored, as for the default
    assert call(L.Activation(L.ACT_LEAKY_RELU, -0.5)) == L.ERR_WORKSPACE


def test_entries_without_a_workspace_check_null_then_activation():
    lib = L.lib()
    f1, nrm, hp = _lin(), L.Norm(P, P), _head()
    lin = lambda a, x=P: lib.swf_linear_fwd_act(C.byref(a), C.byref(f1), x, None, P, 0, 8, 8, 1, None)       # tokens = 0: BAD_SHAPE is the last check
    ln = lambda a, x=P: lib.swf_layernorm_fwd_act(C.byref(a), C.byref(nrm), x, P, 0, 8, 1, None)
    for call in (lin, ln):
        assert call(GOOD, None) == L.ERR_NULL and call(GOOD) == L.ERR_BAD_SHAPE
    # valid sizes, act / elu = 1 (a valid switch): only the descriptor is wrong, and it is refused before the launch a good one would reach
    for bad in (UNKNOWN, NAN, L.Activation(-1, 0.0)):
        assert lib.swf_linear_fwd_act(C.byref(bad), C.byref(f1), P, None, P, 4, 8, 8, 1, None) == L.ERR_UNSUPPORTED
        assert lib.swf_linear_fwd_act(C.byref(bad), C.byref(f1), P, None, P, 4, 8, 8, 0, None) == L.ERR_UNSUPPORTED     # checked even when not applied
        assert lib.swf_layernorm_fwd_act(C.byref(bad), C.byref(nrm), P, P, 4, 8, 1, None) == L.ERR_UNSUPPORTED
        assert lib.swf_layernorm_fwd_act(C.byref(bad), C.byref(nrm), P, P, 4, 8, 0, None) == L.ERR_UNSUPPORTED
    assert lib.swf_linear_fwd_act(C.byref(GOOD), C.byref(f1), P, None, P, 4, 8, 8, 2, None) == L.ERR_UNSUPPORTED        # the switch itself is 0 or 1
    # the head's backward entries: NULL, then the shape, then the activation; a good call would go on to read the BatchNorm scalars
    g = L.HeadGrads()
    bwd = lambda a, x=P, b=1: lib.swf_final_head_bwd_act(C.byref(a), C.byref(hp), x, P, P, P, P, C.byref(g), b, 8, 8, 3, 0, None, 0, None)
    sums = lambda a, x=P, b=1: lib.swf_final_head_bwd_sums_act(C.byref(a), C.byref(hp), x, P, P, P, b, 8, 8, 3, None, 0, None)
    sync = lambda a, x=P, b=1: lib.swf_final_head_bwd_synced_act(C.byref(a), C.byref(hp), x, P, P, P, 64, P, P, C.byref(g), b, 8, 8, 3, None, 0, None)
    for call in (bwd, sums, sync):
        assert call(GOOD, None) == L.ERR_NULL and call(GOOD, P, 0) == L.ERR_BAD_SHAPE
        assert call(UNKNOWN) == L.ERR_UNSUPPORTED and call(NAN) == L.ERR_UNSUPPORTED


def test_block_and_model_descriptors_carry_the_activation():
    lib = L.lib()
    four = (L.BlockStreamParams * 4)(*[_stream_params() for _ in range(4)])
    route = (C.c_int32 * 4)(-7, -7, -7, -7)

    def desc(act=None, prec=L.PREC_FAST, C_=24):
        d = L.BlockDesc(L.AttnDesc(C_, 8, C_ // 8, 8, 8, 0), 4 * C_, 0, prec, 0)
        if act is not None:
            d.act = act
        return d

    fwd = lambda d: lib.swf_basic_block_fwd_route(C.byref(d), four, four, P, P, P, P, 1, 8, 16, route, None, 0, None)
    stage = lambda d: lib.swf_block_stage_fwd_prec(C.byref(d), four, four, P, P, P, P, 1, 8, 16, None, None, route, None, 0, None)
    bwd = lambda d: lib.swf_basic_block_bwd_opt(C.byref(d), four, four, P, P, P, P, P, P, None, None, 1, 8, 16, None, None, None, None, 0, None)
    drop = lambda d: lib.swf_basic_block_fwd_drop(C.byref(d), four, four, P, P, P, P, 1, 8, 16, C.byref(L.Dropout(1, 0.1, 0.1, 0.1)), None, 0, None)
    half = lambda d: lib.swf_mlp_halfblock_fwd(C.byref(d), four, four, P, P, P, P, 1, 8, 16, None, 0, None)
    for call in (fwd, stage, bwd, drop, half):
        assert call(desc()) == L.ERR_WORKSPACE and call(desc(GOOD)) == L.ERR_WORKSPACE
        assert call(desc(UNKNOWN)) == L.ERR_UNSUPPORTED and call(desc(NAN)) == L.ERR_UNSUPPORTED
    assert list(route) == [-7] * 4
    # no workspace depends on the activation: the backward keeps u or act(u) in the one hidden buffer it always had
    for q in (lib.swf_basic_block_workspace_bytes, lib.swf_basic_block_bwd_workspace_bytes, lib.swf_basic_block_drop_workspace_bytes):
        for c in (24, 192):
            assert q(C.byref(desc(C_=c)), 2, 16, 16) == q(C.byref(desc(GOOD, C_=c)), 2, 16, 16) == q(C.byref(desc(L.Activation(), C_=c)), 2, 16, 16) > 0
    # a stage of a non-default activation packs no images (it runs the generic family), and no fused kernel is offered for it
    q = lib.swf_block_stage_prec_workspace_bytes
    assert 0 < q(C.byref(desc(GOOD)), 1, 2, 16, 16)
    assert lib.swf_basic_block_packed_bytes(C.byref(desc())) > 0 and lib.swf_basic_block_packed_bytes(C.byref(desc(GOOD))) == 0
    assert lib.swf_basic_block_pack(C.byref(desc(GOOD)), four, four, P, 1 << 30, None) == L.ERR_UNSUPPORTED
    assert lib.swf_basic_block_fwd_packed(C.byref(desc(GOOD)), P, P, P, P, P, 1, 8, 16, None) == L.ERR_UNSUPPORTED

    md = L.ModelDesc()
    md.levels, md.heads, md.mlp_ratio, md.win_h, md.win_w, md.merge_h, md.merge_w, md.head_ksize = 2, 2, 4, 4, 4, 2, 2, 3
    md.in_dims[0], md.in_dims[1], md.out_dims[0], md.out_dims[1], md.head_dim[0], md.head_dim[1] = 1, 8, 8, 16, 4, 8
    n0, ws0, arena0 = lib.swf_model_param_count(C.byref(md)), lib.swf_model_workspace_bytes(C.byref(md), 1, 16, 16), lib.swf_model_arena_elems(C.byref(md))
    assert n0 > 0 and ws0 > 0
    assert lib.swf_model_forward(C.byref(md), P, P, P, P, 1, 16, 16, None, 0, None) == L.ERR_WORKSPACE
    md.act = GOOD
    assert (lib.swf_model_param_count(C.byref(md)), lib.swf_model_workspace_bytes(C.byref(md), 1, 16, 16), lib.swf_model_arena_elems(C.byref(md))) == \
        (n0, ws0, arena0)
    assert lib.swf_model_forward(C.byref(md), P, P, P, P, 1, 16, 16, None, 0, None) == L.ERR_WORKSPACE
    assert lib.swf_model_forward_packed(C.byref(md), P, P, P, P, P, 1, 16, 16, None, 0, None) == L.ERR_WORKSPACE
    md.act = UNKNOWN
    assert lib.swf_model_forward(C.byref(md), P, P, P, P, 1, 16, 16, None, 0, None) == L.ERR_UNSUPPORTED
    assert lib.swf_model_workspace_bytes(C.byref(md), 1, 16, 16) == 0


def test_model_refuses_sub_modules_that_disagree_on_the_activation():
    from swin_unet_image_fusion_amd import CONFIGS, MyModel
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.GELU())).eval()
    m._check_one_activation()
    k0 = m.graph_key()
    m.mlp_activation_func = nn.ReLU()                      # replaced on the model only: the blocks, patch layers and head still hold GELU
    assert m.graph_key() != k0                             # ... and a graph captured under GELU is not replayed
    with pytest.raises(NotImplementedError, match=r"encoder_list\.0\.1 holds GELU"):
        m._check_one_activation()
    with pytest.raises(NotImplementedError):
        MyModel(**CONFIGS["tiny"].model_kwargs(nn.Tanh())).eval()._check_one_activation()


def test_the_shim_with_elu_is_the_oracle_itself_and_restores_it():
    r = A.reference("block_c8_w4", "elu1", torch.float32, False)
    plain = O.basic_block(r.sd, "", r.x, r.y, cross=True, shift=True, num_heads=2, dims_per_head=4, window_size=(4, 4))
    assert all(torch.equal(a, b) for a, b in zip(r.outs, plain))
    assert O.F is torch.nn.functional and r.min_abs_u > 0.0 and len(r.pre_activations) == 2
    with shimmed(nn.ReLU()) as ns:
        assert O.F is ns and ns.pad is torch.nn.functional.pad
        assert torch.equal(O.F.elu(torch.tensor([-1.0, 2.0])), torch.tensor([0.0, 2.0]))
    assert O.F is torch.nn.functional and ns.min_abs_u == 1.0
    assert torch.equal(nn.ELU()(torch.tensor([-1.0])), torch.tensor([math.expm1(-1.0)], dtype=torch.float32))   # torch itself was never patched


def test_the_shim_changes_the_three_activation_sites():
    g, e = A.reference("model_tiny_16", "gelu", torch.float32, False), A.reference("model_tiny_16", "elu1", torch.float32, False)
    assert not torch.equal(g.outs[0], e.outs[0])
    # 2 patch layers x 2 streams x 2 (encoder, decoder) + 16 blocks x 2 streams + the head
    assert len(g.pre_activations) == 8 + 32 + 1


@pytest.mark.parametrize("unit", [u.name for u in A.BACKWARD_UNITS])
@pytest.mark.parametrize("case", [c.name for c in A.CASES if c.kinked])
def test_kink_condition(unit, case):
    """No pre-activation of the reference sits within rounding of the kink: min |u64| >= 16 max |u32 - u64| over every pre-activation of the
    case, so a GPU test of this case never blames a kernel for the side of 0 a rounding error fell on.  The seeds of
    tests/activation_cases.py are chosen so that this holds; it is no tolerance of the GPU tests."""
    lo, err = A.kink_margin(unit, case)
    assert lo >= 16.0 * err, (lo, err)


@pytest.mark.parametrize("name", A.golden_names())
def test_the_shimmed_oracle_matches_the_reference_run_with_that_activation(name):
    """tests/test_oracle_golden.py's bar, 1e-5 relative, against what the reference itself computed with the activation."""
    case, sd, (x, y), expected, oracle, _, _ = A.golden(name)
    with torch.no_grad(), shimmed(case.make()):
        outs = oracle(sd, x, y)
    assert len(outs) == len(expected)
    for got, exp in zip(outs, expected):
        assert got.shape == exp.shape
        l2, mx = A.G.rel_err(got, exp)
        assert l2 <= 1e-5 and mx <= 1e-5, (l2, mx)


def test_golden_fixtures_are_the_eleven_of_the_tool():
    assert len(A.golden_names()) == 11 and {A.golden(n)[0].name for n in A.golden_names()} == {"gelu", "gelu_tanh", "relu", "leaky0.2", "elu0.5", "silu"}
