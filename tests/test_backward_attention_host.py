"""CPU-only checks of the attention-backward family plumbing (include/swinfuse.h swf_bwd_attn): the `backward_attention` attribute of the
modules (default, validation, push-down by MyModel, not in the state dict) and the validation of the `attention` field of
swf_bwd_options by every *_bwd_opt entry before any launch.  Pointers are fake non-null integers: no call here may reach a kernel
launch.  The kernel itself: tests/test_gpu_backward_phased.py."""
import ctypes as C

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, AutoPathMLP, BasicBlock, MyModel, PatchMergingAndLinearLayer, StateRecorder, WindowAttention,
                                        _lib as L)

P = 4096   # a fake device pointer


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _modules():
    act = nn.ELU(inplace=True)
    return [WindowAttention(8, 2, 4, (4, 4), True, False, True, 0.0, 0.0), AutoPathMLP(8, 32, act, True, 0.0),
            BasicBlock(8, 2, 4, (4, 4), True, True, True, True, 0.0, 0.0, 32, act, 0.0),
            PatchMergingAndLinearLayer(True, True, 1, 8, StateRecorder(), (2, 2), act), MyModel(**CONFIGS["tiny"].model_kwargs(act))]


def test_codes():
    assert (L.BWD_ATTN_THREAD, L.BWD_ATTN_PHASED) == (0, 3)
    assert (L.BWD_ATTN_RAN_NONE, L.BWD_ATTN_RAN_RESIDENT, L.BWD_ATTN_RAN_RECOMPUTE, L.BWD_ATTN_RAN_PHASED) == (0, 1, 2, 3)
    assert C.sizeof(L.BwdOptions) == 8 and C.sizeof(L.BwdRoute) == 20          # the layouts did not move


def test_backward_attention_default_and_validation():
    for m in _modules():
        name = type(m).__name__
        assert m.backward_attention == "thread" and m.backward_tier == "fma", name
        assert (m._bwd_options().gemm, m._bwd_options().attention) == (L.BWD_GEMM_FMA, L.BWD_ATTN_THREAD), name
        m.backward_attention = "phased"
        assert m.backward_attention == "phased" and m._bwd_options().attention == L.BWD_ATTN_PHASED, name
        assert m.backward_tier == "fma" and m._bwd_options().gemm == L.BWD_GEMM_FMA          # backward_tier keeps meaning the GEMM family
        for bad in ("Phased", "recompute", "resident", 3, 0, None, ""):
            with pytest.raises(ValueError):
                m.backward_attention = bad
            assert m.backward_attention == "phased", (name, bad)                              # a refused value changes nothing
        m.backward_tier = "mfma"
        opt = m._bwd_options()
        assert (opt.gemm, opt.attention) == (L.BWD_GEMM_MFMA, L.BWD_ATTN_PHASED)              # the two settings are independent
        m._backward_attention = "nope"                                                        # the raw value is checked where it is used
        with pytest.raises(ValueError):
            m._bwd_options()
        m.backward_attention = "thread"
        assert m._bwd_options().attention == L.BWD_ATTN_THREAD
        assert not any("backward" in k for k in m.state_dict()), name
        m.backward_attention = "phased"
        assert not any("backward" in k for k in m.state_dict()), name


def test_a_state_dict_round_trip_carries_neither_setting():
    act = nn.ELU(inplace=True)
    a, b = MyModel(**CONFIGS["tiny"].model_kwargs(act)), MyModel(**CONFIGS["tiny"].model_kwargs(act))
    a.backward_attention, a.backward_tier = "phased", "mfma"
    b.load_state_dict(a.state_dict(), strict=True)
    assert (b.backward_attention, b.backward_tier) == ("thread", "fma")


def test_model_pushes_its_attention_family_down_for_the_call_only():
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    tiered = [s for s in m.modules() if isinstance(s, (BasicBlock, PatchMergingAndLinearLayer))]
    blocks = [s for s in tiered if isinstance(s, BasicBlock)]
    assert len(blocks) >= 4
    blocks[0].backward_attention = "phased"              # one block with a setting of its own
    blocks[1].backward_tier = "mfma"
    own = [(s.backward_attention, s.backward_tier) for s in tiered]
    seen = []
    m._forward_autograd_stages = lambda x, y: seen.append([(s._bwd_options().attention, s._bwd_options().gemm) for s in tiered]) or x
    x = torch.zeros(1, 1, 16, 16)
    for family, code in (("phased", L.BWD_ATTN_PHASED), ("thread", L.BWD_ATTN_THREAD)):
        m.backward_attention = family
        m._forward_autograd(x, x)
        assert seen[-1] == [(code, L.BWD_GEMM_FMA)] * len(tiered)
        assert [(s.backward_attention, s.backward_tier) for s in tiered] == own
    m.backward_attention, m.backward_tier = "phased", "mfma"
    m._forward_autograd(x, x)
    assert seen[-1] == [(L.BWD_ATTN_PHASED, L.BWD_GEMM_MFMA)] * len(tiered)
    assert [(s.backward_attention, s.backward_tier) for s in tiered] == own
    m._backward_attention = "nope"
    with pytest.raises(ValueError):
        m._forward_autograd(x, x)
    assert [(s.backward_attention, s.backward_tier) for s in tiered] == own and len(seen) == 3
    assert m.backward_routes() == {}


# ---- the entries ---------------------------------------------------------------------------------------------------------------------
def _linear():
    return L.Linear(P, P)


def _stream_params():
    attn = L.AttnParams(_linear(), _linear(), _linear(), _linear(), P)
    return L.BlockStreamParams(L.Norm(P, P), attn, L.Norm(P, P), _linear(), _linear())


def _entries(win=4, head_dim=4, hw=8):
    """name -> call(options, workspace, bytes) with every tensor a fake pointer and valid sizes"""
    lib = L.lib()
    desc = L.BlockDesc(L.AttnDesc(2 * head_dim, 2, head_dim, win, win, 0), 8, 0, L.PREC_FP32, 0)
    px, py, prm, lin, pp = _stream_params(), _stream_params(), _stream_params().attn, _linear(), L.PatchParams(_linear(), L.Norm(P, P))
    block = lambda opt, ws, n: lib.swf_basic_block_bwd_opt(C.byref(desc), C.byref(px), C.byref(py), P, P, P, P, P, P, None, None, 2, hw, hw, None,
                                                           C.byref(opt), None, ws, n, None)
    attention = lambda opt, ws, n: lib.swf_window_attention_bwd_opt(C.byref(desc.attn), C.byref(prm), P, P, P, P, P, 2 * P, 3 * P, None, 2, hw, hw,
                                                                    None, 0, C.byref(opt), None, ws, n, None)
    mlp = lambda opt, ws, n: lib.swf_mlp_bwd_opt(C.byref(lin), C.byref(lin), P, P, P, None, None, 128, 8, 32, None, 0, C.byref(opt), None, ws, n, None)
    patch = lambda opt, ws, n: lib.swf_patch_layer_bwd_opt(C.byref(pp), P, P, P, None, 2, 8, 8, 8, 16, 2, 2, 1, C.byref(opt), None, ws, n, None)
    linear = lambda opt, ws, n: lib.swf_linear_bwd(P, P, P, P, P, P, 300, 40, 16, 0, C.byref(opt), None, ws, n, None)
    return {"basic_block": block, "window_attention": attention, "mlp": mlp, "patch_layer": patch, "linear": linear}


@pytest.mark.parametrize("name", ["basic_block", "window_attention"])
def test_code_3_reaches_the_workspace_check_on_the_entries_with_an_attention_core(name):
    call = _entries()[name]
    for gemm in (L.BWD_GEMM_FMA, L.BWD_GEMM_MFMA):
        assert call(L.BwdOptions(gemm, L.BWD_ATTN_PHASED), P, 1) == L.ERR_WORKSPACE, gemm
    assert b"workspace" in L.lib().swf_last_error_string()
    for attn in (1, 2, -1, 4):
        assert call(L.BwdOptions(0, attn), P, 1 << 30) == L.ERR_UNSUPPORTED, attn
        assert b"unknown attention-backward family" in L.lib().swf_last_error_string()


@pytest.mark.parametrize("name", ["mlp", "patch_layer", "linear"])
def test_entries_without_an_attention_core_accept_code_3_and_ignore_it(name):
    """The choice the header documents: `attention` is validated alike everywhere (0 or 3), then ignored where there is no attention
    core, so that one options struct serves every module of a model."""
    call = _entries()[name]
    for gemm in (L.BWD_GEMM_FMA, L.BWD_GEMM_MFMA):
        assert call(L.BwdOptions(gemm, L.BWD_ATTN_PHASED), P, 1) == L.ERR_WORKSPACE, gemm
        assert call(L.BwdOptions(gemm, L.BWD_ATTN_THREAD), P, 1) == L.ERR_WORKSPACE, gemm
    for attn in (1, 2, -1, 4):
        assert call(L.BwdOptions(0, attn), P, 1 << 30) == L.ERR_UNSUPPORTED, attn


@pytest.mark.parametrize("name", ["basic_block", "window_attention"])
def test_the_families_refuse_different_tiles_before_the_workspace_check(name):
    """16 x 16 at head_dim 48: the thread family refuses the tile with its 269060 B, the phased family gets as far as the workspace; one
    32 x 32 window at head_dim 17: the phased family refuses with ITS byte count.  Both before anything could be launched."""
    lib = L.lib()
    call = _entries(win=16, head_dim=48, hw=16)[name]
    assert call(L.BwdOptions(0, L.BWD_ATTN_THREAD), P, 1) == L.ERR_UNSUPPORTED
    msg = lib.swf_last_error_string().decode()
    assert "LDS" in msg and "269060" in msg and "phased" not in msg, msg
    assert call(L.BwdOptions(0, L.BWD_ATTN_PHASED), P, 1) == L.ERR_WORKSPACE
    call = _entries(win=32, head_dim=17, hw=32)[name]
    assert call(L.BwdOptions(0, L.BWD_ATTN_PHASED), P, 1) == L.ERR_UNSUPPORTED
    msg = lib.swf_last_error_string().decode()
    need = 4 * (2 * 1024 * 32 + 63 * 63 + 3 * 1024 + 16 * 63 * 63)
    assert "LDS" in msg and str(need) in msg and "phased" in msg, msg
    call = _entries(win=8, head_dim=65, hw=8)[name]
    assert call(L.BwdOptions(0, L.BWD_ATTN_PHASED), P, 1) == L.ERR_UNSUPPORTED
    assert "head_dim 65 > 64" in lib.swf_last_error_string().decode()
