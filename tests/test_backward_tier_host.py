"""CPU-only checks of the backward kernel-family plumbing (include/swinfuse.h swf_bwd_options / swf_bwd_route): argument validation of
the *_bwd_opt entries and of the per-layer seam swf_linear_bwd before any launch, the seam's workspace query against the scratch the
module entries carve for the same layer, and the `backward_tier` attribute of the modules (validation, default, push-down by MyModel).
Pointers are fake non-null integers: no call here may reach a kernel launch.  The kernels themselves: tests/test_gpu_backward_tier.py."""
import ctypes as C

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import (CONFIGS, AutoPathMLP, BasicBlock, MyModel, PatchMergingAndLinearLayer, StateRecorder, WindowAttention,
                                        _lib as L)
from tests import bwd_tier_cases as T

P = 4096   # a fake device pointer


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _linear():
    return L.Linear(P, P)


def _stream_params():
    attn = L.AttnParams(_linear(), _linear(), _linear(), _linear(), P)
    return L.BlockStreamParams(L.Norm(P, P), attn, L.Norm(P, P), _linear(), _linear())


def _entries():
    """name -> call(pointer, (M-like sizes), options, workspace, bytes): every new entry with every tensor = `ptr` and valid sizes unless
    overridden"""
    lib = L.lib()
    desc = L.BlockDesc(L.AttnDesc(8, 2, 4, 4, 4, 0), 8, 0, L.PREC_FP32, 0)
    px, py, prm, lin, pp = _stream_params(), _stream_params(), _stream_params().attn, _linear(), L.PatchParams(_linear(), L.Norm(P, P))
    ref = lambda o: None if o is None else C.byref(o)

    def block(ptr, sizes, opt, ws, n):
        b, h, w = sizes or (2, 8, 8)
        return lib.swf_basic_block_bwd_opt(C.byref(desc), C.byref(px), C.byref(py), ptr, ptr, ptr, ptr, ptr, ptr, None, None, b, h, w, None,
                                           ref(opt), None, ws, n, None)

    def attention(ptr, sizes, opt, ws, n):
        b, h, w = sizes or (2, 8, 8)
        q = (ptr, ptr and 2 * ptr, ptr and 3 * ptr)
        return lib.swf_window_attention_bwd_opt(C.byref(desc.attn), C.byref(prm), ptr, ptr, ptr, ptr, *q, None, b, h, w, None, 0, ref(opt), None,
                                                ws, n, None)

    def mlp(ptr, sizes, opt, ws, n):
        tok, c, hid = sizes or (128, 8, 32)
        return lib.swf_mlp_bwd_opt(C.byref(lin), C.byref(lin), ptr, ptr, ptr, None, None, tok, c, hid, None, 0, ref(opt), None, ws, n, None)

    def patch(ptr, sizes, opt, ws, n):
        b, h, w = sizes or (2, 8, 8)
        return lib.swf_patch_layer_bwd_opt(C.byref(pp), ptr, ptr, ptr, None, b, h, w, 8, 16, 2, 2, 1, ref(opt), None, ws, n, None)

    def linear(ptr, sizes, opt, ws, n):
        m, nn_, k = sizes or (300, 40, 16)
        return lib.swf_linear_bwd(ptr, ptr, ptr, ptr, ptr, ptr, m, nn_, k, 0, ref(opt), None, ws, n, None)

    return {"basic_block": block, "window_attention": attention, "mlp": mlp, "patch_layer": patch, "linear": linear}


@pytest.mark.parametrize("name", ["basic_block", "window_attention", "mlp", "patch_layer", "linear"])
def test_new_entries_validate_before_they_launch(name):
    call = _entries()[name]
    assert call(None, None, None, P, 1 << 30) == L.ERR_NULL
    # an unknown family in either field is refused, whatever the other field says; NULL options and all-zero options are today's entry
    for gemm, attn in ((2, 0), (-1, 0), (0, 2), (0, -1), (1, 2), (0, 1)):
        assert call(P, None, L.BwdOptions(gemm, attn), P, 1 << 30) == L.ERR_UNSUPPORTED, (gemm, attn)
    with pytest.raises(NotImplementedError):
        L.check(L.ERR_UNSUPPORTED)
    # every size <= 0 is a bad shape
    good = {"mlp": (128, 8, 32), "linear": (300, 40, 16)}.get(name, (2, 8, 8))
    for i in range(3):
        for bad in (0, -1):
            sizes = tuple(bad if j == i else v for j, v in enumerate(good))
            assert call(P, sizes, L.BwdOptions(1, 0), P, 1 << 30) == L.ERR_BAD_SHAPE, sizes
    # valid arguments in both families get as far as the workspace check and no further
    for opt in (None, L.BwdOptions(0, 0), L.BwdOptions(1, 0)):
        assert call(P, None, opt, P, 1) == L.ERR_WORKSPACE


def test_linear_bwd_workspace_is_the_scratch_of_the_same_layer_in_a_module_entry():
    """swf_mlp_bwd carves h and dh ([tokens][hidden] each) and the scratch its two weight gradients share, sized for the wider of its
    layers: the seam asks for that scratch for either layer of the MLP, whichever of (N, K) is the wider."""
    lib = L.lib()
    up = lambda v: (v + 255) // 256 * 256
    for tok, c, hid in ((128, 8, 32), (300, 24, 96), (8451, 48, 192), (64, 384, 1536)):
        scratch = lib.swf_mlp_bwd_workspace_bytes(tok, c, hid) - 2 * up(tok * hid * 4)
        assert lib.swf_linear_bwd_workspace_bytes(tok, hid, c) == scratch and lib.swf_linear_bwd_workspace_bytes(tok, c, hid) == scratch
    assert all(lib.swf_linear_bwd_workspace_bytes(*s) == 0 for s in ((0, 4, 4), (4, 0, 4), (4, 4, -1)))
    # every GPU case asks for a workspace, and one byte less is refused (dX alone needs none: tests/test_gpu_backward_tier.py)
    for m, n, k in T.LINEAR_SHAPES:
        need = lib.swf_linear_bwd_workspace_bytes(m, n, k)
        assert need >= ((m + 255) // 256) * n * (k + 1) * 4
        for ws, nb in ((P, need - 1), (None, 0)):
            assert lib.swf_linear_bwd(P, P, P, P, P, P, m, n, k, 0, None, None, ws, nb, None) == L.ERR_WORKSPACE


def test_ctypes_structs_match_the_header():
    assert C.sizeof(L.BwdOptions) == 8 and C.sizeof(L.BwdRoute) == 20
    assert [f[0] for f in L.BwdRoute._fields_] == ["dx_fma", "dx_mfma", "dw_fma", "dw_mfma", "attention"]


def _modules():
    act = nn.ELU(inplace=True)
    return [WindowAttention(8, 2, 4, (4, 4), True, False, True, 0.0, 0.0), AutoPathMLP(8, 32, act, True, 0.0),
            BasicBlock(8, 2, 4, (4, 4), True, True, True, True, 0.0, 0.0, 32, act, 0.0),
            PatchMergingAndLinearLayer(True, True, 1, 8, StateRecorder(), (2, 2), act), MyModel(**CONFIGS["tiny"].model_kwargs(act))]


def test_backward_tier_default_and_validation():
    for m in _modules():
        assert m.backward_tier == "fma" and m.backward_gemm == "fma" and m.last_backward_route is None, type(m).__name__
        opt = m._bwd_options()
        assert (opt.gemm, opt.attention) == (L.BWD_GEMM_FMA, L.BWD_ATTN_THREAD)
        m.backward_tier = "mfma"
        assert m.backward_gemm == "mfma" and m._bwd_options().gemm == L.BWD_GEMM_MFMA
        for bad in ("fast", "MFMA", 1, None):
            with pytest.raises(ValueError):
                m.backward_tier = bad
        assert m.backward_tier == "mfma"            # a refused value changes nothing
        m.backward_gemm = "bf16"                    # the part on its own is checked where it is used
        with pytest.raises(ValueError):
            m._bwd_options()
        m.backward_tier = "fma"
        assert "backward_gemm" not in m.state_dict() and not any("backward" in k for k in m.state_dict())


def test_model_pushes_its_backward_tier_down_for_the_call_only():
    """MyModel's differentiable forward runs every block and patch layer in the MODEL's backward tier, as it does with `precision`, and
    gives them their own setting back afterwards."""
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    tiered = [s for s in m.modules() if isinstance(s, (BasicBlock, PatchMergingAndLinearLayer))]
    assert len(tiered) > 4
    tiered[0].backward_tier = "mfma"                 # one sub-module with a setting of its own
    seen = []
    m._forward_autograd_stages = lambda x, y: seen.append([s._bwd_options().gemm for s in tiered]) or x
    x = torch.zeros(1, 1, 16, 16)
    for tier, code in (("mfma", L.BWD_GEMM_MFMA), ("fma", L.BWD_GEMM_FMA)):
        m.backward_tier = tier
        m._forward_autograd(x, x)
        assert seen[-1] == [code] * len(tiered)
        assert [s.backward_tier for s in tiered] == ["mfma"] + ["fma"] * (len(tiered) - 1)
    m.backward_gemm = "nope"
    with pytest.raises(ValueError):
        m._forward_autograd(x, x)
    assert [s.backward_tier for s in tiered] == ["mfma"] + ["fma"] * (len(tiered) - 1)
    assert m.backward_routes() == {}
