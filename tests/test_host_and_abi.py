"""CPU-only checks: the C-ABI library loads and exports every symbol include/swinfuse.h declares,
argument validation returns the documented status codes without touching a GPU, and the host-side
module mirror reproduces the reference's state_dict key set / shapes / aliasing (golden key tables
captured from the real reference)."""
import ctypes as C
import json
import os
import re

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, MyModel, SelfAndCrossBlockPair, WindowAttention, _lib as L
from swin_unet_image_fusion_amd.config import alias_groups_from_tensors, load_recipe_into, make_state_arrays
from tests import golden_util as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _header_functions():
    text = open(os.path.join(REPO, "include", "swinfuse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(swf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    names = _header_functions()
    assert len(names) >= 25
    handle = C.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f"{n} declared in swinfuse.h but not exported"
    # and the ctypes table binds exactly the declared set
    assert sorted(L.SIGNATURES) == names


def test_version_and_status_strings():
    lib = L.lib()
    assert lib.swf_version() == 1
    assert lib.swf_status_string(0) == b"ok"
    assert b"pad" in lib.swf_status_string(L.ERR_PAD)


def test_argument_validation_without_gpu():
    lib = L.lib()
    desc = L.AttnDesc(8, 2, 4, 4, 4, 0)
    prm = L.AttnParams()
    # NULL tensors
    assert lib.swf_window_attention_fwd(C.byref(desc), C.byref(prm), None, None, None, None, None, 1, 8, 8, None, 0, None) == L.ERR_NULL
    # map not a multiple of the window -> BAD_SHAPE (einops error in the reference)
    assert lib.swf_window_attention_fwd(C.byref(desc), C.byref(prm), 1, 1, 1, None, 1, 1, 9, 8, None, 0, None) == L.ERR_BAD_SHAPE
    with pytest.raises(ValueError):
        L.check(L.ERR_BAD_SHAPE)
    # reflect pad >= dim -> ERR_PAD -> RuntimeError (a006:128)
    hm, wm, ho, wo = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    st = lib.swf_merge_out_shape(8, 8, 2, 2, 8, 8, C.byref(hm), C.byref(wm), C.byref(ho), C.byref(wo))
    assert st == L.ERR_PAD
    with pytest.raises(RuntimeError):
        L.check(st)
    assert lib.swf_merge_out_shape(200, 200, 2, 2, 7, 7, C.byref(hm), C.byref(wm), C.byref(ho), C.byref(wo)) == 0
    assert (hm.value, wm.value, ho.value, wo.value) == (100, 100, 105, 105)
    assert lib.swf_merge_out_shape(5, 4, 2, 2, 1, 1, C.byref(hm), C.byref(wm), C.byref(ho), C.byref(wo)) == 0
    assert (hm.value, wm.value) == (3, 2)


def test_patch_prec_entries_validate_without_gpu():
    """swf_patch_merge_fwd_prec / swf_patch_unmerge_fwd_prec refuse bad arguments before anything is packed or launched."""
    lib = L.lib()
    P = 4096   # a fake device pointer
    pp, empty = L.PatchParams(L.Linear(P, P), L.Norm(P, P)), L.PatchParams()
    ln, ln_null = L.PatchLn1(L.Norm(P, P), P, P), L.PatchLn1(L.Norm(P, P), P, None)
    route = C.c_int32(-7)
    merge = lambda prec=L.PREC_FAST, px=pp, py=pp, xi=P, yi=P, xo=P, yo=P, geo=(2, 8, 8, 8, 16, 2, 2, 4, 4), lx=None, ly=None: \
        lib.swf_patch_merge_fwd_prec(prec, C.byref(px) if px else None, C.byref(py) if py else None, xi, yi, xo, yo, *geo,
                                     C.byref(lx) if lx else None, C.byref(ly) if ly else None, C.byref(route), None, 0, None)
    unmerge = lambda prec=L.PREC_FAST, px=pp, py=pp, xi=P, yi=P, sx=None, sy=None, xo=P, yo=P, geo=(2, 8, 8, 5, 7, 16, 8, 2, 2, 9, 14), lx=None, \
        ly=None: lib.swf_patch_unmerge_fwd_prec(prec, C.byref(px) if px else None, C.byref(py) if py else None, xi, yi, sx, sy, xo, yo, *geo,
                                                C.byref(lx) if lx else None, C.byref(ly) if ly else None, C.byref(route), None, 0, None)
    for call in (merge, unmerge):
        assert call() == L.ERR_WORKSPACE                       # everything else in order: the workspace is what is missing
        assert call(py=None, yi=None, yo=None) == L.ERR_WORKSPACE   # one stream
        assert call(px=None) == L.ERR_NULL and call(px=empty) == L.ERR_NULL and call(py=empty) == L.ERR_NULL
        assert call(xi=None) == L.ERR_NULL and call(xo=None) == L.ERR_NULL and call(yi=None) == L.ERR_NULL and call(yo=None) == L.ERR_NULL
        assert call(lx=ln) == L.ERR_NULL and call(ly=ln) == L.ERR_NULL          # planes for every stream or for none
        assert call(lx=ln, ly=ln_null) == L.ERR_NULL
        assert call(py=None, yi=None, yo=None, ly=ln) == L.ERR_NULL
        assert call(lx=ln, ly=ln) == L.ERR_WORKSPACE
        assert call(prec=2) == L.ERR_BAD_SHAPE
    for bad in ((0, 8, 8, 8, 16, 2, 2, 4, 4), (2, 8, 8, 0, 16, 2, 2, 4, 4), (2, 8, 8, 8, -1, 2, 2, 4, 4), (2, 0, 8, 8, 16, 2, 2, 4, 4),
                (2, 8, 8, 8, 16, 0, 2, 4, 4), (2, 8, 8, 8, 16, 2, 2, 4, 0)):
        assert merge(geo=bad) == L.ERR_BAD_SHAPE, bad
        assert lib.swf_patch_merge_prec_workspace_bytes(L.PREC_FAST, 1, *bad) == 0
    # reflect pad >= the dimension it pads: before merging (1x8 map, merge 2), and of the merged 4x4 map up to the 8x8 window
    for pad in ((2, 1, 8, 8, 16, 2, 2, 1, 1), (2, 8, 8, 8, 16, 2, 2, 8, 8)):
        assert merge(geo=pad) == L.ERR_PAD, pad
        assert lib.swf_patch_merge_prec_workspace_bytes(L.PREC_FAST, 1, *pad) == 0
    with pytest.raises(RuntimeError):
        L.check(merge(geo=(2, 8, 8, 8, 16, 2, 2, 8, 8)))
    for bad in ((0, 8, 8, 5, 7, 16, 8, 2, 2, 9, 14), (2, 8, 8, 9, 7, 16, 8, 2, 2, 9, 14), (2, 8, 8, 5, 0, 16, 8, 2, 2, 9, 14),
                (2, 8, 8, 5, 7, 16, 8, 2, 2, 11, 14), (2, 8, 8, 5, 7, 16, 8, 2, 2, 9, 0), (2, 8, 8, 5, 7, 0, 8, 2, 2, 9, 14),
                (2, 8, 8, 5, 7, 16, 8, 2, 0, 9, 14)):
        assert unmerge(geo=bad) == L.ERR_BAD_SHAPE, bad
        assert lib.swf_patch_unmerge_prec_workspace_bytes(L.PREC_FAST, 1, *bad) == 0
    assert unmerge(sx=P) == L.ERR_NULL and unmerge(sy=P) == L.ERR_NULL      # skip for every stream or for none
    assert unmerge(sx=P, sy=P) == L.ERR_WORKSPACE
    for q, geo in ((lib.swf_patch_merge_prec_workspace_bytes, (2, 8, 8, 8, 16, 2, 2, 4, 4)),
                   (lib.swf_patch_unmerge_prec_workspace_bytes, (2, 8, 8, 5, 7, 16, 8, 2, 2, 9, 14))):
        assert q(2, 1, *geo) == 0 and q(L.PREC_FP32, 1, *geo) > 0 and q(L.PREC_FAST, 0, *geo) > 0
    assert route.value == -7   # a refused call reports no route


def test_block_route_entries_validate_without_gpu():
    """swf_basic_block_fwd_route / swf_block_stage_fwd_prec refuse bad arguments before anything is packed or launched, and a refused
    call leaves the caller's route untouched."""
    lib = L.lib()
    P = 4096   # a fake device pointer
    lin = lambda: L.Linear(P, P)
    sp = lambda: L.BlockStreamParams(L.Norm(P, P), L.AttnParams(lin(), lin(), lin(), lin(), P), L.Norm(P, P), lin(), lin())
    four = lambda: (L.BlockStreamParams * 4)(*[sp() for _ in range(4)])
    hole = four()
    hole[2].fc1.weight = None                                # a missing layer in the third block
    good = L.BlockDesc(L.AttnDesc(192, 8, 24, 8, 8, 0), 768, 0, L.PREC_FAST, 1)
    ln, ln_null = L.PatchLn1(L.Norm(P, P), P, P), L.PatchLn1(L.Norm(P, None), P, P)
    route = (C.c_int32 * 4)(-7, -7, -7, -7)
    block = lambda desc=good, px=four(), py=four(), xi=P, yi=P, xo=P, yo=P, m=(2, 8, 16): \
        lib.swf_basic_block_fwd_route(C.byref(desc) if desc else None, px, py, xi, yi, xo, yo, *m, route, None, 0, None)
    stage = lambda desc=good, px=four(), py=four(), xi=P, yi=P, xo=P, yo=P, m=(2, 8, 16), lx=None, ly=None: \
        lib.swf_block_stage_fwd_prec(C.byref(desc) if desc else None, px, py, xi, yi, xo, yo, *m, C.byref(lx) if lx else None,
                                     C.byref(ly) if ly else None, route, None, 0, None)
    for call in (block, stage):
        assert call() == L.ERR_WORKSPACE                           # everything else in order: the workspace is what is missing
        assert call(py=None, yi=None, yo=None) == L.ERR_WORKSPACE   # one stream
        assert call(desc=None) == L.ERR_NULL and call(px=None) == L.ERR_NULL
        assert call(xi=None) == L.ERR_NULL and call(xo=None) == L.ERR_NULL and call(yi=None) == L.ERR_NULL and call(yo=None) == L.ERR_NULL
        for m in ((0, 8, 16), (2, 0, 16), (2, 8, 12), (2, 9, 16)):     # empty batch or map, map no multiple of the window
            assert call(m=m) == L.ERR_BAD_SHAPE, m
        for bad in (L.BlockDesc(L.AttnDesc(0, 8, 24, 8, 8, 0), 768, 0, L.PREC_FAST, 0), L.BlockDesc(L.AttnDesc(192, 8, 24, 8, 0, 0), 768, 0, L.PREC_FAST, 0),
                    L.BlockDesc(L.AttnDesc(192, 8, 24, 8, 8, 0), 0, 0, L.PREC_FAST, 0)):
            assert call(desc=bad) == L.ERR_BAD_SHAPE
    assert stage(px=hole) == L.ERR_NULL and stage(py=hole) == L.ERR_NULL
    assert stage(desc=L.BlockDesc(L.AttnDesc(192, 8, 24, 8, 8, 0), 768, 0, 2, 0)) == L.ERR_BAD_SHAPE       # unknown precision
    assert stage(lx=ln) == L.ERR_NULL and stage(ly=ln) == L.ERR_NULL                                       # planes for every stream or for none
    assert stage(lx=ln, ly=ln_null) == L.ERR_NULL and stage(py=None, yi=None, yo=None, ly=ln) == L.ERR_NULL
    assert stage(lx=ln, ly=ln) == L.ERR_WORKSPACE and stage(py=None, yi=None, yo=None, lx=ln) == L.ERR_WORKSPACE
    q = lib.swf_block_stage_prec_workspace_bytes
    assert q(C.byref(good), 1, 2, 8, 16) > 0 and q(None, 1, 2, 8, 16) == 0 and q(C.byref(good), 1, 2, 8, 12) == 0
    assert q(C.byref(L.BlockDesc(L.AttnDesc(192, 8, 24, 8, 8, 0), 768, 0, 2, 0)), 1, 2, 8, 16) == 0
    assert list(route) == [-7] * 4


def test_block_modules_validate_their_schedule():
    """BasicBlock and SelfAndCrossBlockPair carry the schedule of their own calls (swf_block_desc.schedule), validated like MyModel's."""
    from swin_unet_image_fusion_amd import BasicBlock
    blk = BasicBlock(24, 8, 3, (8, 8), True, True, True, True, 0.0, 0.0, 96, nn.ELU(inplace=True), 0.0)
    assert blk.schedule == "latency" and blk._desc("fast").schedule == 0
    blk.schedule = "throughput"
    assert blk._desc("fast").schedule == 1 and blk._desc("fp32").schedule == 1
    blk.schedule = "fastest"
    with pytest.raises(ValueError, match="schedule"):
        blk._desc("fast")
    pair = SelfAndCrossBlockPair(24, 8, 3, (8, 8), True, True, 0.0, 0.0, 96, nn.ELU(inplace=True), 0.0)
    assert pair.schedule == "latency"
    pair.schedule = "fastest"
    with pytest.raises(ValueError, match="schedule"):      # refused before any tensor is touched
        pair(torch.zeros(1, 24, 8, 8), torch.ones(1, 24, 8, 8))


@pytest.mark.parametrize("cfg_name", ["win8", "win7", "tiny", "tiny7", "win8_4stage", "win16"])
def test_state_dict_matches_reference_key_table(cfg_name):
    with open(os.path.join(G.GOLDEN, f"state_keys_{cfg_name}.json")) as f:
        ref = json.load(f)
    m = MyModel(**CONFIGS[cfg_name].model_kwargs(nn.ELU(inplace=True)))
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref["shapes"].keys())
    for k, shape in ref["shapes"].items():
        assert list(sd[k].shape) == shape, k
    alias = {k: a for k, a in alias_groups_from_tensors(sd).items() if a != k}
    assert alias == ref["alias_of"]


def test_arena_layout_covers_every_parameter_once():
    m = MyModel(**CONFIGS["win8"].model_kwargs(nn.ELU(inplace=True)))
    layout = m.param_layout()
    sd = m.state_dict()
    names = [n for n, _, _ in layout]
    assert len(names) == len(set(names))
    canon = set(alias_groups_from_tensors(sd).values())
    skipped = {k for k in canon if k.endswith("buffer_to_show_device") or k.endswith("num_batches_tracked")}
    assert set(names) == canon - skipped
    end = 0
    for n, off, num in layout:
        assert off >= end and off % 4 == 0 and sd[n].numel() == num
        end = off + num
    assert end <= L.lib().swf_model_arena_elems(C.byref(m._model_desc()))
    # 33 150 453 learnable parameters; the arena also carries BatchNorm running_mean/var (2 + 2)
    assert sum(num for _, _, num in layout) == 33150453 + 4

def test_recipe_is_deterministic_and_module_independent():
    """The weight recipe depends only on the key table, so the reference model (fixtures) and this
    package's mirror get identical tensors."""
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=0, flavor="stress")
    with open(os.path.join(G.GOLDEN, "state_keys_tiny.json")) as f:
        ref = json.load(f)
    arrays = make_state_arrays({k: tuple(v) for k, v in ref["shapes"].items()}, ref["alias_of"], seed=0, flavor="stress")
    sd = m.state_dict()
    for k, a in arrays.items():
        assert torch.equal(sd[k], torch.from_numpy(a).to(sd[k].dtype)), k


def test_forward_refuses_cpu_tensors_and_grad():
    wa = WindowAttention(8, 2, 4, (4, 4), False, False, True, 0.0, 0.0).eval()
    x = torch.zeros(1, 8, 8, 8)
    with torch.no_grad(), pytest.raises(RuntimeError):
        wa(x, x, x)            # CPU tensor: no fallback, loud failure
    with pytest.raises(RuntimeError):
        wa(x.requires_grad_(), x, x)
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))   # training mode
    with torch.no_grad(), pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 16, 16), torch.ones(1, 1, 16, 16))


def test_product_path_never_imports_the_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline leg may touch oracle/ (checker, never product)."""
    pkg = os.path.join(REPO, "swin_unet_image_fusion_amd")
    pat = re.compile(r"^\s*(from\s+oracle|import\s+oracle|from\s+\.+oracle)|import_module\([^)]*oracle|__import__\([^)]*oracle", re.M)
    for root, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py"):
                assert not pat.search(open(os.path.join(root, fn)).read()), f"{fn} imports the oracle"


def test_reference_format_checkpoint_roundtrip(tmp_path):
    """A checkpoint in the reference's on-disk format (a016:243-249) loads strictly through weights_only=True."""
    a = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(a, seed=4, flavor="stress")
    path = tmp_path / "ckpt.pth"
    torch.save({"model_state": a.state_dict(), "optimizer_state": {}, "scheduler_state": {}, "current_epoch": 7}, path)
    b = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    rest = b.load_reference_checkpoint(str(path))
    assert rest["current_epoch"] == 7
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    # aliases stay aliases after loading (one storage behind stage_1.other_module.* and auto_path_win_att.*)
    sd = b.state_dict()
    k1 = "encoder_list.0.3.self_att_block.normal_window_block.auto_path_win_att.window_attention_x.q_for_heads.weight"
    k2 = "encoder_list.0.3.self_att_block.normal_window_block.stage_1.other_module.window_attention_x.q_for_heads.weight"
    assert sd[k1].data_ptr() == sd[k2].data_ptr()


def test_graph_key_follows_in_place_parameter_updates():
    """MyModel keys its weight arena, packed images and graph_key() on the parameters' in-place version counters: an optimizer step or
    an EMA update under no_grad changes the key whatever the order of forwards around it; nothing else does.  Edits that bypass the
    counters (p.data) need refresh_weights(), which its docstring says."""
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True))).eval()
    load_recipe_into(m, seed=1, flavor="stress")
    k0 = m.graph_key()
    assert m.graph_key() == k0
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        _ = [p.clone() for p in m.parameters()]
    assert m.graph_key() == k0
    keys = {k0}
    for opt in (torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9), torch.optim.Adam(m.parameters(), lr=1e-3)):
        for p in m.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
        keys.add(m.graph_key())
    assert len(keys) == 3
    other = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    with torch.no_grad():
        for p, q in zip(m.parameters(), other.parameters()):
            p.mul_(0.9).add_(q, alpha=0.1)
    assert m.graph_key() not in keys
    keys.add(m.graph_key())
    with torch.no_grad():
        next(m.parameters()).data.add_(1.0)
    assert "p.data" in MyModel.refresh_weights.__doc__
    m.refresh_weights()
    assert m.graph_key() not in keys
    keys.add(m.graph_key())
    m.load_state_dict(other.state_dict(), strict=True)
    assert m.graph_key() not in keys


def test_weights_fingerprint_tuple_is_cached_and_rebuilt():
    """graph_key() runs on every runner step: the parameter tuple it sums over is built once, and again after .to() / _apply,
    load_state_dict() and refresh_weights() (which may have replaced Parameter objects)."""
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True))).eval()
    m.graph_key()
    cached = m._fp_params
    assert cached is not None and len(cached) == len(list(m.parameters()))
    m.graph_key()
    assert m._fp_params is cached
    for reset in (lambda: m.float(), lambda: m.load_state_dict(m.state_dict()), m.refresh_weights):
        reset()
        assert m._fp_params is None
        m.graph_key()
        assert m._fp_params is not None
