"""CPU-only checks that every workspace size query is the measure of the carve its entry runs: with one byte less than the query
returns, the entry reports SWF_ERR_WORKSPACE before its first launch, and the need its error text names never exceeds the query.

Pointers are fake non-null integers (16-byte aligned, so the deep-level route is admitted): no call here may reach a kernel launch,
so every shape is chosen such that the entry's FIRST workspace check is the one that needs the query's value.  Left out: entries that
launch without touching the workspace (the single-launch fused patch route, the register-resident and whole-row deep patch kernels,
swf_basic_block_fwd_packed, the layout / pad / crop / add / colour kernels), the pre-packed model
path (its packed images need a GPU) and swf_fusion_loss (tests/test_loss_host.py)."""
import ctypes as C
import re

import pytest

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, _lib as L

P = 4096          # a fake device pointer
NEED = re.compile(rb"need (\d+) B")


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _linear():
    return L.Linear(P, P)


def _attn_params():
    return L.AttnParams(_linear(), _linear(), _linear(), _linear(), P)


def _stream_params():
    return L.BlockStreamParams(L.Norm(P, P), _attn_params(), L.Norm(P, P), _linear(), _linear())


def _refuses(call, need):
    """call(workspace, bytes) -> status.  One byte less than `need` is refused, and so is no workspace at all; the need named in the error
    text is at most `need`."""
    lib = L.lib()
    assert need > 0
    for ws, n in ((P, need - 1), (P, 1), (None, 0)):
        assert call(ws, n) == L.ERR_WORKSPACE, (ws, n, lib.swf_last_error_string())
        m = NEED.search(lib.swf_last_error_string())
        if m:   # the named need is itself enough: the aligned size that ok() asks for, never more than the query
            assert int(m.group(1)) <= need and int(m.group(1)) % 256 == 0, (lib.swf_last_error_string(), need)


def _named_need_at_most(call, need):
    """For an entry that shares a larger query with others: refused with one byte, and the need it names is covered by the query."""
    lib = L.lib()
    assert call(P, 1) == L.ERR_WORKSPACE, lib.swf_last_error_string()
    m = NEED.search(lib.swf_last_error_string())
    assert m and 0 < int(m.group(1)) <= need, (lib.swf_last_error_string(), need)


def _block_desc(c, heads, hd, win, hidden, prec, cross=0):
    return L.BlockDesc(L.AttnDesc(c, heads, hd, win, win, 0), hidden, cross, prec, 0)


# (desc, B, H, W): the attention half is the larger half (hidden = C), so the block's first check needs the whole query
GENERIC_FP32 = (_block_desc(8, 2, 4, 4, 8, L.PREC_FP32), 2, 8, 8)
GENERIC_FAST = (_block_desc(8, 2, 4, 4, 8, L.PREC_FAST), 2, 8, 8)            # C = 8: no LayerNorm folding, no fused kernel
GENERIC_FAST_SPLITK = (_block_desc(512, 8, 64, 8, 512, L.PREC_FAST), 1, 8, 8)  # K = 512: split-K partials; C > 384: no deep route
DEEP = (_block_desc(192, 8, 24, 8, 768, L.PREC_FAST), 2, 16, 16)             # level 3 of the shipped configs
DEEP4 = (_block_desc(384, 8, 48, 8, 1536, L.PREC_FAST), 1, 8, 8)             # level 4
WINDOW = (_block_desc(24, 8, 3, 8, 96, L.PREC_FAST), 1, 8, 8)                # fused window block, weights not pre-packed
WINDOW16 = (_block_desc(48, 8, 6, 16, 192, L.PREC_FAST, cross=1), 1, 16, 16)  # out-of-place kernel called in place: temporary maps


@pytest.mark.parametrize("case", [GENERIC_FP32, GENERIC_FAST, GENERIC_FAST_SPLITK, DEEP, DEEP4, WINDOW, WINDOW16],
                         ids=["generic_fp32", "generic_fast", "generic_fast_splitk", "deep3", "deep4", "window", "window16_in_place"])
def test_basic_block_fwd_needs_exactly_its_query(case):
    lib = L.lib()
    desc, b, h, w = case
    px, py = _stream_params(), _stream_params()
    need = lib.swf_basic_block_workspace_bytes(C.byref(desc), b, h, w)
    _refuses(lambda ws, n: lib.swf_basic_block_fwd(C.byref(desc), C.byref(px), C.byref(py), P, 2 * P, P, 2 * P, b, h, w, ws, n, None), need)


@pytest.mark.parametrize("case", [GENERIC_FP32, GENERIC_FAST, DEEP], ids=["generic_fp32", "generic_fast", "deep3"])
def test_block_pair4_and_half_blocks_are_covered_by_the_block_query(case):
    lib = L.lib()
    desc, b, h, w = case
    four = lambda: (L.BlockStreamParams * 4)(*[_stream_params() for _ in range(4)])
    px, py = four(), four()
    need = lib.swf_basic_block_workspace_bytes(C.byref(desc), b, h, w)
    _refuses(lambda ws, n: lib.swf_block_pair4_fwd(C.byref(desc), px, py, P, 2 * P, 3 * P, 5 * P, b, h, w, ws, n, None), need)
    if desc.attn.channels == 8:   # (the half-block entries have no deep route; at C = 8 no fused half kernel either)
        _named_need_at_most(lambda ws, n: lib.swf_attn_halfblock_fwd(C.byref(desc), px, py, P, 2 * P, 3 * P, 5 * P, b, h, w, ws, n, None), need)
        _named_need_at_most(lambda ws, n: lib.swf_mlp_halfblock_fwd(C.byref(desc), px, py, P, 2 * P, 3 * P, 5 * P, b, h, w, ws, n, None), need)


def test_window_attention_forward():
    lib = L.lib()
    prm = _attn_params()
    for desc, b, h, w in ((L.AttnDesc(8, 2, 4, 4, 4, 0), 2, 8, 8), (L.AttnDesc(512, 8, 64, 8, 8, 0), 1, 8, 8), (L.AttnDesc(24, 8, 3, 16, 16, 0), 2, 32, 32)):   # (large enough maps: the generic route is the larger one)
        need = lib.swf_window_attention_workspace_bytes(C.byref(desc), b, h, w)
        fast = lambda ws, n: lib.swf_window_attention_fwd_prec(C.byref(desc), L.PREC_FAST, C.byref(prm), P, 2 * P, 3 * P, None, 5 * P, b, h, w, ws, n, None)
        _refuses(fast, need)   # the query has no precision argument: the fast tier is the larger one
        _named_need_at_most(lambda ws, n: lib.swf_window_attention_fwd(C.byref(desc), C.byref(prm), P, 2 * P, 3 * P, None, 5 * P, b, h, w, ws, n, None), need)


def test_mlp_and_linear_forward():
    lib = L.lib()
    px, py = _stream_params(), _stream_params()
    lin = _linear()
    for prec, n, c, hid in ((L.PREC_FP32, 128, 8, 32), (L.PREC_FAST, 128, 8, 32), (L.PREC_FAST, 64, 512, 2048)):
        need = lib.swf_mlp_workspace_bytes(prec, n, c, hid)
        _refuses(lambda ws, nb: lib.swf_mlp_fwd(prec, C.byref(px), C.byref(py), P, 2 * P, 3 * P, 5 * P, n, c, hid, ws, nb, None), need)
    assert lib.swf_linear_workspace_bytes(L.PREC_FP32, 64, 2048, 512) == 0 and lib.swf_linear_workspace_bytes(L.PREC_FAST, 64, 8, 8) == 0
    need = lib.swf_linear_workspace_bytes(L.PREC_FAST, 64, 2048, 512)   # K = 2048: four split-K partials
    assert need >= 4 * 64 * 512 * 4
    _refuses(lambda ws, nb: lib.swf_linear_fwd_prec(C.byref(lin), L.PREC_FAST, P, None, 2 * P, 64, 2048, 512, 0, ws, nb, None), need)


def test_backward_and_dropout_entries():
    lib = L.lib()
    desc, b, h, w = GENERIC_FP32
    px, py = _stream_params(), _stream_params()
    drop = L.Dropout(7, 0.1, 0.1, 0.1)
    need = lib.swf_basic_block_bwd_workspace_bytes(C.byref(desc), b, h, w)
    need_drop = lib.swf_basic_block_drop_workspace_bytes(C.byref(desc), b, h, w)
    assert need_drop == need + 2 * b * h * w * desc.hidden * 4   # the dropped hidden activation of both streams
    _refuses(lambda ws, n: lib.swf_basic_block_bwd(C.byref(desc), C.byref(px), C.byref(py), P, P, P, P, P, P, None, None, b, h, w, ws, n, None), need)
    _refuses(lambda ws, n: lib.swf_basic_block_bwd_drop(C.byref(desc), C.byref(px), C.byref(py), P, P, P, P, P, P, None, None, b, h, w,
                                                        C.byref(drop), ws, n, None), need_drop)
    _refuses(lambda ws, n: lib.swf_basic_block_fwd_drop(C.byref(desc), C.byref(px), C.byref(py), P, P, P, P, b, h, w, C.byref(drop), ws, n, None), need_drop)

    ad, prm = desc.attn, _attn_params()
    need = lib.swf_window_attention_bwd_workspace_bytes(C.byref(ad), b, h, w)
    need_drop = lib.swf_window_attention_drop_workspace_bytes(C.byref(ad), b, h, w)
    assert need_drop == need + b * h * w * ad.channels * 4      # the output gradient through the projection mask
    _refuses(lambda ws, n: lib.swf_window_attention_bwd(C.byref(ad), C.byref(prm), P, P, P, P, P, 2 * P, 3 * P, None, b, h, w, ws, n, None), need)
    _refuses(lambda ws, n: lib.swf_window_attention_bwd_drop(C.byref(ad), C.byref(prm), P, P, P, P, P, 2 * P, 3 * P, None, b, h, w, C.byref(drop), 0,
                                                             ws, n, None), need_drop)
    _named_need_at_most(lambda ws, n: lib.swf_window_attention_fwd_drop(C.byref(ad), C.byref(prm), P, P, P, None, P, b, h, w, C.byref(drop), 0, ws, n, None),
                        need_drop)

    lin, tok, c, hid = _linear(), 128, 8, 32
    need = lib.swf_mlp_bwd_workspace_bytes(tok, c, hid)
    need_drop = lib.swf_mlp_drop_workspace_bytes(tok, c, hid)
    assert need_drop == need + tok * hid * 4 + tok * c * 4        # the dropped hidden activation and the masked output gradient
    _refuses(lambda ws, n: lib.swf_mlp_bwd(C.byref(lin), C.byref(lin), P, P, P, None, None, tok, c, hid, ws, n, None), need)
    _refuses(lambda ws, n: lib.swf_mlp_bwd_drop(C.byref(lin), C.byref(lin), P, P, P, None, None, tok, c, hid, C.byref(drop), 0, ws, n, None), need_drop)
    _named_need_at_most(lambda ws, n: lib.swf_mlp_fwd_drop(C.byref(lin), C.byref(lin), P, P, tok, c, hid, C.byref(drop), 0, ws, n, None), need_drop)

    nrm = L.Norm(P, P)
    _refuses(lambda ws, n: lib.swf_layernorm_bwd(C.byref(nrm), P, P, P, None, tok, c, ws, n, None), lib.swf_layernorm_bwd_workspace_bytes(tok, c))

    pp = L.PatchParams(_linear(), L.Norm(P, P))
    for enc, cin, cout in ((1, 8, 16), (0, 16, 8)):
        need = lib.swf_patch_layer_bwd_workspace_bytes(2, 8, 8, cin, cout, 2, 2, enc)
        _refuses(lambda ws, n: lib.swf_patch_layer_bwd(C.byref(pp), P, P, P, None, 2, 8, 8, cin, cout, 2, 2, enc, ws, n, None), need)

    hp = L.HeadParams(P, P, P, P, P, P, P, P)
    need = lib.swf_final_head_bwd_workspace_bytes(2, 16, 16, 3)
    _refuses(lambda ws, n: lib.swf_final_head_bwd(C.byref(hp), P, P, P, P, P, None, 2, 16, 16, 3, 0, ws, n, None), need)
    _named_need_at_most(lambda ws, n: lib.swf_final_head_batch_stats(C.byref(hp), P, P, P, P, None, None, 0.1, 2, 16, 16, 3, ws, n, None), need)


def test_patch_layers_generic_route():
    lib = L.lib()
    pp = L.PatchParams(_linear(), L.Norm(P, P))
    # merge: 13x10 -> reflect pad to 14x10 -> 7x5 -> window pad to 8x8
    need = lib.swf_patch_workspace_bytes(2, 13, 10, 8, 16, 2, 2, 4, 4, 1)
    _refuses(lambda ws, n: lib.swf_patch_merge_fwd(C.byref(pp), P, 2 * P, 2, 13, 10, 8, 16, 2, 2, 4, 4, ws, n, None), need)
    # unmerge of an 8x8 map: the query covers every crop; the largest need is the crop by one column
    need = lib.swf_patch_workspace_bytes(2, 8, 8, 16, 8, 2, 2, 4, 4, 0)
    crops = {(8, 8): None, (7, 8): None, (8, 7): None, (5, 5): None}
    for hm, wm in crops:
        call = lambda ws, n: lib.swf_patch_unmerge_fwd(C.byref(pp), P, None, 2 * P, 2, 8, 8, hm, wm, 16, 8, 2, 2, 2 * hm, 2 * wm, ws, n, None)
        _named_need_at_most(call, need)
        crops[(hm, wm)] = int(NEED.search(lib.swf_last_error_string()).group(1))
    assert max(crops.values()) <= need < max(crops.values()) + 256 and crops[(5, 5)] < crops[(8, 7)]
    _refuses(lambda ws, n: lib.swf_patch_unmerge_fwd(C.byref(pp), P, None, 2 * P, 2, 8, 8, 8, 7, 16, 8, 2, 2, 16, 14, ws, n, None), need)


# (Cin, Cout) of both directions: generic only; register-resident; deep whole-row; deep column-sliced (its conv rows and LN1 planes)
PREC_WIDTHS = {"merge": [(8, 16), (24, 48), (96, 192), (192, 384)], "unmerge": [(16, 8), (48, 24), (192, 96), (384, 192)]}


@pytest.mark.parametrize("dual", [0, 1], ids=["one_stream", "two_streams"])
@pytest.mark.parametrize("prec", [L.PREC_FP32, L.PREC_FAST], ids=["fp32", "fast"])
def test_patch_prec_entries_need_exactly_their_query(prec, dual):
    """swf_patch_merge_fwd_prec / swf_patch_unmerge_fwd_prec: the packed images and the impl's room are one carve, checked before the first
    launch (the pack).  The un-merge query takes the crop; probed against other crops of the same map it is exact at each, largest at one
    of the three crops the crop-agnostic swf_patch_workspace_bytes measures, and monotone in the kept map."""
    lib = L.lib()
    pp = L.PatchParams(_linear(), L.Norm(P, P))
    py, y = (C.byref(pp), 3 * P) if dual else (None, None)
    for cin, cout in PREC_WIDTHS["merge"]:
        geo = (2, 13, 10, cin, cout, 2, 2, 4, 4)
        need = lib.swf_patch_merge_prec_workspace_bytes(prec, dual, *geo)
        _refuses(lambda ws, n: lib.swf_patch_merge_fwd_prec(prec, C.byref(pp), py, P, y, 2 * P, y, *geo, None, None, None, ws, n, None), need)
        if not dual and prec == L.PREC_FP32:   # no image, one stream: the room of today's entry
            assert need == lib.swf_patch_workspace_bytes(*geo, 1)
    for cin, cout in PREC_WIDTHS["unmerge"]:
        needs = {}
        for hm, wm in ((8, 8), (7, 8), (8, 7), (5, 5), (5, 8), (8, 3), (1, 1)):
            geo = (2, 8, 8, hm, wm, cin, cout, 2, 2, 2 * hm - 1, 2 * wm)
            needs[(hm, wm)] = need = lib.swf_patch_unmerge_prec_workspace_bytes(prec, dual, *geo)
            _refuses(lambda ws, n: lib.swf_patch_unmerge_fwd_prec(prec, C.byref(pp), py, P, y, None, None, 2 * P, y, *geo, None, None, None, ws, n, None),
                     need)
        assert max(needs.values()) == max(needs[(8, 8)], needs[(7, 8)], needs[(8, 7)])
        assert needs[(1, 1)] <= needs[(5, 5)] <= needs[(5, 8)] <= needs[(7, 8)] and needs[(8, 3)] <= needs[(8, 7)]
        if not dual and prec == L.PREC_FP32:
            assert max(needs.values()) <= lib.swf_patch_workspace_bytes(2, 8, 8, cin, cout, 2, 2, 4, 4, 0) < max(needs.values()) + 256


STAGE_SHAPES = {"generic_fp32": GENERIC_FP32, "generic_fast": GENERIC_FAST, "deep3": DEEP, "deep4": DEEP4, "window": WINDOW, "window16": WINDOW16,
                "window96_16": (_block_desc(96, 8, 12, 16, 384, L.PREC_FAST, cross=1), 2, 32, 16)}


@pytest.mark.parametrize("sched", [0, 1], ids=["latency", "throughput"])
@pytest.mark.parametrize("name", sorted(STAGE_SHAPES))
def test_block_entries_with_a_route_need_exactly_their_query(name, sched):
    """swf_basic_block_fwd_route shares swf_basic_block_fwd's query.  swf_block_stage_fwd_prec: the eight packed images and the room of
    block_pair4_impl are one carve, checked before the first launch (the pack); the query is a multiple of the carve alignment, covers
    the images plus the largest need of the four blocks, and for the 16x16 kernels that cannot run in place the two temporary maps."""
    lib = L.lib()
    d0, b, h, w = STAGE_SHAPES[name]
    desc = L.BlockDesc(d0.attn, d0.hidden, d0.cross, d0.precision, sched)
    four = lambda: (L.BlockStreamParams * 4)(*[_stream_params() for _ in range(4)])
    px, py = four(), four()
    route = (C.c_int32 * 4)(-7, -7, -7, -7)
    need1 = lib.swf_basic_block_workspace_bytes(C.byref(desc), b, h, w)
    block = lambda ws, n: lib.swf_basic_block_fwd_route(C.byref(desc), px, py, P, 2 * P, P, 2 * P, b, h, w, route, ws, n, None)
    if name == "window96_16":            # (at this map the generic composition, which the query also covers, needs more than the fused route)
        _named_need_at_most(block, need1)
    else:
        _refuses(block, need1)
    need = lib.swf_block_stage_prec_workspace_bytes(C.byref(desc), 1, b, h, w)
    assert need % 256 == 0
    _refuses(lambda ws, n: lib.swf_block_stage_fwd_prec(C.byref(desc), px, py, P, 2 * P, P, 2 * P, b, h, w, None, None, route, ws, n, None), need)
    assert list(route) == [-7] * 4   # a refused call reports no route
    fast = desc.precision == L.PREC_FAST
    images = 8 * max(lib.swf_basic_block_packed_bytes(C.byref(desc)) // 2, 0) if fast else 0
    maps = 2 * b * h * w * desc.attn.channels * 4
    if name.startswith("window"):       # the blocks carve nothing when their images are given; the 16x16 kernels at C = 48 / 96: + two maps
        assert images > 0 and need == images + (maps if "16" in name else 0)
    elif name.startswith("deep"):       # eight deep-level images (they have no public size query) in front of one block's need
        assert need > need1 and (need - need1) % 8 == 0
    else:                                # no images: the room of one block
        assert need == need1
    one = lib.swf_block_stage_prec_workspace_bytes(C.byref(desc), 0, b, h, w)
    assert 0 < one <= need and one % 256 == 0
    _refuses(lambda ws, n: lib.swf_block_stage_fwd_prec(C.byref(desc), px, None, P, None, P, None, b, h, w, None, None, route, ws, n, None), one)


def _model_desc(cfg, prec, sched):
    d = L.ModelDesc()
    d.levels = cfg.n_levels
    for j in range(cfg.n_levels):
        d.in_dims[j], d.out_dims[j], d.head_dim[j] = cfg.in_dims_list[j], cfg.out_dims_list[j], cfg.dims_per_head(j)
    d.heads, d.mlp_ratio = cfg.att_num_heads, cfg.mlp_hidden_dims_ratio
    (d.win_h, d.win_w), (d.merge_h, d.merge_w) = cfg.window_size, cfg.merging_size
    d.head_ksize, d.precision, d.schedule = cfg.final_conv_layer_kernel_size, prec, sched
    return d


@pytest.mark.parametrize("name,hw", [("win8", 256), ("win7", 224), ("win16", 512), ("tiny", 16)])
def test_model_forward_needs_exactly_its_query(name, hw):
    lib = L.lib()
    for prec in (L.PREC_FP32, L.PREC_FAST):
        for sched in (0, 1):
            d = _model_desc(CONFIGS[name], prec, sched)
            need = lib.swf_model_workspace_bytes(C.byref(d), 2, hw, hw)
            _refuses(lambda ws, n: lib.swf_model_forward(C.byref(d), P, P, P, P, 2, hw, hw, ws, n, None), need)


def test_invalid_shapes_give_zero_from_every_query():
    lib = L.lib()
    bd, ad = GENERIC_FP32[0], GENERIC_FP32[0].attn
    md = _model_desc(CONFIGS["tiny"], L.PREC_FAST, 0)
    for b, h, w in ((0, 8, 8), (2, 0, 8), (2, 8, -4)):
        for q in (lib.swf_basic_block_workspace_bytes, lib.swf_basic_block_bwd_workspace_bytes, lib.swf_basic_block_drop_workspace_bytes):
            assert q(C.byref(bd), b, h, w) == 0
        for q in (lib.swf_window_attention_workspace_bytes, lib.swf_window_attention_bwd_workspace_bytes, lib.swf_window_attention_drop_workspace_bytes):
            assert q(C.byref(ad), b, h, w) == 0
        assert lib.swf_model_workspace_bytes(C.byref(md), b, h, w) == 0
        assert lib.swf_block_stage_prec_workspace_bytes(C.byref(bd), 1, b, h, w) == 0
        assert lib.swf_final_head_bwd_workspace_bytes(b, h, w, 3) == 0
        for enc in (0, 1):
            assert lib.swf_patch_workspace_bytes(b, h, w, 8, 16, 2, 2, 4, 4, enc) == 0
            assert lib.swf_patch_layer_bwd_workspace_bytes(b, h, w, 8, 16, 2, 2, enc) == 0
    for enc in (0, 1):
        assert lib.swf_patch_workspace_bytes(2, 8, 8, 0, 16, 2, 2, 4, 4, enc) == 0 and lib.swf_patch_workspace_bytes(2, 8, 8, 8, 16, 0, 2, 4, 4, enc) == 0
    assert lib.swf_patch_workspace_bytes(2, 8, 8, 8, 16, 2, 2, 8, 8, 1) == 0      # window pad of the merged 4x4 map >= the map
    assert lib.swf_model_workspace_bytes(C.byref(md), 2, 2, 2) == 0               # reflect pad >= map at the second level
    md.levels = 0
    assert lib.swf_model_workspace_bytes(C.byref(md), 2, 16, 16) == 0
    assert lib.swf_model_workspace_bytes(None, 2, 16, 16) == 0 and lib.swf_basic_block_workspace_bytes(None, 2, 8, 8) == 0
    for n, c, hid in ((0, 8, 32), (64, 0, 32), (64, 8, -1)):
        assert lib.swf_mlp_workspace_bytes(L.PREC_FAST, n, c, hid) == 0 and lib.swf_linear_workspace_bytes(L.PREC_FAST, n, c, hid) == 0
        assert lib.swf_mlp_bwd_workspace_bytes(n, c, hid) == 0 and lib.swf_mlp_drop_workspace_bytes(n, c, hid) == 0
    assert lib.swf_layernorm_bwd_workspace_bytes(0, 8) == 0 and lib.swf_layernorm_bwd_workspace_bytes(64, 0) == 0


def test_final_head_fwd_takes_the_documented_size():
    """No size query: include/swinfuse.h documents 2*B*H*W floats.  One byte less is refused and the text names exactly that size,
    aligned or not (tests/test_gpu_workspace_exact.py runs it with exactly that many bytes)."""
    lib = L.lib()
    hp = L.HeadParams(P, P, P, P, P, P, P, P)
    for b, h, w in ((3, 5, 7), (1, 16, 65), (2, 16, 16)):
        need = 2 * b * h * w * 4
        for ws, n in ((P, need - 1), (None, 0)):
            assert lib.swf_final_head_fwd(C.byref(hp), P, P, P, b, h, w, 3, ws, n, None) == L.ERR_WORKSPACE
            assert int(NEED.search(lib.swf_last_error_string()).group(1)) == need
