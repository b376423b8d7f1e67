"""GPU parity (run on MI355X with `-m gpu`): every call goes through the C-ABI of libswinfuse.so and is
compared with (a) golden vectors captured from the real reference and (b) the CPU oracle on the same
seeded inputs.  Bars: exact-fp32 tier <= 2e-5 relative (summation-order noise only); 'fast' precision
<= 1e-3 relative (the north-star tolerance; SURVEY.md §7 hard part 3), metric = rel-L2 and max|err|/max|ref|.
"""
import os

import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import (CONFIGS, AddAndLayerNormWithOtherModule, AutoPathMLP, AutoPathWinAtt, BasicBlock,
                                        MyModel, MyPadding, NormalAndShiftWinsBlockPair, PatchMergingAndLinearLayer,
                                        SelfAndCrossBlockPair, StateRecorder, WindowAttention, load_recipe_into, synthetic_pair)
from swin_unet_image_fusion_amd.shard import ShardedFusion
from tests import golden_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_FP32 = 2e-5
TOL_FAST_L2 = 1e-3
# max|err| / max|ref|: the same 1e-3 as the rel-L2 bar (north star: "within 1e-3 relative").  Measured on MI355X
# (profiles/r02_parity.json): whole-model fixtures <= 4e-4, single blocks with stress weights <= 6e-4.
TOL_FAST_MAX = 1e-3

_PARITY_LOG = []   # (test id, rel-L2, max-rel): dumped to gpurun_out/parity.json at the end of the module


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    torch.set_grad_enabled(False)
    yield
    torch.set_grad_enabled(True)
    # per-fixture parity numbers of this run (copied into profiles/ by hand when they are to be judged)
    import json, os
    if os.environ.get("SWF_PARITY_LOG") == "0":   # child runs of tests/test_gpu_switches.py must not overwrite the full record
        return
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "parity.json"), "w") as f:
            json.dump({"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref|; ref = golden vector captured from the "
                                 "reference (or the CPU oracle where the test says so)",
                       "gates": {"fp32": TOL_FP32, "fp32_model": 5e-5, "fast_rel_l2": TOL_FAST_L2, "fast_max_rel": TOL_FAST_MAX},
                       "records": [{"test": t, "rel_l2": a, "max_rel": b} for t, a, b in _PARITY_LOG]}, f, indent=1)
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _test_id(request):
    global _CUR_TEST
    _CUR_TEST = request.node.name
    yield


_CUR_TEST = ""


def _close(got, exp, tol=TOL_FP32, tol_max=None):
    got = got.detach().cpu()
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert torch.isfinite(got).all()
    l2, mx = G.rel_err(got, exp)
    _PARITY_LOG.append((_CUR_TEST, l2, mx))
    assert l2 <= tol and mx <= (tol_max or tol), (l2, mx)
    return l2, mx


def _elu():
    return nn.ELU(inplace=True)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", G.cases("window_attention"))
def test_window_attention(name, precision):
    """a001:448-474 as a stand-alone module, both arithmetic tiers (swf_window_attention_fwd_prec)."""
    meta, arr = G.load(name)
    c = meta["ctor"]
    m = WindowAttention(**c).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.precision = precision
    q = G.randn(meta["in_shape"], meta["seed_q"]).to(DEV)
    kv = G.randn(meta["in_shape"], meta["seed_kv"]).to(DEV) if c["use_cross_attention"] else q
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(m(q, kv, kv), arr["expected"], tol, tmax)
    assert m.forward_(q, kv, kv).shape == q.shape


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", G.cases("basic_block"))
def test_basic_block(name, precision):
    meta, arr = G.load(name)
    m = BasicBlock(**meta["ctor"], mlp_activation_func=_elu()).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.precision = precision
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    ox, oy = m(x, y)
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, arr["expected_x"], tol, tmax)
    _close(oy, arr["expected_y"], tol, tmax)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", G.cases("self_and_cross_block_pair"))
def test_self_and_cross_block_pair(name, precision):
    meta, arr = G.load(name)
    m = SelfAndCrossBlockPair(**meta["ctor"], mlp_activation_func=_elu()).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.precision = precision
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    ox, oy = m(x, y)
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, arr["expected_x"], tol, tmax)
    _close(oy, arr["expected_y"], tol, tmax)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", G.cases("normal_and_shift_block_pair"))
def test_normal_and_shift_block_pair(name, precision):
    """NormalAndShiftWinsBlockPair.forward (a009:90-109) called directly: plain-window block, then shifted-window block."""
    meta, arr = G.load(name)
    m = NormalAndShiftWinsBlockPair(**meta["ctor"], mlp_activation_func=_elu()).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.normal_window_block.precision = m.shifted_window_block.precision = precision
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    ox, oy = m(x, y)
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, arr["expected_x"], tol, tmax)
    _close(oy, arr["expected_y"], tol, tmax)
    fx, fy = m.forward_(x, y)
    assert torch.equal(fx, ox) and torch.equal(fy, oy)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_inner_modules_compose_like_the_block(precision):
    """AutoPathWinAtt / AutoPathMLP / AddAndLayerNormWithOtherModule (a002-a004) each have a HIP-backed
    forward in both tiers; composing them by hand reproduces BasicBlock (a005:138-141) and the golden vector."""
    meta, arr = G.load("bb_cross_shift_w8")
    m = BasicBlock(**meta["ctor"], mlp_activation_func=_elu()).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = precision
    tol = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close_ = lambda a, b: _close(a, b, *tol)
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    assert isinstance(m.stage_1, AddAndLayerNormWithOtherModule) and isinstance(m.auto_path_win_att, AutoPathWinAtt)
    x1, y1 = m.stage_1(x, y)
    x2, y2 = m.stage_2(x1, y1)
    _close_(x2, arr["expected_x"]); _close_(y2, arr["expected_y"])
    # the un-normed sub-modules against the oracle
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    c = meta["ctor"]
    ax, ay = m.auto_path_win_att(x, y)
    rx, ry = O.auto_path_win_att(sd, "auto_path_win_att.", x.cpu(), y.cpu(), cross=True, num_heads=c["num_heads"],
                                 dims_per_head=c["dims_per_head"], window_size=tuple(c["window_size"]), use_cyclic_shift=True)
    _close_(ax, rx); _close_(ay, ry)
    assert isinstance(m.auto_path_mlp, AutoPathMLP)
    mx, my = m.auto_path_mlp(x, y)
    rx, ry = O.auto_path_mlp(sd, "auto_path_mlp.", x.cpu(), y.cpu())
    _close_(mx, rx); _close_(my, ry)


_HALVES = [  # levels 0 / 1 through the fused half-block kernels (window24 / window48_kernel<.., attention half / MLP half>): C, win, hidden, dual, cross, shift, (B,H,W)
    (24, 8, 96, True, True, True, (2, 16, 24)),
    (24, 8, 96, True, False, False, (1, 24, 8)),
    (24, 8, 96, False, False, True, (1, 8, 16)),      # single-path block: one stream through the two-stream kernel
    (24, 7, 96, True, True, True, (1, 14, 21)),
    (24, 8, 4, True, True, False, (3, 8, 8)),         # decoder width: hidden 4
    (48, 8, 192, True, True, True, (2, 16, 24)),
    (48, 8, 96, True, False, True, (1, 8, 24)),       # decoder width
    (48, 8, 192, False, False, False, (3, 8, 8)),
    (48, 7, 192, True, True, True, (1, 21, 14)),
    (96, 8, 384, True, True, True, (1, 16, 24)),
    (96, 8, 192, True, False, False, (2, 8, 8)),      # decoder width
    (96, 8, 384, False, False, True, (1, 16, 8)),
    (96, 7, 384, True, True, True, (1, 14, 14)),
]


@pytest.mark.parametrize("case", _HALVES, ids=[f"C{c[0]}_w{c[1]}_hid{c[2]}_dual{int(c[3])}_c{int(c[4])}s{int(c[5])}" for c in _HALVES])
def test_standalone_halves_level0_fast_vs_oracle(case):
    """a004 around a002 / a003 and the bare a002 / a003 / a001 modules at C = 24 / 48 / 96 in the fast tier: each is ONE launch of the level's
    block kernel with the other half compiled out; compared with the oracle's functions of the same names."""
    C_, win, hid, dual, cross, shift, (b, h, w) = case
    m = BasicBlock(C_, 8, C_ // 8, (win, win), shift, dual, cross, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=31, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, C_, h, w), 701), G.randn((b, C_, h, w), 702)
    m.to(DEV)
    for sub in m.modules():
        if hasattr(sub, "precision"):
            sub.precision = "fast"
    xd, yd = x.to(DEV), (y.to(DEV) if dual else None)
    kw = dict(num_heads=8, dims_per_head=C_ // 8, window_size=(win, win), use_cyclic_shift=shift)
    chk = lambda got, ref: _close(got, ref, TOL_FAST_L2, TOL_FAST_MAX)
    if dual:
        rx, ry = O.auto_path_win_att(sd, "auto_path_win_att.", x, y, cross=cross, **kw)
        ax, ay = m.auto_path_win_att(xd, yd)
        chk(ax, rx); chk(ay, ry)
        rx, ry = O.auto_path_mlp(sd, "auto_path_mlp.", x, y)
        ax, ay = m.auto_path_mlp(xd, yd)
        chk(ax, rx); chk(ay, ry)
        # the two pre-norm residual halves compose to the block (a005:138-141)
        bx, by = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=8, dims_per_head=C_ // 8, window_size=(win, win))
        x1, y1 = m.stage_1(xd, yd)
        x2, y2 = m.stage_2(x1, y1)
        chk(x2, bx); chk(y2, by)
    else:
        wa = m.auto_path_win_att.window_attention_x
        chk(wa(xd, xd, xd), O.window_attention(sd, "auto_path_win_att.window_attention_x.", x, x, x, **kw))
        x1 = m.stage_1(xd, None)
        x2 = m.stage_2(x1, None)
        full = m(xd)
        full = full[0] if isinstance(full, tuple) else full
        chk(x2, full.cpu())      # the fused single-path block (generic fast tier) and the two fused halves agree within the tier's bar


@pytest.mark.parametrize("name", G.cases("patch_layer"))
def test_patch_layer(name):
    meta, arr = G.load(name)
    m = PatchMergingAndLinearLayer(belongs_to_encoder=meta["encoder"], use_dual_path=True, in_dims=meta["in_dims"],
                                   out_dims=meta["out_dims"], patch_merging_size_recorder=StateRecorder(),
                                   merging_or_unmerging_size=(2, 2), activation_func=_elu()).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    ox, oy = m(x, y)
    _close(ox, arr["expected_x"]); _close(oy, arr["expected_y"])


@pytest.mark.parametrize("name", G.cases("padding"))
def test_padding_roundtrip(name):
    meta, arr = G.load(name)
    fr, pr = StateRecorder(), StateRecorder()
    enc = MyPadding(True, tuple(meta["window"]), True, fr, pr).eval()
    dec = MyPadding(False, tuple(meta["window"]), True, fr, pr).eval()
    x, y = G.randn(meta["in_shape"], meta["seed_x"]).to(DEV), G.randn(meta["in_shape"], meta["seed_y"]).to(DEV)
    px, py = enc(x, y)
    assert torch.equal(px.cpu(), arr["padded_x"]) and torch.equal(py.cpu(), arr["padded_y"])   # copies: bit-exact
    ux, uy = dec(px, py)
    assert torch.equal(ux, x) and torch.equal(uy, y)
    assert fr.record_stack == [] and pr.record_stack == []


_MODEL_CASES = G.cases("model")


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("name", _MODEL_CASES)
def test_model_golden(name, precision):
    meta, arr = G.load(name)
    cfg = CONFIGS[meta["config"]]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.precision = precision
    ir, vis = G.model_inputs(meta)
    out = m(ir.to(DEV), vis.to(DEV))
    if precision == "fp32":
        l2, mx = _close(out, arr["expected"], 5e-5)
    else:
        l2, mx = _close(out, arr["expected"], TOL_FAST_L2, TOL_FAST_MAX)
    print(f"{name} [{precision}] rel-L2={l2:.2e} max-rel={mx:.2e}")


@pytest.mark.parametrize("name", [n for n in _MODEL_CASES if any(k in n for k in ("win8_256", "win7_224", "win7_200", "win8_b2", "win8_512"))])
def test_model_golden_throughput_schedule(name):
    """model.schedule = 'throughput' (what ShardedFusion's lanes run): the kernel shapes chosen for several forwards in flight — four
    waves per window at level 2, 64-token MLP tiles at level 3 — against the reference goldens at the fast tier's gates; the batch
    dimension stays separable in this schedule too (shards of a batch are bit-identical rows)."""
    meta, arr = G.load(name)
    cfg = CONFIGS[meta["config"]]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=meta["weight_seed"], flavor=meta["flavor"])
    m.to(DEV)
    m.schedule = "throughput"
    ir, vis = (t.to(DEV) for t in G.model_inputs(meta))
    out = m(ir, vis)
    l2, mx = _close(out, arr["expected"], TOL_FAST_L2, TOL_FAST_MAX)
    print(f"{name} [fast, throughput] rel-L2={l2:.2e} max-rel={mx:.2e}")
    ir4, vis4 = torch.cat([ir, vis, ir, vis]), torch.cat([vis, ir, vis, ir])
    full = m(ir4, vis4)
    assert torch.equal(full[:ir.shape[0]], out)
    assert torch.equal(m(ir4[2 * ir.shape[0]:], vis4[2 * ir.shape[0]:]), full[2 * ir.shape[0]:])
    m.schedule = "latency"
    lat = m(ir, vis)
    _close(lat, arr["expected"], TOL_FAST_L2, TOL_FAST_MAX)
    with pytest.raises(ValueError):
        m.schedule = "fastest"
        m(ir, vis)


def test_model_error_behaviour():
    m = MyModel(**CONFIGS["win8"].model_kwargs(_elu())).eval().to(DEV)
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(1, 128, 128))
    with pytest.raises(RuntimeError):      # BASELINE config 1 as literally written: reflect pad 4 on a 4x4 map (a006:128)
        m(ir, vis)
    wa = WindowAttention(8, 2, 4, (4, 4), True, False, True, 0.0, 0.0).eval().to(DEV)
    bad = torch.zeros(1, 8, 6, 8, device=DEV)
    with pytest.raises(ValueError):        # einops error in the reference: map not a multiple of the window
        wa(bad, bad, bad)
    blk = BasicBlock(8, 2, 4, (4, 4), False, True, True, True, 0.0, 0.0, 16, _elu(), 0.0).eval().to(DEV)
    same = torch.ones(1, 8, 8, 8, device=DEV)
    with pytest.raises(ValueError):        # a005:111-118 (reference: exit())
        blk(same, same.clone())


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_full_size_batch_properties(precision):
    """BASELINE config 2 (B=16, 256x256, win 8) at full size: no CPU oracle run of that size in the test
    budget, so parity rides on size-independent properties — sample 0 equals the B=1 golden vector, the
    batch dimension is separable (any shard of the batch gives bit-identical rows: the multi-GPU
    contract), and repeated launches are bit-identical."""
    meta, arr = G.load("model_win8_256_default")
    cfg = CONFIGS["win8"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=0, flavor="default")
    m.to(DEV)
    m.precision = precision
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(16, 256, 256))
    out = m(ir, vis)
    assert torch.isfinite(out).all()
    tol = (5e-5, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(out[:1], arr["expected"], *tol)
    assert torch.equal(m(ir, vis), out)
    lo, hi = m(ir[:8].contiguous(), vis[:8].contiguous()), m(ir[8:].contiguous(), vis[8:].contiguous())
    assert torch.equal(torch.cat([lo, hi]), out)
    one = m(ir[5:6].contiguous(), vis[5:6].contiguous())
    assert torch.equal(one, out[5:6])


def _full_size_properties(cfg_name, golden, batch, size, precision):
    """finite; sample 0 == the B=1 golden vector of the reference; repeat == repeat; batch shards == rows of the full batch"""
    meta, arr = G.load(golden)
    cfg = CONFIGS[cfg_name]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=0, flavor="default")
    m.to(DEV)
    m.precision = precision
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(batch, size, size))
    out = m(ir, vis)
    assert out.shape == (batch, 1, size, size) and torch.isfinite(out).all()
    tol = (5e-5, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(out[:1], arr["expected"], *tol)
    assert torch.equal(m(ir, vis), out)
    half = batch // 2
    lo, hi = m(ir[:half].contiguous(), vis[:half].contiguous()), m(ir[half:].contiguous(), vis[half:].contiguous())
    assert torch.equal(torch.cat([lo, hi]), out)
    one = m(ir[batch - 3:batch - 2].contiguous(), vis[batch - 3:batch - 2].contiguous())
    assert torch.equal(one, out[batch - 3:batch - 2])


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_full_size_config3_b16_512(precision):
    """BASELINE config 3 at full size: B=16 512x512, win 8 (65 536 level-0 windows, 256x256 merge maps)."""
    _full_size_properties("win8", "model_win8_512_default", 16, 512, precision)


def test_full_size_config5_b8_1024_win16():
    """BASELINE config 5 at full size: B=8 1024x1024, win 16 (t = 256 tokens per window), fast tier (the tier the
    benchmark measures; the exact tier at this size is covered at B=1 512x512 by model_win16_512)."""
    _full_size_properties("win16", "model_win16_1024_default", 8, 1024, "fast")


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_full_size_default_window7_b16_224(precision):
    """The reference's own default configuration (A000_CONFIG.py:55: 7x7 windows) at B=16 224x224: every level on its fused kernel
    (7x7 windows on the 8x8 token grid); sample 0 against the vector captured from the reference."""
    _full_size_properties("win7", "model_win7_224_default", 16, 224, precision)


def test_reference_checkpoint_to_gpu_forward(tmp_path):
    """a checkpoint in the reference's on-disk format (a016:243-249: model_state + optimizer / scheduler
    state + epoch) -> load_reference_checkpoint (weights_only loader, strict 3139-style key set) -> HIP forward ->
    oracle on the same weights (a017:50-54 then a017:72)."""
    cfg = CONFIGS["win8_4stage"]
    src = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(src, seed=17, flavor="stress")
    sd = {k: v.detach().clone() for k, v in src.state_dict().items()}
    path = tmp_path / "state.pth"
    torch.save({"model_state": src.state_dict(), "optimizer_state": {"state": {}, "param_groups": []},
                "scheduler_state": {"last_epoch": 3}, "current_epoch": 3}, path)
    m = MyModel(**cfg.model_kwargs(_elu())).eval().to(DEV)
    extra = m.load_reference_checkpoint(str(path))
    assert extra["current_epoch"] == 3 and "optimizer_state" in extra
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(2, 128, 128, seed_ir=21, seed_vis=22))
    # These stress weights (seed 17) put a patch of ill-conditioned pixels at (b=0, y 45..48, x 64..66): the reference's own fp32
    # answer differs from an fp64 evaluation by 5.5e-6 there, 44x its median (tests/diag_ckpt.py).  The max-error gate is the
    # north star's 1e-3 of max|ref| plus C_ROUNDOFF x the measured fp32 uncertainty (CPU oracle and the GPU's exact tier, both against fp64), and every pixel that needs the second term
    # must be ill-conditioned by the fp64 measure (golden_util.close_conditioned); rel-L2 stays at 1e-3.
    m.precision = "fp32"
    exact = m(ir.to(DEV), vis.to(DEV)).cpu()
    ref, u, pooled, med = G.fp64_uncertainty(O.model_forward, sd, cfg, ir, vis, extra_fp32=(exact,))
    assert float(u.max()) >= G.K_ILL * med      # the conditioning story itself: the fp32 reference is that uncertain somewhere
    _close(exact, ref, 5e-5, None)
    m.precision = "fast"
    l2, mx, n_ill = G.close_conditioned(m(ir.to(DEV), vis.to(DEV)), ref, pooled, med, TOL_FAST_L2, TOL_FAST_MAX)
    _PARITY_LOG.append((_CUR_TEST + "[fast, fp64-conditioned gate, %d pixels beyond 1e-3]" % n_ill, l2, mx))


def _mirror_x_into_y(model):
    """copy every x-stream parameter over its y-stream twin: the two streams then compute the same function"""
    sd = model.state_dict()
    pairs = (("window_attention_x.", "window_attention_y."), ("mlp_x_", "mlp_y_"), ("sequence_x.", "sequence_y."),
             ("norm_layer_1.", "norm_layer_2."), ("mlp_layer_x.", "mlp_layer_y."), ("layer_norm_x.", "layer_norm_y."))
    new = dict(sd)
    for k, v in sd.items():
        for a, b in pairs:
            if a in k and k.replace(a, b) in sd:
                new[k.replace(a, b)] = v.clone()
    model.load_state_dict(new, strict=True)


def test_model_first_forward_identical_streams_guard():
    """a005:98-118: on a model's first forward the reference tests `(x == y).all()` in front of every cross-attention
    block and calls exit(); here MyModel.forward raises ValueError (and the oracle does too).  With mirrored stream
    weights and ir == vis the two streams stay identical up to the first cross block."""
    cfg = CONFIGS["tiny"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=5, flavor="stress")
    _mirror_x_into_y(m)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ir, _ = (torch.from_numpy(a) for a in synthetic_pair(1, 16, 16))
    with pytest.raises(ValueError):
        O.model_forward(sd, cfg, ir, ir.clone())
    m.to(DEV)
    for precision in ("fp32", "fast"):
        m.precision = precision
        m.input_compatibility_with_cross_option = None
        for _ in range(2):   # a failed check is not remembered: the same bad inputs raise again on the next call
            with pytest.raises(ValueError):
                m(ir.to(DEV), ir.clone().to(DEV))
            assert m.input_compatibility_with_cross_option is None
    # distinct inputs pass the check once, later forwards skip it (as the reference does)
    ok = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(ok, seed=5, flavor="stress")
    ok.to(DEV)
    a, b = (torch.from_numpy(t).to(DEV) for t in synthetic_pair(1, 16, 16))
    first = ok(a, b)
    assert ok.input_compatibility_with_cross_option is True
    assert torch.equal(ok(a, b), first)


def test_sharded_fusion_graph_replay_follows_weights_and_inputs():
    """ShardedFusion(use_graph=True) at world_size 1 — the path bench.py times: replay == eager for different inputs, the
    caller's tensors are never adopted or mutated, and load_state_dict / a precision change re-capture instead of
    replaying freed weight addresses."""
    cfg = CONFIGS["win8_4stage"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=0, flavor="default")
    m.to(DEV)
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True)
    ir1, vis1 = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 1, 2))
    ir2, vis2 = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 3, 4))
    keep = ir1.clone()
    o1 = runner.step(ir1, vis1).clone()
    assert runner.graph_active and runner.captures == 1
    assert torch.equal(o1, m(ir1, vis1))
    o2 = runner.step(ir2, vis2).clone()
    assert runner.captures == 1 and torch.equal(o2, m(ir2, vis2)) and not torch.equal(o1, o2)
    assert torch.equal(ir1, keep)                       # the first batch was copied, not adopted as the static buffer
    other = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(other, seed=9, flavor="stress")
    m.load_state_dict(other.state_dict(), strict=True)   # drops the arena and the packed images the graph points at
    o3 = runner.step(ir1, vis1).clone()
    assert runner.captures == 2
    assert torch.equal(o3, m(ir1, vis1)) and not torch.equal(o3, o1)
    assert torch.equal(o3, other.to(DEV)(ir1, vis1))
    m.precision = "fp32"
    o4 = runner.step(ir1, vis1).clone()
    assert runner.captures == 3 and torch.equal(o4, m(ir1, vis1)) and not torch.equal(o4, o3)
    assert torch.equal(runner.fuse_global(ir2, vis2), m(ir2, vis2))


def test_graph_runner_keeps_the_workspace_its_graph_points_into():
    """A captured hipGraph bakes in the address of the library workspace registered for (device, capture-stream handle).  That
    registry replaces (and frees) the buffer when a later call on the same handle needs more bytes — e.g. another model with a larger
    shape that lands on a recycled stream handle.  The runner holds the tensor, so a replay after such a growth still reads and writes
    live memory and equals the eager forward."""
    from swin_unet_image_fusion_amd import modules as M
    cfg = CONFIGS["win8_4stage"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=0, flavor="default")
    m.to(DEV)
    runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True)
    ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 5, 6))
    first = runner.step(ir, vis).clone()
    assert runner.graph_active and runner._ws_ref is not None
    held_ptr, held_bytes = runner._ws_ref.data_ptr(), runner._ws_ref.numel()
    key = (torch.device(DEV).index, runner._cap_stream.cuda_stream)
    assert M._WS[key].data_ptr() == held_ptr
    with torch.cuda.stream(runner._cap_stream):     # a later, larger request on the same stream handle
        M._workspace(4 * held_bytes, torch.device(DEV))
    torch.cuda.synchronize()
    assert M._WS[key].data_ptr() != held_ptr and runner._ws_ref.data_ptr() == held_ptr     # registry moved on, the runner's buffer is alive
    junk = torch.full((held_bytes,), 0x7F, dtype=torch.uint8, device=DEV)                  # would land on the freed block without the hold
    again = runner.step(ir, vis)
    assert torch.equal(again, first) and torch.equal(again, m(ir, vis))
    del junk


def test_pipelined_gather_on_a_one_rank_rccl_group():
    """The GPU branch of the collective (all_gather_into_tensor, async, double-buffered) on the only topology a one-GPU box
    offers: a one-rank RCCL group.  Steps are issued bench.py's way — the wait for step i comes after step i+1 was enqueued —
    and each handle must hold its own step's output."""
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29700 + os.getpid() % 200))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
        created = True
    try:
        cfg = CONFIGS["win8_4stage"]
        m = MyModel(**cfg.model_kwargs(_elu())).eval()
        load_recipe_into(m, seed=0, flavor="default")
        m.to(DEV)
        runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True, force_collective=True)
        ir1, vis1 = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 1, 2))
        ir2, vis2 = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 3, 4))
        h1 = runner.step_async(ir1, vis1)
        h2 = runner.step_async(ir2, vis2)
        g1, g2 = h1.wait(), h2.wait()
        h3 = runner.step_async(ir1, vis1)   # reuses g1's buffers only now
        assert g1.data_ptr() != g2.data_ptr()
        assert torch.equal(g2, m(ir2, vis2))
        g3 = h3.wait()
        assert g3.data_ptr() == g1.data_ptr() and torch.equal(g3, m(ir1, vis1))
        assert torch.equal(runner.step(ir2, vis2), m(ir2, vis2))
    finally:
        if created:
            dist.destroy_process_group()


def test_concurrent_streams_really_overlap():
    """shard.concurrent_streams: the streams it returns run spin kernels side by side (one spin time for all of them), pairs of them
    too, and none of them shares a hardware queue with the caller's stream."""
    from swin_unet_image_fusion_amd.shard import _spin_ms, concurrent_streams
    dev = torch.device(DEV)
    cur = torch.cuda.current_stream(dev)
    ss = concurrent_streams(dev, 3, avoid=[cur])
    assert len(ss) >= 2 and len({s.cuda_stream for s in ss}) == len(ss)
    cycles = 400_000
    one = min(_spin_ms([ss[0]], cycles) for _ in range(3))
    while one < 0.3 and cycles < 1 << 30:
        cycles *= 2
        one = min(_spin_ms([ss[0]], cycles) for _ in range(3))
    ratio = lambda group: min(_spin_ms(group, cycles) / max(_spin_ms(group[:1], cycles), 1e-6) for _ in range(3))
    assert ratio(ss) < 1.5, ratio(ss)
    assert ratio([ss[0], cur]) < 1.5 and ratio([ss[-1], cur]) < 1.5
    assert ratio([ss[0], ss[0]]) > 1.7          # (the measurement does see a shared queue: the same stream twice runs in order)


@pytest.mark.parametrize("lanes", [2, 3])
@pytest.mark.parametrize("collective", [False, True], ids=["local", "one_rank_rccl"])
def test_steps_in_flight_keep_their_own_results(collective, lanes):
    """ShardedFusion(in_flight=2), the way bench.py drives it: step i+1 is enqueued on the other lane (own hipGraph, static buffers,
    workspace, stream) before step i is waited for.  Six different batches: every handle must deliver its own step's output, equal
    bit for bit to the eager forward; a weight change re-captures both lanes."""
    import torch.distributed as dist
    created = False
    if collective and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29700 + os.getpid() % 200))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
        created = True
    try:
        cfg = CONFIGS["win8_4stage"]
        m = MyModel(**cfg.model_kwargs(_elu())).eval()
        load_recipe_into(m, seed=0, flavor="default")
        m.to(DEV)
        runner = ShardedFusion(m, world_size=1, rank=0, use_graph=True, in_flight=lanes, force_collective=collective)
        batches = [tuple(torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 128, 128, 10 + 2 * i, 11 + 2 * i)) for i in range(7)]
        want = [m(ir, vis).clone() for ir, vis in batches]
        got, pending = [], []
        for ir, vis in batches:
            pending.append(runner.step_async(ir, vis))
            if len(pending) == lanes:
                got.append(pending.pop(0).wait().clone())
        while pending:
            got.append(pending.pop(0).wait().clone())
        lanes = runner.in_flight          # (the runner keeps as many lanes as it found distinct hardware queues for: >= 2 on this device)
        assert lanes >= 2 and runner.captures == lanes and runner.graph_active
        assert len({ln.stream.cuda_stream for ln in runner._lanes}) == lanes
        assert len({ln.ws_ref.data_ptr() for ln in runner._lanes}) == lanes
        assert not runner._unissued
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), i
        assert not torch.equal(got[0], got[1])
        other = MyModel(**cfg.model_kwargs(_elu())).eval()
        load_recipe_into(other, seed=9, flavor="stress")
        m.load_state_dict(other.state_dict(), strict=True)
        h1, h2 = runner.step_async(*batches[0]), runner.step_async(*batches[1])
        o1, o2 = h1.wait().clone(), h2.wait().clone()
        assert runner.captures == lanes + 2
        assert torch.equal(o1, m(*batches[0])) and torch.equal(o2, m(*batches[1])) and not torch.equal(o1, got[0])
        assert torch.equal(runner.step(*batches[2]), m(*batches[2]))      # step() waits at once: serial use of the same lanes
    finally:
        if created:
            dist.destroy_process_group()


def test_load_state_dict_roundtrip_refreshes_arena():
    cfg = CONFIGS["tiny"]
    a = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(a, seed=3, flavor="stress")
    b = MyModel(**cfg.model_kwargs(_elu())).eval().to(DEV)
    ir, vis = (torch.from_numpy(t).to(DEV) for t in synthetic_pair(1, 16, 16))
    before = b(ir, vis)
    b.load_state_dict(a.state_dict(), strict=True)      # aliased 3139-style key set loads strictly
    after = b(ir, vis)
    ref = a.to(DEV)(ir, vis)
    assert torch.equal(after, ref) and not torch.equal(before, after)


# ---- wider fused shapes: no reference goldens exist at these widths for a single block, so the checker is the
# ---- CPU oracle (itself pinned to the reference by tests/test_oracle_golden.py) on the same seeded inputs
_WIDE = [  # C, heads, d, hidden, (B,H,W), shift, cross
    (48, 8, 6, 192, (2, 16, 24), False, False),
    (48, 8, 6, 192, (1, 16, 16), True, True),
    (48, 8, 6, 96, (1, 24, 16), True, False),      # decoder width (hidden = in_dims * 4)
    (96, 8, 12, 384, (1, 16, 16), True, True),
    (96, 8, 12, 192, (2, 8, 16), False, True),
    (24, 8, 3, 4, (1, 16, 16), True, True),        # level-0 decoder width (hidden 4) as a single block
    # deep-level widths (which kernels serve them is asserted per block by tests/test_gpu_block_fast.py, through the route code)
    (192, 8, 24, 768, (1, 8, 8), True, True),
    (384, 8, 48, 1536, (2, 8, 8), True, False),
    (192, 8, 24, 384, (2, 8, 8), False, True),      # decoder widths (hidden = in_dims * 4)
    (384, 8, 48, 768, (1, 8, 8), True, True),
    (192, 8, 24, 768, (2, 16, 16), True, False),    # 512 tokens per stream
    (192, 8, 24, 768, (1, 16, 24), True, True),     # map larger than 16x16 (256 tokens)
    (128, 4, 24, 512, (1, 8, 16), True, True),      # heads * d (96) != C: projection K = 96; fused MLP instantiation C = 128
    (256, 8, 24, 1024, (1, 8, 8), False, False),    # heads * d = 192; fused MLP instantiation C = 256
]


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("case", _WIDE, ids=[f"C{c[0]}_hid{c[3]}_s{int(c[5])}c{int(c[6])}" for c in _WIDE])
def test_basic_block_wide_vs_oracle(case, precision):
    c, nh, d, hid, shape, shift, cross = case
    b, h, w = shape
    m = BasicBlock(c, nh, d, (8, 8), shift, True, cross, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=21, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 601), G.randn((b, c, h, w), 602)
    rx, ry = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=nh, dims_per_head=d, window_size=(8, 8))
    m.to(DEV)
    m.precision = precision
    ox, oy = m(x.to(DEV), y.to(DEV))
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, rx, tol, tmax)
    _close(oy, ry, tol, tmax)
    # bit-reproducible across launches (no atomics, no data races)
    ox2, oy2 = m(x.to(DEV), y.to(DEV))
    assert torch.equal(ox, ox2) and torch.equal(oy, oy2)


_SINGLE = [  # single-path blocks (use_dual_path=False, a005:54-76): C, heads, d, hidden, (B,H,W), shift
    (24, 8, 3, 96, (2, 16, 16), True),
    (96, 8, 12, 384, (1, 16, 8), False),
    (192, 8, 24, 768, (2, 8, 16), True),     # deep level 3 with one stream
    (384, 8, 48, 1536, (2, 8, 8), True),     # level 4 with one stream
    (384, 8, 48, 768, (1, 8, 16), False),
]


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("case", _SINGLE, ids=[f"C{c[0]}_hid{c[3]}_s{int(c[5])}" for c in _SINGLE])
def test_basic_block_single_stream_vs_oracle(case, precision):
    """BasicBlock.forward(x) of a single-path block: the x half of the dual-path oracle with self attention (the y stream cannot
    reach it), on the same weights."""
    c, nh, d, hid, shape, shift = case
    b, h, w = shape
    dual = BasicBlock(c, nh, d, (8, 8), shift, True, False, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(dual, seed=23, flavor="stress")
    sd = {k: v.detach().clone() for k, v in dual.state_dict().items()}
    x, y = G.randn((b, c, h, w), 611), G.randn((b, c, h, w), 612)
    rx, _ = O.basic_block(sd, "", x, y, cross=False, shift=shift, num_heads=nh, dims_per_head=d, window_size=(8, 8))
    m = BasicBlock(c, nh, d, (8, 8), shift, False, False, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})
    m.to(DEV)
    m.precision = precision
    out = m(x.to(DEV))
    ox = out[0] if isinstance(out, tuple) else out
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, rx, tol, tmax)


_WIN7 = [  # 7x7 windows (the reference's default, A000_CONFIG.py:55) at every level width: C, heads, d, hidden, (B,H,W), shift, cross
    (24, 8, 3, 96, (2, 14, 21), True, True),
    (48, 8, 6, 192, (2, 14, 21), True, True),
    (48, 8, 6, 96, (1, 21, 14), False, False),
    (96, 8, 12, 384, (1, 14, 14), True, True),
    (96, 8, 12, 192, (2, 7, 14), True, False),
    (24, 8, 3, 4, (1, 14, 14), True, True),         # level-0 decoder width, 7x7 windows
    # more than 16 windows per map (tests/test_gpu_block_fast.py asserts which level-2 kernel runs either side of that boundary)
    (96, 8, 12, 384, (1, 35, 35), True, False),
    (96, 8, 12, 192, (1, 35, 35), True, True),
    (192, 8, 24, 768, (2, 14, 14), True, True),
    (192, 8, 24, 384, (1, 7, 7), False, True),
    (384, 8, 48, 1536, (2, 7, 7), True, True),      # one window per map: the shift mask covers most of the score tile
    (384, 8, 48, 768, (1, 14, 7), True, False),
]


@pytest.mark.parametrize("case", _WIN7, ids=[f"C{c[0]}_hid{c[3]}_s{int(c[5])}c{int(c[6])}" for c in _WIN7])
def test_basic_block_window7_fast_vs_oracle(case):
    c, nh, d, hid, shape, shift, cross = case
    b, h, w = shape
    m = BasicBlock(c, nh, d, (7, 7), shift, True, cross, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=23, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 611), G.randn((b, c, h, w), 612)
    rx, ry = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=nh, dims_per_head=d, window_size=(7, 7))
    m.to(DEV)
    m.precision = "fast"
    ox, oy = m(x.to(DEV), y.to(DEV))
    _close(ox, rx, TOL_FAST_L2, TOL_FAST_MAX)
    _close(oy, ry, TOL_FAST_L2, TOL_FAST_MAX)
    ox2, oy2 = m(x.to(DEV), y.to(DEV))
    assert torch.equal(ox, ox2) and torch.equal(oy, oy2)


def test_fused_block_beyond_2gb_runs_in_batch_slices():
    """The register-resident block kernels address a stream's map through 32-bit buffer offsets: a map of 2^31 bytes or more is
    launched in batch slices (kernels_window.hip: launch_window_block).  B=22 at C=96 on a 512x512 map is 2.2 GB per stream =
    slices of 21 + 1 images; images are independent, so every image must equal — bit for bit — the same image run alone."""
    c, nh, d, hid, b, h, w = 96, 8, 12, 384, 22, 512, 512
    assert b * h * w * c * 4 >= 2 ** 31 and 21 * h * w * c * 4 < 2 ** 31
    m = BasicBlock(c, nh, d, (8, 8), True, True, True, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=29, flavor="stress")
    m.to(DEV)
    m.precision = "fast"
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((b, c, h, w), device=DEV, generator=g)
    y = torch.randn((b, c, h, w), device=DEV, generator=g)
    ox, oy = m(x, y)
    assert bool(torch.isfinite(ox).all()) and bool(torch.isfinite(oy).all())
    for i in (0, 20, 21):   # first image, last image of the first slice, the image of the second slice
        sx, sy = m(x[i:i + 1].contiguous(), y[i:i + 1].contiguous())
        assert torch.equal(ox[i:i + 1], sx) and torch.equal(oy[i:i + 1], sy), i
    del x, y, ox, oy
    torch.cuda.empty_cache()


def test_block_prepack_matches_per_call_pack():
    """swf_basic_block_pack + swf_basic_block_fwd_packed == swf_basic_block_fwd (same kernel, weights packed once)."""
    import ctypes as C
    from swin_unet_image_fusion_amd import _lib as L
    from swin_unet_image_fusion_amd.modules import _ptr, _stream
    m = BasicBlock(24, 8, 3, (8, 8), True, True, True, True, 0.0, 0.0, 96, _elu(), 0.0).eval()
    load_recipe_into(m, seed=5, flavor="stress")
    m.to(DEV)
    x, y = G.randn((2, 24, 16, 16), 1).to(DEV), G.randn((2, 24, 16, 16), 2).to(DEV)
    ref_x, ref_y = m(x, y)
    lib = L.lib()
    desc = m._desc("fast")
    n = lib.swf_basic_block_packed_bytes(C.byref(desc))
    assert n > 0
    packed = torch.empty(n, dtype=torch.uint8, device=DEV)
    px, py = m._stream_params("x"), m._stream_params("y")
    L.check(lib.swf_basic_block_pack(C.byref(desc), C.byref(px), C.byref(py), packed.data_ptr(), n, _stream(x.device)))
    xn, yn = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
    ox, oy = torch.empty_like(xn), torch.empty_like(yn)
    L.check(lib.swf_basic_block_fwd_packed(C.byref(desc), packed.data_ptr(), _ptr(xn), _ptr(yn), _ptr(ox), _ptr(oy), 2, 16, 16,
                                           _stream(x.device)))
    assert torch.equal(ox.permute(0, 3, 1, 2), ref_x) and torch.equal(oy.permute(0, 3, 1, 2), ref_y)
    # in place is allowed: a window is read and written by one workgroup only
    L.check(lib.swf_basic_block_fwd_packed(C.byref(desc), packed.data_ptr(), _ptr(xn), _ptr(yn), _ptr(xn), _ptr(yn), 2, 16, 16,
                                           _stream(x.device)))
    assert torch.equal(xn, ox) and torch.equal(yn, oy)
    d32 = m._desc("fp32")
    assert lib.swf_basic_block_packed_bytes(C.byref(d32)) == 0


def test_model_packed_weights_follow_load_state_dict():
    """The fused levels run from a packed weight buffer derived once per arena; load_state_dict must invalidate both."""
    cfg = CONFIGS["win8_4stage"]
    a = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(a, seed=9, flavor="stress")
    b = MyModel(**cfg.model_kwargs(_elu())).eval().to(DEV)
    ir, vis = (torch.from_numpy(t).to(DEV) for t in synthetic_pair(1, 128, 128))
    before = b(ir, vis)
    assert b._packed is not None and b._packed.numel() > 16
    b.load_state_dict(a.state_dict(), strict=True)
    assert b._packed is None and b._arena is None
    after = b(ir, vis)
    assert torch.equal(after, a.to(DEV)(ir, vis)) and not torch.equal(before, after)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_ragged_640x512_vs_oracle(precision):
    """The repo's sample images are 640x512: level maps 320x256 ... 20x16 -> the deepest two need
    reflect padding to a multiple of 8, folded into the merge gather / unmerge scatter index maps; the fused kernels
    then run on the padded maps."""
    cfg = CONFIGS["win8"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=0, flavor="default")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(1, 512, 640))
    ref = O.model_forward(sd, cfg, ir, vis)
    m.to(DEV)
    m.precision = precision
    out = m(ir.to(DEV), vis.to(DEV))
    if precision == "fp32":
        _close(out, ref, 5e-5)
    else:
        _close(out, ref, TOL_FAST_L2, TOL_FAST_MAX)


@pytest.mark.parametrize("precision", ["fp32", "fast"])
def test_nonsquare_batch3_vs_oracle(precision):
    """B=3 384x256 pairs, stress weights: odd batch, non-square maps (192x128 ... 12x8 -> the deepest level needs window
    padding), every fast-tier kernel family at shapes that differ from the benchmark's (window counts that do not divide the
    CU count, 64-token tile tails in the deep-level GEMMs / MLP kernel)."""
    cfg = CONFIGS["win8"]
    m = MyModel(**cfg.model_kwargs(_elu())).eval()
    load_recipe_into(m, seed=3, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(3, 256, 384, seed_ir=11, seed_vis=12))
    ref = O.model_forward(sd, cfg, ir, vis)
    m.to(DEV)
    m.precision = precision
    out = m(ir.to(DEV), vis.to(DEV))
    if precision == "fp32":
        _close(out, ref, 5e-5)
    else:
        _close(out, ref, TOL_FAST_L2, TOL_FAST_MAX)
    # shards of the batch reproduce the rows of the full batch bit for bit (the multi-GPU contract)
    part = m(ir[1:].to(DEV), vis[1:].to(DEV))
    assert torch.equal(part, out[1:])


@pytest.mark.parametrize("case", [(24, 3, 96, (1, 32, 48), True, True), (24, 3, 96, (2, 48, 32), False, False), (24, 3, 4, (1, 32, 32), True, False),
                                  (24, 3, 96, (2, 16, 16), True, True),
                                  (24, 3, 4, (3, 16, 48), False, True), (48, 6, 192, (2, 16, 32), True, False),
                                  (48, 6, 192, (1, 32, 48), True, True), (48, 6, 96, (2, 16, 16), True, True), (48, 6, 96, (1, 48, 32), False, False),
                                  (96, 12, 384, (1, 16, 16), True, True), (96, 12, 192, (2, 32, 16), True, False), (96, 12, 384, (1, 32, 48), False, True),
                                  (192, 24, 768, (1, 32, 16), True, True), (192, 24, 384, (2, 16, 16), False, False),
                                  (384, 48, 1536, (1, 16, 16), False, True)],
                         ids=["C24", "C24_plain_self", "C24_hid4_shift", "C24_onewin", "C24_hid4_cross", "C48", "C48_cross", "C48_hid96_onewin", "C48_hid96_plain", "C96_onewin", "C96_hid192_shift", "C96_plain_cross", "C192_deep_shift_cross", "C192_deep_hid384", "C384_onewin"])
def test_window16_block_fast_vs_oracle(case):
    """16x16 windows (BASELINE config 5): the fast tier runs the MFMA attention core with online softmax over key
    tiles (256-token windows do not fit a score tile in LDS); checked against the oracle incl. a single-window map,
    where the shift mask covers 75 % of the entries."""
    c, d, hid, (b, h, w), shift, cross = case
    m = BasicBlock(c, 8, d, (16, 16), shift, True, cross, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=31, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 701), G.randn((b, c, h, w), 702)
    rx, ry = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=8, dims_per_head=d, window_size=(16, 16))
    m.to(DEV)
    m.precision = "fast"
    ox, oy = m(x.to(DEV), y.to(DEV))
    _close(ox, rx, TOL_FAST_L2, TOL_FAST_MAX)
    _close(oy, ry, TOL_FAST_L2, TOL_FAST_MAX)
    ox2, oy2 = m(x.to(DEV), y.to(DEV))
    assert torch.equal(ox, ox2) and torch.equal(oy, oy2)


_ODD = [  # C, heads, d, win, hidden, (B,H,W), shift, cross — shapes no fused kernel covers
    (5, 3, 2, (2, 3), 7, (2, 4, 9), True, True),        # odd C, heads*d != C, rectangular window, scalar (non-float4) paths
    (10, 2, 5, (4, 8), 20, (1, 8, 16), True, False),
    (7, 1, 7, (7, 7), 3, (1, 14, 7), True, True),        # one head, hidden < C
    (36, 4, 9, (3, 3), 50, (3, 6, 9), False, True),
    (24, 8, 3, (7, 7), 96, (1, 14, 21), True, True),     # model dims with the reference's default window 7
    (64, 2, 64, (4, 4), 128, (1, 8, 8), True, False),    # head_dim at the attention core's limit (64)
]


@pytest.mark.parametrize("precision", ["fp32", "fast"])
@pytest.mark.parametrize("case", _ODD, ids=[f"C{c[0]}_h{c[1]}x{c[2]}_w{c[3][0]}x{c[3][1]}" for c in _ODD])
def test_basic_block_odd_shapes_vs_oracle(case, precision):
    c, nh, d, win, hid, (b, h, w), shift, cross = case
    m = BasicBlock(c, nh, d, win, shift, True, cross, True, 0.0, 0.0, hid, _elu(), 0.0).eval()
    load_recipe_into(m, seed=41, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 801), G.randn((b, c, h, w), 802)
    rx, ry = O.basic_block(sd, "", x, y, cross=cross, shift=shift, num_heads=nh, dims_per_head=d, window_size=win)
    m.to(DEV)
    m.precision = precision
    ox, oy = m(x.to(DEV), y.to(DEV))
    tol, tmax = (TOL_FP32, None) if precision == "fp32" else (TOL_FAST_L2, TOL_FAST_MAX)
    _close(ox, rx, tol, tmax)
    _close(oy, ry, tol, tmax)


def test_single_path_block_and_pair():
    """use_dual_path=False (reference a012:84-101 smoke loop): one stream, cross flag ignored (a002:83)."""
    m = SelfAndCrossBlockPair(8, 2, 4, (4, 4), False, True, 0.0, 0.0, 16, _elu(), 0.0).eval()
    load_recipe_into(m, seed=51, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = G.randn((2, 8, 8, 12), 901)
    # oracle composition for a single stream: every block is self-attention on x
    r = x
    for grp in ("self_att_block.", "cross_att_block."):
        for blk, shift in (("normal_window_block.", False), ("shifted_window_block.", True)):
            p = grp + blk
            n = O.layer_norm_channels(r, sd[p + "stage_1.norm_layer_1.weight"], sd[p + "stage_1.norm_layer_1.bias"])
            r = r + O.window_attention(sd, p + "auto_path_win_att.window_attention_x.", n, n, n, num_heads=2, dims_per_head=4,
                                       window_size=(4, 4), use_cyclic_shift=shift)
            n = O.layer_norm_channels(r, sd[p + "stage_2.norm_layer_1.weight"], sd[p + "stage_2.norm_layer_1.bias"])
            hdn = torch.nn.functional.elu(torch.nn.functional.conv2d(n, sd[p + "auto_path_mlp.mlp_x_1.weight"], sd[p + "auto_path_mlp.mlp_x_1.bias"]))
            r = r + torch.nn.functional.conv2d(hdn, sd[p + "auto_path_mlp.mlp_x_2.weight"], sd[p + "auto_path_mlp.mlp_x_2.bias"])
    m.to(DEV)
    out = m(x.to(DEV))
    assert isinstance(out, torch.Tensor)
    _close(out, r, 2e-5)


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("shape", [(2, 2, 3), (1, 16, 65), (2, 33, 64), (1, 17, 130), (3, 5, 7)])
def test_final_head_edge_shapes_vs_oracle(shape, ksize):
    """swf_final_head_fwd (a013:126-152) called directly: the fused 3x3 kernel on maps smaller than, equal to and straddling its
    64x16 tile (reflect halos crossing tile and image edges), and the two-kernel path for another kernel size."""
    import ctypes as C
    from swin_unet_image_fusion_amd import _lib as L
    from swin_unet_image_fusion_amd.modules import _ptr, _stream
    b, h, w = shape
    if ksize // 2 >= min(h, w):
        pytest.skip("reflect pad >= map (raises, covered by the error-path tests)")
    gen = torch.Generator().manual_seed(100 * h + w + ksize)
    sd = {"final_layer.0.weight": torch.randn(2, 2, ksize, ksize, generator=gen) * 0.3, "final_layer.0.bias": torch.randn(2, generator=gen) * 0.1,
          "final_layer.1.weight": torch.rand(2, generator=gen) + 0.5, "final_layer.1.bias": torch.randn(2, generator=gen) * 0.1,
          "final_layer.1.running_mean": torch.randn(2, generator=gen) * 0.1, "final_layer.1.running_var": torch.rand(2, generator=gen) + 0.5,
          "final_layer.3.weight": torch.randn(1, 2, ksize, ksize, generator=gen) * 0.3, "final_layer.3.bias": torch.randn(1, generator=gen) * 0.1}
    x, y = torch.randn(b, 1, h, w, generator=gen), torch.randn(b, 1, h, w, generator=gen)
    ref = O.final_head(sd, x, y, ksize)
    dv = {k: v.to(DEV).contiguous() for k, v in sd.items()}
    hp = L.HeadParams(_ptr(dv["final_layer.0.weight"]), _ptr(dv["final_layer.0.bias"]), _ptr(dv["final_layer.1.weight"]),
                      _ptr(dv["final_layer.1.bias"]), _ptr(dv["final_layer.1.running_mean"]), _ptr(dv["final_layer.1.running_var"]),
                      _ptr(dv["final_layer.3.weight"]), _ptr(dv["final_layer.3.bias"]))
    xd, yd = x.to(DEV).contiguous(), y.to(DEV).contiguous()     # one channel: NCHW == NHWC
    out = torch.full((b, 1, h, w), float("nan"), device=DEV)
    ws = torch.empty(b * h * w * 2 + 64, dtype=torch.float32, device=DEV)
    L.check(L.lib().swf_final_head_fwd(C.byref(hp), _ptr(xd), _ptr(yd), _ptr(out), b, h, w, ksize, _ptr(ws), ws.numel() * 4,
                                       _stream(xd.device)))
    _close(out, ref)
