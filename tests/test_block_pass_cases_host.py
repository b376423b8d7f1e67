"""CPU-only: the case table of the later-pass tests (tests/block_pass_cases.py) against the source text and against itself.

The grid rules that block_pass_cases.grid() restates are read out of the kernels' host code by regular expression and evaluated: a
later change of a rule fails here, instead of quietly leaving tests/test_gpu_block_passes.py with launches of one pass.  On 64, 256
and 304 CUs every case makes three passes with a ragged last one under the 2 GB bound of win_rows_fit, and some workgroup of every
shifted 8x8 / 7x7 case meets an edge window and then an interior one, another the reverse.  Every image the GPU test gates on 256 CUs is
well conditioned, as tests/test_block_cases_host.py holds its table: fp32 oracle == fp64 oracle within TOL_FP32 / 4."""
import os
import re
from dataclasses import replace

import pytest
import torch

from tests import block_cases as BC
from tests import block_pass_cases as P
from tests import golden_util as G

TOL_FP32 = 2e-5   # tests/test_gpu_parity.py
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "swin_unet_image_fusion_amd", "csrc")
RUNS = P.runs(P.ALL)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def _eval(expr, **names):
    """A grid expression of the host code (integers, std::min, num_cus(), L::WAVES) evaluated as Python; a tuple for dim3(x, y)."""
    assert re.fullmatch(r"[\w\s(),+*/:]+", expr), expr
    py = expr.replace("std::min", "min").replace("num_cus()", "cus").replace("L::WAVES", "waves").replace("/", "//")
    return eval(py, {"__builtins__": {}, "min": min}, names)


def _shape(C, win, hw=None, hidden=None):
    hidden = hidden or next(h[0] for c, h in BC.LEVELS.values() if c == C)
    return BC.Case("block", C, 8, C // 8, hidden, win, 1, *(hw or (P.MAP_W16 if win == 16 else P.MAP_3X6[win])), table=False)


def test_grid_rules_are_the_ones_in_the_source():
    w24, w48, w96, host = _src("kernels_win24.hip"), _src("kernels_win48.hip"), _src("kernels_win96.hip"), _src("win_host.h")
    waves = {24: int(_one(r"constexpr int W24_WAVES = (\d+);", w24)), 48: int(_one(r"constexpr int W48_WAVES = (\d+);", w48)),
             96: int(_one(r"struct L96 \{\s*static constexpr int [^;]*\bWAVES = (\d+);", w96))}
    _one(r"struct L24 \{\s*static constexpr int [^;]*\bWAVES = W24_WAVES;", w24)
    _one(r"struct L48 \{\s*static constexpr int [^;]*\bWAVES = W48_WAVES;", w48)
    assert waves == P.WAVES
    rule88 = _one(r"const int grid = (std::min\(nwin, L::WAVES \* num_cus\(\)\));", host)
    rule_x8 = _one(r"window96x8_kernel<HID, WS>\), dim3\((.*?)\), dim3\(512\)", w96)
    rule16 = {24: _one(r"window24w16_kernel<HID>\), dim3\((.*?)\), dim3\(256\)", w24), 48: _one(r"window48w16_kernel<HID>\), dim3\((.*?)\), dim3\(256\)", w48),
              96: _one(r"window96w16_kernel<HID>\), dim3\((.*?)\), dim3\(256\)", w96)}
    assert "grid" in rule_x8 and all("nwin" in r for r in rule16.values())
    # the MLP half: tiles of 64 tokens of the longer list through the 8x8 rule; the rule of the eight-wave kernel looks at the map and the schedule
    _one(r"const int nwin = \(ntok \+ 63\) / 64;\s*return raw \? win_launch_as<L, WIN_MLP, true>", host)
    _one(r"d\.schedule != SWF_SCHED_THROUGHPUT && \(a\.H / WS\) \* \(a\.W / WS\) <= 16\)", w96)
    for cus in P.CU_COUNTS + (5, 7):
        for C in (24, 48, 96):
            for b in (1, 2, 7, 40, 41, 300, 1000):
                for win in (8, 7):
                    c = replace(_shape(C, win), B=b)
                    nwin = b * c.windows_per_map
                    want = _eval(rule88, nwin=nwin, cus=cus, waves=waves[C])
                    assert P.grid(c, BC.LATENCY, cus) == P.grid(c, BC.THROUGHPUT, cus) == want, (C, win, b, cus)
                    assert P.grid(c, BC.LATENCY, cus, mlp_tokens=64 * nwin - 63) == want     # as many tiles as windows
                    if C == 96:   # a map of 15 windows: eight waves per window in the latency schedule only
                        c = replace(_shape(C, win, P.MAP_3X5[win]), B=b)
                        g = _eval(rule88, nwin=b * 15, cus=cus, waves=waves[C])
                        assert P.grid(c, BC.THROUGHPUT, cus) == g and P.grid(c, BC.LATENCY, cus) == _eval(rule_x8, grid=g, cus=cus), (win, b, cus)
                c = replace(_shape(C, 16), B=b)
                got = _eval(rule16[C], nwin=b * c.windows_per_map, cus=cus)
                assert (got if C == 24 else got[0]) == P.grid(c, BC.LATENCY, cus) == P.grid(c, BC.THROUGHPUT, cus), (C, b, cus)
                assert C == 24 or got[1] == 2   # grid.y: the stream
    # the paired form of level 2 (one pass by construction) ends at 2 x CUs windows: no three-pass batch takes it
    _one(r"d\.schedule == SWF_SCHED_THROUGHPUT && pairs <= num_cus\(\)\)", w96)
    for cus in P.CU_COUNTS:
        for p, _, s in RUNS:
            c = P.batch(p, s, cus)
            assert c.C != 96 or c.win == 16 or (c.B * c.windows_per_map + 1) // 2 > cus


def test_the_table_has_the_cases_it_names():
    blocks = [(p.shape.C, p.shape.hidden, p.shape.win, p.shape.windows_per_map, p.shape.shift, p.shape.cross, p.schedules) for p in P.BLOCKS]
    one, both = ("latency",), ("latency", "throughput")
    for lvl in (0, 1, 2):
        c, hids = BC.LEVELS[lvl]
        wpm = 18 if lvl == 2 else 15
        for win in (8, 7):
            for hid in hids:
                assert (c, hid, win, wpm, True, True, one) in blocks
        for sh, cr in ((False, True), (True, False), (False, False)):
            assert (c, hids[0], 8, wpm, sh, cr, one) in blocks
        assert (c, hids[0], 16, 6, True, True, one) in blocks
    for hid in BC.LEVELS[2][1]:
        for win in (8, 7):
            assert (96, hid, win, 15, True, True, both) in blocks     # window96x8_kernel / the four-wave kernel on the same map
    assert (48, 96, 16, 6, True, True, one) in blocks
    assert len(P.BLOCKS) == 29
    assert [(p.shape.C, p.shape.win, p.schedules) for p in P.STAGES] == [(24, 8, one), (48, 8, one), (96, 8, both), (48, 16, one)]
    assert len({p.id for p in P.ALL}) == len(P.ALL) and len(RUNS) == 38
    seeds = sorted(p.shape.seed for p in P.ALL)
    assert all(b - a >= 3 for a, b in zip(seeds, seeds[1:]))          # seed, seed + 1, seed + 2 are the case's own
    for p in P.ALL:   # both schedules exactly where the expected route differs; x8 exactly on the 15-window maps at C = 96 in latency
        c = p.shape
        assert c.H % c.win == 0 and c.W % c.win == 0 and c.C < 128 and c.dual and c.B == 1
        assert (len(p.schedules) == 2) == BC.schedule_changes_the_kernel(c)
        assert P.x8(c, BC.LATENCY) == (c.C == 96 and c.win != 16 and c.windows_per_map <= 16) and not P.x8(c, BC.THROUGHPUT)
        r = BC.route(replace(c, kind="block"), BC.LATENCY)
        assert r & BC.L.BLOCK_FAMILY_MASK == BC.L.BLOCK_WINDOW and bool(r & BC.L.BLOCK_WIN_W16) == (c.win == 16)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_every_case_makes_three_passes_with_a_ragged_last_one(cus):
    for p, sname, s in RUNS:
        c = P.batch(p, s, cus)
        g, nwin = P.grid(c, s, cus), c.B * c.windows_per_map
        assert g == P.cap(c, s, cus) and P.passes(nwin, g) == 3 and nwin % g != 0, (p.id, sname, c.B, nwin, g)
        wpm = c.windows_per_map                                                    # the smallest such batch, or one more image than that
        assert 2 * nwin >= 5 * g and (2 * (nwin - wpm) < 5 * g or ((nwin - wpm) % g == 0 and 2 * (nwin - 2 * wpm) < 5 * g))
        assert g % c.windows_per_map != 0                                          # a workgroup moves through the map from pass to pass
        assert c.B * c.H * c.W * c.C * 4 < 2 ** 31                                 # win_rows_fit
        assert P.passes(P.chunk_images(c, s, cus) * c.windows_per_map, g) == 1     # the chunks of the bitwise comparison: first pass only
        assert P.chunk_images(c, s, cus) >= 2
        images = P.gated_images(c, g)
        if c.kind == "block" and c.win != 16:
            assert images is None
        else:
            spans = [P.image_passes(c, g, i) for i in images]
            assert all(sum(s_ == (q, q) for s_ in spans) >= 2 for q in (1, 2, 3)) and c.B - 1 in images and len(images) <= 10
            straddlers = [i for i in range(c.B) if len(set(P.image_passes(c, g, i))) == 2]
            assert set(straddlers) <= set(images) and len(straddlers) == sum(1 for q in (1, 2) if q * g % c.windows_per_map)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_a_workgroup_meets_an_edge_window_and_then_an_interior_one_and_the_reverse(cus):
    """The bias tile of a level-0 workgroup gets -inf added for an edge window and is reloaded afterwards: both orders must occur."""
    for p, sname, s in RUNS:
        c = P.batch(p, s, cus)
        if c.kind != "block" or c.win == 16 or not c.shift:
            continue
        g, nwin = P.grid(c, s, cus), c.B * c.windows_per_map
        orders = {(P.edge(c, w), P.edge(c, w + g)) for w in range(nwin - g)}          # a workgroup runs w, w + g, w + 2g
        assert orders == {(True, True), (True, False), (False, True), (False, False)}, (p.id, sname, orders)
        third = {(P.edge(c, w), P.edge(c, w + g)) for w in range(g, nwin - g)}     # the step into the third pass alone
        assert (True, False) in third and (False, True) in third, (p.id, sname)


@pytest.mark.parametrize("cus", P.CU_COUNTS)
def test_mlp_half_batches(cus):
    per = P.MLP_MAP[0] * P.MLP_MAP[1]
    for lvl in P.HALF_LEVELS:
        C = BC.LEVELS[lvl][0]
        assert P.half_case(C).C == C and P.half_case(C).hidden == 4 * C
        for dual in (True, False):
            n = P.mlp_batch(C, dual, cus) * per
            n0, n1 = P.mlp_slot_tokens(n, dual)
            assert n0 + n1 == (2 * n if dual else n) and n0 >= n1 and (dual or n0 % 64 == 0)
            g = P.grid(P.half_case(C), BC.LATENCY, cus, mlp_tokens=n0)
            t0, t1 = -(-n0 // 64), -(-n1 // 64)
            assert g == P.WAVES[C] * cus and P.passes(t0, g) == 3 and t0 % g != 0 and 2 * t0 >= 5 * g
            assert n1 % 64 != 0 and t1 > 2 * g                                     # the partial tile lies in the last pass
            assert n * C * 4 < 2 ** 31
            nc = P.mlp_chunk_images(C, dual, cus) * per
            assert P.passes(-(-P.mlp_slot_tokens(nc, dual)[0] // 64), g) == 1 and 4 * nc > n   # first-pass-only chunks, at most four


# ---- conditioning of what the GPU test gates on 256 CUs -------------------------------------------------------------------------------
def _well_conditioned(tag, pairs):
    for a, b in pairs:
        l2, mx = G.rel_err(a, b)
        print(f"[block-pass-cases] {tag}: fp32 vs fp64 rel-L2 {l2:.3e} max-rel {mx:.3e}")
        assert l2 <= TOL_FP32 / 4 and mx <= TOL_FP32 / 4, (tag, l2, mx)


@pytest.mark.parametrize("run", RUNS, ids=P.run_id)
def test_gated_images_are_well_conditioned(run):
    p, sname, s = run
    c = P.batch(p, s, 256)
    images = P.gated_images(c, P.grid(c, s, 256))
    ref32, ref64 = (BC.reference(c, dt, images) for dt in (torch.float32, torch.float64))
    assert ref64[0].shape == (c.B if images is None else len(images), c.C, c.H, c.W)
    _well_conditioned(f"{P.run_id(run)} seed {c.seed}", zip(ref32, ref64))
    BC.inputs.cache_clear()   # tens of MB a case: block_cases keeps what it draws, which suits its own small maps


@pytest.mark.parametrize("C", [BC.LEVELS[lvl][0] for lvl in P.HALF_LEVELS])
def test_half_block_references_are_well_conditioned(C):
    case = P.batch(P.find("block", C, 4 * C, 8, P.MAP_3X5[8]), BC.LATENCY, 256)
    images = P.gated_images(case, P.grid(case, BC.LATENCY, 256), sample=True)
    sd = P.half_module(C, True).state_dict()
    x, y = (t[images] for t in BC.inputs(case))
    for i, (a, b) in enumerate(zip(P.attn_half_reference(sd, case, x, y, torch.float32), P.attn_half_reference(sd, case, x, y))):
        _well_conditioned(f"attention half C={C} {'with LN1' if i else 'raw'}", zip(a, b))
    BC.inputs.cache_clear()
    for dual in (True, False):
        x, y = P.mlp_inputs(C, P.mlp_batch(C, dual, 256))
        sd = P.half_module(C, dual).state_dict()
        got32, got64 = (P.mlp_half_reference(sd, x, y if dual else None, dt) for dt in (torch.float32, torch.float64))
        for i, (a, b) in enumerate(zip(got32, got64)):
            _well_conditioned(f"MLP half C={C} dual={dual} {'with LN2' if i else 'raw'}", zip(a, b))
