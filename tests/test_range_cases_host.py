"""CPU-only: the magnitude regimes of tests/regime_cases.py (vscale, qkbal, mlpsmall, spike) are what they claim to be, are well
conditioned, and the format emulation (tests/format_emulation.py) shows the edge of the fast tier's formats where DESIGN says it is.

Conditioning: as tests/test_regime_cases_host.py: the float32 oracle agrees with the float64 oracle to a quarter of the floor of the bound
the GPU test applies (TOL_FP32 / 4 on both metrics; a spike rung per output channel), the backward to a quarter of the BLOCK criterion; a
pair that misses gets the next seed (regime_cases.RANGE_SEED_OVERRIDE) or is dropped (RANGE_DROPPED, at most one in ten).
Invariance: vscale and qkbal scale by powers of two, so the float64 oracle returns the base case's bits; a regime that changed the
function would test nothing.  ELU: at mlpsmall16 the fp32 exp2 - 1 of the fast tier is the whole error, and the emulation has to show it.
Edge: every RANGE_BEYOND rung makes the emulation of every family non-finite somewhere, no kept rung does.  The envelope (emulation
against the float64 oracle per (case, regime), the worst per level and regime) must equal profiles/r26_range_envelope.json."""
import json
import math
import os
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

from tests import block_cases as BC
from tests import bwd_tree_cases as BT
from tests import format_emulation as FE
from tests import regime_cases as RC
from tests.gpu_guard import record_dir
from tests.test_regime_cases_host import PROFILES, TOL_FP32, _committed, _float32_oracle

GROUPS = ((RC.FAST_BLOCKS, RC.RANGE_FORWARD), (RC.ATTN_CASES, RC.RANGE_ATTENTION), (RC.EXACT_BLOCKS, RC.RANGE_EXACT))
RANGE_PAIRS = [p for cases, regimes in GROUPS for p in RC.pairs(cases, regimes)]
PRESERVING = [p for p in RANGE_PAIRS if all(op in RC.FUNCTION_PRESERVING for op, _ in RC.parse(p[1]))]


def _finite(errs):
    return all(math.isfinite(e) for e in errs)


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
def test_the_ladders_are_what_the_regimes_were_asked_to_be():
    assert RC.RANGE_FORWARD == ("vscale-16", "vscale-12", "vscale+12", "qkbal-12", "qkbal+12", "mlpsmall12", "mlpsmall16", "spike16", "spike64")
    assert RC.RANGE_ATTENTION == ("vscale-16", "vscale+12", "qkbal-12", "qkbal+12")
    assert RC.RANGE_EXACT == ("vscale+12", "qkbal-12", "mlpsmall16", "spike16")
    assert RC.RANGE_BACKWARD == ("vscale+12", "qkbal+12") and RC.RANGE_BEYOND == ("vscale+16", "qkbal-16")
    assert RC.RANGE_BWD_NAMES == ("att_d12_w8", "att_d48_w8", "refused_att_d48_w16", "block_c96_w8")
    assert RC.parse("vscale-16") == [("vscale", -16.0)] and RC.parse("qkbal+12_spike64") == [("qkbal", 12.0), ("spike", 64.0)]
    assert len(RC.FAST_BLOCKS) == 16 and len(RC.ATTN_CASES) == 6 and len(RC.EXACT_BLOCKS) == 5
    # dropped rungs and other seeds: known pairs, at most one in ten per group, a seed within the eight tries
    every = {(c.id, r) for cases, regimes in GROUPS for c in cases for r in regimes}
    backward = {(n, r) for n in RC.RANGE_BWD_NAMES for r in RC.RANGE_BACKWARD}
    assert set(RC.RANGE_DROPPED) <= every | backward and set(RC.RANGE_SEED_OVERRIDE) <= (every | backward) - set(RC.RANGE_DROPPED)
    assert not set(RC.RANGE_SEED_OVERRIDE) & set(RC.SEED_OVERRIDE) and not set(RC.RANGE_DROPPED) & set(RC.DROPPED)
    for cases, regimes in GROUPS:
        dropped = [p for p in RC.RANGE_DROPPED if p[0] in {c.id for c in cases} and p[1] in regimes]
        assert 10 * len(dropped) <= len(cases) * len(regimes), dropped
    assert 10 * len([p for p in RC.RANGE_DROPPED if p in backward]) <= len(backward)
    by_id = {c.id: c for c in RC.FAST_BLOCKS + RC.EXACT_BLOCKS + RC.ATTN_CASES}
    by_id.update({n: (RC.BP.find(n) if n == RC.BWD_PHASED else RC.BW.find(n)) for n in RC.RANGE_BWD_NAMES})
    for (cid, _), seed in RC.RANGE_SEED_OVERRIDE.items():
        k, rem = divmod(seed - by_id[cid].seed, RC.SEED_STEP)
        assert rem == 0 and 1 <= k <= RC.MAX_SEED_TRIES, (cid, seed)
    # the backward table: the cases they come from, wired as tests/regime_cases.BACKWARD_CASES are
    assert len(RC.RANGE_BACKWARD_CASES) + len([p for p in RC.RANGE_DROPPED if p in backward]) == 8
    assert RC.RANGE_MFMA_REGIME in RC.RANGE_BACKWARD and RC.BWD_BLOCK in RC.RANGE_BWD_NAMES
    for c in RC.RANGE_BACKWARD_CASES:
        name = c.id[:-len(c.regime) - 1]
        base = RC.BP.find(name) if name == RC.BWD_PHASED else RC.BW.find(name)
        assert replace(c, name=name, regime="", seed=base.seed) == base and base.regime == ""
        assert (c.route == RC.BP.PHASED) == (name == RC.BWD_PHASED)


def test_a_magnitude_regime_scales_what_it_names_and_nothing_else():
    case = RC.FAST_BLOCKS[0]
    sd0 = BC.make_module(case).state_dict()
    def suffix(k):      # the MLP's layers are also named as items 0 and 3 of sequence_x / sequence_y
        for s in "xy":
            k = k.replace(f"sequence_{s}.0.", f"mlp_{s}_1.").replace(f"sequence_{s}.3.", f"mlp_{s}_2.")
        return ".".join(k.rsplit(".", 2)[-2:])
    for regime, want in (("vscale+12", {"v_for_heads.weight": 2.0 ** 12, "v_for_heads.bias": 2.0 ** 12, "linear_projection.weight": 2.0 ** -12}),
                         ("vscale-16", {"v_for_heads.weight": 2.0 ** -16, "v_for_heads.bias": 2.0 ** -16, "linear_projection.weight": 2.0 ** 16}),
                         ("qkbal-12", {"q_for_heads.weight": 2.0 ** -12, "q_for_heads.bias": 2.0 ** -12, "k_for_heads.weight": 2.0 ** 12,
                                       "k_for_heads.bias": 2.0 ** 12}),
                         ("mlpsmall16", {f"mlp_{s}_1.{p}": 2.0 ** -16 for s in "xy" for p in ("weight", "bias")}
                                        | {f"mlp_{s}_2.weight": 2.0 ** 16 for s in "xy"})):
        sd1 = RC.make_module(case, regime).state_dict()
        assert sd0.keys() == sd1.keys()
        changed = {k for k in sd0 if not torch.equal(sd0[k], sd1[k])}
        assert {suffix(k) for k in changed} == set(want), (regime, sorted(changed))
        for k in changed:      # every alias of a tensor carries the factor once
            assert torch.equal(sd1[k], sd0[k] * want[suffix(k)]), (regime, k)
    with pytest.raises(ValueError):
        RC.make_module(RC.ATTN_CASES[0], "mlpsmall16")
    # spike: channel C // 3 of both streams, opposite offsets; every other channel untouched
    (x0, y0), (x1, y1) = RC.inputs(case, RC.BASE), RC.inputs(case, "spike64")
    c0 = case.C // 3
    keep = [c for c in range(case.C) if c != c0]
    assert torch.equal(x1[:, keep], x0[:, keep]) and torch.equal(y1[:, keep], y0[:, keep])
    assert torch.equal(x1[:, c0], 64 * x0[:, c0] + 64) and torch.equal(y1[:, c0], 64 * y0[:, c0] - 64)
    assert float(x1[:, c0].mean()) > 32 and float(y1[:, c0].mean()) < -32
    assert RC.per_channel("spike16") and RC.per_channel("gain4_spike16") and not RC.per_channel("vscale+12")


def test_the_per_channel_measure_sees_what_the_whole_tensor_measure_hides():
    ref = torch.ones(1, 4, 2, 2, dtype=torch.float64)
    ref[:, 1] = 1000.0
    got = ref.clone()
    got[:, 2] *= 1.01
    whole, channels = RC.worst_errors([got], [ref], RC.BASE), RC.worst_errors([got], [ref], "spike16")
    assert whole[0] < 1e-4 and whole[1] < 1e-4
    assert abs(channels[0] - 0.01) < 1e-12 and abs(channels[1] - 0.01) < 1e-12
    got[0, 3, 0, 0] = float("nan")
    assert not _finite(RC.worst_errors([got], [ref], "spike16")) and not _finite(RC.worst_errors([got], [ref], RC.BASE))


# ---- conditioning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RANGE_PAIRS, ids=RC.pair_id)
def test_range_rung_is_well_conditioned(pair):
    case, regime = pair
    ref64 = RC.reference64(case, regime)
    ref32 = _float32_oracle(lambda: RC.reference(case, regime, torch.float32))
    assert all(bool(torch.isfinite(t).all()) for t in ref64)
    l2, mx = RC.worst_errors(ref32, ref64, regime)
    print(f"[range-cases] {case.id} {regime} seed {case.seed}: fp32 vs fp64 rel-L2 {l2:.3e} max-rel {mx:.3e} (bound {TOL_FP32 / 4:.2e}"
          f"{', per channel' if RC.per_channel(regime) else ''})")
    assert l2 <= TOL_FP32 / 4 and mx <= TOL_FP32 / 4, (case.id, regime, case.seed, l2, mx)


@pytest.mark.parametrize("case", RC.RANGE_BACKWARD_CASES, ids=lambda c: c.id)
def test_backward_range_rung_is_well_conditioned(case):
    ref64 = BT.reference64(case)
    ref32 = _float32_oracle(lambda: BT.reference(case, torch.float32))
    b_in, b_par = (b / 4 for b in BT.BOUNDS["block"])
    for mode in BT.MODES:
        e_in, e_par, which = BT.measure("block", *ref32[mode], *ref64[mode])
        print(f"[range-cases] {case.id} seed {case.seed} {mode}: fp32 vs fp64 inputs {e_in:.3e} (bound {b_in:.2e}) parameters {e_par:.3e} "
              f"at {which} (bound {b_par:.2e})")
        assert e_in <= b_in and e_par <= b_par, (case.id, case.seed, mode, e_in, e_par, which)
        assert all(bool(torch.isfinite(g).all()) for g in list(ref64[mode][0].values()) + list(ref64[mode][1].values()))


# ---- the regimes do what they say -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PRESERVING + RC.pairs(RC.FAST_BLOCKS + RC.ATTN_CASES, RC.RANGE_BEYOND), ids=RC.pair_id)
def test_vscale_and_qkbal_leave_the_float64_oracle_unchanged_bit_for_bit(pair):
    case, regime = pair
    got, base = RC.reference64(case, regime), RC.reference64(case, RC.BASE)
    assert len(got) == len(base) and all(torch.equal(g, b) for g, b in zip(got, base)), (case.id, regime)
    assert not all(torch.equal(RC.state(case, regime)[k], v) for k, v in RC.state(case, RC.BASE).items())


def _fc1_outputs(case, regime):
    """fc1's outputs (the ELU's arguments) of both streams, float64 oracle"""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in RC.state(case, regime).items()}
    x, y = (t.double() for t in RC.inputs(case, regime))
    ln = lambda z, name: RC.O.layer_norm_channels(z, sd[name + ".weight"], sd[name + ".bias"])
    nx, ny = ln(x, "stage_1.norm_layer_1"), ln(y, "stage_1.norm_layer_2")
    kw = dict(num_heads=case.heads, dims_per_head=case.head_dim, window_size=(case.win, case.win), use_cyclic_shift=case.shift)
    px, py = "auto_path_win_att.window_attention_x.", "auto_path_win_att.window_attention_y."
    kx, ky = (ny, nx) if case.cross else (nx, ny)
    x, y = x + RC.O.window_attention(sd, px, nx, kx, kx, **kw), y + RC.O.window_attention(sd, py, ny, ky, ky, **kw)
    nx, ny = ln(x, "stage_2.norm_layer_1"), ln(y, "stage_2.norm_layer_2")
    return [F.conv2d(z, sd[f"auto_path_mlp.mlp_{s}_1.weight"], sd[f"auto_path_mlp.mlp_{s}_1.bias"]) for z, s in ((nx, "x"), (ny, "y"))]


@pytest.mark.parametrize("regime", ("mlpsmall12", "mlpsmall16"))
@pytest.mark.parametrize("case", RC.FAST_BLOCKS + RC.EXACT_BLOCKS, ids=lambda c: c.id)
def test_mlpsmall_shrinks_the_elu_arguments(case, regime):
    k = RC.parse(regime)[0][1]
    small, base = _fc1_outputs(case, regime), _fc1_outputs(case, RC.BASE)
    for s, b in zip(small, base):
        top, top0 = float(s.abs().max()), float(b.abs().max())
        assert 0 < top <= 2.0 ** -k * top0, (case.id, regime, top, top0)
        assert bool((s < 0).any()) and float(s[s < 0].abs().max()) <= 2.0 ** -k * top0      # the branch of ELU that the fast tier approximates
    if regime == "mlpsmall16":    # not function-preserving: the reference is the oracle on the transformed state
        assert not torch.equal(RC.reference64(case, regime)[0], RC.reference64(case, RC.BASE)[0])


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def test_every_family_declares_the_elu_its_source_shows():
    f = FE.FORMATS
    assert FE.Format().elu == "" and FE.OFF.elu == "" and FE.EXP2_ONLY.elu == ""
    assert {k: v.elu for k, v in f.items()} == {"win": "folded", "win16": "folded", "qkvattn": "exp2m1", "core8": "exp2m1", "core16": "exp2m1"}


@pytest.mark.parametrize("regime", RC.RANGE_FORWARD)
@pytest.mark.parametrize("case", RC.FAST_BLOCKS[::3], ids=lambda c: c.id)
def test_with_every_rounding_off_the_emulation_is_still_the_oracle(case, regime):
    got, ref = RC._evaluate(case, regime, torch.float64, FE.OFF), RC.reference64(case, regime)
    assert len(got) == len(ref) and all(torch.equal(g, r) for g, r in zip(got, ref))


def _elu_off(case, regime):
    fmt = replace(FE.FORMATS[RC.family(case)], elu="")
    return RC.worst_errors(RC._evaluate(case, regime, torch.float64, fmt), RC.reference64(case, regime), regime)


@pytest.mark.parametrize("case", RC.FAST_BLOCKS, ids=lambda c: c.id)
def test_the_elu_is_visible_at_mlpsmall16_and_modelled(case):
    c16 = RC.seeded(case, "mlpsmall16")
    on, off = RC.emulation_errors(c16, "mlpsmall16"), _elu_off(c16, "mlpsmall16")
    on1, off1 = RC.emulation_errors(case, RC.BASE), _elu_off(case, RC.BASE)
    print(f"[range-cases] {case.id} ({RC.family(case)}): mlpsmall16 rel-L2 with the fast ELU {on[0]:.3e}, with float64 ELU {off[0]:.3e}, ratio "
          f"{on[0] / off[0]:.2f}; gain1 {on1[0]:.4e} / {off1[0]:.4e}")
    assert on[0] >= 2.0 * off[0], (case.id, on, off)
    assert abs(on1[0] - off1[0]) <= 0.01 * off1[0], (case.id, on1, off1)        # at fc2 of order 1: the same to two digits


@pytest.mark.parametrize("family", sorted(FE.FORMATS))
def test_the_edge_of_the_format_is_where_design_says(family):
    """the first rung past the edge is non-finite for every family, somewhere; no rung the GPU runs is"""
    cases = [c for c in RC.FAST_BLOCKS + RC.ATTN_CASES if RC.family(c) == family]
    assert cases
    for regime in RC.RANGE_BEYOND:
        broken = [c.id for c in cases if not _finite(RC.emulation_errors(c, regime))]
        print(f"[range-cases] {family} {regime}: the emulation is non-finite on {len(broken)} of {len(cases)} cases")
        assert broken, (family, regime)
        assert all(bool(torch.isfinite(t).all()) for c in cases for t in RC.reference64(c, regime)), "the oracle itself has the range"
    for c in cases:
        for regime in (RC.RANGE_FORWARD if c.kind == "block" else RC.RANGE_ATTENTION):
            assert _finite(RC.emulation_errors(RC.seeded(c, regime), regime)), (c.id, regime)


# ---- the envelope ---------------------------------------------------------------------------------------------------------------------
def _envelope():
    levels = {c: lvl for lvl, (c, _) in BC.LEVELS.items()}
    kept = {(c.id, r) for c, r in RANGE_PAIRS}
    records, worst = [], {}
    for case in RC.FAST_BLOCKS + RC.ATTN_CASES:
        for regime in (RC.BASE,) + (RC.RANGE_FORWARD if case.kind == "block" else RC.RANGE_ATTENTION + RC.RANGE_ATTENTION_SPIKES) + RC.RANGE_BEYOND:
            c = RC.seeded(case, regime)
            l2, mx = RC.emulation_errors(c, regime)
            finite = _finite((l2, mx))
            records.append({"case": case.id, "kind": case.kind, "level": levels[case.C], "window": case.win, "family": RC.family(case),
                            "regime": regime, "seed": c.seed, "finite": finite, "rel_l2": l2 if finite else None,
                            "max_rel": mx if finite else None, "per_channel": RC.per_channel(regime),
                            "in_the_gpu_test": (case.id, regime) in kept})
            w = worst.setdefault(f"level{levels[case.C]}_c{case.C}", {}).setdefault(case.kind, {}).setdefault(
                regime, {"finite": True, "rel_l2": 0.0, "max_rel": 0.0})
            if not finite:
                w.update(finite=False, rel_l2=None, max_rel=None)
            elif w["finite"]:
                w.update(rel_l2=max(w["rel_l2"], l2), max_rel=max(w["max_rel"], mx))
    return {"metric": "rel-L2 = |out-ref|_2/|ref|_2, max-rel = max|out-ref|/max|ref| of tests/format_emulation.py (the float64 oracle with the "
                      "fast tier's declared roundings, the fp32 ELU among them) against the float64 oracle, worst of the two streams; spike "
                      "regimes: per output channel, the worst channel; finite = false: the emulation returned inf or NaN; cases and "
                      "regimes: tests/regime_cases.py",
            "worst_per_level_and_regime": worst,
            "beyond_the_edge": list(RC.RANGE_BEYOND),
            "dropped_from_the_gpu_test": [list(p) for p in RC.RANGE_DROPPED],
            "seed_overrides": [[cid, r, s] for (cid, r), s in RC.RANGE_SEED_OVERRIDE.items()],
            "records": records}


def test_range_envelope_of_the_fast_tier_format_is_the_committed_one():
    env = _envelope()
    try:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "range_envelope.json"), "w") as f:
            json.dump(env, f, indent=1)
    except OSError:
        pass
    assert os.path.isdir(PROFILES)
    want = _committed("r26_range_envelope.json")
    assert env["beyond_the_edge"] == want["beyond_the_edge"]
    assert env["dropped_from_the_gpu_test"] == want["dropped_from_the_gpu_test"] and env["seed_overrides"] == want["seed_overrides"]
    key = lambda r: (r["case"], r["regime"])
    got, ref = {key(r): r for r in env["records"]}, {key(r): r for r in want["records"]}
    assert got.keys() == ref.keys()
    close = lambda a, b: (a is None and b is None) or (a is not None and b is not None and abs(a - b) <= 0.1 * b)
    for k, r in got.items():
        for field in ("rel_l2", "max_rel"):     # float64 sums in another order can flip a rounding of the emulation
            assert close(r[field], ref[k][field]), (k, field, r[field], ref[k][field])
        assert {f: r[f] for f in r if f not in ("rel_l2", "max_rel")} == {f: ref[k][f] for f in ref[k] if f not in ("rel_l2", "max_rel")}
    for lvl, kinds in env["worst_per_level_and_regime"].items():
        for kind, regimes in kinds.items():
            for regime, w in regimes.items():
                w0 = want["worst_per_level_and_regime"][lvl][kind][regime]
                assert w["finite"] == w0["finite"] and close(w["rel_l2"], w0["rel_l2"]) and close(w["max_rel"], w0["max_rel"]), (lvl, kind, regime)
    assert {(l, k, r) for l, ks in env["worst_per_level_and_regime"].items() for k, rs in ks.items() for r in rs} == \
        {(l, k, r) for l, ks in want["worst_per_level_and_regime"].items() for k, rs in ks.items() for r in rs}
    # what DESIGN says: a V/proj imbalance of 2^+12 and a Q/K imbalance of 2^+12 cost nothing (within 2 % of the base figure), Q
    # x 2^-12 at most a fifth (the deep levels scale Q after its linear layer, so its small elements reach f16's subnormals first), 2^-16
    # on V is finite and worse, the rungs past the edge are non-finite at every level
    for lvl, kinds in env["worst_per_level_and_regime"].items():
        for kind, regimes in kinds.items():
            base = regimes[RC.BASE]["rel_l2"]
            for r, slack in (("vscale+12", 0.02), ("qkbal+12", 0.02), ("qkbal-12", 0.2)):
                assert abs(regimes[r]["rel_l2"] - base) <= slack * base, (lvl, kind, r, regimes[r], base)
            assert regimes["vscale-16"]["finite"] and regimes["vscale-16"]["rel_l2"] > 1.5 * base, (lvl, kind)
            assert not any(regimes[r]["finite"] for r in RC.RANGE_BEYOND), (lvl, kind)
