"""Regimes of sharp softmax as transformations of existing cases (tests/test_gpu_regimes.py on the GPU, tests/test_regime_cases_host.py
for the conditioning of every (case, regime), the honesty of the format emulation and the envelope table on the CPU).

Every other parity test draws activations from G.randn / synthetic_pair and weights from an initialisation recipe: attention logits of
order 1, nearly flat softmax rows.  A regime takes a case of tests/block_cases.py (or a WindowAttention case below, or a case of
tests/bwd_width_cases.py) and changes the weights of its MODULE in place and / or its inputs; no shape changes, so block_cases.route()
still names the kernel that has to run.

    gainG      q_for_heads.weight and .bias of every WindowAttention x G: logits x G
    table8     relative_position_bias_table x 8
    ramp+1     table[i, j] = +4 (i + j / n_cols) + 0.25 table_old[i, j]: every query's maximum lies in the last key rows, the running
               maximum of an online softmax grows at every key tile
    ramp-1     the same with -4: the maximum is in the first key tile, later tiles underflow
    flatE      x = bx + E x0 with bx a seeded randn(B, C, 1, 1), y likewise from another draw (a cross block refuses x == y): every token
               of an image is the same vector, or nearly
    a_b        a, then b

Regimes of operand MAGNITUDE (tests/test_gpu_range.py on the GPU, tests/test_range_cases_host.py on the CPU): the logits keep their size,
the operands of the f16 and split-bf16 products and of the fp32 ELU move towards the ends of their formats.  K is a power of two's
exponent, so the first two leave the float64 oracle's output unchanged bit for bit.

    vscale+K   v_for_heads.weight and .bias x 2^K, linear_projection.weight x 2^-K (its bias untouched): V and the un-normalised P.V sum
               towards the top (+) or the subnormals (-) of f16
    qkbal+K    q_for_heads.weight and .bias x 2^K, k_for_heads.weight and .bias x 2^-K: the same logits out of an unbalanced Q and K
    mlpsmallK  auto_path_mlp.mlp_{x,y}_1.weight and .bias x 2^-K, mlp_{x,y}_2.weight x 2^K: ELU arguments of order 2^-K, where exp2(u) - 1
               cancels, times a large fc2.  Not function-preserving (ELU is not linear); no WindowAttention case has an MLP
    spikeA     inputs only: with c0 = C // 3, x[:, c0] = A x[:, c0] + A and y[:, c0] = A y[:, c0] - A: one channel dominates the mean
               and the variance of every LayerNorm row, with opposite sign in the two streams.  Errors of a spike rung are taken PER OUTPUT
               CHANNEL (worst_errors): the untouched residual in channel c0 would otherwise set the scale and hide the rest

The float64 reference is the CPU oracle on the transformed module's state_dict; `emulation` is tests/format_emulation.py on the same
state: the oracle in float64 with the roundings the fast tier's kernels declare."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace
from typing import Dict, List, Tuple

import torch
from torch import nn

from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import WindowAttention, _lib as L, load_recipe_into
from tests import block_cases as BC
from tests import bwd_phased_cases as BP
from tests import bwd_width_cases as BW
from tests import format_emulation as FE
from tests import golden_util as G

BASE = "gain1"                                                    # the untransformed case
GAIN_LADDER = ("gain4", "gain16", "gain64")
FORWARD = GAIN_LADDER + ("table8", "ramp+1", "ramp-1", "flat1e-2", "flat0", "gain16_table8")
ATTENTION_REGIMES = ("gain16", "ramp+1", "ramp-1")
EXACT = ("gain16", "gain64", "ramp+1", "ramp-1", "table8", "flat1e-2")
BACKWARD = ("gain4", "gain16", "ramp+1", "table8")
MFMA_REGIME = "gain16"                                            # backward_tier = "mfma" against the default tier on the block case
RAMP_SLOPE, RAMP_KEEP = 4.0, 0.25
# magnitude ladders: (group, where it runs) in tests/test_gpu_range.py
RANGE_FORWARD = ("vscale-16", "vscale-12", "vscale+12", "qkbal-12", "qkbal+12", "mlpsmall12", "mlpsmall16", "spike16", "spike64")
RANGE_ATTENTION = ("vscale-16", "vscale+12", "qkbal-12", "qkbal+12")          # no spike: nothing normalises the input of WindowAttention alone
RANGE_EXACT = ("vscale+12", "qkbal-12", "mlpsmall16", "spike16")
RANGE_BACKWARD = ("vscale+12", "qkbal+12")
RANGE_BWD_NAMES = ("att_d12_w8", "att_d48_w8", "refused_att_d48_w16", "block_c96_w8")
RANGE_MFMA_REGIME = "vscale+12"
RANGE_ATTENTION_SPIKES = ("spike16", "spike1024")                             # in the envelope record only: what an un-normalised outlier costs
RANGE_BEYOND = ("vscale+16", "qkbal-16")                                      # the first rungs past the edge of f16: never on the GPU
FUNCTION_PRESERVING = ("vscale", "qkbal")
OPS = ("gain", "table", "ramp", "flat", "vscale", "qkbal", "mlpsmall", "spike")
MAX_SEED_TRIES = 8                                                # next seed = the case's + SEED_STEP, at most this many times
SEED_STEP = 100000


# ---- the transformations ------------------------------------------------------------------------------------------------------------
def parse(regime: str) -> List[Tuple[str, float]]:
    ops = []
    for part in regime.split("_"):
        op = next((o for o in OPS if part.startswith(o)), None)
        if op is None:
            raise ValueError(f"unknown regime {regime!r}")
        ops.append((op, float(part[len(op):])))
    return ops


def apply_to_module(m: nn.Module, regime: str) -> nn.Module:
    """The weight part of `regime`, in place on every WindowAttention of `m` (the state_dict's aliased keys follow)."""
    atts = [a for a in m.modules() if isinstance(a, WindowAttention)]
    assert atts, "no WindowAttention in the module"
    with torch.no_grad():
        for op, arg in parse(regime):
            if op == "mlpsmall":
                mlps = [a for a in m.modules() if hasattr(a, "mlp_x_1")]
                if not mlps:
                    raise ValueError(f"{regime!r} needs an MLP: it does not apply to WindowAttention alone")
                for a in mlps:
                    for s in ("x", "y"):
                        if hasattr(a, f"mlp_{s}_1"):
                            fc1, fc2 = getattr(a, f"mlp_{s}_1"), getattr(a, f"mlp_{s}_2")
                            fc1.weight.mul_(2.0 ** -arg)
                            fc1.bias.mul_(2.0 ** -arg)
                            fc2.weight.mul_(2.0 ** arg)
            for a in atts:
                if op == "gain":
                    a.q_for_heads.weight.mul_(arg)
                    if a.q_for_heads.bias is not None:
                        a.q_for_heads.bias.mul_(arg)
                elif op == "vscale":
                    a.v_for_heads.weight.mul_(2.0 ** arg)
                    if a.v_for_heads.bias is not None:
                        a.v_for_heads.bias.mul_(2.0 ** arg)
                    a.linear_projection.weight.mul_(2.0 ** -arg)
                elif op == "qkbal":
                    for lin, k in ((a.q_for_heads, arg), (a.k_for_heads, -arg)):
                        lin.weight.mul_(2.0 ** k)
                        if lin.bias is not None:
                            lin.bias.mul_(2.0 ** k)
                elif op == "table":
                    a.relative_position_bias_table.mul_(arg)
                elif op == "ramp":
                    t = a.relative_position_bias_table
                    rows, cols = t.shape
                    i = torch.arange(rows, dtype=t.dtype)[:, None]
                    j = torch.arange(cols, dtype=t.dtype)[None, :]
                    t.copy_(arg * RAMP_SLOPE * (i + j / cols) + RAMP_KEEP * t)
    return m


def transform_inputs(regime: str, ins: Tuple[torch.Tensor, ...], seed: int) -> Tuple[torch.Tensor, ...]:
    """The input part of `regime` (`flat` and `spike` have one); `seed`: the case's."""
    for op, arg in parse(regime):
        if op == "spike":
            x, y = (t.clone() for t in ins)
            c0 = x.shape[1] // 3
            x[:, c0] = arg * x[:, c0] + arg
            y[:, c0] = arg * y[:, c0] - arg
            ins = (x, y)
        if op == "flat":
            ins = tuple(G.randn((t.shape[0], t.shape[1], 1, 1), seed + 31 + k) + arg * t for k, t in enumerate(ins))
    return ins


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AttnCase:
    """One WindowAttention (8 heads of C / 8 channels, shifted, k = v = the other tensor) with precision = "fast": no residual and no
    MLP dilute an error of the attention."""
    C: int
    win: int
    B: int
    H: int
    W: int
    seed: int = 0
    kind: str = "attention"
    heads: int = 8

    @property
    def head_dim(self) -> int:
        return self.C // 8

    @property
    def id(self) -> str:
        return f"attention_c{self.C}_w{self.win}_b{self.B}_{self.H}x{self.W}"


# the smallest maps of block_cases.BLOCK_MAPS at these windows: six 8x8 windows in two images; two 16x16 windows
ATTN_CASES = [AttnCase(c, win, *m, seed=8100 + 10 * i)
              for i, (c, win, m) in enumerate((c, win, m) for c in (24, 48, 96) for win, m in ((8, (2, 16, 24)), (16, (1, 16, 32))))]

# fast tier: every level at its wide hidden width on the first map of windows 8, 7 and 16 as cross_shift, and the C = 96 self_plain case
FAST_BLOCKS = [BC.find("block", c, hids[0], win, BC.BLOCK_MAPS[lvl][win][0]) for lvl, (c, hids) in BC.LEVELS.items() for win in (8, 7, 16)]
FAST_BLOCKS.append(BC.find("block", 96, 384, 8, BC.BLOCK_MAPS[2][8][0], shift=False, cross=False))
EXACT_BLOCKS = [BC.find("block", BC.LEVELS[lvl][0], BC.LEVELS[lvl][1][0], 8, m, prec=L.PREC_FP32) for lvl, m in BC.FP32_MAPS]
assert len(FAST_BLOCKS) == 16 and len(EXACT_BLOCKS) == 5

# backward: one attention case per DMAX class on 8x8, one 7x7, the 16x16 window of the thread family (no 16x16 tile fits its resident
# form: bwd_width_cases.lds_resident(16, 16, d) > 96 KB for every d, so this is the recompute kernel), the (256-token, d = 48) tile of the
# phased family, and the C = 96 block
BWD_THREAD = ("att_d12_w8", "att_d24_w8", "att_d48_w8", "att_d48_w7", "att_d12_w16")
BWD_PHASED = "refused_att_d48_w16"
BWD_BLOCK = "block_c96_w8"

# Conditioning (tests/test_regime_cases_host.py): the float32 oracle agrees with the float64 oracle to a quarter of the bound the GPU test
# applies.  (case id, regime) -> seed where the case's own seed misses; the next seed is the case's + SEED_STEP, at most MAX_SEED_TRIES
# times.  A seed was taken only where it met 0.9 of the bound with the float32 oracle on 1, 4 and 8 threads: at C = 384 its rounding moves
# by a factor of two with the way the sums are split.  DROPPED: the rungs where no seed did (at most one (case, regime) in ten).  Every one
# is gain64: there the float32 oracle itself sits at 5e-6 .. 1.1e-5 of the float64 one from C = 96 up, so a quarter of the exact tier's gate
# cannot be told from the reference's own rounding.
SEED_OVERRIDE: Dict[Tuple[str, str], int] = {
    ("block_c48h8x6_hid192_w8_b2_16x24_cross_shift", "gain64"): 303124,
    ("block_c48h8x6_hid192_w7_b1_14x21_cross_shift", "gain64"): 203128,
    ("block_c48h8x6_hid192_w8_b2_16x24_cross_shift_fp32", "gain64"): 303246,
    ("att_d48_w8", "gain16"): 106260,          # backward cases: (name in bwd_width_cases, regime)
    ("att_d12_w16", "gain16"): 206290,
}
DROPPED: Tuple[Tuple[str, str], ...] = tuple((i, "gain64") for i in (
    "block_c96h8x12_hid384_w8_b2_16x24_cross_shift", "block_c96h8x12_hid384_w7_b1_28x28_cross_shift",
    "block_c96h8x12_hid384_w16_b2_32x16_cross_shift", "block_c96h8x12_hid384_w8_b2_16x24_self_plain",
    "block_c192h8x24_hid768_w8_b1_16x16_cross_shift", "block_c192h8x24_hid768_w16_b1_16x32_cross_shift",
    "block_c384h8x48_hid1536_w8_b2_8x8_cross_shift", "block_c384h8x48_hid1536_w7_b1_7x7_cross_shift",
    "block_c384h8x48_hid1536_w16_b1_16x16_cross_shift",
    "block_c96h8x12_hid384_w8_b2_16x24_cross_shift_fp32", "block_c192h8x24_hid768_w8_b1_16x16_cross_shift_fp32",
    "block_c384h8x48_hid1536_w8_b2_8x8_cross_shift_fp32"))


# ... and of the magnitude ladders, by the same rule (kept apart: the sharp-softmax tables above are a committed record)
RANGE_SEED_OVERRIDE: Dict[Tuple[str, str], int] = {}
RANGE_DROPPED: Tuple[Tuple[str, str], ...] = ()


def _seed(cid: str, regime: str, default: int) -> int:
    return SEED_OVERRIDE.get((cid, regime), RANGE_SEED_OVERRIDE.get((cid, regime), default))


def seeded(case, regime: str):
    return replace(case, seed=_seed(case.id, regime, case.seed))


def pairs(cases, regimes) -> List[tuple]:
    """(case with the regime's seed, regime) of every rung that is kept"""
    return [(seeded(c, r), r) for c in cases for r in regimes if (c.id, r) not in DROPPED + RANGE_DROPPED]


def pair_id(p) -> str:
    return f"{p[0].id}-{p[1]}" if isinstance(p, tuple) else str(p)


def backward_case(name: str, regime: str) -> BW.Case:
    c = BP.find(name) if name == BWD_PHASED else BW.find(name)
    return replace(c, name=f"{c.name}-{regime}", regime=regime, seed=_seed(name, regime, c.seed))


BACKWARD_CASES = [backward_case(n, r) for n in BWD_THREAD + (BWD_PHASED, BWD_BLOCK) for r in BACKWARD if (n, r) not in DROPPED]
RANGE_BACKWARD_CASES = [backward_case(n, r) for n in RANGE_BWD_NAMES for r in RANGE_BACKWARD if (n, r) not in RANGE_DROPPED]


# ---- modules, inputs, references ------------------------------------------------------------------------------------------------------
def make_module(case, regime: str) -> nn.Module:
    """The package's module of the case (CPU, eval, stress recipe) with the regime applied in place"""
    if isinstance(case, AttnCase):
        m = WindowAttention(case.C, case.heads, case.head_dim, (case.win, case.win), True, True, True, 0.0, 0.0)
        m.eval()
        load_recipe_into(m, seed=case.seed, flavor="stress")
    else:
        m = BC.make_module(case)
    return m if regime == BASE else apply_to_module(m, regime)


@functools.lru_cache(maxsize=None)
def state(case, regime: str):
    return {k: v.detach().clone() for k, v in make_module(case, regime).state_dict().items()}


@functools.lru_cache(maxsize=None)
def inputs(case, regime: str):
    """NCHW float32: (x, y) of a block, (q, kv) of an attention case"""
    shape = (case.B, case.C, case.H, case.W)
    ins = (G.randn(shape, case.seed + 1), G.randn(shape, case.seed + 2))
    return ins if regime == BASE else transform_inputs(regime, ins, case.seed)


def _evaluate(case, regime: str, dtype, fmt):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state(case, regime).items()}
    a, b = (t.to(dtype) for t in inputs(case, regime))
    kw = dict(num_heads=case.heads, dims_per_head=case.head_dim, window_size=(case.win, case.win))
    with torch.no_grad():
        if isinstance(case, AttnCase):
            if fmt is None:
                return (O.window_attention(sd, "", a, b, b, use_cyclic_shift=True, **kw),)
            return (FE.window_attention(sd, "", a, b, b, use_cyclic_shift=True, fmt=fmt, **kw),)
        if fmt is None:
            return O.basic_block(sd, "", a, b, cross=case.cross, shift=case.shift, **kw)
        return FE.basic_block(sd, "", a, b, cross=case.cross, shift=case.shift, fmt=fmt, **kw)


def reference(case, regime: str, dtype=torch.float64):
    """The CPU oracle on the regime's state and inputs, evaluated in `dtype`: a tuple of NCHW outputs"""
    return _evaluate(case, regime, dtype, None)


@functools.lru_cache(maxsize=None)
def reference64(case, regime: str):
    return reference(case, regime, torch.float64)


def family(case) -> str:
    return FE.attention_family(case.C, case.heads, case.head_dim, case.win) if isinstance(case, AttnCase) else \
        FE.block_family(case.C, case.heads, case.head_dim, case.win)


@functools.lru_cache(maxsize=None)
def emulation(case, regime: str):
    """The float64 oracle with the declared roundings of the kernel family that serves the case"""
    return _evaluate(case, regime, torch.float64, FE.FORMATS[family(case)])


@functools.lru_cache(maxsize=None)
def emulation_errors(case, regime: str) -> Tuple[float, float]:
    """(rel-L2, max-rel) of the emulation against the float64 oracle, the worst output (a spike rung: the worst channel)"""
    return worst_errors(emulation(case, regime), reference64(case, regime), regime)


def per_channel(regime: str) -> bool:
    return any(op == "spike" for op, _ in parse(regime))


def worst_errors(got, ref, regime: str = BASE) -> Tuple[float, float]:
    """(rel-L2, max-rel), the worst of the outputs (NCHW).  A spike regime: each output channel against that channel's own reference,
    the worst channel."""
    if per_channel(regime):
        errs = [G.rel_err(g[:, c], r[:, c]) for g, r in zip(got, ref) for c in range(r.shape[1])]
    else:
        errs = [G.rel_err(g, r) for g, r in zip(got, ref)]
    nan = float("nan")        # max() would pass over a NaN that is not its first argument
    return tuple(nan if any(e[i] != e[i] for e in errs) else max(e[i] for e in errs) for i in (0, 1))
