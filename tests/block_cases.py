"""Case table and float64 reference of the per-block and per-stage parity tests of the fast tier (tests/test_gpu_block_fast.py on the
GPU, tests/test_block_cases_host.py for the conditioning of every case and the invariants of the route table on the CPU).

A block case is one BasicBlock (width, window, shift / cross, one or two streams, tier) at one map; a stage case is one
SelfAndCrossBlockPair (four blocks) at one map.  The maps are the smallest at which each kernel can still go wrong, not the
workload's.  Weights are the `stress` recipe loaded into the package's module, inputs G.randn; the reference is the CPU oracle
(oracle/swin_fusion_oracle.py) evaluated in the dtype asked for.  Tensors here are NCHW, as the oracle takes them; the GPU test permutes.

Every case carries the route code (swf_block_route) the block dispatch is expected to report for it in either schedule:
route() / stage_routes() restate, per family, which kernel serves which shape."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace
from typing import List, Tuple

import torch
from torch import nn

from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import BasicBlock, SelfAndCrossBlockPair, _lib as L, load_recipe_into
from tests import golden_util as G

LATENCY, THROUGHPUT = L.SCHED_LATENCY, L.SCHED_THROUGHPUT
SCHEDULES = [("latency", LATENCY), ("throughput", THROUGHPUT)]

# level -> (C, (wide hidden, narrow hidden)): encoder and decoder widths of the shipped configurations
LEVELS = {0: (24, (96, 4)), 1: (48, (192, 96)), 2: (96, (384, 192)), 3: (192, (768, 384)), 4: (384, (1536, 768))}
# level -> window -> maps (B, H, W); the first map of a window also runs the other three (shift, cross) combinations
BLOCK_MAPS = {
    0: {8: [(2, 16, 24)], 7: [(1, 14, 21)], 16: [(1, 16, 32)]},
    1: {8: [(2, 16, 24)], 7: [(1, 14, 21)],
        16: [(2, 16, 16), (1, 32, 16)]},            # one window per map (the shift mask covers 75 % of the tile); a second window
    2: {8: [(2, 16, 24), (1, 32, 32), (1, 24, 48)],  # 6 windows; exactly 16 (the boundary of the eight-wave rule); 18
        7: [(1, 28, 28), (1, 21, 42)],               # 16 and 18 windows
        16: [(2, 32, 16)]},
    3: {8: [(1, 16, 16), (1, 16, 24), (3, 8, 8)],    # 256 tokens: the last map with the folded projection; the first without; one window per image
        7: [(1, 7, 7), (3, 7, 14)],                  # 49 tokens: less than one tile; 294: a tail for the 32- and the 64-token tiles
        16: [(1, 16, 32)]},                          # no fused Q/K/V + attention kernel: the 16x16 core
    4: {8: [(2, 8, 8), (1, 8, 16)], 7: [(1, 7, 7), (3, 7, 14)], 16: [(1, 16, 16)]},
}
# off-model deep widths that are live instantiations: (C, heads, head_dim, hidden, window, map)
OFF_MODEL = [
    (128, 4, 24, 512, 8, (1, 8, 16)),
    (256, 8, 24, 1024, 8, (1, 8, 8)),
    (192, 8, 24, 640, 8, (1, 8, 16)),    # 640 % 192 != 0: 64-token tiles in both schedules
    (384, 8, 48, 640, 8, (1, 8, 8)),     # the four-wave C = 384 kernel, which no shipped configuration reaches
]
ONE_STREAM = [(96, 384, (2, 16, 16)), (384, 1536, (2, 16, 16)), (192, 768, (2, 8, 16))]   # window 8
FP32_MAPS = [(lvl, BLOCK_MAPS[lvl][8][0]) for lvl in LEVELS]                               # one map per level, exact tier
# (C, hidden, window, map): four blocks, in place
STAGES = [
    (24, 96, 8, (2, 16, 16)),
    (48, 192, 16, (1, 32, 32)),      # 16x16 ping-pong
    (96, 384, 8, (1, 32, 32)),       # 16 windows: the schedule changes the kernel
    (96, 384, 16, (1, 32, 32)),      # 16x16 ping-pong
    (192, 768, 8, (2, 16, 16)),      # folded projection + LN1 chain
    (192, 768, 8, (1, 16, 24)),      # LN1 chain without the folded projection
    (192, 384, 7, (3, 7, 14)),       # token-tile tails
    (192, 768, 16, (1, 16, 32)),     # the 16x16 core at a deep level
    (384, 1536, 8, (2, 8, 8)),
    (384, 768, 7, (1, 7, 14)),
]
# B = 3 maps for the checks that need no tolerance: every width with 8x8 windows, the 16x16 kernels (in place: through temporaries)
B3_BLOCK_W8, B3_BLOCK_W16 = (3, 16, 8), (3, 16, 16)
B3_STAGES = [(24, 96, 8, (3, 16, 16)), (96, 384, 16, (3, 16, 16)), (192, 768, 8, (3, 8, 8)), (384, 1536, 8, (3, 8, 8))]

# Seeds are picked so that the float32 oracle agrees with the float64 oracle to TOL_FP32 / 4 on every case (a LayerNorm row of tiny
# variance amplifies any arithmetic difference): tests/test_block_cases_host.py holds every case to that.  Default seed = 3100 + the
# case's index; cases that miss the bound with it are listed here by id.
SEED_OVERRIDE: dict = {}


@dataclass(frozen=True)
class Case:
    kind: str                 # "block" | "stage"
    C: int
    heads: int
    head_dim: int
    hidden: int
    win: int
    B: int
    H: int
    W: int
    shift: bool = True        # blocks only
    cross: bool = True
    dual: bool = True
    prec: int = L.PREC_FAST
    seed: int = 0
    table: bool = True        # part of the parity table (False: the B = 3 cases of the bitwise checks)

    @property
    def id(self) -> str:
        s = f"{self.kind}_c{self.C}h{self.heads}x{self.head_dim}_hid{self.hidden}_w{self.win}_b{self.B}_{self.H}x{self.W}"
        if self.kind == "block":
            s += ("_cross" if self.cross else "_self") + ("_shift" if self.shift else "_plain")
        return s + ("" if self.dual else "_one") + ("" if self.prec == L.PREC_FAST else "_fp32")

    @property
    def deep(self) -> bool:
        return self.prec == L.PREC_FAST and self.C >= 128

    @property
    def windows_per_map(self) -> int:
        return (self.H // self.win) * (self.W // self.win)


def _blk(c, heads, hd, hid, win, m, **kw) -> Case:
    return Case("block", c, heads, hd, hid, win, *m, **kw)


def _cases() -> List[Case]:
    out: List[Case] = []
    for lvl, (c, hids) in LEVELS.items():
        for hid in hids:
            for win, maps in BLOCK_MAPS[lvl].items():
                for i, m in enumerate(maps):
                    out.append(_blk(c, 8, c // 8, hid, win, m))
                    if i == 0:
                        out += [_blk(c, 8, c // 8, hid, win, m, shift=sh, cross=cr) for sh, cr in ((False, True), (True, False), (False, False))]
    out += [_blk(c, h, d, hid, win, m) for c, h, d, hid, win, m in OFF_MODEL]
    out += [_blk(c, 8, c // 8, hid, 8, m, cross=False, dual=False) for c, hid, m in ONE_STREAM]   # a single path has no cross attention
    out += [_blk(LEVELS[lvl][0], 8, LEVELS[lvl][0] // 8, LEVELS[lvl][1][0], 8, m, prec=L.PREC_FP32) for lvl, m in FP32_MAPS]
    out += [Case("stage", c, 8, c // 8, hid, win, *m) for c, hid, win, m in STAGES]
    # the bitwise checks: cross and self block of every width, stages at four widths
    widths = [(c, 8, c // 8, hid) for c, hids in LEVELS.values() for hid in hids] + [(c, h, d, hid) for c, h, d, hid, _, _ in OFF_MODEL]
    for c, h, d, hid in widths:
        out += [_blk(c, h, d, hid, 8, B3_BLOCK_W8, cross=cr, table=False) for cr in (True, False)]
    for c in (24, 48, 96, 192):
        out += [_blk(c, 8, c // 8, 4 * c, 16, B3_BLOCK_W16, cross=cr, table=False) for cr in (True, False)]
    out += [Case("stage", c, 8, c // 8, hid, win, *m, table=False) for c, hid, win, m in B3_STAGES]
    assert len({c.id for c in out}) == len(out)
    return [replace(c, seed=SEED_OVERRIDE.get(c.id, 3100 + i)) for i, c in enumerate(out)]


ALL = _cases()
BLOCKS = [c for c in ALL if c.kind == "block" and c.table]
STAGE_CASES = [c for c in ALL if c.kind == "stage" and c.table]
DEEP_STAGES = [c for c in STAGE_CASES if c.deep]
B3_BLOCKS = [c for c in ALL if c.kind == "block" and not c.table]
B3_STAGE_CASES = [c for c in ALL if c.kind == "stage" and not c.table]
CASES = BLOCKS + STAGE_CASES          # what is compared with the float64 oracle


def find(kind: str, C: int, hidden: int, win: int, m: Tuple[int, int, int], **kw) -> Case:
    want = dict(shift=True, cross=True, dual=True, prec=L.PREC_FAST, table=True)
    want.update(kw)
    return next(c for c in ALL if (c.kind, c.C, c.hidden, c.win, (c.B, c.H, c.W)) == (kind, C, hidden, win, tuple(m))
                and all(getattr(c, k) == v for k, v in want.items() if not (kind == "stage" and k in ("shift", "cross"))))


# ---- expected routes ---------------------------------------------------------------------------------------------------------------
def schedule_changes_the_kernel(c: Case) -> bool:
    """The two places where the fast tier has a choice of kernel shape: level 2 with 8x8 / 7x7 windows on maps of 16 windows or fewer
    (eight waves per window, or four), and the fused MLP at C = 192 with a hidden width that is a multiple of 192 (32-token tiles, or 64)."""
    if c.prec != L.PREC_FAST:
        return False
    return (c.C == 96 and c.dual and c.win in (7, 8) and c.windows_per_map <= 16) or (c.C == 192 and c.hidden % 192 == 0)


def route(c: Case, schedule: int, *, in_place: bool = False, prepacked: bool = False) -> int:
    """swf_block_route of one block of the case's shape (kind "stage": with the case's own shift / cross fields)."""
    if c.prec != L.PREC_FAST:
        return L.BLOCK_GENERIC
    pre = L.BLOCK_PREPACKED if prepacked else 0
    if c.C < 128:                                            # levels 0 - 2: one register-resident launch, which needs two streams
        if not c.dual:
            return L.BLOCK_GENERIC
        r = L.BLOCK_WINDOW | pre
        if c.win == 16:
            r |= L.BLOCK_WIN_W16
            if c.C != 24 and c.cross and in_place:           # one workgroup per (window, stream): a cross block cannot run in place
                r |= L.BLOCK_VIA_TMP
        elif c.C == 96 and schedule == LATENCY and c.windows_per_map <= 16:
            r |= L.BLOCK_WIN_X8
        return r
    r = L.BLOCK_DEEP | pre
    square = c.heads * c.head_dim == c.C                     # the fragment-major projection kernels take square weights
    fused_mlp = c.C in (128, 192, 256, 384) and c.hidden % 128 == 0
    qkvattn = (c.C, c.heads, c.head_dim) == (192, 8, 24) and c.win in (7, 8)
    fold = qkvattn and fused_mlp and c.H * c.W <= 256
    attnproj = (c.C, c.heads, c.head_dim) == (384, 8, 48) and c.win in (7, 8)
    if qkvattn:
        r |= L.BLOCK_DEEP_QKVATTN | (L.BLOCK_DEEP_FOLD_PROJ if fold else 0)
    elif square and c.C in (192, 384):
        r |= L.BLOCK_DEEP_QKV
    if attnproj:
        r |= L.BLOCK_DEEP_ATTNPROJ
    elif not qkvattn and c.win == 16:
        r |= L.BLOCK_DEEP_CORE16
    if not fold and not attnproj and square and c.C in (192, 384):
        r |= L.BLOCK_DEEP_PROJ
    if fused_mlp:
        r |= L.BLOCK_MLP_FUSED
        chunks = c.hidden // 128
        if c.C == 384 and c.hidden % 256 == 0:
            r |= L.BLOCK_MLP_WIDE8
            splits = c.hidden // 256
        elif c.C == 192 and c.hidden % 192 == 0:
            r |= L.BLOCK_MLP_TOK32 if schedule == LATENCY else L.BLOCK_MLP_TOK64
            splits = 1
        else:
            r |= L.BLOCK_MLP_TOK64
            splits = (2 if chunks % 2 == 0 else 1) if c.C <= 256 else (chunks // 2 if chunks % 2 == 0 else chunks)
        if splits > 1:
            r |= L.BLOCK_MLP_SPLIT
    return r


def stage_blocks(c: Case) -> List[Case]:
    """The four blocks of a stage as block cases: self / plain, self / shifted, cross / plain, cross / shifted."""
    return [replace(c, kind="block", shift=bool(i & 1), cross=i >= 2) for i in range(4)]


def stage_routes(c: Case, schedule: int, handoff: bool = False) -> List[int]:
    """The four codes of swf_block_stage_fwd_prec: every block runs from the images the entry packed; the two cross blocks of a kernel
    that cannot run in place go through the temporaries; at the deep widths each block's MLP leaves the next block's LN1 planes."""
    out = []
    for i, b in enumerate(stage_blocks(c)):
        images = c.prec == L.PREC_FAST and (c.dual or c.C >= 128)
        r = route(b, schedule, prepacked=images)
        if r & L.BLOCK_FAMILY_MASK == L.BLOCK_WINDOW and c.win == 16 and c.C != 24 and i >= 2:
            r |= L.BLOCK_VIA_TMP
        if r & L.BLOCK_MLP_FUSED:
            r |= (L.BLOCK_LN1_GIVEN if i > 0 else 0) | (L.BLOCK_LN1_WRITTEN if i < 3 or handoff else 0)
        out.append(r)
    return out


# ---- weights, inputs, reference ----------------------------------------------------------------------------------------------------
def make_module(c: Case) -> nn.Module:
    """The package's module of the case with the stress recipe (CPU, eval).  Always built with two streams: a one-stream case uses
    its x stream (a self-attention block's streams do not see each other)."""
    win = (c.win, c.win)
    if c.kind == "stage":
        m = SelfAndCrossBlockPair(c.C, c.heads, c.head_dim, win, True, True, 0.0, 0.0, c.hidden, nn.ELU(inplace=True), 0.0)
    else:
        m = BasicBlock(c.C, c.heads, c.head_dim, win, c.shift, True, c.cross, True, 0.0, 0.0, c.hidden, nn.ELU(inplace=True), 0.0)
    m.eval()
    load_recipe_into(m, seed=c.seed, flavor="stress")
    return m


@functools.lru_cache(maxsize=None)
def state(c: Case):
    return {k: v.detach().clone() for k, v in make_module(c).state_dict().items()}


@functools.lru_cache(maxsize=None)
def inputs(c: Case):
    shape = (c.B, c.C, c.H, c.W)
    return G.randn(shape, c.seed + 1), G.randn(shape, c.seed + 2)


@functools.lru_cache(maxsize=None)
def ln1_params(c: Case):
    """gamma, beta per stream of the first block of a stage that would run next (float32 [C]): what a hand-off request passes."""
    g = lambda k: 1 + 0.2 * G.randn((c.C,), c.seed + 10 + k)
    b = lambda k: 0.1 * G.randn((c.C,), c.seed + 20 + k)
    return (g(0), b(0)), (g(1), b(1))


def reference(c: Case, dtype=torch.float64, images=None):
    """(out_x, out_y), NCHW, evaluated in `dtype` (a one-stream case: compare out_x).  images: evaluate these images of the batch only
    (images do not see each other: tests/block_pass_cases.py gates a sample of a large batch)."""
    x, y = (t.to(dtype) if images is None else t[list(images)].to(dtype) for t in inputs(c))
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state(c).items()}
    kw = dict(num_heads=c.heads, dims_per_head=c.head_dim, window_size=(c.win, c.win))
    with torch.no_grad():
        if c.kind == "stage":
            return O.self_and_cross_block_pair(sd, "", x, y, **kw)
        return O.basic_block(sd, "", x, y, cross=c.cross, shift=c.shift, **kw)


@functools.lru_cache(maxsize=None)
def reference64(c: Case):
    return reference(c, torch.float64)


def ln1_reference(c: Case, dtype=torch.float64):
    """LayerNorm of the stage's reference output with ln1_params, per stream, NCHW, both in `dtype`."""
    outs = reference64(c) if dtype == torch.float64 else reference(c, dtype)
    return tuple(O.layer_norm_channels(o, g.to(dtype), b.to(dtype)) for o, (g, b) in zip(outs, ln1_params(c)))
