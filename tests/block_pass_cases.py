"""Case table of the parity tests past the first pass of the window loop of the level 0 - 2 block kernels (tests/test_gpu_block_passes.py
on the GPU; tests/test_block_pass_cases_host.py holds the grid rules restated here to the source text, every case to three passes on 64,
256 and 304 CUs, and every gated image to the conditioning bar of tests/test_block_cases_host.py, on the CPU).

The register-resident kernels (window24 / window48 / window96_kernel, window96x8_kernel, windowNNw16_kernel) run
`for (win = blockIdx.x; win < nwin; win += gridDim.x)` on a grid capped by the CU count and carry state from one pass to the next (K / V
double buffers, the bias tile in registers, barriers taken on later passes only, vectors staged on the first pass only).  Every case of
tests/block_cases.py has at most 18 windows, so there the loop body runs once per workgroup.  A case here is a per-image map; its batch
comes from the device's CU count (batch()): the smallest B with B * windows_per_map >= 2.5 * grid, one more if the window count is a
multiple of the grid, so every launch makes three passes and about half the workgroups run the third.  The maps are chosen so that a
workgroup meets other window positions in successive passes (grid mod windows_per_map != 0): 3 x 5 windows at levels 0 / 1 and for the
eight-wave kernel of level 2 (at most 16 windows per image: the latency schedule takes it), 3 x 6 for level 2's four-wave kernel (more
than 16: both schedules take it), 2 x 3 for the 16x16 kernels.  Weights: the stress recipe; inputs: G.randn; reference: the float64
oracle, as in tests/block_cases.py, whose Case, route table and reference this table reuses.

Levels 3 and 4 (C >= 128) are not here on purpose: their kernels launch one workgroup per token tile, with no stride loop, so there is no
later pass to reach.  The paired form of level 2 (throughput schedule, at most 2 x CUs windows: tests/test_gpu_win96_pair.py) makes one
pass by construction; the first-pass-only chunks of the GPU test take it, the three-pass batches are past its rule."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import torch

from swin_unet_image_fusion_amd import _lib as L
from tests import block_cases as BC

MAP_3X5 = {8: (24, 40), 7: (21, 35)}     # window -> (H, W)
MAP_3X6 = {8: (24, 48), 7: (21, 42)}
MAP_W16 = (32, 48)                       # 2 x 3 windows of 16x16
WAVES = {24: 3, 48: 2, 96: 2}            # resident workgroups per CU of the 8x8 / 7x7 kernel (W24_WAVES, W48_WAVES, L96::WAVES)
TILE = 64                                # tokens per tile of the MLP half
CU_COUNTS = (64, 256, 304)               # what the host test holds the table to

# Default seed = 9000 + 3 x the case's index (the inputs take seed + 1 and seed + 2).  tests/test_block_pass_cases_host.py holds every
# gated image to fp32 oracle == fp64 oracle within TOL_FP32 / 4; a case that misses it gets another seed here, by id.
SEED_OVERRIDE: dict = {}


# ---- the grid rules ----------------------------------------------------------------------------------------------------------------
def cap(case: BC.Case, schedule: int, cus: int) -> int:
    """The most workgroups along x a launch of the case's block kernel gets on `cus` CUs, whatever the window count.
      8x8 / 7x7, all levels, and the tiles of the MLP half: WAVES * cus     csrc/win_host.h, win_launch_as (`L::WAVES * num_cus()`)
      window96x8_kernel: min(that, cus)                                     csrc/kernels_win96.hip, L96::launch (`std::min(grid, num_cus())`)
      16x16, C = 24: 2 * cus                                                csrc/kernels_win24.hip, launch16
      16x16, C = 48: cus, grid.y = stream                                   csrc/kernels_win48.hip, launch16
      16x16, C = 96: (cus + 1) / 2, grid.y = stream                         csrc/kernels_win96.hip, L96::launch16"""
    if case.win == 16:
        return {24: 2 * cus, 48: cus, 96: (cus + 1) // 2}[case.C]
    g = WAVES[case.C] * cus
    return min(g, cus) if x8(case, schedule) else g


def grid(case: BC.Case, schedule: int, cus: int, mlp_tokens: int = 0) -> int:
    """gridDim.x of the case's launch: the window count under cap(); with mlp_tokens the MLP half's launch on the longer of its token
    lists (csrc/win_host.h, win_launch_half: ceil(ntok / 64) tiles dealt by the 8x8 rule)."""
    if mlp_tokens:
        return min(-(-mlp_tokens // TILE), WAVES[case.C] * cus)
    return min(case.B * case.windows_per_map, cap(case, schedule, cus))


def passes(n: int, g: int) -> int:
    """Trips of the busiest workgroup through the loop: n windows (or tiles) on g workgroups."""
    return -(-n // g)


def x8(case: BC.Case, schedule: int) -> bool:
    """The eight-wave kernel of level 2 serves the case (a stage: all four blocks; the rule looks at width, window and map only)."""
    return bool(BC.route(replace(case, kind="block"), schedule) & L.BLOCK_WIN_X8)


def batch_size(case: BC.Case, schedule: int, cus: int) -> int:
    g, wpm = cap(case, schedule, cus), case.windows_per_map
    b = -(-5 * g // (2 * wpm))
    return b + 1 if (b * wpm) % g == 0 else b


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PassCase:
    shape: BC.Case                  # B = 1: the per-image map; batch() makes the case that runs
    schedules: Tuple[str, ...]      # both where the expected route differs between them; else the existing suite holds them bit-equal

    @property
    def id(self) -> str:            # static: no batch size in it
        c = self.shape
        s = f"{c.kind}_c{c.C}_hid{c.hidden}_w{c.win}_{c.H}x{c.W}"
        return s + (("_cross" if c.cross else "_self") + ("_shift" if c.shift else "_plain") if c.kind == "block" else "")


def _cases() -> List[PassCase]:
    shapes: List[BC.Case] = []
    blk = lambda c, hid, win, hw, **kw: shapes.append(BC.Case("block", c, 8, c // 8, hid, win, 1, *hw, table=False, **kw))
    for lvl in (0, 1, 2):
        c, hids = BC.LEVELS[lvl]
        maps = MAP_3X6 if lvl == 2 else MAP_3X5
        for hid in hids:
            for win in (8, 7):
                blk(c, hid, win, maps[win])
        for sh, cr in ((False, True), (True, False), (False, False)):
            blk(c, hids[0], 8, maps[8], shift=sh, cross=cr)
    for hid in BC.LEVELS[2][1]:                      # 15 windows per image: window96x8_kernel in the latency schedule
        for win in (8, 7):
            blk(96, hid, win, MAP_3X5[win])
    for lvl in (0, 1, 2):
        blk(BC.LEVELS[lvl][0], BC.LEVELS[lvl][1][0], 16, MAP_W16)
    blk(48, BC.LEVELS[1][1][1], 16, MAP_W16)
    for lvl in (0, 1, 2):
        shapes.append(BC.Case("stage", BC.LEVELS[lvl][0], 8, BC.LEVELS[lvl][0] // 8, BC.LEVELS[lvl][1][0], 8, 1, *MAP_3X5[8], table=False))
    shapes.append(BC.Case("stage", 48, 8, 6, 192, 16, 1, *MAP_W16, table=False))     # ping-pong through temporaries
    out = []
    for i, c in enumerate(shapes):
        routes = [BC.stage_routes(c, s) if c.kind == "stage" else BC.route(c, s) for _, s in BC.SCHEDULES]
        pc = PassCase(c, tuple(n for n, _ in BC.SCHEDULES) if routes[0] != routes[1] else (BC.SCHEDULES[0][0],))
        out.append(replace(pc, shape=replace(c, seed=SEED_OVERRIDE.get(pc.id, 9000 + 3 * i))))
    assert len({p.id for p in out}) == len(out)
    return out


ALL = _cases()
BLOCKS = [p for p in ALL if p.shape.kind == "block"]
STAGES = [p for p in ALL if p.shape.kind == "stage"]
SCHED = dict(BC.SCHEDULES)


def runs(cases: List[PassCase]):
    """(case, schedule name, schedule) of every launch kind the table asks for."""
    return [(p, n, SCHED[n]) for p in cases for n in p.schedules]


def run_id(r) -> str:
    return f"{r[0].id}-{r[1]}"


def find(kind: str, C: int, hidden: int, win: int, hw: Tuple[int, int], shift: bool = True, cross: bool = True) -> PassCase:
    return next(p for p in ALL if (p.shape.kind, p.shape.C, p.shape.hidden, p.shape.win, (p.shape.H, p.shape.W)) == (kind, C, hidden, win, tuple(hw))
                and (kind == "stage" or (p.shape.shift, p.shape.cross) == (shift, cross)))


def batch(p: PassCase, schedule: int, cus: int) -> BC.Case:
    """The case as it runs on a device of `cus` CUs: three passes, the last one ragged."""
    return replace(p.shape, B=batch_size(p.shape, schedule, cus))


def chunk_images(case: BC.Case, schedule: int, cus: int) -> int:
    """Images per first-pass-only launch: as many whole images as the capped grid has workgroups."""
    return max(1, cap(case, schedule, cus) // case.windows_per_map)


def image_passes(case: BC.Case, g: int, i: int) -> Tuple[int, int]:
    """The passes (from 1) in which the first and the last window of image i run."""
    wpm = case.windows_per_map
    return i * wpm // g + 1, ((i + 1) * wpm - 1) // g + 1


def gated_images(case: BC.Case, g: int, sample: bool = False) -> Optional[List[int]]:
    """None: the whole batch meets the float64 oracle (8x8 / 7x7 blocks: 1.4 - 2.9 s of CPU time).  16x16 blocks (5 - 15 s for the whole
    batch) and stages (four blocks): the first and the last image whose windows lie wholly in each pass, every image that straddles a
    pass boundary, and the last image; `sample` asks for these whatever the case (the attention half: three references a case).
    (The bitwise comparison with first-pass-only launches covers every image either way.)"""
    if case.kind == "block" and case.win != 16 and not sample:
        return None
    spans = [image_passes(case, g, i) for i in range(case.B)]
    pick = {case.B - 1}
    for p in range(1, passes(case.B * case.windows_per_map, g) + 1):
        whole = [i for i, s in enumerate(spans) if s == (p, p)]
        assert len(whole) >= 2, (case.id, g, p)
        pick.update((whole[0], whole[-1]))
    pick.update(i for i, s in enumerate(spans) if s[0] != s[1])
    return sorted(pick)


def edge(case: BC.Case, win_index: int) -> bool:
    """A shifted 8x8 / 7x7 window in the last window row or column: the one whose bias tile gets -inf added (and is reloaded after)."""
    nwx = case.W // case.win
    r = win_index % case.windows_per_map
    return case.shift and (r // nwx == case.H // case.win - 1 or r % nwx == nwx - 1)


@functools.lru_cache(maxsize=2)   # a batch is tens of MB a stream: only what consecutive tests share stays
def reference64(case: BC.Case, images: Optional[Tuple[int, ...]] = None):
    return BC.reference(case, torch.float64, images)


# ---- the half-block modes (levels 0 / 1 through the modules) -----------------------------------------------------------------------
HALF_LEVELS = (0, 1)
MLP_MAP = MAP_3X5[7]             # 735 tokens an image: odd, so B steers the remainder mod 64


def mlp_batch(C: int, dual: bool, cus: int) -> int:
    """Images of MLP_MAP for three passes of the MLP half with a ragged last pass and a partial last tile.  One stream: the list is split
    between the kernel's two stream slots (csrc/swf_api.hip, mlp_half24), so the launch is sized by the first slot's share."""
    g, per = WAVES[C] * cus, MLP_MAP[0] * MLP_MAP[1]
    b = -(-5 * g * TILE // (2 * per)) * (1 if dual else 2)
    while True:
        n = b * per
        tiles = -(-mlp_slot_tokens(n, dual)[0] // TILE)
        if n % TILE and tiles % g and 2 * tiles >= 5 * g:
            return b
        b += 1


def mlp_slot_tokens(n: int, dual: bool) -> Tuple[int, int]:
    """Tokens in the two stream slots of the MLP half for n tokens per stream."""
    if dual:
        return n, n
    n0 = min(n, ((n + 1) // 2 + TILE - 1) // TILE * TILE)
    return n0, n - n0


def mlp_chunk_images(C: int, dual: bool, cus: int) -> int:
    """Images per launch whose tiles all run in the first pass."""
    g, per = WAVES[C] * cus, MLP_MAP[0] * MLP_MAP[1]
    b = g * TILE * (1 if dual else 2) // per
    while -(-mlp_slot_tokens(b * per, dual)[0] // TILE) > g:
        b -= 1
    return b


def half_case(C: int) -> BC.Case:
    """The block whose weights and 3 x 5 map the half-block tests use: wide hidden, 8x8, cross + shift."""
    lvl = next(l for l in HALF_LEVELS if BC.LEVELS[l][0] == C)
    return find("block", C, BC.LEVELS[lvl][1][0], 8, MAP_3X5[8]).shape


def half_module(C: int, dual: bool):
    """BasicBlock of half_case(C) with the stress recipe (CPU, eval); one stream: a single-path block of the same seed."""
    c = half_case(C)
    if dual:
        return BC.make_module(c)
    m = BC.BasicBlock(c.C, c.heads, c.head_dim, (c.win, c.win), c.shift, False, False, True, 0.0, 0.0, c.hidden, BC.nn.ELU(inplace=True), 0.0)
    m.eval()
    BC.load_recipe_into(m, seed=c.seed, flavor="stress")
    return m


def mlp_inputs(C: int, b: int):
    shape = (b, C, *MLP_MAP)
    return BC.G.randn(shape, 9800 + C), BC.G.randn(shape, 9801 + C)


def _cast(sd, dtype):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach()) for k, v in sd.items()}


def attn_half_reference(sd, case: BC.Case, x, y, dtype=torch.float64):
    """(raw, with LN1 and the residual): the oracle's auto_path_win_att on x, y, and x + auto_path_win_att(LN1(x), LN1(y)), each a pair."""
    sd, x, y = _cast(sd, dtype), x.to(dtype), y.to(dtype)
    kw = dict(cross=case.cross, num_heads=case.heads, dims_per_head=case.head_dim, window_size=(case.win, case.win), use_cyclic_shift=case.shift)
    with torch.no_grad():
        raw = BC.O.auto_path_win_att(sd, "auto_path_win_att.", x, y, **kw)
        nx = BC.O.layer_norm_channels(x, sd["stage_1.norm_layer_1.weight"], sd["stage_1.norm_layer_1.bias"])
        ny = BC.O.layer_norm_channels(y, sd["stage_1.norm_layer_2.weight"], sd["stage_1.norm_layer_2.bias"])
        ax, ay = BC.O.auto_path_win_att(sd, "auto_path_win_att.", nx, ny, **kw)
    return raw, (x + ax, y + ay)


def mlp_half_reference(sd, x, y=None, dtype=torch.float64):
    """(raw, with LN2 and the residual): the oracle's auto_path_mlp, and x + auto_path_mlp(LN2(x)); y None: the one stream of a
    single-path block (the oracle's function is the dual one: it runs with the x stream's weights in both places)."""
    sd, x = _cast(sd, dtype), x.to(dtype)
    dual = y is not None
    y = y.to(dtype) if dual else x
    if not dual:
        sd.update({k.replace("mlp_x_", "mlp_y_"): v for k, v in sd.items() if "mlp_x_" in k})
        sd.update({k.replace("norm_layer_1", "norm_layer_2"): v for k, v in sd.items() if k.startswith("stage_2.norm_layer_1")})
    with torch.no_grad():
        raw = BC.O.auto_path_mlp(sd, "auto_path_mlp.", x, y)
        nx = BC.O.layer_norm_channels(x, sd["stage_2.norm_layer_1.weight"], sd["stage_2.norm_layer_1.bias"])
        ny = BC.O.layer_norm_channels(y, sd["stage_2.norm_layer_2.weight"], sd["stage_2.norm_layer_2.bias"])
        mx, my = BC.O.auto_path_mlp(sd, "auto_path_mlp.", nx, ny)
    full = (x + mx, y + my)
    return (raw, full) if dual else (raw[:1], full[:1])
