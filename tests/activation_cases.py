"""The activations mlp_activation_func may hold, and the units they are tested on (tests/test_activation_host.py on the CPU,
tests/test_gpu_activation.py on the GPU).

A case is (name, factory of the torch module, the (kind, param) it must map to, whether its derivative jumps).  A unit is one module of
this package at one small shape together with the oracle function that restates it; `reference(unit, case)` runs the shimmed oracle
once per (unit, case, dtype) with autograd and is cached, so the host and the GPU tests share one reference and leave it unchanged.

Shapes are the smallest at which the generic kernels take each of their paths: odd hidden widths, more than one 64-row GEMM tile, the
split-K reduce (K >= 384 and K >= 1024), the vector LayerNorm widths 1 / 2 / 4, the scalar LayerNorm and scatter (Cout % 4 != 0) and
both head kernels.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, Optional, Tuple

import torch
from torch import nn

from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import (CONFIGS, AutoPathMLP, BasicBlock, MyModel, PatchMergingAndLinearLayer, StateRecorder, load_recipe_into,
                                        synthetic_pair)
from swin_unet_image_fusion_amd import _lib as L
from tests import golden_util as G
from tests.activation_oracle import shimmed


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    make: Callable[[], nn.Module]
    kind: int
    param: float
    kinked: bool          # the derivative is discontinuous at 0: the kink condition applies to its backward cases


CASES = (
    Case("elu1", lambda: nn.ELU(alpha=1.0), L.ACT_ELU1, 0.0, False),            # the control: today's path
    Case("elu0.5", lambda: nn.ELU(alpha=0.5), L.ACT_ELU, 0.5, True),
    Case("elu2", lambda: nn.ELU(alpha=2.0), L.ACT_ELU, 2.0, True),
    Case("relu", lambda: nn.ReLU(), L.ACT_RELU, 0.0, True),
    Case("leaky0.01", lambda: nn.LeakyReLU(0.01), L.ACT_LEAKY_RELU, 0.01, True),
    Case("leaky0.2", lambda: nn.LeakyReLU(0.2), L.ACT_LEAKY_RELU, 0.2, True),
    Case("leaky-0.5", lambda: nn.LeakyReLU(-0.5), L.ACT_LEAKY_RELU, -0.5, True),
    Case("gelu", lambda: nn.GELU(approximate="none"), L.ACT_GELU, 0.0, False),
    Case("gelu_tanh", lambda: nn.GELU(approximate="tanh"), L.ACT_GELU_TANH, 0.0, False),
    Case("silu", lambda: nn.SiLU(), L.ACT_SILU, 0.0, False),
)
CASE = {c.name: c for c in CASES}


@dataclasses.dataclass(frozen=True)
class Unit:
    name: str
    build: Callable[[nn.Module], nn.Module]                 # activation -> module of this package (CPU, eval())
    oracle: Callable                                        # (sd, x, y) -> tuple of outputs
    in_shape: Tuple[int, ...]
    dual: bool = True
    seed: int = 0                                           # weights; inputs use seed + 1 .., chosen so that the kink condition holds
    call: Optional[Callable] = None                         # (module, x, y) -> outputs, where it is not module(x, y)
    in01: bool = False                                      # inputs ~U[0, 1) (images) instead of N(0, 1)
    ref_build: Optional[Callable] = None                    # the module whose state dict the oracle runs on, where `build`'s lacks keys


def _block(name, C_, nh, d, win, hid, shape, shift, cross, dual, seed):
    b, h, w = shape
    mk = lambda two: lambda act: BasicBlock(C_, nh, d, (win, win), shift, two, cross and dual, True, 0.0, 0.0, hid, act, 0.0).eval()
    return Unit(name, mk(dual),
                lambda sd, x, y: O.basic_block(sd, "", x, y, cross=cross and dual, shift=shift, num_heads=nh, dims_per_head=d, window_size=(win, win)),
                (b, C_, h, w), dual, seed, ref_build=None if dual else mk(True))


def _mlp(name, C_, hid, shape, seed):
    b, h, w = shape
    return Unit(name, lambda act: AutoPathMLP(C_, hid, act, True, 0.0).eval(), lambda sd, x, y: O.auto_path_mlp(sd, "", x, y), (b, C_, h, w), True, seed)


def _patch(enc, cin, cout, shape, seed):
    b, h, w = shape
    return Unit(f"patch_{'enc' if enc else 'dec'}_{cin}_{cout}",
                lambda act: PatchMergingAndLinearLayer(belongs_to_encoder=enc, use_dual_path=True, in_dims=cin, out_dims=cout,
                                                       patch_merging_size_recorder=StateRecorder(), merging_or_unmerging_size=(2, 2),
                                                       activation_func=act).eval(),
                lambda sd, x, y: O.patch_layer(sd, "", x, y, encoder=enc, merging_size=(2, 2)), (b, cin, h, w), True, seed)


def _tiny_cfg(ksize=3):
    return dataclasses.replace(CONFIGS["tiny"], final_conv_layer_kernel_size=ksize)


def _head(ksize, shape, seed):
    b, h, w = shape
    cfg = _tiny_cfg(ksize)
    return Unit(f"head_k{ksize}", lambda act: MyModel(**cfg.model_kwargs(act)).eval(), lambda sd, x, y: (O.final_head(sd, x, y, ksize),), (b, 1, h, w),
                True, seed, call=lambda m, x, y: m.do_final_layer(x, y))


def _model(name, shape, seed):
    b, h, w = shape
    cfg = _tiny_cfg()
    return Unit(name, lambda act: MyModel(**cfg.model_kwargs(act)).eval(), lambda sd, x, y: (O.model_forward(sd, cfg, x, y),), (b, 1, h, w), True, seed,
                in01=True)


# the shifted cross block at two widths, a single-path block
BLOCK_C8 = _block("block_c8_w4", 8, 2, 4, 4, 32, (2, 8, 12), True, True, True, 100)
BLOCK_C24 = _block("block_c24_w8", 24, 8, 3, 8, 96, (1, 16, 16), True, True, True, 110)
BLOCK_SINGLE = _block("block_c16_single", 16, 2, 8, 4, 40, (2, 8, 8), True, False, False, 120)
# K >= 384 and K >= 1024 reach the split-K reduce epilogues of the fast tier (fc2's K = hidden; fc1's at C = 256 is below them)
MLP_C96 = _mlp("mlp_c96", 96, 384, (1, 8, 8), 138)
MLP_C256 = _mlp("mlp_c256", 256, 1024, (1, 8, 8), 140)
PATCHES = (_patch(True, 1, 24, (2, 16, 12), 150), _patch(True, 8, 16, (1, 8, 8), 160), _patch(False, 16, 8, (1, 4, 6), 170),
           _patch(False, 24, 1, (2, 8, 8), 180), _patch(True, 96, 192, (1, 4, 4), 190), _patch(False, 384, 192, (1, 2, 2), 200))
HEAD_K3 = _head(3, (2, 12, 20), 210)     # head_fused3
HEAD_K5 = _head(5, (1, 9, 11), 220)      # the two-launch path
MODEL_16 = _model("model_tiny_16", (1, 16, 16), 232)
MODEL_18x22 = _model("model_tiny_pad_18x22", (1, 18, 22), 240)

FORWARD_UNITS = (BLOCK_C8, BLOCK_C24, BLOCK_SINGLE, MLP_C96, MLP_C256, *PATCHES, HEAD_K3, HEAD_K5, MODEL_16, MODEL_18x22)
BACKWARD_UNITS = (BLOCK_C8, BLOCK_C24, MLP_C96, *PATCHES, HEAD_K3, MODEL_16)
UNIT = {u.name: u for u in FORWARD_UNITS}


def inputs(unit: Unit):
    if unit.in01:
        b, _, h, w = unit.in_shape
        ir, vis = synthetic_pair(b, h, w, seed_ir=unit.seed + 1, seed_vis=unit.seed + 2)
        return torch.from_numpy(ir), torch.from_numpy(vis)
    return G.randn(unit.in_shape, unit.seed + 1), G.randn(unit.in_shape, unit.seed + 2)


def module_for(unit: Unit, case: Case, act: Optional[nn.Module] = None) -> nn.Module:
    """The unit's module with the case's activation (or `act`) and the reference's weights (CPU)."""
    m = unit.build(act if act is not None else case.make())
    own = m.state_dict()
    m.load_state_dict({k: v.detach() for k, v in reference(unit.name, case.name, torch.float32, False).sd.items() if k in own})
    return m


@dataclasses.dataclass
class Reference:
    sd: dict               # state dict the oracle ran on (leaf tensors; .grad filled when with_grad)
    x: torch.Tensor
    y: torch.Tensor
    outs: tuple            # detached outputs
    weights: tuple         # the linear functional's weights, one per output
    pre_activations: list  # every tensor the activation was applied to
    min_abs_u: float


@functools.lru_cache(maxsize=None)
def reference(unit_name: str, case_name: str, dtype: torch.dtype = torch.float32, with_grad: bool = True) -> Reference:
    """The shimmed oracle on the unit, with autograd of a generic linear functional of the outputs as the loss."""
    unit, case = UNIT[unit_name], CASE[case_name]
    m = (unit.ref_build or unit.build)(case.make())
    load_recipe_into(m, seed=unit.seed, flavor="stress")
    sd = {k: v.detach().clone().to(dtype if v.is_floating_point() else v.dtype).requires_grad_(with_grad and v.is_floating_point() and "running" not in k)
          for k, v in m.state_dict().items()}
    x, y = (t.to(dtype).requires_grad_(with_grad) for t in inputs(unit))
    with torch.set_grad_enabled(with_grad), shimmed(case.make(), keep=True) as ns:   # (whatever mode an earlier test left behind)
        outs = tuple(unit.oracle(sd, x, y))
        if not unit.dual:
            outs = outs[:1]      # (the oracle is dual-path only: a single-path unit is its x stream)
        weights = tuple(G.randn(tuple(o.shape), unit.seed + 10 + i).to(dtype) for i, o in enumerate(outs))
        if with_grad:
            sum((o * wt).sum() for o, wt in zip(outs, weights)).backward()
    return Reference(sd, x, y, tuple(o.detach() for o in outs), weights, ns.pre_activations, ns.min_abs_u)


def kink_margin(unit_name: str, case_name: str) -> Tuple[float, float]:
    """(min |u64|, max |u32 - u64|) over every pre-activation of the case: a test that compares a derivative which jumps at 0 is only
    meaningful when no pre-activation of the reference sits within rounding of 0."""
    r32, r64 = reference(unit_name, case_name, torch.float32, False), reference(unit_name, case_name, torch.float64, False)
    lo = min(float(u.abs().min()) for u in r64.pre_activations)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(r32.pre_activations, r64.pre_activations))
    return lo, err


# ---- goldens written by the reference itself with these activations (tools/make_activation_golden.py) ------------------------------
GOLDEN_KINDS = ("act_basic_block", "act_patch_layer", "act_model")


def golden_names():
    return [n for kind in GOLDEN_KINDS for n in G.cases(kind)]


def golden(name: str):
    """(case, state dict, (x, y), expected outputs, oracle(sd, x, y) -> outputs, build(act) -> this package's module, model?) of a fixture."""
    meta, arr = G.load(name)
    case, sd = CASE[meta["activation"]], G.recipe_state(meta)
    if meta["kind"] == "act_model":
        cfg = CONFIGS[meta["config"]]
        return (case, sd, G.model_inputs(meta), (arr["expected"],), lambda s, x, y: (O.model_forward(s, cfg, x, y),),
                lambda act: MyModel(**cfg.model_kwargs(act)).eval(), True)
    xy = G.randn(meta["in_shape"], meta["seed_x"]), G.randn(meta["in_shape"], meta["seed_y"])
    exp = (arr["expected_x"], arr["expected_y"])
    if meta["kind"] == "act_basic_block":
        c = meta["ctor"]
        oracle = lambda s, x, y: O.basic_block(s, "", x, y, cross=c["use_cross_attr"], shift=c["use_cyclic_shift"], num_heads=c["num_heads"],
                                               dims_per_head=c["dims_per_head"], window_size=tuple(c["window_size"]))
        return case, sd, xy, exp, oracle, lambda act: BasicBlock(**{**c, "window_size": tuple(c["window_size"])}, mlp_activation_func=act).eval(), False
    enc = meta["encoder"]
    build = lambda act: PatchMergingAndLinearLayer(belongs_to_encoder=enc, use_dual_path=True, in_dims=meta["in_dims"], out_dims=meta["out_dims"],
                                                   patch_merging_size_recorder=StateRecorder(), merging_or_unmerging_size=(2, 2),
                                                   activation_func=act).eval()
    return case, sd, xy, exp, lambda s, x, y: O.patch_layer(s, "", x, y, encoder=enc, merging_size=(2, 2)), build, False
