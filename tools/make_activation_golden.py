"""Generate tests/golden/act_* by running the REAL reference on the CPU with an activation other than ELU(alpha=1).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_activation_golden.py REFERENCE_DIR

REFERENCE_DIR is a checkout of RainbowZL0/swin-unet-image-fusion.  It is imported, never copied: only data leaves — expected outputs
and the case descriptions.  Weights and inputs are not stored: they come from the seeded recipes of swin_unet_image_fusion_amd/config.py,
as for every fixture of oracle/make_golden.py (which documents the `a008_loss` stub registered below: a013 imports the training-only
loss, which needs kornia).

The fixtures' meta["kind"] values are new names (act_basic_block, act_patch_layer, act_model): tests/golden_util.cases(kind) feeds the
parametrised tests of the existing files by kind, and those run ELU.  meta["activation"] names the case of tests/activation_cases.py.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    sys.exit(__doc__)
sys.path.insert(0, REPO)
sys.path.insert(0, sys.argv[1])
_stub = types.ModuleType("a008_loss")
_stub.MyLoss = object
sys.modules["a008_loss"] = _stub

from a005_BasicBlock import BasicBlock                      # noqa: E402
from a010_StateRecorder import StateRecorder                # noqa: E402
from a011_PatchOperation import PatchMergingAndLinearLayer  # noqa: E402
from a013_ModelDefinition import MyModel                    # noqa: E402

from swin_unet_image_fusion_amd.config import CONFIGS, alias_groups_from_tensors, load_recipe_into, synthetic_pair  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
torch.set_grad_enabled(False)

ACTIVATIONS = {   # the names of tests/activation_cases.py
    "gelu": lambda: nn.GELU(approximate="none"), "gelu_tanh": lambda: nn.GELU(approximate="tanh"), "relu": lambda: nn.ReLU(),
    "leaky0.2": lambda: nn.LeakyReLU(0.2), "elu0.5": lambda: nn.ELU(alpha=0.5), "silu": lambda: nn.SiLU(),
}


def randn(shape, seed):
    return torch.from_numpy(np.random.default_rng(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


def key_table(module):
    sd = module.state_dict()
    alias = alias_groups_from_tensors(sd)
    return {"shapes": {k: list(v.shape) for k, v in sd.items()}, "alias_of": {k: a for k, a in alias.items() if a != k}}


def save(name, meta, **arrays):
    np.savez_compressed(os.path.join(OUT, name + ".npz"), meta=np.array(json.dumps(meta)), **{k: v.numpy() for k, v in arrays.items()})
    print("wrote", name, {k: tuple(v.shape) for k, v in arrays.items()})


def gen_blocks():
    c, nh, d, win, hid, (b, h, w) = 24, 8, 3, (8, 8), 96, (1, 16, 16)      # the bb_cross_shift_w8 shape
    for act in ("gelu", "leaky0.2", "elu0.5"):
        kw = dict(in_out_dims=c, num_heads=nh, dims_per_head=d, window_size=win, use_cyclic_shift=True, use_dual_path=True, use_cross_attr=True,
                  use_qkv_bias=True, attention_drop_ratio=0.0, linear_after_att_drop_ratio=0.0, mlp_hidden_dims=hid, mlp_drop_ratio=0.0)
        m = BasicBlock(**kw, mlp_activation_func=ACTIVATIONS[act]()).eval()
        load_recipe_into(m, seed=12, flavor="stress")
        x, y = randn((b, c, h, w), 201), randn((b, c, h, w), 202)
        ox, oy = m(x.clone(), y.clone())
        save(f"act_bb_cross_shift_w8_{act}", dict(kind="act_basic_block", activation=act, ctor=kw, in_shape=[b, c, h, w], seed_x=201, seed_y=202,
                                                  weight_seed=12, flavor="stress", keys=key_table(m)), expected_x=ox, expected_y=oy)


def gen_patch():
    for tag, enc, cin, cout, (b, h, w) in [("enc_8_16", True, 8, 16, (1, 8, 8)), ("dec_16_8", False, 16, 8, (1, 4, 6)), ("dec_24_1", False, 24, 1, (2, 8, 8))]:
        for act in ("gelu_tanh", "relu"):
            m = PatchMergingAndLinearLayer(belongs_to_encoder=enc, use_dual_path=True, in_dims=cin, out_dims=cout,
                                           patch_merging_size_recorder=StateRecorder(), merging_or_unmerging_size=(2, 2),
                                           activation_func=ACTIVATIONS[act]()).eval()
            load_recipe_into(m, seed=14, flavor="stress")
            x, y = randn((b, cin, h, w), 401), randn((b, cin, h, w), 402)
            ox, oy = m(x.clone(), y.clone())
            save(f"act_pm_{tag}_{act}", dict(kind="act_patch_layer", activation=act, encoder=enc, in_dims=cin, out_dims=cout, in_shape=[b, cin, h, w],
                                             seed_x=401, seed_y=402, weight_seed=14, flavor="stress", keys=key_table(m)), expected_x=ox, expected_y=oy)


def gen_models():
    for name, (b, h, w), act in [("act_model_tiny_16", (2, 16, 16), "gelu"), ("act_model_tiny_pad_18x22", (1, 18, 22), "silu")]:
        m = MyModel(**CONFIGS["tiny"].model_kwargs(ACTIVATIONS[act]())).eval()
        load_recipe_into(m, seed=0, flavor="stress")
        ir, vis = synthetic_pair(b, h, w)
        out = m(torch.from_numpy(ir), torch.from_numpy(vis))
        save(name, dict(kind="act_model", activation=act, config="tiny", in_shape=[b, 1, h, w], seed_ir=1, seed_vis=2, weight_seed=0, flavor="stress",
                        keys_file="state_keys_tiny.json"), expected=out)


if __name__ == "__main__":
    gen_blocks()
    gen_patch()
    gen_models()
