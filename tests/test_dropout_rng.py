"""Training-mode dropout without a GPU: the numpy restatement of Philox4x32-10 against Random123's known answers, the keep rule, the
dropout restatement of BasicBlock with every ratio 0 against the oracle, the swf_dropout layout, argument checks of the new entries
and the [0, 1] range check of the modules."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import AutoPathMLP, BasicBlock, WindowAttention, _lib as L, load_recipe_into
from tests import dropout_util as D
from tests import golden_util as G


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    got = D.philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
    assert tuple(int(w[0]) for w in got) == want


def test_mask_rule():
    seed = 0x0123456789ABCDEF
    m = D.mask_np(seed, 1, 2, 4001, 0.25)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(0.25))
    assert set(np.unique(m).tolist()) == {0.0, float(scale)}
    # element i is word i % 4 of the counter i // 4: a prefix of a longer mask is the shorter mask
    assert np.array_equal(D.mask_np(seed, 1, 2, 17, 0.25), m[:17])
    # the counter holds the site and the stream: other values give other masks; p = 0 keeps everything, p = 1 nothing
    assert not np.array_equal(D.mask_np(seed, 0, 2, 4001, 0.25), m) and not np.array_equal(D.mask_np(seed, 1, 3, 4001, 0.25), m)
    assert np.all(D.mask_np(seed, 0, 0, 99, 0.0) == 1.0) and np.all(D.mask_np(seed, 0, 0, 99, 1.0) == 0.0)


def test_block_restatement_with_ratios_zero_is_the_oracle():
    b, c, h, w, nh, d, win, hid = 1, 8, 8, 8, 2, 4, 4, 16
    m = BasicBlock(c, nh, d, (win, win), True, True, True, True, 0.0, 0.0, hid, nn.ELU(inplace=True), 0.0)
    load_recipe_into(m, seed=5, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x, y = G.randn((b, c, h, w), 901), G.randn((b, c, h, w), 902)
    kw = dict(cross=True, shift=True, num_heads=nh, dims_per_head=d, window_size=(win, win))
    ref = O.basic_block(sd, "", x, y, **kw)
    ones = lambda s, site, width: D.nchw_mask(np.ones(b * h * w * width, np.float32), b, h, w, width)
    for got in (D.block_drop(sd, "", x, y, ones, **kw), D.block_drop(sd, "", x, y, lambda *a: None, **kw)):
        for g, r in zip(got, ref):
            assert torch.allclose(g, r, rtol=1e-5, atol=1e-6)


def test_dropout_struct_and_argument_checks():
    assert C.sizeof(L.Dropout) == 24 and L.Dropout.attn_p.offset == 8 and L.Dropout.mlp_p.offset == 16
    lib = L.lib()
    assert lib.swf_dropout_mask(1, 0, 0, 16, 0.5, None, None) == L.ERR_NULL
    for stream, site, count, p in ((0, 4, 16, 0.5), (-1, 0, 16, 0.5), (0, 0, 0, 0.5), (0, 0, 16, 1.5), (0, 0, 16, float("nan"))):
        assert lib.swf_dropout_mask(1, stream, site, count, p, 256, None) == L.ERR_BAD_SHAPE
    desc = L.BlockDesc(L.AttnDesc(8, 2, 4, 4, 4, 0), 16, 0, 0)
    p = L.BlockStreamParams()
    assert lib.swf_basic_block_fwd_drop(C.byref(desc), C.byref(p), None, 1, None, 1, None, 1, 8, 8, None, None, 0, None) == L.ERR_NULL
    assert lib.swf_basic_block_drop_workspace_bytes(C.byref(desc), 1, 8, 8) > lib.swf_basic_block_bwd_workspace_bytes(C.byref(desc), 1, 8, 8)
    assert lib.swf_window_attention_drop_workspace_bytes(C.byref(desc.attn), 1, 8, 8) > 0
    assert lib.swf_mlp_drop_workspace_bytes(64, 8, 16) > lib.swf_mlp_bwd_workspace_bytes(64, 8, 16)


@pytest.mark.parametrize("bad", [-0.1, 1.5])
def test_ratios_outside_unit_interval_raise_at_the_first_train_forward(bad):
    x = torch.zeros(1, 8, 8, 8)
    mods = [BasicBlock(8, 2, 4, (4, 4), False, True, False, True, bad, 0.0, 16, nn.ELU(), 0.0),
            BasicBlock(8, 2, 4, (4, 4), False, True, False, True, 0.0, 0.0, 16, nn.ELU(), 0.0),
            WindowAttention(8, 2, 4, (4, 4), False, False, True, 0.0, bad),
            AutoPathMLP(8, 16, nn.ELU(), True, 0.0)]
    # (an MLP ratio outside [0, 1] already fails at construction, in the nn.Dropout the reference builds too: set it afterwards)
    mods[1].mlp_drop_ratio = bad
    mods[3].drop_ratio = bad
    for m in mods:        # eval() never looks at the ratios; train() checks them before anything runs
        m.train()
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            m(x, x, x) if isinstance(m, WindowAttention) else m(x, x)
