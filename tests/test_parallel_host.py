"""CPU-only checks of the data-parallel surface: the new library entries (swf_tensors_gather / _scatter, the four entries of the head's
BatchNorm over a batch that spans ranks) validate their arguments without a device, header / exports / ctypes table agree, and
DataParallelStep's bookkeeping (segment offsets, one all-reduce per reduction, none at world size 1, equal shards, refusing a
non-contiguous gradient) with stand-ins for the library calls and a recording collective."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
from torch import nn

import __graft_entry__ as entry
from swin_unet_image_fusion_amd import CONFIGS, DataParallelStep, MyModel, _lib as L, load_recipe_into, parallel

NEW = ("swf_tensors_gather", "swf_tensors_scatter", "swf_final_head_stats_pass", "swf_final_head_stats_finish", "swf_final_head_bwd_sums",
       "swf_final_head_bwd_synced")
P = 0x10000   # a made-up device address: never dereferenced, every check comes before the first HIP call


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()


def _table(numels, flat=0x100000, gather=True):
    """A filled host table whose flat side addresses consecutive unpadded segments of `flat`."""
    lib, n = L.lib(), len(numels)
    offs = np.concatenate([[0], np.cumsum(numels)[:-1]]).astype(np.uint64)
    seg = (np.uint64(flat) + 4 * offs).astype(np.uint64)
    other = np.array([0x40000000 + 0x100000 * i for i in range(n)], dtype=np.uint64)
    dst, src = (seg, other) if gather else (other, seg)
    nbytes = lib.swf_adam_table_bytes(n, int(sum(numels)))
    host = C.create_string_buffer(nbytes)
    arrays = [dst, src, dst, dst, np.array(numels, dtype=np.int64), np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)]
    assert lib.swf_adam_table_fill(host, nbytes, n, *[a.ctypes.data for a in arrays]) == L.OK
    return host, nbytes, n


def test_gather_and_scatter_validate_arguments_without_gpu():
    lib = L.lib()
    numels = [1, 3, 225, 4096, 4097, 3 * 4096 + 5]
    total, flat = sum(numels), 0x100000
    for gather in (True, False):
        host, nbytes, n = _table(numels, flat, gather)
        call = ((lambda tab, dev, nb, nt, fl, ne: lib.swf_tensors_gather(tab, dev, nb, nt, fl, ne, 0.5, None)) if gather else
                (lambda tab, dev, nb, nt, fl, ne: lib.swf_tensors_scatter(tab, dev, nb, nt, fl, ne, None)))
        assert call(None, P, nbytes, n, flat, total) == L.ERR_NULL
        assert call(host, None, nbytes, n, flat, total) == L.ERR_NULL
        assert call(host, P, nbytes, n, None, total) == L.ERR_NULL
        assert call(host, P, nbytes, 0, flat, total) == L.ERR_BAD_SHAPE
        assert call(host, P, nbytes, -3, flat, total) == L.ERR_BAD_SHAPE
        assert call(host, P, n * C.sizeof(L.AdamTensor) - 1, n, flat, total) == L.ERR_WORKSPACE   # too small for its rows
        assert call(host, P, n * C.sizeof(L.AdamTensor) + 8, n, flat, total) == L.ERR_WORKSPACE   # rows fit, the chunk map does not
        # the rows must address exactly the unpadded running-sum segments, and end inside the flat buffer
        assert call(host, P, nbytes, n, flat + 16, total) == L.ERR_BAD_SHAPE
        assert call(host, P, nbytes, n, flat, total - 1) == L.ERR_BAD_SHAPE
        rows = (L.AdamTensor * n).from_buffer(host)
        if gather:
            rows[2].param = rows[2].param + 4
        else:
            rows[2].grad = rows[2].grad + 4
        assert call(host, P, nbytes, n, flat, total) == L.ERR_BAD_SHAPE
        assert b"row 2" in lib.swf_last_error_string()
    host, nbytes, n = _table(numels, flat, False)
    rows = (L.AdamTensor * n).from_buffer(host)
    rows[1].grad = None   # a scatter has no zero rows: its source is the flat buffer
    assert lib.swf_tensors_scatter(host, P, nbytes, n, flat, total, None) == L.ERR_NULL


def test_head_entries_validate_arguments_without_gpu():
    lib = L.lib()
    hp = L.HeadParams(P, P, P, P, P, P, P, P)
    b, h, w, ks = 2, 16, 16, 3
    need = lib.swf_final_head_bwd_workspace_bytes(b, h, w, ks)
    assert need > 0
    # ERR_PAD: a 3x3 head on a 1 x W map (reflect padding needs a map larger than the pad)
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 0, None, P, b, 1, w, ks, P, need, None) == L.ERR_PAD
    assert lib.swf_final_head_bwd_sums(C.byref(hp), P, P, P, P, b, 1, w, ks, P, need, None) == L.ERR_PAD
    assert lib.swf_final_head_bwd_synced(C.byref(hp), P, P, P, P, b * w, P, P, None, b, 1, w, ks, P, need, None) == L.ERR_PAD
    # ERR_WORKSPACE: valid arguments and no workspace (for the finish, which needs none, the buffer of the sums itself)
    n = b * h * w
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 0, None, P, b, h, w, ks, None, 0, None) == L.ERR_WORKSPACE
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 1, P, P, b, h, w, ks, P, 16, None) == L.ERR_WORKSPACE
    assert lib.swf_final_head_stats_finish(P, 0, n, 0, P, P, None, None, 0.1, None) == L.ERR_WORKSPACE
    assert lib.swf_final_head_bwd_sums(C.byref(hp), P, P, P, P, b, h, w, ks, None, 0, None) == L.ERR_WORKSPACE
    assert lib.swf_final_head_bwd_synced(C.byref(hp), P, P, P, P, 2 * n, P, P, None, b, h, w, ks, None, 0, None) == L.ERR_WORKSPACE
    assert lib.swf_final_head_bwd_synced(C.byref(hp), P, P, P, P, 2 * n, P, P, None, b, h, w, ks, P, need - 1, None) == L.ERR_WORKSPACE
    # ERR_NULL / ERR_BAD_SHAPE
    assert lib.swf_final_head_stats_pass(None, P, P, 0, None, P, b, h, w, ks, P, need, None) == L.ERR_NULL
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 0, None, None, b, h, w, ks, P, need, None) == L.ERR_NULL
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 1, None, P, b, h, w, ks, P, need, None) == L.ERR_NULL      # pass 1 without a mean
    assert lib.swf_final_head_stats_pass(C.byref(hp), P, P, 2, P, P, b, h, w, ks, P, need, None) == L.ERR_BAD_SHAPE
    assert lib.swf_final_head_stats_finish(None, 8, n, 0, P, P, None, None, 0.1, None) == L.ERR_NULL
    assert lib.swf_final_head_stats_finish(P, 8, 0, 0, P, P, None, None, 0.1, None) == L.ERR_BAD_SHAPE
    assert lib.swf_final_head_bwd_sums(C.byref(hp), P, P, None, P, b, h, w, ks, P, need, None) == L.ERR_NULL
    assert lib.swf_final_head_bwd_sums(C.byref(hp), P, P, P, None, b, h, w, ks, P, need, None) == L.ERR_NULL
    assert lib.swf_final_head_bwd_synced(C.byref(hp), P, P, P, None, 2 * n, P, P, None, b, h, w, ks, P, need, None) == L.ERR_NULL
    assert lib.swf_final_head_bwd_synced(C.byref(hp), P, P, P, P, n - 1, P, P, None, b, h, w, ks, P, need, None) == L.ERR_BAD_SHAPE   # whole < part


def test_header_exports_and_signatures_agree():
    with open(entry.REPO + "/include/swinfuse.h") as f:
        header = f.read()
    handle = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in swinfuse.h"
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} is not bound"
        decl = re.search(name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name
    assert L.lib().swf_version() == 1


# ---- DataParallelStep with stand-ins ---------------------------------------------------------------------------------------------
class Recorder:
    """A collective that records: world_size ranks of which this is `rank`; all_reduce_ leaves the tensor as it is unless `peer` says
    what the other ranks add."""

    def __init__(self, world_size=2, rank=0, peer=None):
        self.world_size, self.rank, self.peer = world_size, rank, peer
        self.reduced, self.broadcasts = [], []

    def all_reduce_(self, t):
        self.reduced.append(t)
        if self.peer is not None:
            t += self.peer(t)
        return t

    def broadcast_(self, t, src=0):
        self.broadcasts.append((t, src))
        return t


@pytest.fixture
def copies(monkeypatch):
    """The library's gather / scatter replaced by torch on the CPU: -> the list of (gather, pointers, scale) calls."""
    calls = []

    def run(self, gather, pointers, scale, device):
        calls.append((gather, list(pointers), scale))
        if gather:
            self.flat.zero_()
    monkeypatch.setattr(parallel._FlatTable, "run", run)
    return calls


def _tiny_with_grads():
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=0, flavor="stress")
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    return m


def test_segments_are_the_running_sum_in_parameter_order_and_one_all_reduce(copies):
    m, coll = _tiny_with_grads(), Recorder(2, 0)
    dp = DataParallelStep(m, None, None, group=coll)
    list(m.parameters())[3].grad = None   # contributes zeros, receives its segment
    dp.reduce_gradients()
    params = list(m.parameters())
    want = np.concatenate([[0], np.cumsum([p.numel() for p in params])[:-1]]).tolist()
    assert dp._grads.offsets == want and dp._grads.total == sum(p.numel() for p in params)
    assert len(coll.reduced) == 1 and coll.reduced[0] is dp._grads.flat
    assert len(copies) == 1 and copies[0][0] is True and copies[0][2] == 0.5 and copies[0][1][3] is None
    base = dp._grads.flat.data_ptr()
    for p, off in zip(params, want):
        assert p.grad.shape == p.shape and p.grad.data_ptr() == base + 4 * off
    flat = dp._grads.flat
    dp.reduce_gradients()   # the buffer is reused
    assert dp._grads.flat is flat and len(coll.reduced) == 2 and len(copies) == 2


def test_no_collective_at_world_size_one_without_force(copies):
    m = _tiny_with_grads()
    grads = [p.grad for p in m.parameters()]
    for group in (None, Recorder(1, 0)):
        dp = DataParallelStep(m, None, None, group=group)
        dp.reduce_gradients()
        dp.broadcast_state()
        assert not copies and all(p.grad is g for p, g in zip(m.parameters(), grads))
        if group is not None:
            assert not group.reduced and not group.broadcasts
    coll = Recorder(1, 0)
    DataParallelStep(m, None, None, group=coll, force_collective=True).reduce_gradients()
    assert len(coll.reduced) == 1 and len(copies) == 1 and copies[0][2] == 1.0


def test_non_contiguous_gradient_raises_before_any_call(copies):
    m, coll = _tiny_with_grads(), Recorder(2, 1)
    p = next(q for q in m.parameters() if q.dim() == 2 and q.shape[0] > 1 and q.shape[1] > 1)
    p.grad = torch.ones(p.shape[1], p.shape[0]).t()
    with pytest.raises(RuntimeError, match="not contiguous"):
        DataParallelStep(m, None, None, group=coll).reduce_gradients()
    assert not copies and not coll.reduced


def test_unequal_shards_raise_value_error_naming_both_counts():
    passes, finishes = [], []

    def other_rank(count):
        def peer(t):
            add = torch.zeros_like(t)
            if t.numel() > 2:   # the first exchange: rank 1's slot
                add[2 + 2 * 1], add[3 + 2 * 1] = float(count >> 20), float(count & 0xFFFFF)
            return add
        return peer

    run_pass = lambda k, sums: passes.append(k)
    run_finish = lambda k, sums, count: finishes.append((k, count))
    n = 3 * (1 << 20) + 17   # needs both parts of the count
    total = parallel.synced_batch_stats(Recorder(2, 0, other_rank(n)), n, "cpu", run_pass, run_finish)
    assert total == 2 * n and passes == [0, 1] and finishes == [(0, 2 * n), (1, 2 * n)]
    coll = Recorder(2, 0, other_rank(384))
    with pytest.raises(ValueError, match=r"rank 1 holds 384 .* rank 0 holds 512"):
        parallel.synced_batch_stats(coll, 512, "cpu", run_pass, run_finish)
    assert len(coll.reduced) == 1   # it travelled with the first statistics exchange
