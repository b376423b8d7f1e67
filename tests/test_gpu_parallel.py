"""Data-parallel training on one GPU, one process: the gather / scatter kernel bit for bit against torch, the head's BatchNorm over a
batch handed over in two halves (statistics and backward) against float64 torch on the whole batch, and DataParallelStep without a
group and with a one-rank collective against training.train_step, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import __graft_entry__ as entry
from oracle import swin_fusion_oracle as O
from swin_unet_image_fusion_amd import (CONFIGS, DataParallelStep, FusedAdam, MyLoss, MyModel, _lib as L, load_recipe_into, synthetic_pair,
                                        train_step)
from swin_unet_image_fusion_amd.modules import _stream
from tests import golden_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUMELS = [1, 3, 225, 4096, 4097, 3 * 4096 + 5]   # later segments start misaligned; the last tensor spans four chunks


@pytest.fixture(scope="module", autouse=True)
def _built():
    entry.build()
    yield


class _Tables:
    """A gather and a scatter table over the same tensors, in pinned host memory, with one device image each."""

    def __init__(self, sources, outputs, flat):
        lib, n = L.lib(), len(sources)
        self.n, self.flat = n, flat
        numel = np.array([t.numel() for t in outputs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(numel)[:-1]])
        seg = np.array([flat.data_ptr() + 4 * int(o) for o in offs], dtype=np.uint64)
        self.nbytes = lib.swf_adam_table_bytes(n, int(numel.sum()))
        ones = np.ones(n, dtype=np.float32)
        self.host, self.dev = [], []
        for gather in (True, False):
            tens = sources if gather else outputs
            other = np.array([seg[i] if t is None else t.data_ptr() for i, t in enumerate(tens)], dtype=np.uint64)
            dst, src = (seg, other) if gather else (other, seg)
            host = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
            L.check(lib.swf_adam_table_fill(host.data_ptr(), self.nbytes, n, dst.ctypes.data, src.ctypes.data, dst.ctypes.data, dst.ctypes.data,
                                            numel.ctypes.data, ones.ctypes.data, ones.ctypes.data))
            if gather:
                rows = (L.AdamTensor * n).from_address(host.data_ptr())
                for i, t in enumerate(tens):
                    if t is None:
                        rows[i].grad = None   # a NULL source: a zero segment
            self.host.append(host)
            self.dev.append(torch.empty(self.nbytes, dtype=torch.uint8, device=DEV))

    def gather(self, scale):
        L.check(L.lib().swf_tensors_gather(self.host[0].data_ptr(), self.dev[0].data_ptr(), self.nbytes, self.n, self.flat.data_ptr(),
                                           self.flat.numel(), scale, _stream(DEV)))

    def scatter(self):
        L.check(L.lib().swf_tensors_scatter(self.host[1].data_ptr(), self.dev[1].data_ptr(), self.nbytes, self.n, self.flat.data_ptr(),
                                            self.flat.numel(), _stream(DEV)))


def test_gather_and_scatter_are_torch_cat_bit_for_bit():
    tensors = [G.randn((n,), 1000 + i).to(DEV) for i, n in enumerate(NUMELS)]
    total = sum(NUMELS)
    guard = torch.full((total + 64,), 7.0, device=DEV)
    flat = guard[32:32 + total]
    outs_guard = [torch.full((n + 16,), 9.0, device=DEV) for n in NUMELS]
    # segment offsets 0, 1, 4, 229, 4325, 8422: phases 0, 1, 0, 1, 1, 2 (elements past a 16-byte boundary).  The tensors start at
    # phase 0 except the last two: one in its segment's phase (scalar head, then 16-byte loads AND stores), one in another
    starts = [8, 8, 8, 8, 9, 11]
    outs = [g[s:s + n] for g, s, n in zip(outs_guard, starts, NUMELS)]
    for null in (None, 2, 5):
        sources = [None if i == null else t for i, t in enumerate(tensors)]
        tab = _Tables(sources, outs, flat)
        for scale in (1.0, 0.5, 1.0 / 3.0):                          # the later calls reuse the table
            want = torch.cat([torch.zeros_like(t) if i == null else t * scale for i, t in enumerate(tensors)])
            flat.fill_(5.0)
            tab.gather(scale)
            assert torch.equal(flat, want), (null, scale)
            for o in outs:
                o.fill_(3.0)
            tab.scatter()
            off = 0
            for o, n in zip(outs, NUMELS):
                assert torch.equal(o, want[off:off + n]), (null, scale, n)
                off += n
    torch.cuda.synchronize()
    assert bool((guard[:32] == 7.0).all()) and bool((guard[32 + total:] == 7.0).all())
    for g, s, n in zip(outs_guard, starts, NUMELS):
        assert bool((g[:s] == 9.0).all()) and bool((g[s + n:] == 9.0).all())

    # one replay in a captured graph on a side stream: the upload and the launch are all there is
    tab = _Tables(tensors, outs, flat)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tab.gather(0.5)
        tab.scatter()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        tab.gather(0.5)
        tab.scatter()
    for t in tensors:
        t.mul_(-1.5)
    flat.fill_(5.0)
    for o in outs:
        o.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    want = torch.cat([t * 0.5 for t in tensors])
    assert torch.equal(flat, want) and torch.equal(torch.cat(outs), want)


# ---- the head over two halves -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def head():
    """The tiny model's head, a batch of four whose halves have different means, and float64 torch on the whole batch."""
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=3, flavor="stress")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("final_layer")}
    x, y = (torch.from_numpy(a) for a in synthetic_pair(4, 11, 9, seed_ir=911, seed_vis=912))   # U[0, 1)
    x[2:] *= 0.5
    y[2:] *= 0.5
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    conv1 = lambda a, b: F.conv2d(F.pad(torch.cat([a, b], 1), (1, 1, 1, 1), mode="reflect"), sd64["final_layer.0.weight"], sd64["final_layer.0.bias"])
    z = conv1(x.double(), y.double())
    halves = [conv1(x[:2].double(), y[:2].double()).mean((0, 2, 3)), conv1(x[2:].double(), y[2:].double()).mean((0, 2, 3))]
    assert float((halves[0] - halves[1]).abs().max()) > 1e-2, halves          # the halves' batch means differ
    m.to(DEV).train()
    return dict(model=m, sd64=sd64, x=x, y=y, z=z, halves=halves)


def _head_call_args(m, x, y):
    b, _, h, w = x.shape
    lib = L.lib()
    need = lib.swf_final_head_bwd_workspace_bytes(b, h, w, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    return b, h, w, ws, need


def _global_stats(m, x, y, running):
    """Both passes over the two halves, the sums added on the device, finished with the global count -> stats (mean[2], var[2])."""
    lib, hp, st = L.lib(), m._head_params(), _stream(DEV)
    stats = torch.zeros(4, device=DEV)
    halves = [(x[:2].contiguous().to(DEV), y[:2].contiguous().to(DEV)), (x[2:].contiguous().to(DEV), y[2:].contiguous().to(DEV))]
    count = 4 * 11 * 9
    for k in (0, 1):
        parts = []
        for hx, hy in halves:
            b, h, w, ws, need = _head_call_args(m, hx, hy)
            s = torch.zeros(2, device=DEV)
            L.check(lib.swf_final_head_stats_pass(C.byref(hp), hx.data_ptr(), hy.data_ptr(), k, stats.data_ptr(), s.data_ptr(), b, h, w, 3,
                                                  ws.data_ptr(), need, st))
            parts.append(s)
        total = parts[0] + parts[1]
        L.check(lib.swf_final_head_stats_finish(total.data_ptr(), 8, count, k, stats.data_ptr(), stats.data_ptr() + 8,
                                                running[0].data_ptr() if k else None, running[1].data_ptr() if k else None, 0.1, st))
    return stats, halves, count


def test_head_statistics_over_two_halves_match_torch_on_the_whole_batch(head):
    m, z = head["model"], head["z"]
    mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    rm, rv = head["sd64"]["final_layer.1.running_mean"].clone(), head["sd64"]["final_layer.1.running_var"].clone()
    F.batch_norm(z, rm, rv, None, None, training=True, momentum=0.1)
    bn = m.final_layer[1]
    running = [bn.running_mean.detach().clone(), bn.running_var.detach().clone()]
    stats, halves, _ = _global_stats(m, head["x"], head["y"], running)
    close = lambda got, ref: torch.allclose(got.cpu().double(), ref, rtol=1e-5, atol=1e-6)
    assert close(stats[:2], mean) and close(stats[2:], var), (stats, mean, var)
    assert close(running[0], rm) and close(running[1], rv), (running, rm, rv)
    # either half alone misses it
    lib, hp = L.lib(), m._head_params()
    for hx, hy in halves:
        b, h, w, ws, need = _head_call_args(m, hx, hy)
        alone = torch.zeros(4, device=DEV)
        L.check(lib.swf_final_head_batch_stats(C.byref(hp), hx.data_ptr(), hy.data_ptr(), alone.data_ptr(), alone.data_ptr() + 8, None, None, 0.1,
                                               b, h, w, 3, ws.data_ptr(), need, _stream(DEV)))
        assert not close(alone[:2], mean)


def test_head_backward_over_two_halves_matches_autograd_on_the_whole_batch(head):
    m, x, y = head["model"], head["x"], head["y"]
    sd = {k: (v.clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in head["sd64"].items()}
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    wgt = G.randn((4, 1, 11, 9), 913)
    out = O.final_head(sd, x64, y64, 3, training=True)
    (out * wgt.double()).sum().backward()

    bn = m.final_layer[1]
    running = [bn.running_mean.detach().clone(), bn.running_var.detach().clone()]
    stats, halves, count = _global_stats(m, x, y, running)
    lib, hp, st = L.lib(), m._head_params(), _stream(DEV)
    hp.bn_mean, hp.bn_var = stats.data_ptr(), stats.data_ptr() + 8
    gouts = [wgt[:2].contiguous().to(DEV), wgt[2:].contiguous().to(DEV)]
    sums = []
    for (hx, hy), go in zip(halves, gouts):
        b, h, w, ws, need = _head_call_args(m, hx, hy)
        s = torch.zeros(4, device=DEV)
        L.check(lib.swf_final_head_bwd_sums(C.byref(hp), hx.data_ptr(), hy.data_ptr(), go.data_ptr(), s.data_ptr(), b, h, w, 3, ws.data_ptr(), need, st))
        sums.append(s)
    total = sums[0] + sums[1]
    names = ("final_layer.0.weight", "final_layer.0.bias", "final_layer.1.weight", "final_layer.1.bias", "final_layer.3.weight",
             "final_layer.3.bias")
    gxs, gys, pgrads = [], [], []
    for (hx, hy), go in zip(halves, gouts):
        b, h, w, ws, need = _head_call_args(m, hx, hy)
        ws.fill_(0xA5)                                   # nothing survives in the workspace from the first phase
        gx, gy = torch.empty_like(hx), torch.empty_like(hy)
        bufs = [torch.empty(tuple(sd[k].shape), device=DEV) for k in names]
        grads = L.HeadGrads(*[t.data_ptr() for t in bufs])
        L.check(lib.swf_final_head_bwd_synced(C.byref(hp), hx.data_ptr(), hy.data_ptr(), go.data_ptr(), total.data_ptr(), count, gx.data_ptr(),
                                              gy.data_ptr(), C.byref(grads), b, h, w, 3, ws.data_ptr(), need, st))
        gxs.append(gx); gys.append(gy); pgrads.append(bufs)
    gmax = max(float(sd[k].grad.abs().max()) for k in names)

    def err(got, ref):
        got, ref = got.detach().cpu().double(), ref.detach().double()
        return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * gmax)

    worst = {"gx": err(torch.cat(gxs), x64.grad), "gy": err(torch.cat(gys), y64.grad)}
    for i, k in enumerate(names):
        worst[k] = err(pgrads[0][i] + pgrads[1][i], sd[k].grad)
    print("head backward over two halves, worst relative errors:", worst)
    assert max(worst.values()) <= 5e-3, worst


@pytest.mark.parametrize("clip,wd", [(None, 0.0), (1.0, 1e-2)])
def test_adam_step_does_not_depend_on_the_alignment_of_a_gradient(clip, wd):
    """After reduce_gradients() every p.grad is a view at some 4-byte address of the flat buffer: FusedAdam must give the bits it gives
    for a 16-byte-aligned gradient (sizes: below one group of four, with a tail, one chunk, several chunks with a tail)."""
    gen = torch.Generator().manual_seed(0)
    for n in (3, 225, 4096, 10000):
        p0 = torch.randn(n, generator=gen)
        grads = [torch.randn(n, generator=gen) * 10 for _ in range(2)]
        results = []
        for offset in (0, 1, 2, 3):
            p = p0.to(DEV).requires_grad_()
            opt = FusedAdam([p], lr=1e-3, max_grad_norm=clip, weight_decay=wd)
            for g in grads:
                buf = torch.zeros(n + 4, device=DEV)
                buf[offset:offset + n].copy_(g)
                p.grad = buf[offset:offset + n]
                opt.step()
            results.append([p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()])
        for offset, res in enumerate(results):
            assert all(torch.equal(a, b) for a, b in zip(res, results[0])), (n, offset)


# ---- DataParallelStep against train_step --------------------------------------------------------------------------------------------
class OneRank:
    """An in-process collective of one rank: the sum over one rank is the tensor itself."""
    world_size, rank = 1, 0

    def __init__(self):
        self.reduced = 0

    def all_reduce_(self, t):
        self.reduced += 1
        return t

    def broadcast_(self, t, src=0):
        return t


def _two_steps(make_step):
    m = MyModel(**CONFIGS["tiny"].model_kwargs(nn.ELU(inplace=True)))
    load_recipe_into(m, seed=5, flavor="stress")
    m.to(DEV).train()
    opt = FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    step = make_step(m, MyLoss(), opt)
    losses = []
    for i in range(2):
        ir, vis = (torch.from_numpy(a).to(DEV) for a in synthetic_pair(2, 16, 16, seed_ir=31 + i, seed_vis=41 + i))
        loss, _ = step(ir, vis)
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    state = [p.detach().clone() for p in m.parameters()]
    state += [opt.state[p][k].clone() for p in m.parameters() for k in ("exp_avg", "exp_avg_sq")]
    state += [b.detach().clone() for b in m.buffers()]
    return state, losses, opt.last_grad_norm.clone()


@pytest.fixture(scope="module")
def plain_steps():
    return _two_steps(lambda m, loss, opt: (lambda ir, vis: train_step(m, loss, opt, ir, vis)))


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(s, t) for s, t in zip(a[0], b[0])) and \
        all(torch.equal(s, t) for s, t in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def test_step_without_a_group_is_train_step_bit_for_bit(plain_steps):
    got = _two_steps(lambda m, loss, opt: DataParallelStep(m, loss, opt, group=None).step)
    assert _same(got, plain_steps)


def test_step_with_a_forced_one_rank_collective_is_train_step_bit_for_bit(plain_steps):
    coll = OneRank()
    holder = {}

    def make(m, loss, opt):
        holder["dp"] = DataParallelStep(m, loss, opt, group=coll, force_collective=True)
        return holder["dp"].step
    got = _two_steps(make)
    assert coll.reduced == 2                                          # one all-reduce per step
    dp = holder["dp"]
    params = list(dp.model.parameters())
    assert all(p.grad.data_ptr() == dp._grads.flat.data_ptr() + 4 * off for p, off in zip(params, dp._grads.offsets))
    assert _same(got, plain_steps)
