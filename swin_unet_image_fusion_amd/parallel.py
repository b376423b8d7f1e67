"""Data-parallel training: one model replica per GPU, ONE gradient all-reduce per step, and a head BatchNorm whose batch spans the
ranks ("Data-parallel step").

A step on W ranks with B / W pairs each computes the gradient of the same function as a one-rank step on all B pairs; the only
difference is the order in which fp32 partial sums are added.  The head's BatchNorm2d is the one place where the batch couples samples:
its statistics and the two means of its backward are per-channel sums, which are added over the ranks (all-reduce SUM) and divided by
the element count of the whole batch.  Every other gradient is a sum over samples of a loss that is a MEAN over the local batch, so with
equal shards the average of the ranks' gradients is the gradient of the global mean: `reduce_gradients()` gathers all gradients into one
flat buffer scaled by 1 / W (swf_tensors_gather, one launch), all-reduces that buffer once, and points every `p.grad` at its segment.

The collective is an object with `world_size`, `rank`, `all_reduce_(tensor)` (sum, in place) and `broadcast_(tensor, src)`;
`TorchCollective` wraps a torch.distributed group (RCCL in production; gloo, staged through the host, where two ranks share one
device in tests: a rehearsal of the control flow, not of RCCL).  Anything with those four members is accepted.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Callable, List, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .modules import _stream
from .optim import _Table, _Work
from .training import train_step

__all__ = ["TorchCollective", "DataParallelStep", "synced_batch_stats"]

_COUNT_BITS = 20   # an element count travels as two fp32 values (high part, low 20 bits): exact up to 2^44 elements


class TorchCollective:
    """The collective interface over a torch.distributed process group (None: the default group)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        if not dist.is_available() or not dist.is_initialized():
            raise RuntimeError("TorchCollective: torch.distributed has no initialised process group")
        self._dist, self.group = dist, group
        self.world_size, self.rank = dist.get_world_size(group), dist.get_rank(group)
        self._staged = dist.get_backend(group) == "gloo"   # gloo: device tensors go through the host

    def all_reduce_(self, tensor: Tensor) -> Tensor:
        if self._staged and tensor.is_cuda:
            host = tensor.cpu()
            self._dist.all_reduce(host, op=self._dist.ReduceOp.SUM, group=self.group)
            tensor.copy_(host)
        else:
            self._dist.all_reduce(tensor, op=self._dist.ReduceOp.SUM, group=self.group)
        return tensor

    def broadcast_(self, tensor: Tensor, src: int = 0) -> Tensor:
        root = self._dist.get_global_rank(self.group, src) if self.group is not None else src
        if self._staged and tensor.is_cuda:
            host = tensor.cpu()
            self._dist.broadcast(host, src=root, group=self.group)
            tensor.copy_(host)
        else:
            self._dist.broadcast(tensor, src=root, group=self.group)
        return tensor


def _as_collective(group):
    if all(hasattr(group, name) for name in ("world_size", "rank", "all_reduce_", "broadcast_")):
        return group
    return TorchCollective(group)


def synced_batch_stats(collective, n_local: int, device, run_pass: Callable, run_finish: Callable) -> int:
    """The two-pass batch statistics of the head over a batch that spans the ranks: pass 0, all-reduce, finish (mean), pass 1,
    all-reduce, finish (variance, running statistics).  `run_pass(k, sums)` leaves this rank's two per-channel sums of pass k in `sums`
    (2 floats on `device`), `run_finish(k, sums, count)` finishes pass k from the summed sums and the element count of the whole batch.
    Every rank's own count travels with the first exchange (slot 2 + 2 rank, in two exact fp32 parts); shards of different size raise
    ValueError, because the average of the ranks' gradients is the gradient of the global mean only for equal shards.
    -> the element count per channel of the whole batch."""
    world, rank = collective.world_size, collective.rank
    first = torch.zeros(2 + 2 * world, dtype=torch.float32, device=device)
    run_pass(0, first[:2])
    mine = torch.zeros(2 * world, dtype=torch.float32)
    mine[2 * rank], mine[2 * rank + 1] = float(n_local >> _COUNT_BITS), float(n_local & ((1 << _COUNT_BITS) - 1))
    first[2:].copy_(mine)
    collective.all_reduce_(first)
    parts = first[2:].cpu().tolist()
    counts = [(int(parts[2 * r]) << _COUNT_BITS) + int(parts[2 * r + 1]) for r in range(world)]
    for r, c in enumerate(counts):
        if c != n_local:
            raise ValueError(f"data-parallel step: shards must be equal in size, but rank {r} holds {c} elements per channel of the head's "
                             f"batch and rank {rank} holds {n_local}")
    total = sum(counts)
    run_finish(0, first[:2], total)
    second = torch.zeros(2, dtype=torch.float32, device=device)
    run_pass(1, second)
    collective.all_reduce_(second)
    run_finish(1, second, total)
    return total


class _FlatTable:
    """The optimiser's table (optim._Table: two pinned host copies, the device image) describing `tensors` as consecutive unpadded
    segments of one flat fp32 buffer, allocated once."""

    def __init__(self, tensors: List[Tensor], device):
        self.numels = [t.numel() for t in tensors]
        self.offsets, total = [], 0
        for n in self.numels:
            self.offsets.append(total)
            total += n
        self.total, self.n = total, len(tensors)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.table: Optional[_Table] = None   # pinned host copies and the device image: with the first launch

    def segments(self) -> List[int]:
        base = self.flat.data_ptr()
        return [base + 4 * off for off in self.offsets]

    def run(self, gather: bool, pointers: List[Optional[int]], scale: float, device) -> None:
        """gather: flat <- scale * tensors (a None pointer: a zero segment); scatter: tensors <- flat.  One upload, one launch."""
        segs = self.segments()
        if self.table is None:
            self.table = _Table(self.n, self.total, device)
        if gather:
            dst, src = segs, [p if p is not None else s for p, s in zip(pointers, segs)]   # the fill refuses NULL: set after it
        else:
            dst, src = pointers, segs
        work = _Work(None, [], [], (dst, src, dst, dst, self.numels))
        work.n = self.n
        ones = np.ones(self.n, dtype=np.float32)   # step_size / bc2_sqrt: not read by the copy
        args = self.table.fill(work, ones, ones)
        if gather and any(p is None for p in pointers):
            rows = (L.AdamTensor * self.n).from_address(args[0])
            for i, p in enumerate(pointers):
                if p is None:
                    rows[i].grad = None
        stream = torch.cuda.current_stream(device)
        if gather:
            L.check(L.lib().swf_tensors_gather(*args, self.flat.data_ptr(), self.total, scale, _stream(device)))
        else:
            L.check(L.lib().swf_tensors_scatter(*args, self.flat.data_ptr(), self.total, _stream(device)))
        self.table.sent(stream)


def _flat_ok(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"DataParallelStep: {what} of shape {tuple(t.shape)} lives on {t.device}; the gather runs on the GPU only")
    if t.layout != torch.strided or not t.is_contiguous():
        raise RuntimeError(f"DataParallelStep: {what} of shape {tuple(t.shape)} is not a contiguous dense tensor")


class DataParallelStep:
    """`training.train_step` on one rank of a data-parallel group: forward, clamp, loss, zero_grad, backward, ONE gradient all-reduce,
    optimiser step.

    `group`: a collective object (see the module text), a torch.distributed group, or None.  With `group=None` or a world size of 1,
    and without `force_collective`, nothing here touches a collective: `reduce_gradients()` does nothing and `step` IS `train_step`,
    bit for bit.  `force_collective=True` at world size 1 runs the gather and a one-rank all-reduce, the rehearsal of the RCCL path on
    a box with one GPU (as ShardedFusion's); with `group=None` it takes torch.distributed's default group.

    `sync_head_bn`: while a step (or a `head_sync()` block) runs, the head's BatchNorm takes its batch statistics, and the means of its
    backward, over the batches of ALL ranks; with False every rank normalises with its own batch, which is a different optimisation
    problem from the one-rank run at the same global batch.

    Shards must be equal in size (the loss is a mean over the local batch); the head's first exchange carries every rank's element
    count and a difference raises ValueError.

    After `reduce_gradients()` every `p.grad` is a VIEW of one flat buffer that this object owns and reuses: the views are valid until
    the next `reduce_gradients()`.  `FusedAdam` reads them in place (its gradient-norm clipping therefore clips the reduced gradient);
    clone a gradient that has to outlive the step.
    """

    def __init__(self, model, loss_fn, optimizer, group=None, sync_head_bn: bool = True, force_collective: bool = False):
        self.model, self.loss_fn, self.optimizer = model, loss_fn, optimizer
        self.sync_head_bn, self.force_collective = bool(sync_head_bn), bool(force_collective)
        if group is None and force_collective:
            group = TorchCollective(None)
        self.collective = None if group is None else _as_collective(group)
        self.world_size = 1 if self.collective is None else int(self.collective.world_size)
        self.rank = 0 if self.collective is None else int(self.collective.rank)
        self.active = self.collective is not None and (self.world_size > 1 or self.force_collective)
        self._grads: Optional[_FlatTable] = None
        self._state: Optional[_FlatTable] = None

    # ---- state ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def broadcast_state(self, src: int = 0) -> None:
        """Every rank takes rank `src`'s model state: all fp32 parameters and buffers of the state dict through one gather, one
        broadcast and one scatter; the others (num_batches_tracked) are broadcast on their own.  The version counters of what was
        written are bumped, so the model's weight arena and graph_key() follow."""
        if not self.active:
            return
        state = list(self.model.state_dict(keep_vars=True).values())
        dense = [t for t in state if t.dtype == torch.float32 and t.numel() > 0]
        for t in dense:
            _flat_ok(t, "a parameter or buffer")
        if dense:
            device = dense[0].device
            if self._state is None or self._state.numels != [t.numel() for t in dense] or self._state.flat.device != device:
                self._state = _FlatTable(dense, device)
            ptrs = [t.data_ptr() for t in dense]
            self._state.run(True, ptrs, 1.0, device)
            self.collective.broadcast_(self._state.flat, src)
            self._state.run(False, ptrs, 1.0, device)
        rest = [t for t in state if t.dtype != torch.float32 and t.numel() > 0]
        for t in rest:
            self.collective.broadcast_(t.data, src)
        torch.autograd.graph.increment_version(dense + rest)
        if hasattr(self.model, "refresh_weights"):   # buffers are outside the model's weight fingerprint
            self.model.refresh_weights()

    # ---- gradients --------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reduce_gradients(self) -> None:
        """p.grad <- the mean over the ranks of p.grad, for every parameter, through ONE all-reduce: a gather of all gradients in
        model.parameters() order (the reference's order) scaled by 1 / world_size, the all-reduce, then `p.grad` becomes a view of its
        segment (no unpack pass).  A gradient that is None on this rank contributes zeros and receives the reduced segment."""
        if not self.active:
            return
        params = [p for p in self.model.parameters() if p.numel() > 0]
        ptrs: List[Optional[int]] = []
        for p in params:   # everything is validated before the first call
            g = p.grad
            if g is None:
                ptrs.append(None)
                continue
            if g.layout != torch.strided:
                raise RuntimeError("FusedAdam does not support sparse gradients")
            if not g.is_contiguous():
                raise RuntimeError(f"FusedAdam.step(): the gradient of a parameter of shape {tuple(p.shape)} is not contiguous")
            if g.dtype != torch.float32:
                raise RuntimeError(f"DataParallelStep: the gradient of a parameter of shape {tuple(p.shape)} is {g.dtype}; the kernels are fp32 only")
            ptrs.append(g.data_ptr())
        if not params:
            return
        device = params[0].device
        if self._grads is None or self._grads.numels != [p.numel() for p in params] or self._grads.flat.device != device:
            self._grads = _FlatTable(params, device)
        t = self._grads
        t.run(True, ptrs, 1.0 / self.world_size, device)
        self.collective.all_reduce_(t.flat)
        for p, off, n in zip(params, t.offsets, t.numels):
            p.grad = t.flat[off:off + n].view_as(p)

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @contextmanager
    def head_sync(self):
        """Inside the block the model's head normalises over the batches of all ranks (when `sync_head_bn` and the group has more
        than one rank).  `step` runs in one; open it around a hand-written forward and backward."""
        on = self.active and self.sync_head_bn and self.world_size > 1
        before = getattr(self.model, "_head_collective", None)
        if on:
            self.model._head_collective = self.collective
        try:
            yield
        finally:
            if on:
                self.model._head_collective = before

    def step(self, ir_shard: Tensor, vis_shard: Tensor):
        """`training.train_step`'s order on this rank's shard with `reduce_gradients()` between backward() and optimizer.step().
        -> (loss, detail) of THIS rank's shard."""
        if not self.active:
            return train_step(self.model, self.loss_fn, self.optimizer, ir_shard, vis_shard)
        with self.head_sync():
            fusion = self.model(ir_shard, vis_shard)
            fusion = torch.clamp_(fusion, min=0, max=1)
            loss, detail = self.loss_fn.calcu_total_loss(fusion_images=fusion, ir_images=ir_shard, vis_images=vis_shard)
            self.optimizer.zero_grad()
            loss.backward()
        self.reduce_gradients()
        self.optimizer.step()
        return loss, detail
