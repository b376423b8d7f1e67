"""torch.optim.Adam's step on libswinfuse: one HIP launch per parameter group, whatever the number of tensors.

`FusedAdam` keeps exactly torch.optim.Adam's state (`step` as a CPU scalar tensor, `exp_avg`, `exp_avg_sq`) and the param_group keys
it writes, so each optimiser's `state_dict()` loads into the other and a checkpoint of the reference's training script (a016:243-249)
resumes here.  A step describes the tensors of a group in a table in pinned host memory (swf_adam_table_fill), which swf_adam_step
sends to the device with one asynchronous copy and updates with one kernel; with `max_grad_norm` two more launches compute the global
gradient norm first and the update reads the clip coefficient from device memory.  No synchronisation, no read-back.

Constructing the optimiser, `state_dict()`, `load_state_dict()` and `zero_grad()` need neither the library nor a GPU; `step()` does,
and raises on anything it would otherwise have to copy: there is no fallback to torch's own update.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .modules import _stream

__all__ = ["FusedAdam"]


def _step_dtype() -> torch.dtype:
    """The dtype torch.optim.Adam gives its `step` tensors."""
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


class _Table:
    """The table of one group: two pinned host copies used alternately, each guarded by the event recorded behind its upload, and the
    device image.  Filling step n + 1's table therefore never touches the copy step n's upload may still be reading."""

    def __init__(self, n_tensors: int, total_elems: int, device):
        self.capacity = (n_tensors, total_elems)
        self.nbytes = L.lib().swf_adam_table_bytes(n_tensors, total_elems)
        if not self.nbytes:
            raise ValueError(f"no table for {n_tensors} tensors of {total_elems} elements")
        self.host = [torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.dev = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        self.events: List[Optional[torch.cuda.Event]] = [None, None]
        self.flip = 0

    def holds(self, n_tensors: int, total_elems: int) -> bool:
        return n_tensors <= self.capacity[0] and total_elems <= self.capacity[1]

    def fill(self, w: "_Work", step_size: np.ndarray, bc2_sqrt: np.ndarray):
        """Write the rows and the chunk map into the free host copy -> the (host, device, bytes, n_tensors) arguments of an entry."""
        k, self.flip = self.flip, self.flip ^ 1
        if self.events[k] is not None:
            self.events[k].synchronize()   # the upload from two steps ago: long done, this does not wait on the device
        arrays = (w.param, w.grad, w.exp_avg, w.exp_avg_sq, w.numel, step_size, bc2_sqrt)
        L.check(L.lib().swf_adam_table_fill(self.host[k].data_ptr(), self.nbytes, w.n, *[a.ctypes.data for a in arrays]))
        self.current = k
        return self.host[k].data_ptr(), self.dev.data_ptr(), self.nbytes, w.n

    def sent(self, stream: torch.cuda.Stream) -> None:
        ev = self.events[self.current] or torch.cuda.Event()
        ev.record(stream)
        self.events[self.current] = ev


class _Work:
    """What one step updates in one group: device addresses and sizes as arrays, the step tensors, the parameters."""

    def __init__(self, group: Optional[dict], params: List[Tensor], steps: List[Tensor], columns):
        self.group, self.params, self.steps, self.n = group, params, steps, len(params)
        param, grad, exp_avg, exp_avg_sq, numel = columns
        self.param, self.grad = np.array(param, dtype=np.uint64), np.array(grad, dtype=np.uint64)
        self.exp_avg, self.exp_avg_sq = np.array(exp_avg, dtype=np.uint64), np.array(exp_avg_sq, dtype=np.uint64)
        self.numel = np.array(numel, dtype=np.int64)

    @staticmethod
    def union(works: List["_Work"]) -> "_Work":
        names = ("param", "grad", "exp_avg", "exp_avg_sq", "numel")
        return _Work(None, [p for w in works for p in w.params], [],
                     [np.concatenate([getattr(w, name) for w in works]) for name in names])


class FusedAdam(torch.optim.Optimizer):
    """Drop-in for `torch.optim.Adam(params, lr, betas, eps, weight_decay)` (the reference's optimiser, a016:67) whose step runs as HIP
    kernels of libswinfuse.  Per element, in torch's order:

        g' = clip * g (+ weight_decay * p);  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2
        p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

    with t the parameter's own step count (a parameter without a gradient is skipped and its count does not advance).  Per-group `lr`,
    `betas`, `eps` and `weight_decay` are read at every step, so torch's schedulers work unchanged.

    `max_grad_norm` (None = off) clips the global L2 norm of all gradients as `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`
    before `Adam.step()` would: clip = min(1, max_grad_norm / (norm + 1e-6)).  UNLIKE clip_grad_norm_, the factor is applied inside the
    update and `p.grad` IS NOT MODIFIED.  `last_grad_norm` is a 1-element device tensor with the norm of the last clipped step (None
    before one), for logging without a synchronisation.  It is a view of a buffer the optimiser owns on the parameters' device and is
    written in place by every clipped step; should the parameters move to another device the buffer is allocated anew there, and a
    view taken earlier no longer follows: read `optimizer.last_grad_norm` afresh instead of keeping it.

    step() raises rather than copies: for a parameter on the CPU, not fp32 or not contiguous, and for a gradient that is sparse or not
    contiguous (torch itself keeps a gradient in its parameter's dtype and on its device).  `amsgrad=True` and `maximize=True` raise ValueError.  The kernel writes the parameters
    through raw pointers; step() then bumps their version counters (torch.autograd.graph.increment_version), which MyModel's weight
    arena and graph_key() follow.  Steps are expected on one stream; a step on another stream first waits for the previous one.
    Every step compares the addresses of each parameter and of its two moments with the ones it validated; a tensor that moved or was
    replaced is validated again.  All groups are validated before the first launch; the step counts advance after a group's launch
    was accepted, so an error leaves them where they were (with several groups, a launch failure in a later group leaves the earlier
    groups stepped).
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, *, amsgrad=False,
                 maximize=False):
        if amsgrad:
            raise ValueError("FusedAdam: amsgrad=True is not provided")
        if maximize:
            raise ValueError("FusedAdam: maximize=True is not provided")
        if isinstance(lr, Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (None switches clipping off)")
        # the keys torch.optim.Adam writes, so that either optimiser's state_dict loads into the other
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Optional[Tensor] = None
        self._norm: Optional[Tensor] = None      # device float[2]: norm, clip coefficient
        self._recs = {}                          # parameter -> (its address, its state dict, the addresses of exp_avg and exp_avg_sq, numel)
        self._tables = {}                        # group index (or "all") -> _Table
        self._last_stream = None

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._tables = {}

    def load_state_dict(self, state_dict) -> None:
        """torch's load (moments cast to each parameter's device and dtype), then `step` back to the CPU scalar tensor the
        non-capturable torch.optim.Adam keeps, whatever the saving optimiser kept (fused=True keeps it on the device)."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("FusedAdam: the loaded param_groups ask for amsgrad / maximize, which are not provided")
            if group.get("decoupled_weight_decay"):
                raise ValueError("FusedAdam: the loaded param_groups ask for decoupled weight decay (AdamW), which is not provided")
        for st in self.state.values():
            if "step" in st:
                s = st["step"]
                st["step"] = (s.detach().to(device="cpu", dtype=_step_dtype()).reshape(()).clone() if isinstance(s, Tensor)
                              else torch.tensor(float(s), dtype=_step_dtype()))
        self._recs = {}

    def _record(self, p: Tensor):
        """Validate a parameter and its state once (again when its storage moved); create the state as torch does, at step 0."""
        if not p.is_cuda:
            raise RuntimeError(f"FusedAdam.step(): parameter of shape {tuple(p.shape)} lives on {p.device}; the step runs on the GPU only "
                               "(there is no CPU path): move the model to the GPU before the first step")
        if p.dtype != torch.float32:
            raise RuntimeError(f"FusedAdam.step(): parameter of shape {tuple(p.shape)} is {p.dtype}; the kernels are fp32 only")
        if p.layout != torch.strided or not p.is_contiguous():
            raise RuntimeError(f"FusedAdam.step(): parameter of shape {tuple(p.shape)} is not a contiguous dense tensor")
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=_step_dtype())
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for key in ("exp_avg", "exp_avg_sq"):
            t = st[key]
            if t.device != p.device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                raise RuntimeError(f"FusedAdam.step(): state '{key}' of a parameter of shape {tuple(p.shape)} must be a contiguous fp32 "
                                   f"tensor of that shape on {p.device} (got {tuple(t.shape)}, {t.dtype}, {t.device})")
        if st["step"].is_cuda:
            raise RuntimeError("FusedAdam.step(): state 'step' must be a CPU tensor (load the state through load_state_dict)")
        rec = (p.data_ptr(), st, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
        self._recs[p] = rec
        return rec

    def _gather(self, group: dict) -> Optional[_Work]:
        """The parameters of `group` that have a gradient, validated; nothing is launched or advanced here.  torch itself keeps a
        gradient on its parameter's device and in its dtype (assigning another raises), so layout and strides are what is left to check.
        A parameter or a moment whose address is not the validated one (moved, or `optimizer.state[p]` replaced) is validated again."""
        params, steps, ps, gs, ms, vs, ns = [], [], [], [], [], [], []
        get, state = self._recs.get, self.state
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if g.layout != torch.strided:
                raise RuntimeError("FusedAdam does not support sparse gradients")
            if not g.is_contiguous():
                raise RuntimeError(f"FusedAdam.step(): the gradient of a parameter of shape {tuple(p.shape)} is not contiguous")
            rec = get(p)
            if rec is not None:
                st = rec[1]
                if (rec[0] != p.data_ptr() or state.get(p) is not st or len(st) != 3 or st["exp_avg"].data_ptr() != rec[2]
                        or st["exp_avg_sq"].data_ptr() != rec[3] or st["step"].is_cuda):
                    rec = None
            if rec is None:
                rec = self._record(p)
            if rec[4] == 0:
                continue
            params.append(p)
            steps.append(rec[1]["step"])
            ps.append(rec[0]); gs.append(g.data_ptr()); ms.append(rec[2]); vs.append(rec[3]); ns.append(rec[4])
        return _Work(group, params, steps, (ps, gs, ms, vs, ns)) if params else None

    def _table(self, key, w: _Work, groups: List[dict], device) -> _Table:
        """The table behind `key`, sized once for every parameter of `groups` (a later step may carry more gradients than this one)."""
        t = self._tables.get(key)
        if t is None or t.dev.device != device or not t.holds(w.n, int(w.numel.sum())):
            params = [p for g in groups for p in g["params"] if p.numel() > 0]   # empty parameters never get a row
            t = self._tables[key] = _Table(len(params), sum(p.numel() for p in params), device)
        return t

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        works = [(gi, self._gather(group)) for gi, group in enumerate(self.param_groups)]
        works = [(gi, w) for gi, w in works if w is not None]
        if not works:
            return loss
        device = works[0][1].params[0].device
        if any(w.params[0].device != device for _, w in works):
            raise RuntimeError("FusedAdam.step(): all parameters must live on one GPU")
        lib, raw_stream, stream = L.lib(), _stream(device), torch.cuda.current_stream(device)
        if self._last_stream is not None and self._last_stream[0] != raw_stream:
            stream.wait_event(self._last_stream[1])   # the previous step's kernels still read the device tables
        clip = self.max_grad_norm is not None
        norm_ptr, norm_ready = None, 0
        if clip:
            if self._norm is None or self._norm.device != device:
                self._norm = torch.zeros(2, dtype=torch.float32, device=device)
                self.last_grad_norm = self._norm[:1]
            norm_ptr = self._norm.data_ptr()
            if len(works) > 1:   # the norm spans every group: one pass over the union of their tensors, then the groups read it
                u = _Work.union([w for _, w in works])
                table = self._table("all", u, self.param_groups, device)
                zeros = np.zeros(u.n, dtype=np.float32)
                L.check(lib.swf_adam_grad_norm(float(self.max_grad_norm), *table.fill(u, zeros, zeros), norm_ptr, raw_stream))
                table.sent(stream)
                norm_ready = 1
        for gi, w in works:
            group = w.group
            beta1, beta2 = group["betas"]
            t = torch.stack(w.steps).to(torch.float64).numpy() + 1.0   # the counts this step will have; committed below
            step_size = (float(group["lr"]) / (1.0 - beta1 ** t)).astype(np.float32)
            bc2_sqrt = np.sqrt(1.0 - beta2 ** t).astype(np.float32)
            desc = L.AdamDesc(beta1, beta2, group["eps"], group["weight_decay"], float(self.max_grad_norm) if clip else 0.0, norm_ready)
            table = self._table(gi, w, [group], device)
            L.check(lib.swf_adam_step(C.byref(desc), *table.fill(w, step_size, bc2_sqrt), norm_ptr, raw_stream))
            table.sent(stream)
            torch._foreach_add_(w.steps, 1.0)
            torch.autograd.graph.increment_version(w.params)
        ev = self._last_stream[1] if self._last_stream is not None else torch.cuda.Event()
        ev.record(stream)
        self._last_stream = (raw_stream, ev)
        return loss
