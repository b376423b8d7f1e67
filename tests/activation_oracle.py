"""The CPU oracle with an activation other than ELU(alpha=1).

oracle/swin_fusion_oracle.py hard-codes `F.elu` in its three activation sites (the MLP, the patch layers, the head) and is not edited.
`shimmed(act)` runs the oracle's own functions with the module-level name `F` of that module replaced, for the length of a `with`, by a
small namespace whose `elu` is the chosen torch activation and which forwards every other attribute to torch.nn.functional.  torch
itself is not patched: nn.ELU and F.elu keep working everywhere else.  The namespace also records min |u| over every pre-activation it
was called with (the kink condition of tests/test_activation_host.py) and keeps the pre-activations themselves when asked to.
"""
from __future__ import annotations

import contextlib
from typing import List

import torch
import torch.nn.functional as TF

from oracle import swin_fusion_oracle as O


class ActivationNamespace:
    """Stands in for `torch.nn.functional` inside the oracle: `elu` is the activation under test."""

    def __init__(self, act: torch.nn.Module, keep: bool = False):
        self._act, self._keep = act, keep
        self.min_abs_u = float("inf")
        self.pre_activations: List[torch.Tensor] = []

    def elu(self, u: torch.Tensor) -> torch.Tensor:
        if u.numel():
            self.min_abs_u = min(self.min_abs_u, float(u.detach().abs().min()))
        if self._keep:
            self.pre_activations.append(u.detach().clone())
        return self._act(u)

    def __getattr__(self, name):
        return getattr(TF, name)


@contextlib.contextmanager
def shimmed(act: torch.nn.Module, keep: bool = False):
    """with shimmed(nn.GELU()) as ns: O.basic_block(...) runs with GELU where the oracle says ELU; ns.min_abs_u afterwards."""
    ns, saved = ActivationNamespace(act, keep), O.F
    O.F = ns
    try:
        yield ns
    finally:
        O.F = saved
