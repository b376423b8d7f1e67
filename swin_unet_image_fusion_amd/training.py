"""The reference's training loop body and its checkpoint format (a016_train.py), host side only: every line is the reference's own
torch call on this package's model, loss and optimiser; there is no arithmetic here beyond what that loop does.
"""
from __future__ import annotations

import torch
from torch import Tensor

__all__ = ["train_step", "validate", "fractional_epoch", "save_training_state", "load_training_state"]

STATE_KEYS = ("model_state", "optimizer_state", "scheduler_state", "current_epoch")   # a016:243-248


def train_step(model, loss_fn, optimizer, ir: Tensor, vis: Tensor):
    """One iteration of a016:150-165, in its order: forward, clamp_(0, 1), calcu_total_loss, zero_grad, backward, step.
    -> (loss, the loss's detail dict).  The caller steps the scheduler (a016:167, `scheduler.step(fractional_epoch(...))`).
    The model comes configured: its `backward_tier` and `backward_attention` are read by its own forward and nothing here touches
    them (a `win16` model at five stages needs backward_attention = "phased": its level-4 tile does not fit the default family)."""
    fusion = model(ir, vis)
    fusion = torch.clamp_(fusion, min=0, max=1)
    loss, detail = loss_fn.calcu_total_loss(fusion_images=fusion, ir_images=ir, vis_images=vis)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss, detail


def validate(model, loss_fn, loader, metrics=None):
    """The reference's vali() (a016:198-236) without the figure it saves: remember model.training, eval(), and under no_grad per batch
    forward, clamp_(0, 1), loss_fn.calcu_total_loss (which feeds the loss's own recorder, as the reference's val_loss_calculator is
    fed) and, when `metrics` (a FusionMetrics) is given, its update; then restore the mode.  `loader` yields the reference's batch
    dicts (`ir`, `vis` first: PairLoader) or (ir, vis) pairs, already on the model's device.  -> metrics.compute(), or None."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                ir, vis = list(batch.values())[:2] if isinstance(batch, dict) else batch[:2]
                fusion = model(ir, vis)
                fusion = torch.clamp_(fusion, min=0, max=1)
                loss_fn.calcu_total_loss(fusion_images=fusion, ir_images=ir, vis_images=vis)
                if metrics is not None:
                    metrics.update(fusion, ir, vis)
    finally:
        if was_training:
            model.train()
    return metrics.compute() if metrics is not None else None


def fractional_epoch(epoch: int, iter_in_epoch: int, iters_per_epoch: int) -> float:
    """The argument of the reference's scheduler.step (a016:110); epoch and iter_in_epoch count from 1 as the reference's do."""
    return epoch - 1 + (iter_in_epoch - 1) / iters_per_epoch


def save_training_state(path, model, optimizer, scheduler, epoch: int) -> None:
    """Write the reference's checkpoint (a016:243-249): exactly its four keys, readable by torch.load(weights_only=True)."""
    state = {
        "model_state": model.state_dict(),
        "optimizer_state": optimizer.state_dict(),
        "scheduler_state": scheduler.state_dict(),
        "current_epoch": int(epoch),
    }
    torch.save(state, path)


def load_training_state(path, model, optimizer, scheduler, map_location="cpu") -> int:
    """What a016:306-331 does: load model (strictly, through MyModel.load_reference_checkpoint: weights_only=True, nothing in the file
    is executed), optimiser and scheduler, -> the next epoch (the saved one has finished).  The optimiser state is indexed by the
    position of each parameter in model.parameters(), which is the reference's order (tests/golden/param_order_win7.json), so a
    checkpoint of the reference's script resumes here and the reverse.  A file that lacks one of the four keys raises KeyError before
    anything is loaded."""
    peek = torch.load(path, map_location="cpu", weights_only=True, mmap=True)   # the keys first: nothing is loaded from a file that lacks one
    missing = [k for k in STATE_KEYS if not isinstance(peek, dict) or k not in peek]
    del peek
    if missing:
        raise KeyError(f"{path}: not a training checkpoint of the reference's format, {missing} missing")
    rest = model.load_reference_checkpoint(path, map_location=map_location)
    optimizer.load_state_dict(rest["optimizer_state"])
    scheduler.load_state_dict(rest["scheduler_state"])
    return int(rest["current_epoch"]) + 1
