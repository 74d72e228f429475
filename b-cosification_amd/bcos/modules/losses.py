"""The classification losses of the B-cosification recipes at the reference's import path (bcos/modules/losses.py:36-139).

Both are compositions of torch operators on [B, classes] logits -- there is no hot path to move to the device.  The CLIP distillation
losses of the same reference file are not part of this package.
"""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["BinaryCrossEntropyLoss", "UniformOffLabelsBCEWithLogitsLoss"]


def _dense_targets(x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """class indices -> one-hot rows in the logits' dtype; dense targets pass through"""
    if target.shape == x.shape:
        return target
    return F.one_hot(target, num_classes=x.shape[-1]).to(dtype=x.dtype)


class BinaryCrossEntropyLoss(nn.Module):
    """BCE-with-logits on dense or sparse (class index) targets, with label smoothing as torch.nn.CrossEntropyLoss applies it
    (t (1 - s) + s / classes, also for sparse targets) and an optional threshold that turns the targets into 0 / 1 after smoothing."""

    def __init__(self, smoothing=0.0, target_threshold: Optional[float] = None, weight: Optional[torch.Tensor] = None,
                 reduction: str = "mean", pos_weight: Optional[torch.Tensor] = None):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"smoothing must lie in [0, 1), got {smoothing}")
        self.smoothing = smoothing
        self.target_threshold = target_threshold
        self.reduction = reduction
        self.register_buffer("weight", weight)
        self.register_buffer("pos_weight", pos_weight)

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if x.shape[0] != target.shape[0]:
            raise ValueError(f"{x.shape[0]} logit rows, {target.shape[0]} targets")
        target = _dense_targets(x, target)
        if self.smoothing > 0.0:
            target = target * (1 - self.smoothing) + self.smoothing / x.shape[-1]
        if self.target_threshold is not None:
            target = (target > self.target_threshold).to(dtype=target.dtype)
        return F.binary_cross_entropy_with_logits(x, target, self.weight, pos_weight=self.pos_weight, reduction=self.reduction)

    def extra_repr(self) -> str:
        parts = [f"reduction={self.reduction}"]
        if self.smoothing > 0:
            parts.append(f"smoothing={self.smoothing}")
        if self.target_threshold is not None:
            parts.append(f"target_threshold={self.target_threshold}")
        for name in ("weight", "pos_weight"):
            if getattr(self, name) is not None:
                parts.append(f"{name}={getattr(self, name).shape}")
        return ", ".join(parts)


class UniformOffLabelsBCEWithLogitsLoss(nn.Module):
    """BCE-with-logits whose off-label targets are raised to `off_label` (1 / classes when it is unset or zero); the true class keeps 1.
    With 5 classes and class 3: targets [0.2, 0.2, 0.2, 1.0, 0.2]."""

    def __init__(self, reduction: str = "mean", off_label: Optional[float] = None):
        super().__init__()
        self.reduction = reduction
        self.off_label = off_label

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if x.shape[0] != target.shape[0]:
            raise ValueError(f"{x.shape[0]} logit rows, {target.shape[0]} targets")
        floor = self.off_label if self.off_label else 1.0 / x.shape[-1]
        target = _dense_targets(x, target).clamp(min=floor)
        return F.binary_cross_entropy_with_logits(x, target, reduction=self.reduction)

    def extra_repr(self) -> str:
        parts = [f"reduction={self.reduction}"]
        if self.off_label is not None:
            parts.append(f"off_label={self.off_label}")
        return ", ".join(parts)
