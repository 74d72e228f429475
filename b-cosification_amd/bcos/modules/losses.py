"""The losses of the B-cosification recipes at the reference's import path (bcos/modules/losses.py:36-139, 576-694).

The two classification losses are compositions of torch operators on [B, classes] logits -- there is no hot path to move to the device.
SigLipLoss, the objective of the CLIP recipe (experiment_parameters.py:61-62), is: float32 device tensors take the fused
bcos_hip.ops.siglip_loss (loss and every gradient in one library call), anything else the same formula as torch operators
(siglip_loss_torch).  The ClipLoss / DistillClipLoss / CoCaLoss / InfoNCE family of the same reference file, which no recipe of the
reference uses, is not part of this package.
"""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .common import DetachableModule

__all__ = ["BinaryCrossEntropyLoss", "UniformOffLabelsBCEWithLogitsLoss", "SigLipLoss"]


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


def siglip_loss_torch(image_features, text_features, logit_scale, logit_bias=None, *, pos_offset=0, cos_scaling=0, detach=False):
    """SigLipLoss.get_logits / _loss of the reference (losses.py:612-638) as torch operators, on any device and dtype:
    image_features [N, D] (cos_scaling = 0) or [L, N, D] (cos_scaling >= 1), text_features [M, D]; column pos_offset + i is row i's
    positive, pos_offset < 0 is the reference's negative_only.  With M = world_size * N and pos_offset = rank * N it is the sum the
    reference's forward builds from its neighbour exchanges (:643-692)."""
    logits = image_features @ text_features.T
    if cos_scaling > 0:
        w = torch.pow(logits, cos_scaling - 1).abs()
        logits = (logits * (w.detach() if detach else w)).mean(0)
    n, m = logits.shape
    if logit_scale is not None:
        logits = logit_scale * logits
    if logit_bias is not None:
        logits = logits + logit_bias
    labels = -torch.ones((n, m), device=logits.device, dtype=logits.dtype)
    if pos_offset >= 0:
        rows = torch.arange(n, device=logits.device)
        labels[rows, rows + pos_offset] = 1
    return -F.logsigmoid(labels * logits).sum() / n


def _host_scalar(v):
    """a logit scale / bias the fused op can take as a constant: None, a Python number, or a CPU tensor outside the graph (the
    reference's training step builds its fixed scale and bias on the host, trainer.py:689-697)"""
    return v is None or not torch.is_tensor(v) or (v.device.type == "cpu" and v.numel() == 1 and not v.requires_grad)


def _device_scalar(v, device):
    return torch.is_tensor(v) and v.device == device and v.dtype == torch.float32 and v.numel() == 1


class SigLipLoss(DetachableModule):
    """Sigmoid loss for language-image pre-training (Zhai et al. 2023, arXiv:2303.15343) as the CLIP B-cosification recipe uses it for
    distillation -- the reference's class (losses.py:576-694) with its constructor and forward signature.

    `image_features` [N, D] with cos_scaling = 0, or [(HW), N, D] (attn_unpool head) with an integer cos_scaling >= 1: every location's
    logit times |logit|^(cos_scaling - 1), averaged over the locations; in explanation mode (`detach`) that factor is a constant.
    `text_features` [N, D].  Both are expected L2-normalised, as the training step passes them (bcos_hip.clip_head.distill_loss
    normalises inside the same call).  A fractional cos_scaling is NaN in the reference (torch.pow of a negative base): refused.

    world_size > 1: the other ranks' text features enter as negatives, every term divided by the local batch size.  They are
    all-gathered (torch.distributed, default group) rather than passed around the ring, so no gradient reaches them: text features that
    require a gradient are refused -- the recipe's teacher is frozen.  The reference's multi-rank sum drops cos_scaling from its negative
    terms (:659-665), which fails on [(HW), N, D] features; here cos_scaling >= 1 with world_size > 1 is refused."""

    def __init__(self, cache_labels=False, rank=0, world_size=1, bidir=True, use_horovod=False):
        super().__init__()
        self.cache_labels = cache_labels
        self.rank = rank
        self.world_size = world_size
        assert not use_horovod
        self.use_horovod = use_horovod
        self.bidir = bidir
        self.prev_num_logits = 0
        self.labels = {}

    def forward(self, image_features, text_features, logit_scale, logit_bias, output_dict=False, cos_scaling=0):
        if cos_scaling != int(cos_scaling) or cos_scaling < 0:
            raise ValueError(f"SigLipLoss: cos_scaling must be a non-negative integer, got {cos_scaling} (a fractional power of a negative "
                             "cosine is NaN in the reference)")
        cos_scaling = int(cos_scaling)
        if image_features.dim() != (3 if cos_scaling > 0 else 2) or text_features.dim() != 2:
            raise ValueError(f"SigLipLoss: image features are [N, D] with cos_scaling = 0 and [(HW), N, D] with cos_scaling >= 1, text "
                             f"features [N, D]; got {tuple(image_features.shape)}, {tuple(text_features.shape)}, cos_scaling {cos_scaling}")
        pos_offset = 0
        if self.world_size > 1:
            if text_features.requires_grad:
                raise NotImplementedError("SigLipLoss: world_size > 1 with text features that require a gradient is not supported (the "
                                          "features are all-gathered, not exchanged with gradient; the recipe's teacher is frozen)")
            if cos_scaling > 0:
                raise NotImplementedError("SigLipLoss: cos_scaling >= 1 with world_size > 1 (the reference's negative terms drop it)")
            import torch.distributed as dist
            parts = [torch.empty_like(text_features) for _ in range(self.world_size)]
            dist.all_gather(parts, text_features.contiguous())
            text_features = torch.cat(parts, 0)
            pos_offset = self.rank * image_features.shape[-2]
        fused = (image_features.is_cuda and image_features.dtype == torch.float32 and text_features.dtype == torch.float32
                 and text_features.device == image_features.device
                 and all(_host_scalar(v) or _device_scalar(v, image_features.device) for v in (logit_scale, logit_bias)))
        if fused:
            from bcos_hip import ops
            scale = 1.0 if logit_scale is None else (float(logit_scale) if _host_scalar(logit_scale) else logit_scale)
            bias = 0.0 if logit_bias is None else (float(logit_bias) if _host_scalar(logit_bias) else logit_bias)
            loss = ops.siglip_loss(image_features, text_features, scale, bias, pos_offset=pos_offset, p=cos_scaling, detach_pow=self.detach)
        else:
            loss = siglip_loss_torch(image_features, text_features, logit_scale, logit_bias, pos_offset=pos_offset,
                                     cos_scaling=cos_scaling, detach=self.detach)
        return {"contrastive_loss": loss} if output_dict else loss
