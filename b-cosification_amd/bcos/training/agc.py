"""Adaptive gradient clipping (Brock et al., https://arxiv.org/abs/2102.06171) at the reference's import path (bcos/training/agc.py).

Every B-cosification recipe sets `use_agc=True`, and its trainer calls `adaptive_clip_grad_(self.parameters())` before each optimizer step
(bcos/training/trainer.py:872-883).  The reference walks the parameters in Python (two norms and eight elementwise launches per tensor);
here the whole list is one call of `bcos_agc_clip` (include/bcos_hip.h, csrc/bcos_agc.hip).  `unitwise_norm` stays a pure-torch
function on any device: it is also the restatement the tests hold the kernel to.
"""
import torch

from bcos_hip import ops

__all__ = ["unitwise_norm", "adaptive_clip_grad_"]


def _unit_dims(x: torch.Tensor):
    """The dimensions unitwise_norm reduces over: all of them (None) for a tensor that squeezes to at most one dimension, the row for a
    matrix or 3-D tensor, the filter for an OIHW tensor."""
    if x.squeeze().ndim <= 1:
        return None
    if x.ndim == 4:
        return (1, 2, 3)
    if x.ndim in (2, 3):
        return 1
    raise ValueError(f"Expected 1 <= x.ndim <= 4. Got x.ndim={x.ndim}")


def unitwise_norm(x: torch.Tensor, norm_type: float = 2.0) -> torch.Tensor:
    """Norm of every unit of `x`, kept in the reduced dimensions (a 0-d tensor when the whole tensor is one unit)."""
    dims = _unit_dims(x)
    if dims is None:
        return x.norm(norm_type)
    return x.norm(norm_type, dim=dims, keepdim=True)


def adaptive_clip_grad_(parameters, clip_factor: float = 0.01, eps: float = 1e-3, norm_type: float = 2.0):
    """Per unit: max_norm = max(||p_u||, eps) * clip_factor; a gradient unit whose norm is not below max_norm is scaled to max_norm
    (gradient norms floored at 1e-6).  `parameters`: a tensor or an iterable of tensors; those without a gradient are skipped.  The
    parameters and gradients must be contiguous fp32 HIP tensors (no CPU fallback: bcos_hip.lib.BcosHipError otherwise)."""
    if norm_type != 2.0:
        raise NotImplementedError(f"adaptive_clip_grad_: only the 2-norm runs on the device (norm_type={norm_type})")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    ops.agc_clip(parameters, clip_factor=clip_factor, eps=eps)
