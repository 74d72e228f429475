"""Detachable (centred) norms for B-cos transformers on MI355X.

Reference: bcos/modules/norms/centered_norms.py -- `DetachableLayerNorm` :187-245 is the one the B-cosified ViTs use
(SURVEY.md a10).  In explanation mode its variance is a constant while the mean stays differentiable, so
    y = w (x - mean(x)) / std (+ b),    d y / d x  applied to g:   h - mean(h),  h = g w / std.
Forward and that input gradient are one-wavefront-per-row HIP kernels (bcos_layernorm_fwd / _bwd_detached).
The 2-D group-norm variants (`DetachableGroupNorm2d` :93-160 and its instance / layer-norm forms: the conv stems of the
ViT-C models) follow the same rule per (image, group) on NHWC data (bcos_groupnorm_fwd / _bwd_detached).
"""
import torch.nn as nn
from torch import Tensor

from bcos.modules import _hipfn
from bcos.modules.common import DetachableModule

from ._norm_fns import _GroupNormFn, _RowNormFn

__all__ = ["DetachableLayerNorm", "DetachablePositionNorm2d", "DetachableGroupNorm2d", "DetachableGNInstanceNorm2d", "DetachableGNLayerNorm2d"]


class DetachableLayerNorm(nn.LayerNorm, DetachableModule):
    """nn.LayerNorm over the last dimension whose variance is detached in explanation mode (reference :187-245)."""

    def __init__(self, *args, **kwargs):
        DetachableModule.__init__(self)
        super().__init__(*args, **kwargs)

    def forward(self, input: Tensor) -> Tensor:
        if len(self.normalized_shape) != 1:
            raise NotImplementedError("the HIP LayerNorm normalises over the last dimension only")
        return _RowNormFn.apply(input, self.weight, self.bias, self.eps, self.detach, True)

    @classmethod
    def from_standard_module(cls, standard_module: nn.LayerNorm, model_config: dict):
        new = cls(normalized_shape=standard_module.normalized_shape, eps=standard_module.eps,
                  elementwise_affine=standard_module.elementwise_affine)
        if model_config.get("weights", None) is not None:
            new.weight.data = standard_module.weight.data
            if standard_module.bias is not None:
                new.bias.data = standard_module.bias.data
        return new


class DetachablePositionNorm2d(nn.LayerNorm, DetachableModule):
    """LayerNorm over the channels of every position of a [N,C,H,W] tensor (reference :251-298; the norm of the B-cos ConvNeXts):
    on the NHWC image that is a LayerNorm over rows, so forward and gradients are those of _RowNormFn -- explanation mode keeps
    the variance constant and the mean differentiable (:283-298), otherwise F.layer_norm's gradient (:277-281)."""

    def __init__(self, features: int, eps: float = 1e-5, affine: bool = True, device=None, dtype=None) -> None:
        assert isinstance(features, int), f"Provide #features as an int not {type(features)=}"
        DetachableModule.__init__(self)
        super().__init__(normalized_shape=features, eps=eps, elementwise_affine=affine, device=device, dtype=dtype)
        self.features = features

    def forward(self, x: Tensor) -> Tensor:
        assert x.dim() == 4, f"input should be 4D not {x.dim()}D"
        y = _RowNormFn.apply(_hipfn.to_nhwc(x), self.weight, self.bias, self.eps, self.detach, True)
        return _hipfn.from_nhwc(y)


class DetachableGroupNorm2d(nn.GroupNorm, DetachableModule):
    """nn.GroupNorm over [N,C,H,W] whose variance is detached in explanation mode (reference :93-160; the norm of the
    conv stems of the ViT-C models).  Forward and the explanation-mode input gradient are HIP kernels
    (bcos_groupnorm_fwd / _bwd_detached)."""

    def __init__(self, *args, **kwargs):
        DetachableModule.__init__(self)
        super().__init__(*args, **kwargs)

    def forward(self, input: Tensor) -> Tensor:
        assert input.dim() == 4, f"Expected 4D input got {input.dim()}D instead!"
        assert input.shape[1] % self.num_groups == 0, (
            "Number of channels in input should be divisible by num_groups, "
            f"but got input of shape {input.shape} and num_groups={self.num_groups}")
        return _GroupNormFn.apply(input, self.weight, self.bias, self.num_groups, self.eps, self.detach, True)

    @classmethod
    def from_standard_module(cls, mod: nn.GroupNorm, model_config: dict):
        new = cls(num_groups=mod.num_groups, num_channels=mod.num_channels, eps=mod.eps, affine=mod.affine)
        if model_config.get("weights", None) is not None and mod.affine:
            new.weight.data = mod.weight.data
            if mod.bias is not None:
                new.bias.data = mod.bias.data
        return new


class DetachableGNInstanceNorm2d(DetachableGroupNorm2d):
    def __init__(self, num_channels: int, *args, **kwargs):
        super().__init__(num_channels, num_channels, *args, **kwargs)


class DetachableGNLayerNorm2d(DetachableGroupNorm2d):
    """A CNN detachable layer norm: one group (reference :175-186)."""

    def __init__(self, num_channels: int, *args, **kwargs):
        super().__init__(1, num_channels, *args, **kwargs)
