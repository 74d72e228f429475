"""Group norm without centering on MI355X, with its instance-norm and layer-norm forms.

Reference: bcos/modules/norms/uncentered_norms/groupnorm_uncentered.py -- functional :21-61, GroupNormUncentered2d :64-79,
GNInstanceNormUncentered2d :82-89, GNLayerNormUncentered2d :92-99.  Per (image, group) of a [N,C,H,W] tensor:
    var = x.var(unbiased=False) over the group (CENTRED),   y = weight * x / sqrt(var + eps) + bias      (x itself is divided)
On NHWC data one workgroup owns an (image, group) (csrc/bcos_norms.hip; the autograd Function is _norm_fns._GroupNormFn, centered=False):
    explanation mode (`detach`: var a constant)   gx = gy weight / std                               bcos_groupnorm_unc_bwd_detached
    training mode                                 gx = r h - r^3 (x - mean) (sum_group h x) / n      bcos_groupnorm_unc_bwd
    weight / bias gradients                       sum gy (x r), sum gy                               bcos_colsum
"""
from typing import Optional

import torch.nn as nn
from torch import Tensor

from bcos.modules.common import DetachableModule
from bcos.modules.norms._norm_fns import _GroupNormFn

__all__ = ["group_norm_uncentered", "GroupNormUncentered2d", "GNInstanceNormUncentered2d", "GNLayerNormUncentered2d"]


def group_norm_uncentered(input: Tensor, num_groups: int, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                          eps: float = 1e-5, detach: bool = False):
    """Un-centered group norm on batched [N,C,H,W] input (reference :21-61)."""
    assert input.dim() == 4, f"Expected 4D input got {input.dim()}D instead!"
    assert input.shape[1] % num_groups == 0, (
        "Number of channels in input should be divisible by num_groups, "
        f"but got input of shape {input.shape} and num_groups={num_groups}")
    return _GroupNormFn.apply(input, weight, bias, num_groups, eps, detach, False)


class GroupNormUncentered2d(nn.GroupNorm, DetachableModule):
    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, affine: bool = True) -> None:
        DetachableModule.__init__(self)
        super().__init__(num_groups, num_channels, eps, affine)

    def forward(self, input: Tensor) -> Tensor:
        return group_norm_uncentered(input, self.num_groups, self.weight, self.bias, self.eps, detach=self.detach)


class GNInstanceNormUncentered2d(GroupNormUncentered2d):
    """one group per channel (reference :82-89)"""

    def __init__(self, num_channels: int, *args, **kwargs):
        super().__init__(num_channels, num_channels, *args, **kwargs)


class GNLayerNormUncentered2d(GroupNormUncentered2d):
    """one group (reference :92-99)"""

    def __init__(self, num_channels: int, *args, **kwargs):
        super().__init__(1, num_channels, *args, **kwargs)
