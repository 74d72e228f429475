"""Group norm without centering on MI355X, with its instance-norm and layer-norm forms.

Reference: bcos/modules/norms/uncentered_norms/groupnorm_uncentered.py -- functional :21-61, GroupNormUncentered2d :64-79,
GNInstanceNormUncentered2d :82-89, GNLayerNormUncentered2d :92-99.  Per (image, group) of a [N,C,H,W] tensor:
    var = x.var(unbiased=False) over the group (CENTRED),   y = weight * x / sqrt(var + eps) + bias      (x itself is divided)
On NHWC data one workgroup owns an (image, group) (csrc/bcos_unorm.hip):
    explanation mode (`detach`: var a constant)   gx = gy weight / std                               bcos_groupnorm_unc_bwd_detached
    training mode                                 gx = r h - r^3 (x - mean) (sum_group h x) / n      bcos_groupnorm_unc_bwd
    weight / bias gradients                       sum gy (x r), sum gy                               bcos_colsum
"""
from typing import Optional

import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from bcos_hip import ops

from bcos.modules import _hipfn
from bcos.modules.common import DetachableModule

from .posnorm_uncentered import _colsum

__all__ = ["group_norm_uncentered", "GroupNormUncentered2d", "GNInstanceNormUncentered2d", "GNLayerNormUncentered2d"]


class _GroupNormUncFn(Function):
    """uncentered GroupNorm on the NHWC image of a logical [N,C,H,W] tensor; follows centered_norms._GroupNormFn"""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, detach):
        _hipfn.require_hip(x, "GroupNormUncentered2d")
        xh = _hipfn.to_nhwc(x)
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        need = ctx.needs_input_grad[0] or (weight is not None and ctx.needs_input_grad[1]) or (bias is not None and ctx.needs_input_grad[2])
        y, rstd = ops.groupnorm_unc_fwd(xh, groups, w, b, eps, want_rstd=need)
        ctx.detach_mode, ctx.groups, ctx.w, ctx.has_bias = detach, groups, w, bias is not None
        if rstd is not None:
            ctx.save_for_backward(rstd, *([xh] if not detach else []))
        return _hipfn.from_nhwc(y)

    @staticmethod
    def backward(ctx, gy):
        rstd = ctx.saved_tensors[0]
        gh = _hipfn.to_nhwc(gy)
        if ctx.detach_mode:         # explanation mode: variance constant, the input gradient only
            return _hipfn.from_nhwc(ops.groupnorm_unc_bwd_detached(gh, ctx.groups, ctx.w, rstd)), None, None, None, None, None
        xh = ctx.saved_tensors[1]
        need_w = ctx.w is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gx, xr = ops.groupnorm_unc_bwd(gh, xh, ctx.groups, ctx.w, rstd, want_xr=need_w)
        Cc = gh.shape[-1]
        g2 = gh.reshape(-1, Cc)
        gw = _colsum(g2, xr.reshape(-1, Cc)) if need_w else None
        gb = _colsum(g2) if need_b else None
        return _hipfn.from_nhwc(gx), gw, gb, None, None, None


def group_norm_uncentered(input: Tensor, num_groups: int, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                          eps: float = 1e-5, detach: bool = False):
    """Un-centered group norm on batched [N,C,H,W] input (reference :21-61)."""
    assert input.dim() == 4, f"Expected 4D input got {input.dim()}D instead!"
    assert input.shape[1] % num_groups == 0, (
        "Number of channels in input should be divisible by num_groups, "
        f"but got input of shape {input.shape} and num_groups={num_groups}")
    return _GroupNormUncFn.apply(input, weight, bias, num_groups, eps, detach)


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
