"""AllNormUncentered2d on MI355X: one variance for the whole [N,C,H,W] tensor.

Reference: bcos/modules/norms/uncentered_norms/allnorm_uncentered.py -- functional :19-56, class :59-122.  weight, bias and
running_var have shape [1] (the class builds an nn.BatchNorm2d over ONE feature, :70-74).
    training:  var = x.var(unbiased=False) over everything (CENTRED), running_var <- (1 - m) running_var + m var,
               y = weight * x / sqrt(var + eps) + bias                                   (x itself is divided)
    eval:      the same with var = running_var: a per-tensor affine map, linear in x
No kernel of its own -- the composition batchnorm_uncentered.py uses, with every per-channel vector a broadcast scalar:
    statistics   bcos_colsum (column sums; then the centred squares against the broadcast global mean), each finished by a
                 fixed-order sum over the channels (bcos_colsum again, over the [C] vector as a column)
    forward      bcos_channel_affine
    gradient     explanation mode (`detach`): gx = gy weight / std (bcos_channel_affine);
                 training mode: gx = r h - r^3 (x - mean) (sum h x) / n, h = gy weight (bcos_channel_axpby)
    weight / bias gradients   r sum gy x,  sum gy
"""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor
from torch.autograd import Function

from bcos_hip import ops

from bcos.modules import _hipfn
from bcos.modules.common import DetachableModule

from .batchnorm_uncentered import _ChannelAffineFn

__all__ = ["AllNormUncentered2d"]          # (the reference's; all_norm_uncentered_2d is importable from this module, as there)


def _total(v: Tensor) -> Tensor:
    """sum of a [C] vector -> [1], in one fixed order (bcos_colsum over the vector as the first of four columns)"""
    return ops.colsum(F.pad(v.reshape(-1, 1), (0, 3)))[:1]


def _bcast(v: Tensor, c: int) -> Tensor:
    return v.reshape(1).expand(c).contiguous()


class _AllStatsFn(Function):
    """y = x / sqrt(var_all(x) + eps) * weight + bias with gradients to x, weight [1] and bias [1]."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, detach, stats_out):
        _hipfn.require_hip(x, "AllNormUncentered2d")
        xh = _hipfn.to_nhwc(x)
        c = xh.shape[-1]
        if c % 4 != 0:
            raise _hipfn.BcosHipError(f"AllNormUncentered2d HIP kernels need C % 4 == 0 (got {c})")
        x2 = xh.view(-1, c)
        n = x2.numel()
        mean = _total(ops.colsum(x2)) / n
        mean_b = _bcast(mean, c)
        var = _total(ops.colsum(x2, x2, mean_b, mean_b)) / n            # centred second moment: x.var(unbiased=False)
        stats_out.append(var)
        rstd = torch.rsqrt(var + eps)
        g = rstd if weight is None else weight.detach().reshape(1) * rstd
        y_cl, y = _hipfn.empty_cl(x.shape[0], c, x.shape[2], x.shape[3], x.device)
        ops.channel_affine(xh, _bcast(g, c), _bcast(bias.detach(), c) if bias is not None else None, out=y)
        ctx.save_for_backward(xh, mean_b, rstd, g)
        ctx.flags = (bool(detach), weight is not None, bias is not None)
        return y_cl

    @staticmethod
    def backward(ctx, gy):
        xh, mean_b, rstd, g = ctx.saved_tensors
        detach, has_w, has_b = ctx.flags
        c = xh.shape[-1]
        gh = _hipfn.to_nhwc(gy)
        g2, x2 = gh.view(-1, c), xh.view(-1, c)
        n = x2.numel()
        gx_cl = gw = gb = None
        need_w = has_w and ctx.needs_input_grad[1]
        sgx = _total(ops.colsum(g2, x2)) if need_w or (ctx.needs_input_grad[0] and not detach) else None
        if ctx.needs_input_grad[0]:
            gx_cl, gx = _hipfn.empty_cl(gy.shape[0], c, gy.shape[2], gy.shape[3], gy.device)
            if detach:                                                # variance held constant: one scale for everything
                ops.channel_affine(gh, _bcast(g, c), None, out=gx)
            else:                                                     # + dL/dvar * 2 (x - mean) / n
                coef = -(g * sgx) * rstd * rstd / n
                ops.channel_axpby(gh, _bcast(g, c), xh, mean_b, _bcast(coef, c), out=gx)
        if need_w:
            gw = sgx * rstd                                           # sum gy * x / std
        if has_b and ctx.needs_input_grad[2]:
            gb = _total(ops.colsum(g2))
        return gx_cl, gw, gb, None, None, None


def all_norm_uncentered_2d(input: Tensor, running_var: Optional[Tensor], weight: Optional[Tensor] = None,
                           bias: Optional[Tensor] = None, training: bool = False, momentum: float = 0.1, eps: float = 1e-5,
                           detach: bool = False):
    """Functional form (reference :19-56).  Accepts only batched [N,C,H,W] tensors; weight, bias and running_var hold one value."""
    assert input.dim() == 4, "input should be a 4d tensor!"
    if training:
        stats = []
        out = _AllStatsFn.apply(input, weight, bias, eps, detach, stats)
        if running_var is not None:
            with torch.no_grad():
                running_var.copy_((1 - momentum) * running_var + momentum * stats[0].view_as(running_var))
        return out
    assert running_var is not None, "running_var must be defined in eval mode"
    c = input.shape[1]
    rstd = (1.0 / (running_var.detach() + eps).sqrt()).reshape(1).expand(c)
    wb = weight.reshape(1).expand(c) if weight is not None else None       # (expand: autograd sums the channels' gradients back to [1])
    bb = bias.reshape(1).expand(c) if bias is not None else None
    scale = rstd if wb is None else wb.detach() * rstd
    shift = bb.detach().contiguous() if bb is not None else None
    return _ChannelAffineFn.apply(input, scale.contiguous(), shift, wb, bb, rstd.contiguous())


class AllNormUncentered2d(nn.BatchNorm2d, DetachableModule):
    def __init__(self, num_features: int, *args, **kwargs) -> None:
        DetachableModule.__init__(self)
        # normalised over the whole tensor: ONE feature, whatever `num_features` says (reference :68-74)
        super().__init__(1, *args, **kwargs)

    def forward(self, input):
        self._check_input_dim(input)
        momentum = 0.0 if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            if self.momentum is None:                                  # cumulative moving average (reference :91-92)
                momentum = 1.0 / float(self.num_batches_tracked)
        use_batch_stats = self.training or (self.running_mean is None and self.running_var is None)
        running_var = self.running_var if (not self.training or self.track_running_stats) else None
        return all_norm_uncentered_2d(input, running_var, self.weight, self.bias, training=use_batch_stats, momentum=momentum,
                                      eps=self.eps, detach=self.detach)
