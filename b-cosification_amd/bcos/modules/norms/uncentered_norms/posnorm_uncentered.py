"""PositionNormUncentered2d (PNU) on MI355X.

Reference: bcos/modules/norms/uncentered_norms/posnorm_uncentered.py -- class :17-37, forward :39-58.  Per position of a [N,C,H,W]
tensor, over its channels:
    var = x.var(dim=1, unbiased=False)  (the CENTRED second moment),   y = weight * x / sqrt(var + eps) + bias
-- the value that is divided is x itself, not x - mean.  On the NHWC image a position is a row, so forward and gradients are the row
kernels of csrc/bcos_unorm.hip (one wavefront per row):
    explanation mode (`detach`: var a constant)   gx = gy weight / std                              bcos_layernorm_unc_bwd_detached
    training mode                                 gx = r h - r^3 (x - mean) (sum_c h x) / C         bcos_layernorm_unc_bwd
    weight / bias gradients                       sum gy (x r), sum gy                              bcos_colsum
"""
import torch.nn as nn
from torch import Tensor
from torch.autograd import Function

from bcos_hip import ops

from bcos.modules import _hipfn
from bcos.modules.common import DetachableModule

__all__ = ["PositionNormUncentered2d"]


def _colsum(a2d, b2d=None):
    """column sums of a (* b) over rows of ANY width: the kernel moves float4, ragged widths are padded with zero columns and cut back"""
    c = a2d.shape[1]
    if c % 4 == 0:
        return ops.colsum(a2d, b2d)
    return ops.colsum(_hipfn._pad_last(a2d).contiguous(), _hipfn._pad_last(b2d).contiguous() if b2d is not None else None)[:c].contiguous()


class _RowNormUncFn(Function):
    """the uncentered norm over the last dimension of x [..., D]; follows centered_norms._LayerNormFn"""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, detach):
        _hipfn.require_hip(x, "PositionNormUncentered2d")
        D = x.shape[-1]
        x2 = x.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        need_x = ctx.needs_input_grad[0]
        need_wb = (weight is not None and ctx.needs_input_grad[1]) or (bias is not None and ctx.needs_input_grad[2])
        y, rstd = ops.layernorm_unc_fwd(x2, w, b, eps, want_rstd=need_x or need_wb)
        ctx.detach_mode = detach
        ctx.w = w
        ctx.has_bias = bias is not None
        if rstd is not None:
            ctx.save_for_backward(rstd, *([x2] if not detach else []))
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, gy):
        rstd = ctx.saved_tensors[0]
        g2 = gy.reshape(-1, gy.shape[-1])
        g2 = g2 if g2.is_contiguous() else g2.contiguous()
        if ctx.detach_mode:
            # explanation mode: the input gradient only (the affine parameters receive gradients in training mode)
            gx, _ = ops.layernorm_unc_bwd_detached(g2, ctx.w, rstd)
            return gx.view(gy.shape), None, None, None, None
        x2 = ctx.saved_tensors[1]
        need_w = ctx.w is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gx, xr = ops.layernorm_unc_bwd(g2, x2, ctx.w, rstd, want_xr=need_w)
        gw = _colsum(g2, xr) if need_w else None
        gb = _colsum(g2) if need_b else None
        return gx.view(gy.shape), gw, gb, None, None


class PositionNormUncentered2d(nn.LayerNorm, DetachableModule):
    """Uncentered position norm over the channels of every position of a [N,C,H,W] tensor (reference :17-58)."""

    def __init__(self, features: int, eps: float = 1e-5, affine: bool = True, device=None, dtype=None) -> None:
        assert isinstance(features, int), f"Provide #features as an int not {type(features)=}"
        DetachableModule.__init__(self)
        super().__init__(normalized_shape=features, eps=eps, elementwise_affine=affine, device=device, dtype=dtype)
        self.features = features

    def forward(self, x: Tensor) -> Tensor:
        assert x.dim() == 4, f"input should be 4D not {x.dim()}D"
        y = _RowNormUncFn.apply(_hipfn.to_nhwc(x), self.weight, self.bias, self.eps, self.detach)
        return _hipfn.from_nhwc(y)
