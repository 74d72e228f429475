"""PositionNormUncentered2d (PNU) on MI355X.

Reference: bcos/modules/norms/uncentered_norms/posnorm_uncentered.py -- class :17-37, forward :39-58.  Per position of a [N,C,H,W]
tensor, over its channels:
    var = x.var(dim=1, unbiased=False)  (the CENTRED second moment),   y = weight * x / sqrt(var + eps) + bias
-- the value that is divided is x itself, not x - mean.  On the NHWC image a position is a row, so forward and gradients are the row
kernels of csrc/bcos_norms.hip (one wavefront per row; the autograd Function is _norm_fns._RowNormFn with centered=False):
    explanation mode (`detach`: var a constant)   gx = gy weight / std                              bcos_layernorm_unc_bwd_detached
    training mode                                 gx = r h - r^3 (x - mean) (sum_c h x) / C         bcos_layernorm_unc_bwd
    weight / bias gradients                       sum gy (x r), sum gy                              bcos_colsum
"""
import torch.nn as nn
from torch import Tensor

from bcos.modules import _hipfn
from bcos.modules.common import DetachableModule
from bcos.modules.norms._norm_fns import _RowNormFn

__all__ = ["PositionNormUncentered2d"]


class PositionNormUncentered2d(nn.LayerNorm, DetachableModule):
    """Uncentered position norm over the channels of every position of a [N,C,H,W] tensor (reference :17-58)."""

    def __init__(self, features: int, eps: float = 1e-5, affine: bool = True, device=None, dtype=None) -> None:
        assert isinstance(features, int), f"Provide #features as an int not {type(features)=}"
        DetachableModule.__init__(self)
        super().__init__(normalized_shape=features, eps=eps, elementwise_affine=affine, device=device, dtype=dtype)
        self.features = features

    def forward(self, x: Tensor) -> Tensor:
        assert x.dim() == 4, f"input should be 4D not {x.dim()}D"
        y = _RowNormFn.apply(_hipfn.to_nhwc(x), self.weight, self.bias, self.eps, self.detach, False)
        return _hipfn.from_nhwc(y)
