"""The autograd Functions behind the row and group norms, centred and uncentered (kernels: csrc/bcos_norms.hip).

`centered=True`:  y = weight (x - mean) / std + bias -- DetachableLayerNorm / DetachablePositionNorm2d / DetachableGroupNorm2d
`centered=False`: y = weight x / std + bias, the same centred variance -- PositionNormUncentered2d / GroupNormUncentered2d
In explanation mode (`detach`) the variance is a constant and only the input receives a gradient; otherwise nothing is detached and the
affine parameters receive theirs as column sums over gy and gy * x_n (x_n: the second result of ops.layernorm_bwd / ops.groupnorm_bwd).
"""
from torch.autograd import Function

from bcos_hip import ops

from bcos.modules import _hipfn


def _flavour(centered):
    """the keyword the ops take: `centered=False` where a norm is uncentered and nothing where it is centred, so that a centred call
    reads as it always did (recorded launch traces, stand-ins of the ops that know the centred norms only)"""
    return {} if centered else {"centered": False}


def _affine_grads(g2, xn2, need_w, need_b, centered):
    """(sum_rows gy x_n, sum_rows gy) over [rows, C].  ops.colsum moves float4; at a channel count not divisible by 4 the two flavours take
    paths of their own, which give different bits: the centred norms a torch reduction, the uncentered ones zero columns padded on and
    cut back."""
    c = g2.shape[1]
    if c % 4 == 0 or not (need_w or need_b):
        return (ops.colsum(g2, xn2) if need_w else None), (ops.colsum(g2) if need_b else None)
    if centered:
        return ((g2 * xn2).sum(0) if need_w else None), (g2.sum(0) if need_b else None)
    gp = _hipfn._pad_last(g2).contiguous()
    gw = ops.colsum(gp, _hipfn._pad_last(xn2).contiguous())[:c].contiguous() if need_w else None
    return gw, (ops.colsum(gp)[:c].contiguous() if need_b else None)


class _RowNormFn(Function):
    """the norm over the last dimension of x [..., D]: one wavefront per row"""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, detach, centered):
        _hipfn.require_hip(x, "DetachableLayerNorm" if centered else "PositionNormUncentered2d")
        D = x.shape[-1]
        x2 = x.reshape(-1, D)
        x2 = x2 if x2.is_contiguous() else x2.contiguous()
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        need_x = ctx.needs_input_grad[0]
        need_wb = (weight is not None and ctx.needs_input_grad[1]) or (bias is not None and ctx.needs_input_grad[2])
        y, rstd = ops.layernorm_fwd(x2, w, b, eps, want_rstd=need_x or need_wb, **_flavour(centered))
        ctx.detach_mode, ctx.centered, ctx.w, ctx.has_bias = detach, centered, w, bias is not None
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
            gx, _ = ops.layernorm_bwd_detached(g2, ctx.w, rstd, **_flavour(ctx.centered))
            return gx.view(gy.shape), None, None, None, None, None
        # training mode (centred: F.layer_norm's gradient, centered_norms.py:200-202): nothing detached
        x2 = ctx.saved_tensors[1]
        need_w = ctx.w is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gx, xn = ops.layernorm_bwd(g2, x2, ctx.w, rstd, want_xhat=need_w, **_flavour(ctx.centered))
        gw, gb = _affine_grads(g2, xn, need_w, need_b, ctx.centered)
        return gx.view(gy.shape), gw, gb, None, None, None


class _GroupNormFn(Function):
    """the group norm on the NHWC image of a logical [N,C,H,W] tensor: one workgroup per (image, group)"""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps, detach, centered):
        _hipfn.require_hip(x, "DetachableGroupNorm2d" if centered else "GroupNormUncentered2d")
        xh = _hipfn.to_nhwc(x)
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        need = ctx.needs_input_grad[0] or (weight is not None and ctx.needs_input_grad[1]) or (bias is not None and ctx.needs_input_grad[2])
        y, rstd = ops.groupnorm_fwd(xh, groups, w, b, eps, want_rstd=need, **_flavour(centered))
        ctx.detach_mode, ctx.centered, ctx.groups, ctx.w, ctx.has_bias = detach, centered, groups, w, bias is not None
        if rstd is not None:
            ctx.save_for_backward(rstd, *([xh] if not detach else []))
        return _hipfn.from_nhwc(y)

    @staticmethod
    def backward(ctx, gy):
        rstd = ctx.saved_tensors[0]
        gh = _hipfn.to_nhwc(gy)
        if ctx.detach_mode:         # explanation mode: variance constant, the input gradient only
            gx = ops.groupnorm_bwd_detached(gh, ctx.groups, ctx.w, rstd, **_flavour(ctx.centered))
            return _hipfn.from_nhwc(gx), None, None, None, None, None, None
        xh = ctx.saved_tensors[1]   # training mode (centred: F.group_norm's gradient, reference :109-113)
        need_w = ctx.w is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gx, xn = ops.groupnorm_bwd(gh, xh, ctx.groups, ctx.w, rstd, want_xhat=need_w, **_flavour(ctx.centered))
        Cc = gh.shape[-1]
        gw, gb = _affine_grads(gh.reshape(-1, Cc), xn.reshape(-1, Cc) if need_w else None, need_w, need_b, ctx.centered)
        return _hipfn.from_nhwc(gx), gw, gb, None, None, None, None
