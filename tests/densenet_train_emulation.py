"""CPU restatements of the four training-mode dense-block entry points (TEST INFRASTRUCTURE, beside densenet_emulation.py): what
include/bcos_hip.h documents for bcos_slice_batch_stats, bcos_bn_reader_finish, bcos_slice_relu_bwd_colsums and bcos_slice_bn_bwd_acc.
The `*64` forms evaluate the documented maps in float64 from the fp32 inputs and return the header's bounds as formulas of the INPUTS;
the stand-ins for the bcos_hip.ops wrappers keep the documented contracts that tests rely on without a device: a column's statistics
depend on that column alone (each column is summed on its own, contiguous copy), the ReLU gate is the fp32 forward's decision, and with
no variance term `slice_bn_bwd_acc` is densenet_emulation.slice_affine_bwd_acc."""
import torch

import densenet_emulation as DE

ULP = 2.0 ** -23
TINY = 2.0 ** -149          # (the smallest denormal, as in densenet_emulation.py: a bound of exactly zero still admits it)


def col_plan(rows):
    """(nblk, rpb) of the column reductions: a function of `rows` alone (include/bcos_hip.h)"""
    b = min((rows + 127) // 128, 1024)
    rpb = (rows + b - 1) // b
    return (rows + rpb - 1) // rpb, rpb


def depth(rows):
    """D(rows) of the header: no addend passes through more additions"""
    nblk, rpb = col_plan(rows)
    return (rpb + 31) // 32 + (nblk + 15) // 16 + 56


def ws_floats(rows, C):
    return 3 * col_plan(rows)[0] * C


def _cols64(x):
    """[rows, C] slice -> [C, rows] float64, contiguous: every column reduced on its own"""
    return DE._f32(x).reshape(-1, x.shape[-1]).t().contiguous().double()


def slice_batch_stats64(x):
    """-> (mean64, var64, bound_mean, bound_var) per channel"""
    xc = _cols64(x)
    mean = xc.mean(1)
    var = ((xc - mean[:, None]) ** 2).mean(1)
    A, R = xc.abs().amax(1), (xc - mean[:, None]).abs().amax(1)
    D = depth(xc.shape[1])
    return mean, var, ULP * 3 * D * A + TINY, ULP * D * (16 * R * R + 2 * R * A) + TINY


def slice_relu_bwd_colsums64(d, x, gvec, shift=None):
    """-> (sgx64, sg64, bound_sgx, bound_sg, gate)"""
    gate = DE.pre_activation32(x, gvec, shift) > 0
    C = x.shape[-1]
    gd = torch.where(gate.reshape(-1, C), DE._f32(d).reshape(-1, C).double(), torch.zeros((), dtype=torch.float64))
    gdx = gd * DE._f32(x).reshape(-1, C).double()
    D = depth(gd.shape[0])
    return gdx.sum(0), gd.sum(0), ULP * D * gdx.abs().sum(0) + TINY, ULP * D * gd.abs().sum(0) + TINY, gate


def slice_bn_bwd_acc64(d, g_old, x, scale=None, shift=None, mean=None, coef=None, accumulate=True):
    """-> (g in float64, the header's per-element bound, gate)"""
    if coef is None:
        return DE.slice_affine_bwd_acc64(d, g_old, x, scale, shift, True, accumulate)
    C = x.shape[-1]
    p = DE._f32(d).reshape(-1, C).double()
    if scale is not None:
        p = p * DE._f32(scale).double()
    gate = (DE.pre_activation32(x, scale, shift) > 0).reshape(p.shape)
    p = torch.where(gate, p, torch.zeros((), dtype=torch.float64))
    t = DE._f32(x).reshape(-1, C).double()
    if mean is not None:
        t = t - DE._f32(mean).double()
    t = t * DE._f32(coef).double()
    old = DE._f32(g_old).reshape(-1, C).double() if accumulate else torch.zeros_like(p)
    return old + p + t, ULP * (old.abs() + 2 * p.abs() + 2 * t.abs()) + 2.0 ** -149, gate


# ---- stand-ins for the bcos_hip.ops wrappers (same signatures) ---------------------------------------------------------------------
def slice_batch_stats(x, mean, var):
    xc = _cols64(x)
    m = xc.mean(1)
    mean.copy_(m.float())
    var.copy_(((xc - m[:, None]) ** 2).mean(1).float())
    return mean, var


def bn_reader_finish(var, weight, eps, running_var=None, momentum=0.0):
    rstd = torch.rsqrt(var + eps)
    g = rstd.clone() if weight is None else weight * rstd
    if running_var is not None:
        running_var.copy_((1 - momentum) * running_var + momentum * var)
    return rstd, g


def slice_relu_bwd_colsums(d, x, gvec, shift=None, rstd=None, want_sg=False, want_gw=False, want_coef=False):
    sgx64, sg64, _, _, _ = slice_relu_bwd_colsums64(d, x, gvec, shift)
    sgx = sgx64.float()
    rows = x.numel() // x.shape[-1]
    gw = sgx * rstd if want_gw else None
    coef = -(gvec * sgx) * rstd * rstd / rows if want_coef else None
    return sgx, (sg64.float() if want_sg else None), gw, coef


def slice_bn_bwd_acc(d, g, x, scale=None, shift=None, mean=None, coef=None, accumulate=True):
    if coef is None:
        return DE.slice_affine_bwd_acc(d, g, x, scale, shift, True, accumulate)
    p = DE._f32(d).reshape(g.shape)
    if scale is not None:
        p = p * DE._f32(scale)
    p = torch.where(DE.pre_activation32(x, scale, shift) > 0, p, torch.zeros(()))
    p = p + (DE._f32(x) - (DE._f32(mean) if mean is not None else 0.0)) * DE._f32(coef)
    g.copy_(g + p if accumulate else p)
    return g


def install(monkeypatch):
    from bcos_hip import ops
    for name in ("slice_batch_stats", "bn_reader_finish", "slice_relu_bwd_colsums", "slice_bn_bwd_acc"):
        monkeypatch.setattr(ops, name, globals()[name])
