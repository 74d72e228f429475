"""CPU restatements of the dense-block entry points (TEST INFRASTRUCTURE, beside cpu_emulation.py): what include/bcos_hip.h documents for
bcos_slice_affine_rows and bcos_slice_affine_bwd_acc.  `slice_affine_rows64` / `slice_affine_bwd_acc64` evaluate the documented maps in
float64 and return the header's rounding bounds as formulas of the INPUTS; the fp32 forms reproduce the documented order of roundings
(product, sum, [max], [product]) with torch's fp32 arithmetic, which is what the gate of the backward map is defined by.  The
`-m "not gpu"` tests monkeypatch bcos_hip.ops with `slice_affine_rows` / `slice_affine_bwd_acc`; the GPU tests judge the kernels against
all of it."""
import torch

ULP = 2.0 ** -23


def _f32(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().float()


def pre_activation32(x, scale=None, shift=None):
    """fl(fl(x * scale) + shift) in fp32: the value whose sign is the ReLU's decision in both entry points"""
    v = _f32(x).clone()
    if scale is not None:
        v = v * _f32(scale)
    if shift is not None:
        v = v + _f32(shift)
    return v


def slice_affine_rows32(x, scale=None, shift=None, mul=None, relu=False):
    """-> (y fp32 with the documented roundings, row maxima as int32 bit patterns)"""
    v = pre_activation32(x, scale, shift)
    if relu:
        v = torch.where(v > 0, v, torch.zeros(()))          # (fmaxf(v, 0): NaN and -0 become +0)
    if mul is not None:
        v = v * _f32(mul).reshape(v.shape)
    am = v.abs().reshape(-1, v.shape[-1]).amax(1).contiguous().view(torch.int32)
    return v, am


def slice_affine_rows64(x, scale=None, shift=None, mul=None, relu=False):
    """-> (y64, bound, y64_pre): y64 = the documented map in float64 from the fp32 inputs (the ReLU decided as the header defines it, on
    the fp32 pre-activation); bound = 2^-23 (|x scale| + |x scale + shift|) |mul|, which covers the three roundings (product 2^-24 |x s|,
    sum 2^-24 |v|, mul 2^-24 |y|) -- a sum that cancels keeps the product's rounding error, so no bound relative to y alone exists with
    a shift; y64_pre = float64(fp32 pre-activation, after the ReLU) * mul, from which the kernel's value is ONE rounding away."""
    xs = _f32(x).double()
    if scale is not None:
        xs = xs * _f32(scale).double()
    v = xs + _f32(shift).double() if shift is not None else xs
    pre = pre_activation32(x, scale, shift)
    if relu:
        v = torch.where(pre > 0, v, torch.zeros((), dtype=torch.float64))
        pre = torch.where(pre > 0, pre, torch.zeros(()))
    m = _f32(mul).double().reshape(v.shape) if mul is not None else torch.ones((), dtype=torch.float64)
    return v * m, ULP * (xs.abs() + v.abs()) * m.abs() + 2.0 ** -149, pre.double() * m


def slice_affine_bwd_acc64(d, g_old, x=None, scale=None, shift=None, relu=False, accumulate=True):
    """-> (g in float64, per-element bound 2^-23 (|g_old| + |d scale|) of include/bcos_hip.h, gate as bool)"""
    p = _f32(d).double()
    if scale is not None:
        p = p * _f32(scale).double()
    gate = torch.ones_like(p, dtype=torch.bool)
    if relu:
        gate = (pre_activation32(x, scale, shift) > 0).reshape(p.shape)
        p = torch.where(gate, p, torch.zeros((), dtype=torch.float64))
    old = _f32(g_old).double().reshape(p.shape) if accumulate else torch.zeros_like(p)
    return old + p, ULP * (old.abs() + p.abs()) + 2.0 ** -149, gate


# ---- stand-ins for the bcos_hip.ops wrappers (same signatures) ---------------------------------------------------------------------
def slice_affine_rows(x, scale=None, shift=None, mul=None, relu=False, out=None, want_absmax=True):
    y, am = slice_affine_rows32(x, scale, shift, mul, relu)
    if out is None:
        return y.contiguous()
    out.copy_(y)
    return out, (am if want_absmax else None)


def slice_affine_bwd_acc(d, g, x=None, scale=None, shift=None, relu=False, accumulate=True):
    p = _f32(d).reshape(g.shape)
    if scale is not None:
        p = p * _f32(scale)
    if relu:
        p = torch.where(pre_activation32(x, scale, shift) > 0, p, torch.zeros(()))
    g.copy_(g + p if accumulate else p)
    return g


def install(monkeypatch):
    from bcos_hip import ops
    monkeypatch.setattr(ops, "slice_affine_rows", slice_affine_rows)
    monkeypatch.setattr(ops, "slice_affine_bwd_acc", slice_affine_bwd_acc)
