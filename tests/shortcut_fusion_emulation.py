"""Torch interpreter of ops.shortcut_conv3_fwd (TEST INFRASTRUCTURE, beside cpu_emulation.py): what include/bcos_hip.h documents for
bcos_shortcut_conv3_fwd -- the results of the two forward launches it stands for, the shortcut's output rounded to fp32 as the first
launch stores it -- composed from cpu_emulation.tapconv.  The `-m "not gpu"` tests monkeypatch bcos_hip.ops with it on top of
cpu_emulation.install."""
import torch

import cpu_emulation
from bcos_hip.lib import BCOS_CONV_EPS


def shortcut_conv3_fwd(x, wd, h, w3, *, stride=1, csc_d=None, csh_d=None, csc_3=None, csh_3=None, want_scale=False, flags=0,
                       track_absmax=None, b=2.0, bias_d=None, bias_3=None, relu_gate=None, max_out=1, groups=1, contraction=None):
    from bcos_hip import ops
    N, H, W, kd = x.shape
    k3, c4, s = h.shape[-1], wd.shape[0], int(stride)
    assert (k3, kd, s, c4) in ((64, 64, 1, 256), (128, 256, 2, 512)) and b == 2.0 and max_out == 1 and groups == 1
    assert bias_d is None and bias_3 is None and relu_gate is None
    assert tuple(wd.shape) == (c4, 1, 1, kd) and tuple(w3.shape) == (c4, 1, 1, k3)
    gd = ops.fwd_geom(N, H, W, kd, c4, 1, 1, s, s, 0, 0)
    P, Q = gd["P"], gd["Q"]
    assert tuple(h.shape) == (N, P, Q, k3)
    idn = torch.empty((N, P, Q, c4), dtype=torch.float32)             # (fp32: what the shortcut launch stores)
    td = torch.empty_like(idn) if want_scale else None
    cpu_emulation.tapconv(x, wd, gd, out=idn, scale_out=td, ch_scale=csc_d, ch_shift=csh_d, bcos_mode=BCOS_CONV_EPS, b=b)
    out = torch.empty_like(idn)
    t3 = torch.empty_like(idn) if want_scale else None
    cpu_emulation.tapconv(h, w3, ops.fwd_geom(N, P, Q, k3, c4, 1, 1, 1, 1, 0, 0), out=out, scale_out=t3, ch_scale=csc_3, ch_shift=csh_3,
                          addend=idn, bcos_mode=BCOS_CONV_EPS, b=b, relu=True, flags=flags)
    if track_absmax is not False:
        ops._attach_absmax(out, out.reshape(-1, c4).abs().amax(1).view(torch.int32))
    return out, t3, td


def install(monkeypatch):
    """the emulator over bcos_hip.ops (after cpu_emulation.install).  The emulated launches emit no per-pixel maxima, and the engine
    asks for those of both inputs of the fused call: the emulated tapconv and stem pool therefore attach the real maxima of their
    output (ops._attach_absmax, what the device launches do) where they are asked to track them.  Nothing else is patched."""
    from bcos_hip import ops
    monkeypatch.setattr(ops, "shortcut_conv3_fwd", shortcut_conv3_fwd)
    inner = ops.tapconv

    def tapconv(a, wt, geom, **kw):
        inner(a, wt, geom, **kw)
        out = kw.get("out")
        if out is not None and kw.get("track_absmax") is not False and out.is_contiguous():
            ops._attach_absmax(out, out.reshape(-1, out.shape[-1]).abs().amax(1).view(torch.int32))
    monkeypatch.setattr(ops, "tapconv", tapconv)
    inner_pool = ops.avgpool2d_fwd

    def avgpool2d_fwd(x, k, s, p, out=None, want_absmax=False):
        y = inner_pool(x, k, s, p, out=out, want_absmax=want_absmax)
        if want_absmax:
            ops._attach_absmax(y, y.reshape(-1, y.shape[-1]).abs().amax(1).view(torch.int32))
        return y
    monkeypatch.setattr(ops, "avgpool2d_fwd", avgpool2d_fwd)
