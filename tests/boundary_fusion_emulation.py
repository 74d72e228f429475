"""Torch interpreter of ops.boundary_conv3_grad (TEST INFRASTRUCTURE, beside cpu_emulation.py): what include/bcos_hip.h documents for
bcos_boundary_conv3_grad -- the results of the two launches it stands for, the tensor between them rounded to fp32 as the first launch
stores it -- composed from cpu_emulation.tapconv.  The `-m "not gpu"` tests monkeypatch bcos_hip.ops with it on top of
cpu_emulation.install."""
import torch

import cpu_emulation
from bcos_hip.lib import BCOS_EPI_GATE2_FROM_MUL, BCOS_EPI_MUL_FROM_ACT


def _geom(N, H, W, cin, cout):
    return dict(N=N, H=H, W=W, C=cin, P=H, Q=W, in_sh=1, in_sw=1, dh0=0, dw0=0, dstep_h=1, dstep_w=1, TH=1, TW=1, OH=H, OW=W,
                out_sh=1, out_sw=1, out_h0=0, out_w0=0, Cout=cout)


def boundary_conv3_grad(g1, w1t, addend, t3, w3t, t2, *, mul2=None, mul_norm=None, mul_csc=None, mul_csh=None, track_absmax=None,
                        track_absmax2=None, b=2.0, contraction=None):
    N, H, W, c1 = g1.shape
    c4 = addend.shape[-1]
    assert tuple(w1t.shape) == (c4, 1, 1, c1) and tuple(w3t.shape) == (c1, 1, 1, c4) and (c1, c4) == (64, 256) and b == 2.0
    G = torch.empty((N, H, W, c4), dtype=torch.float32)
    out2 = torch.empty((N, H, W, c4), dtype=torch.float32)
    cpu_emulation.tapconv(g1, w1t, _geom(N, H, W, c1, c4), out=G, out2=out2, addend=addend, mul=t3, mul2=mul2, flags=BCOS_EPI_GATE2_FROM_MUL)
    g3 = torch.empty((N, H, W, c1), dtype=torch.float32)
    kw = dict(mul_norm=mul_norm, mul_csc=mul_csc, mul_csh=mul_csh, flags=BCOS_EPI_MUL_FROM_ACT) if mul_norm is not None else {}
    cpu_emulation.tapconv(G, w3t, _geom(N, H, W, c4, c1), out=g3, mul=t2, **kw)
    return g3, out2


def install(monkeypatch):
    """the emulator over bcos_hip.ops (after cpu_emulation.install).  The emulated launches emit no per-pixel maxima, and the engine
    asks for those of the gradient it hands to the fused call: the emulated tapconv therefore attaches the real maxima of `out`
    (ops._attach_absmax, what the device launch does) where a launch is asked to track them.  Nothing else is patched."""
    from bcos_hip import ops
    monkeypatch.setattr(ops, "boundary_conv3_grad", boundary_conv3_grad)
    inner = ops.tapconv

    def tapconv(a, wt, geom, **kw):
        inner(a, wt, geom, **kw)
        out = kw.get("out")
        if out is not None and kw.get("track_absmax") is not False and out.is_contiguous():
            ops._attach_absmax(out, out.reshape(-1, out.shape[-1]).abs().amax(1).view(torch.int32))
    monkeypatch.setattr(ops, "tapconv", tapconv)
