"""Torch interpreter of ops.stem_conv_fwd (TEST INFRASTRUCTURE, beside cpu_emulation.py): what include/bcos_hip.h documents for
bcos_stem_conv_fwd -- the results of bcos_prep_input followed by the stem's forward launch -- composed from cpu_emulation.prep_input and
cpu_emulation.tapconv.  The `-m "not gpu"` tests monkeypatch bcos_hip.ops with it on top of cpu_emulation.install."""
import torch

import cpu_emulation
from bcos_hip.lib import BCOS_CONV_EPS


def stem_conv_fwd(x_nchw, w, mean6, std6, *, add_inverse=False, ch_scale=None, ch_shift=None, relu=True, want_scale=False, want_norm=False,
                  flags=0, track_absmax=None, b=2.0, bias=None, relu_gate=None, max_out=1, groups=1, contraction=None):
    from bcos_hip import ops
    assert tuple(w.shape) == (64, 7, 7, 8) and x_nchw.shape[1] == (3 if add_inverse else 6)
    assert b == 2.0 and max_out == 1 and groups == 1 and bias is None and relu_gate is None
    xn = cpu_emulation.prep_input(x_nchw, mean6, std6, cpad=8, add_inverse=add_inverse)
    N, H, W, _ = xn.shape
    g = ops.fwd_geom(N, H, W, 8, 64, 7, 7, 2, 2, 3, 3)
    y = torch.empty((N, g["P"], g["Q"], 64), dtype=torch.float32)
    t = torch.empty_like(y) if want_scale else None
    norm = torch.empty((N, g["P"], g["Q"]), dtype=torch.float32) if want_norm else None
    cpu_emulation.tapconv(xn, w, g, out=y, scale_out=t, norm_out=norm, ch_scale=ch_scale, ch_shift=ch_shift, bcos_mode=BCOS_CONV_EPS, b=b,
                          relu=relu, flags=flags)
    return y, t, norm


def install(monkeypatch):
    """the emulator over bcos_hip.ops (after cpu_emulation.install); nothing else is patched"""
    from bcos_hip import ops
    monkeypatch.setattr(ops, "stem_conv_fwd", stem_conv_fwd)
