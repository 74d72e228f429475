"""`-m gpu`: bcos_shortcut_conv3_fwd (include/bcos_hip.h) against the two forward launches it replaces -- bit for bit -- and the engine
with the fusion on and off.

The reference is the library's own pair (ops.conv2d_fwd for the shortcut, ops.conv2d_fwd with addend / ReLU / gate bit for conv3), so
every comparison is torch.equal: out, t3, td and the per-pixel maxima of out.  Every output of the C call sits between NaN / -1 canaries
that must survive.  Shapes against the 64-row tile: rows of two images in a tile and a ragged last tile, less than one tile, several
tiles; the stride-2 inputs have odd and even extents."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 256
# (K3, Kd, stride, C4) -> (N, H, W) of the block input
CASES = [((64, 64, 1, 256), s) for s in ((3, 9, 7), (1, 5, 5), (2, 19, 10))] + \
        [((128, 256, 2, 512), s) for s in ((2, 11, 9), (1, 5, 5), (3, 10, 14))]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


class Canary:
    """an output buffer between NaN (float) / -1 (maxima) canaries, itself filled with the canary value"""

    def __init__(self, numel, dtype=torch.float32):
        self.numel = numel
        self.buf = torch.full((PAD + numel + PAD,), float("nan") if dtype == torch.float32 else -1, device=DEV, dtype=dtype)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * PAD

    def take(self):
        for edge in (self.buf[:PAD], self.buf[PAD + self.numel:]):
            assert bool(torch.isnan(edge).all() if edge.dtype == torch.float32 else (edge == -1).all()), "canary overwritten"
        return self.buf[PAD:PAD + self.numel].clone()


_INPUTS = {}


def make_inputs(cfg, shape):
    """seeded operands (made once per case, never modified): activations over several decades with all-zero pixels, static banks"""
    from bcos_hip import ops
    if (cfg, shape) in _INPUTS:
        return _INPUTS[(cfg, shape)]
    (k3, kd, s, c4), (N, H, W) = cfg, shape
    P, Q = (H + s - 1) // s, (W + s - 1) // s
    gen = torch.Generator().manual_seed(1000 * k3 + 100 * N + 10 * H + W)
    rnd = lambda *sh: torch.randn(*sh, generator=gen)      # noqa: E731
    x = rnd(N, H, W, kd) * torch.exp2(torch.randint(-8, 4, (N, H, W, 1), generator=gen).float())
    h = rnd(N, P, Q, k3).abs() * torch.exp2(torch.randint(-8, 4, (N, P, Q, 1), generator=gen).float())
    x[0, 0, 0] = 0                    # on the stride grid: the shortcut's patch norm is sqrt(1e-6)
    x[-1, -1 - (H - 1) % s, -1 - (W - 1) % s] = 0
    h[0, 0, 0] = 0
    h[-1, -1, -1] = 0
    wd = rnd(c4, 1, 1, kd) * 0.2 * torch.exp2(torch.randint(-3, 3, (c4, 1, 1, 1), generator=gen).float())
    w3 = rnd(c4, 1, 1, k3) * 0.2 * torch.exp2(torch.randint(-3, 3, (c4, 1, 1, 1), generator=gen).float())
    d = lambda t: t.to(DEV).contiguous()                   # noqa: E731
    t = dict(x=ops.ensure_absmax(d(x)), h=ops.ensure_absmax(d(h)), wd=ops.mark_static(d(wd)), w3=ops.mark_static(d(w3)),
             csc_d=d(rnd(c4) * 0.5 + 1.0), csh_d=d(rnd(c4) * 0.1), csc_3=d(rnd(c4) * 0.5 + 1.0), csh_3=d(rnd(c4) * 0.1),
             stride=s, P=P, Q=Q)
    _INPUTS[(cfg, shape)] = t
    return t


def pair(t, keep, track):
    """the two launches the engine issues today"""
    from bcos_hip import lib as L, ops
    s = t["stride"]
    idn, td, _ = ops.conv2d_fwd(t["x"], t["wd"], stride=(s, s), ch_scale=t["csc_d"], ch_shift=t["csh_d"], want_scale=keep, track_absmax=False)
    out, t3, _ = ops.conv2d_fwd(t["h"], t["w3"], ch_scale=t["csc_3"], ch_shift=t["csh_3"], addend=idn, relu=True, want_scale=keep,
                                flags=L.BCOS_EPI_SCALE_GATE_LSB if keep else 0, track_absmax=track)
    return out, t3, td, ops.absmax_of(out)


@pytest.mark.parametrize("track", [True, False], ids=["maxima", "nomaxima"])
@pytest.mark.parametrize("keep", [True, False], ids=["kept", "fwdonly"])
@pytest.mark.parametrize("cfg,shape", CASES, ids=[f"k{c[0]}s{c[2]}-{'x'.join(map(str, s))}" for c, s in CASES])
def test_fused_call_equals_the_two_launches(lib, cfg, shape, keep, track):
    from bcos_hip import lib as L, ops
    assert L.get_contraction_mode() == "f16x2"
    t = make_inputs(cfg, shape)
    (k3, kd, s, c4), (N, H, W) = cfg, shape
    out_r, t3_r, td_r, am_r = pair(t, keep, track)
    frac = float((out_r > 0).float().mean())
    assert 0.1 <= frac <= 0.9, frac                  # both ReLU outcomes
    assert (am_r is not None) == track
    flags = L.BCOS_EPI_SCALE_GATE_LSB if keep else 0
    # through the binding: allocation, maxima attached as tapconv attaches them
    out, t3, td = ops.shortcut_conv3_fwd(t["x"], t["wd"], t["h"], t["w3"], stride=s, csc_d=t["csc_d"], csh_d=t["csh_d"], csc_3=t["csc_3"],
                                         csh_3=t["csh_3"], want_scale=keep, flags=flags, track_absmax=track)
    assert torch.equal(out, out_r) and (ops.absmax_of(out) is not None) == track
    if track:
        assert torch.equal(ops.absmax_of(out), am_r)
    assert (t3 is None and td is None) if not keep else (torch.equal(t3, t3_r) and torch.equal(td, td_r))
    if keep:
        assert bool(((t3.view(torch.int32) & 1) == 1)[out > 0].all()) and bool((t3[out == 0] == 0).all())      # the gate bit
    # through the C ABI with every output between canaries
    M = N * t["P"] * t["Q"]
    c_out, c_t3, c_td, c_am = Canary(M * c4), Canary(M * c4), Canary(M * c4), Canary(M, torch.int32)
    a = L.ShortcutConv3()
    for k in ("x", "h", "csc_d", "csh_d", "csc_3", "csh_3"):
        setattr(a, k, t[k].data_ptr())
    a.x_absmax, a.h_absmax = ops.absmax_of(t["x"]).data_ptr(), ops.absmax_of(t["h"]).data_ptr()
    a.wd_f16x2, a.w3_f16x2 = t["wd"]._bcos_wt2_t1[1].data_ptr(), t["w3"]._bcos_wt2_t1[1].data_ptr()
    a.out = c_out.ptr
    if keep:
        a.t3, a.td = c_t3.ptr, c_td.ptr
    if track:
        a.out_absmax = c_am.ptr
    a.N, a.H, a.W, a.K3, a.Kd, a.C4, a.kh, a.kw, a.stride = N, H, W, k3, kd, c4, 1, 1, s
    a.max_out, a.groups, a.contraction, a.flags, a.b = 1, 1, L.CONTRACT_F16X2, flags, 2.0
    L.check(lib.bcos_shortcut_conv3_fwd(C.byref(a), ops._stream()), "bcos_shortcut_conv3_fwd")
    torch.cuda.synchronize()
    assert torch.equal(c_out.take().view_as(out_r), out_r)
    got_t3, got_td, got_am = c_t3.take(), c_td.take(), c_am.take()
    if keep:
        assert torch.equal(got_t3.view_as(t3_r), t3_r) and torch.equal(got_td.view_as(td_r), td_r)
    else:
        assert bool(torch.isnan(got_t3).all()) and bool(torch.isnan(got_td).all())
    assert torch.equal(got_am, am_r) if track else bool((got_am == -1).all())


@pytest.mark.parametrize("sites", [1, 2], ids=["default", "both-configs"])
def test_engine_fusion_on_off_equal_and_counted(lib, monkeypatch, sites):
    """by default the engine fuses layer1.0 only (layer2.0 measured no gain, layer3.0 / layer4.0 are not supported by the call); with
    both supported configurations handed to it, layer2.0 too"""
    from bcos_hip import engine, passes, synth
    if sites == 2:
        monkeypatch.setattr(engine, "_SHORTCUT_CONFIGS", ((64, 64, 1, 256), (128, 256, 2, 512)))
    net = synth.build_bcosified_resnet("resnet50").to(DEV)
    x = synth.synthetic_images(3, size=64, seed=7).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, x)
    eng = engine.attach(net)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 1)
    try:
        for streams in (1, 2):
            eng.subbatch_streams = streams
            res = {}
            for on in (False, True):
                engine.set_shortcut_fusion(on)
                engine.SHORTCUT_FUSION_CALLS = engine.BOUNDARY_FUSION_CALLS = 0
                with torch.no_grad():
                    logits = eng.forward(x)
                n_fwd = engine.SHORTCUT_FUSION_CALLS
                out = eng.explain(x, want_weights=True)
                res[on] = (logits, out, n_fwd, engine.SHORTCUT_FUSION_CALLS - n_fwd, engine.BOUNDARY_FUSION_CALLS)
            (l0, o0, f0, e0, b0), (l1, o1, f1, e1, b1) = res[False], res[True]
            assert (f0, e0) == (0, 0) and (f1, e1) == (sites * streams, sites * streams) and b0 == b1
            assert torch.equal(l0, l1) and set(o0) == set(o1)
            for k, v in o1.items():
                assert torch.equal(v, o0[k]), (streams, k)
    finally:
        engine.set_shortcut_fusion(None)
