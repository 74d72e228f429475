"""`-m gpu`: bcos_stem_conv_fwd (include/bcos_hip.h) against the two launches it replaces -- bit for bit -- and the engine with the
fused stem launch on and off.

The reference is the library's own pair (ops.prep_input, then ops.conv2d_fwd on the prepared copy), so every comparison is torch.equal:
y, t, the patch norms and the per-pixel maxima of y.  Every output of the C call sits between NaN / -1 canaries that must survive, and
arrays not asked for keep their fill.  Shapes against the 16 x 16 tile of output pixels: 38 x 38 images give a 19 x 19 output (ragged
tiles in both directions), 20 x 150 images a 10 x 75 output (one partial row of tiles, four full column tiles and a partial one).
Inputs: `rgb` 3 channels with AddInverse and the ImageNet statistics; `six` 6 channels; `six0` 6 channels with mean 0, so that the
all-zero region of image 0 gives rows whose operand maximum is zero -- and image 2 of it holds one pixel 2^-23 below the rest, which
sends that image from the per-image operand scale to the per-row one (tile_body_d's rule, both sides of it)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 256
SHAPES = [(3, 38, 38), (3, 20, 150)]
KINDS = ["rgb", "six", "six0"]
MODES = ["kept", "rebuild", "fwdonly"]      # t stored | the patch norms (the multiplier is rebuilt from y) | neither


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


def make_inputs(kind, shape):
    """seeded operands (made once per case, never modified)"""
    from bcos_hip import ops
    if (kind, shape) in _INPUTS:
        return _INPUTS[(kind, shape)]
    N, H, W = shape
    cx = 3 if kind == "rgb" else 6
    gen = torch.Generator().manual_seed(100 * H + W + len(kind))
    x = torch.rand(N, cx, H, W, generator=gen)
    x[0, :, 2:18, 4:24] = 0                  # larger than a 7 x 7 window
    x[1, :, 0, 0] = 0
    x[1, :, 1, 1] = 1
    x[-1, :, -1, -1] = 1
    x[-1, :, -1, 0] = 0
    if kind == "six0":
        x[2, :, 5, 5] = 2.0 ** -23
    mean = torch.tensor([0.485, 0.456, 0.406, 0.515, 0.544, 0.594]) if kind != "six0" else torch.zeros(6)
    std = torch.tensor([0.229, 0.224, 0.225, 0.229, 0.224, 0.225])
    w = torch.randn(64, 7, 7, 8, generator=gen) * 0.1 * torch.exp2(torch.randint(-3, 3, (64, 1, 1, 1), generator=gen).float())
    w[..., 6:] = 0                            # the two padding channels, as the engine builds the bank
    d = lambda t: t.to(DEV).contiguous()      # noqa: E731
    t = dict(x=d(x), mean=d(mean), std=d(std), w=ops.mark_static(d(w)), csc=d(torch.randn(64, generator=gen) * 0.5 + 1.0),
             csh=d(torch.randn(64, generator=gen) * 0.1), add_inverse=cx == 3, P=(H - 1) // 2 + 1, Q=(W - 1) // 2 + 1)
    _INPUTS[(kind, shape)] = t
    return t


def pair(t, mode, track):
    """the two launches the engine issues without the fused call"""
    from bcos_hip import ops
    xn = ops.prep_input(t["x"], t["mean"], t["std"], cpad=8, add_inverse=t["add_inverse"], want_absmax=True)
    y, sc, nrm = ops.conv2d_fwd(xn, t["w"], stride=(2, 2), padding=(3, 3), ch_scale=t["csc"], ch_shift=t["csh"], relu=True,
                                want_scale=mode == "kept", want_norm=mode == "rebuild", track_absmax=track)
    return xn, y, sc, nrm, ops.absmax_of(y)


def fused(t, mode, track):
    from bcos_hip import ops
    y, sc, nrm = ops.stem_conv_fwd(t["x"], t["w"], t["mean"], t["std"], add_inverse=t["add_inverse"], ch_scale=t["csc"], ch_shift=t["csh"],
                                   relu=True, want_scale=mode == "kept", want_norm=mode == "rebuild", track_absmax=track)
    return y, sc, nrm, ops.absmax_of(y)


def assert_same(got, ref):
    for name, g, r in zip(("y", "t", "norm", "maxima"), got, ref):
        assert (g is None) == (r is None), name
        assert g is None or torch.equal(g, r), name


@pytest.mark.parametrize("track", [True, False], ids=["maxima", "nomaxima"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_fused_call_equals_the_two_launches(lib, shape, kind, mode, track):
    from bcos_hip import lib as L, ops
    assert L.get_contraction_mode() == "f16x2"
    t = make_inputs(kind, shape)
    N, H, W = shape
    xn, y_r, t_r, n_r, am_r = pair(t, mode, track)
    frac = float((y_r > 0).float().mean())
    assert 0.1 <= frac <= 0.9, frac                      # both ReLU outcomes: closed gates are present
    assert (am_r is not None) == track
    am_x = ops.absmax_of(xn)
    if kind == "six0":
        assert int((am_x.view(N, H, W)[0, 2:18, 4:24] != 0).sum()) == 0          # rows whose 49 taps are all zero: the zero-maximum scale
        assert bool((y_r[0, 3:7, 4:10] == t["csh"].clamp(min=0)).all())          # lin = 0 there: what the shift and the ReLU leave
    assert bool((t["x"][1, :, 0, 0] == 0).all()) and bool((t["x"][1, :, 1, 1] == 1).all())      # pixels at 0 and 1 exactly
    # through the binding
    assert_same(fused(t, mode, track), (y_r, t_r, n_r, am_r))
    # through the C ABI with every output between canaries; the operand-scale rule of the reference (no arena: the per-image range)
    M = N * t["P"] * t["Q"]
    c_y, c_t, c_n, c_am = Canary(M * 64), Canary(M * 64), Canary(M), Canary(M, torch.int32)
    rng = torch.empty(2, N, device=DEV, dtype=torch.int32)
    L.check(lib.bcos_stem_image_range(t["x"].data_ptr(), t["mean"].data_ptr(), t["std"].data_ptr(), rng[0].data_ptr(), rng[1].data_ptr(),
                                      N, t["x"].shape[1], H, W, int(t["add_inverse"]), ops._stream()), "bcos_stem_image_range")
    ref_rng, _ = ops.image_absmax(am_x, N, H * W)
    assert torch.equal(rng, ref_rng)
    a = L.StemConv()
    a.x, a.mean6, a.std6, a.csc, a.csh = (t[k].data_ptr() for k in ("x", "mean", "std", "csc", "csh"))
    a.w_f16x2 = t["w"]._bcos_wt2_t49[1].data_ptr()
    a.x_imgmax, a.x_imgmin = rng[0].data_ptr(), rng[1].data_ptr()
    a.y = c_y.ptr
    if mode == "kept":
        a.t = c_t.ptr
    if mode == "rebuild":
        a.norm_out = c_n.ptr
    if track:
        a.y_absmax = c_am.ptr
    a.N, a.Cx, a.H, a.W, a.add_inverse = N, t["x"].shape[1], H, W, int(t["add_inverse"])
    a.Cout, a.kh, a.kw, a.stride, a.padding, a.relu = 64, 7, 7, 2, 3, 1
    a.max_out, a.groups, a.contraction, a.flags, a.b = 1, 1, L.CONTRACT_F16X2, 0, 2.0
    L.check(lib.bcos_stem_conv_fwd(C.byref(a), ops._stream()), "bcos_stem_conv_fwd")
    torch.cuda.synchronize()
    assert torch.equal(c_y.take().view_as(y_r), y_r)
    got_t, got_n, got_am = c_t.take(), c_n.take(), c_am.take()
    assert torch.equal(got_t.view_as(y_r), t_r) if mode == "kept" else bool(torch.isnan(got_t).all())
    assert torch.equal(got_n.view_as(n_r), n_r) if mode == "rebuild" else bool(torch.isnan(got_n).all())
    assert torch.equal(got_am, am_r) if track else bool((got_am == -1).all())


@pytest.mark.parametrize("kind", KINDS)
def test_per_row_scales_inside_an_engine_pass(lib, kind):
    """with an engine's arena and images of 2048 pixels and more the tapconv launch is handed no plain per-image range and scans every
    row's taps: the fused call then computes none either"""
    from bcos_hip import ops
    t = make_inputs(kind, SHAPES[1])
    with ops.absmax_arena(ops.AbsmaxArena(), DEV):
        ref = pair(t, "kept", True)[1:]
        ref = tuple(None if v is None else v.clone() for v in ref)
    with ops.absmax_arena(ops.AbsmaxArena(), DEV):
        got = tuple(None if v is None else v.clone() for v in fused(t, "kept", True))
    assert_same(got, ref)


def test_gate_bit_and_no_relu(lib):
    from bcos_hip import lib as L, ops
    t = make_inputs("rgb", SHAPES[0])
    xn = ops.prep_input(t["x"], t["mean"], t["std"], cpad=8, add_inverse=True, want_absmax=True)
    for relu, flags in ((True, L.BCOS_EPI_SCALE_GATE_LSB), (False, 0)):
        y_r, t_r, _ = ops.conv2d_fwd(xn, t["w"], stride=(2, 2), padding=(3, 3), ch_scale=t["csc"], ch_shift=t["csh"], relu=relu,
                                     want_scale=True, flags=flags, track_absmax=False)
        y, sc, _ = ops.stem_conv_fwd(t["x"], t["w"], t["mean"], t["std"], add_inverse=True, ch_scale=t["csc"], ch_shift=t["csh"], relu=relu,
                                     want_scale=True, flags=flags, track_absmax=False)
        assert torch.equal(y, y_r) and torch.equal(sc, t_r), relu
        if relu:
            assert bool(((sc.view(torch.int32) & 1) == 1)[y > 0].all()) and bool((sc[y == 0] == 0).all())
        else:
            assert bool((y < 0).any())


@pytest.mark.parametrize("arch", ["resnet50", "resnet18"])
def test_engine_stem_kernel_on_off_equal_and_counted(lib, monkeypatch, arch):
    from bcos_hip import engine, ops, passes, synth
    net = synth.build_bcosified_resnet(arch).to(DEV)
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
                engine.set_stem_kernel(on)
                engine.STEM_KERNEL_CALLS = 0
                with torch.no_grad():
                    logits = eng.forward(x)
                n_fwd = engine.STEM_KERNEL_CALLS
                out = eng.explain(x, want_weights=True)
                torch.cuda.synchronize()
                res[on] = (logits, out, n_fwd, engine.STEM_KERNEL_CALLS - n_fwd)
            (l0, o0, f0, e0), (l1, o1, f1, e1) = res[False], res[True]
            assert (f0, e0) == (0, 0) and (f1, e1) == (streams, streams)          # one call per pass
            assert torch.equal(l0, l1) and set(o0) == set(o1)
            for k, v in o1.items():
                assert torch.equal(v, o0[k]), (streams, k)
        # the per-contraction timing records: as many as with the pair, the same flops; the bytes of the padded copy the tapconv launch
        # books as its A operand (ops.tapconv books no read of the maxima) become those of the raw image
        eng.subbatch_streams = 1
        recs = {}
        for on in (False, True):
            engine.set_stem_kernel(on)
            ops.KERNEL_TIMING = []
            try:
                eng.explain(x)
                torch.cuda.synchronize()
                recs[on] = ops.KERNEL_TIMING
            finally:
                ops.KERNEL_TIMING = None
        assert len(recs[True]) == len(recs[False]) and sum(r[2] for r in recs[True]) == sum(r[2] for r in recs[False])
        N, cx, H, W = x.shape
        assert sum(r[3] for r in recs[False]) - sum(r[3] for r in recs[True]) == 4 * N * H * W * 8 - 4 * N * cx * H * W
    finally:
        engine.set_stem_kernel(None)


def test_clip_stem_keeps_its_launches(lib):
    """CLIP's ModifiedResNet has a 3-conv stem: no call"""
    from bcos_hip import engine, synth
    net = synth.build_bcosified_clip_rn50().to(DEV).eval()
    x = synth.synthetic_images(2, size=224, seed=3).to(DEV)
    eng = engine.attach(net)
    engine.set_stem_kernel(True)
    try:
        engine.STEM_KERNEL_CALLS = 0
        with torch.no_grad():
            eng.forward(x)
        assert engine.STEM_KERNEL_CALLS == 0 and len(eng.stem) == 3
    finally:
        engine.set_stem_kernel(None)
