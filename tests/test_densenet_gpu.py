"""`-m gpu`: the two dense-block kernels against their restatement (tests/densenet_emulation.py) and against bcos_channel_affine_rows,
and the B-cosified DenseNets against the fixtures recorded from the reference (tests/golden/make_golden_densenet.py).

Bounds.  Kernels: what include/bcos_hip.h states -- bits where it states bits, 2 fp32 ulps for the `mul` stage, 2^-23 (|g_old| + |d scale|)
for the accumulation.  Networks: logits 1e-4 relative L2, classes exact, W(x) and maps max(1e-4, 3 d_ref) with the fixture's recorded
fp32-vs-fp64 distance d_ref of the reference (1.7e-6 for DenseNet-121, so the bound evaluates to 1e-4), in relative L2 and in the worst
element per image over the map's peak; completeness |sum m - (logit - logit_bias)| <= 1e-4 sum |m| per image on our own output."""
import itertools

import pytest
import torch

import densenet_cases as DC
import densenet_emulation as DE

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = 197
CHANNELS = (4, 36, 104, 256)          # lanes per row 1, 64 (looping, C / 4 = 9), 64 (26), 64 (exactly one pass)
MODES = ("f32", "bf16x3", "f16x2")


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _pitches(C):
    return [(xp, yp) for xp in (C, C + 28, 1024) for yp in (0, C + 8)]


def _inputs(C, seed):
    """rows of random values with, in channels 0..3 of the first rows, inputs whose pre-activation x * scale + shift rounds to +0, -0,
    the smallest normals of either sign and subnormals (the decisions a gate rebuilt with another rounding would get wrong)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, C, generator=g)
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    shift = torch.randn(C, generator=g) * 0.5
    tiny, sub = 2.0 ** -126, 2.0 ** -149
    scale[:4] = torch.tensor([0.5, 1.0, 0.5, 1.0])
    shift[:4] = torch.tensor([-1.0, 0.0, 0.0, tiny])
    x[:5, 0] = torch.tensor([2.0, 2.0 + 2.0 ** -22, 2.0 - 2.0 ** -22, -2.0, 0.0])           # +0, 2^-23, -2^-23, -2, -1
    x[:5, 1] = torch.tensor([tiny, -tiny, tiny / 2, -0.0, 0.0])                              # smallest normals, a subnormal, -0, +0
    x[:5, 2] = torch.tensor([tiny, sub, -sub, 3 * sub, -tiny])                               # 2^-127, ties to +0, to -0, 2^-149 * 2, -2^-127
    x[:5, 3] = torch.tensor([-tiny, -tiny / 2, -2 * tiny, sub - tiny, 0.0])                  # +0, 2^-127, -2^-126, 2^-149, 2^-126
    mul = torch.randn(ROWS, C, generator=g)
    d = (torch.rand(ROWS, C, generator=g) + 0.5) * torch.where(torch.rand(ROWS, C, generator=g) < 0.5, -1.0, 1.0)
    g_old = torch.randn(ROWS, C, generator=g)
    return x, scale, shift, mul, d, g_old


def _pitched(values, pitch):
    """[ROWS, pitch] NaN canvas on the device with `values` in channels [0, C) -> (canvas, its slice)"""
    C = values.shape[1]
    canvas = torch.full((ROWS, pitch), float("nan"), device=DEV)
    canvas[:, :C] = values.to(DEV)
    return canvas, canvas[:, :C]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("C", CHANNELS)
def test_slice_affine_rows(lib, C):
    from bcos_hip import ops
    x, scale, shift, mul, _, _ = _inputs(C, seed=C)
    for (xp, yp), (has_sc, has_sh, has_mul, relu) in itertools.product(_pitches(C), itertools.product((False, True), repeat=4)):
        what = (C, xp, yp, has_sc, has_sh, has_mul, relu)
        X, xs = _pitched(x, xp)
        X0 = X.clone()
        sc, sh, mu = (scale.to(DEV) if has_sc else None), (shift.to(DEV) if has_sh else None), (mul.to(DEV) if has_mul else None)
        if yp:
            Y = torch.full((ROWS, yp), float("nan"), device=DEV)
            y, am = ops.slice_affine_rows(xs, sc, sh, mu, relu=relu, out=Y[:, :C])
            assert bool(Y[:, C:].isnan().all()), what                         # canaries behind every output row
        else:
            y = ops.slice_affine_rows(xs, sc, sh, mu, relu=relu)
            am = ops.absmax_of(y)
            assert y.is_contiguous() and am is not None, what
        assert _same_bits(X, X0), what                                        # x is only read
        y, am = y.cpu(), am.cpu()
        assert not bool(y.isnan().any()), what                                # (a read outside [0, C) would have met a NaN)
        want, want_am = DE.slice_affine_rows32(x, scale if has_sc else None, shift if has_sh else None, mul if has_mul else None, relu)
        assert torch.equal(am, want_am), what                                  # row maxima: bits
        y64, bound, y64_pre = DE.slice_affine_rows64(x, scale if has_sc else None, shift if has_sh else None, mul if has_mul else None, relu)
        assert bool(((y.double() - y64).abs() <= bound).all()), what
        if has_mul:
            # 2 fp32 ulps of the float64 value: of the whole map where no sum can cancel (no shift), of float64(pre-activation) * mul
            # otherwise (the pre-activation itself is held to bits below)
            ref = y64 if not has_sh else y64_pre
            assert bool(((y.double() - ref).abs() <= 2 * DE.ULP * ref.abs() + 2.0 ** -149).all()), what
        else:
            assert torch.equal(y, want), what                                  # values (a ReLU may leave either zero)
            if not relu:
                assert _same_bits(y, want), what
            if has_sc and not yp:
                twin = ops.channel_affine_rows(xs.contiguous(), sc, sh, None, relu=relu)
                assert _same_bits(y.to(DEV), twin) and torch.equal(am.to(DEV), ops.absmax_of(twin)), what


@pytest.mark.parametrize("C", CHANNELS)
def test_slice_affine_bwd_acc(lib, C):
    from bcos_hip import ops
    x, scale, shift, _, d, g_old = _inputs(C, seed=100 + C)
    dd = d.to(DEV)
    for (xp, gp), (has_sc, has_sh, relu, acc) in itertools.product(_pitches(C), itertools.product((False, True), repeat=4)):
        what = (C, xp, gp, has_sc, has_sh, relu, acc)
        X, xs = _pitched(x, xp)
        X0 = X.clone()
        sc, sh = (scale.to(DEV) if has_sc else None), (shift.to(DEV) if has_sh else None)
        pitch = gp or C
        G = torch.full((ROWS, pitch), float("nan"), device=DEV)               # accumulate = 0 must ignore what g holds: NaN everywhere
        if acc:
            G[:, :C] = g_old.to(DEV)
        ops.slice_affine_bwd_acc(dd, G[:, :C], xs if relu else None, sc, sh, relu=relu, accumulate=acc)
        assert _same_bits(X, X0) and _same_bits(dd.cpu(), d), what
        assert bool(G[:, C:].isnan().all()), what
        got = G[:, :C].cpu()
        assert not bool(got.isnan().any()), what
        g64, bound, gate = DE.slice_affine_bwd_acc64(d, g_old, x, scale if has_sc else None, shift if has_sh else None, relu, acc)
        assert bool(((got.double() - g64).abs() <= bound).all()), what
        if relu:
            # the gate is the forward KERNEL's own decision: y > 0 of bcos_slice_affine_rows on the same slice, element for element
            y = ops.slice_affine_rows(xs, sc, sh, None, relu=True).cpu()
            if not acc:
                assert torch.equal(got != 0, y > 0), what                      # (d and scale are nonzero: an open gate leaves a nonzero)
            else:
                assert torch.equal(got != g_old, y > 0), what                  # |d scale| >= 0.25 against |g_old| ~ 1: an open gate moves g
            assert torch.equal(gate, y > 0), what


def _on_device(stem):
    net, meta, data, x = DC.golden_net(stem)
    return net.to(DEV), meta, data, x.to(DEV)


@pytest.fixture(scope="module")
def tiny(lib):
    return _on_device("densenet_tiny")


@pytest.fixture(scope="module")
def d121(lib):
    return _on_device("densenet121_small")


@pytest.mark.parametrize("mode", MODES)
def test_densenet_tiny_module_path(tiny, mode):
    from bcos_hip import lib as blib
    net, meta, data, x = tiny
    prev = blib.get_contraction_mode()
    blib.set_contraction_mode(mode)
    try:
        with torch.no_grad():
            assert DC.rel(net(x), data["logits"]) <= 1e-4
        out = net.explain_batch(x)
    finally:
        blib.set_contraction_mode(prev)
    DC.check_against_fixture(out, data, 1e-4, 1e-4, f"densenet_tiny, module path, {mode}")
    assert float(DC.completeness_residual(x, out, meta["logit_bias"]).max()) <= 1e-4


def test_densenet121_module_path(d121):
    net, meta, data, x = d121
    bound = max(1e-4, 3 * max(meta["d_ref"]["weights"], meta["d_ref"]["maps"]))
    out = net.explain_batch(x)
    DC.check_against_fixture(out, data, 1e-4, bound, "densenet121_small, module path")
    resid = DC.completeness_residual(x, out, meta["logit_bias"])
    print("completeness", resid.tolist())
    assert float(resid.max()) <= 1e-4


def test_densenet121_reference_state_dict_loads_strictly(d121):
    """a B-cosified DenseNet-121 state dict with the reference's recorded keys and shapes loads with strict=True into the factory's net"""
    import warnings
    from bcos.experiments.ImageNet.bcosification.experiment_parameters import CONFIGS
    from bcos.experiments.ImageNet.bcosification.model import get_model
    net, meta, data, x = d121
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fresh = get_model(CONFIGS["densenet_121"]["model"]).to(DEV).eval()
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state_keys"]
    fresh.load_state_dict(sd, strict=True)
    with torch.no_grad():
        assert DC.rel(fresh(x), data["logits"]) <= 1e-4


def test_tiny_batch_of_64_equals_its_halves(tiny):
    """64 images of 64 x 64: the explanation of the batch carries the bits of the explanations of its two halves, and of a second call"""
    from bcos_hip import synth
    net, meta, data, _ = tiny
    x = synth.synthetic_images(64, seed=9, size=64).to(DEV)
    whole, again = net.explain_batch(x), net.explain_batch(x)
    lo, hi = net.explain_batch(x[:32]), net.explain_batch(x[32:])
    for k in ("logits", "dynamic_linear_weights", "contribution_map"):
        assert torch.equal(whole[k], again[k]), k
        assert torch.equal(whole[k], torch.cat([lo[k], hi[k]])), k


# ---- the fused plan (bcos_hip/densenet_engine.py) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_densenet_tiny_plan(tiny, mode):
    from bcos_hip import densenet_engine, lib as blib
    net, meta, data, x = tiny
    prev = blib.get_contraction_mode()
    blib.set_contraction_mode(mode)
    eng = densenet_engine.attach(net)
    try:
        with torch.no_grad():
            fwd = net(x)                              # forward-only pass: conv2 written into its slice through out_pitch
        out = net.explain_batch(x)                    # explanation pass: dense conv2 + placement
    finally:
        densenet_engine.detach(net)
        blib.set_contraction_mode(prev)
    assert torch.equal(fwd, out["logits"]), mode
    DC.check_against_fixture(out, data, 1e-4, 1e-4, f"densenet_tiny, plan, {mode}")
    assert float(DC.completeness_residual(x, out, meta["logit_bias"]).max()) <= 1e-4


def test_densenet121_plan(d121):
    from bcos_hip import densenet_engine
    net, meta, data, x = d121
    bound = max(1e-4, 3 * max(meta["d_ref"]["weights"], meta["d_ref"]["maps"]))
    eng = densenet_engine.attach(net)
    try:
        out = net.explain_batch(x)
        tg = eng.explain_targets(x, torch.tensor([int(data["prediction"][0]), 3], device=DEV), want_weights=True)
    finally:
        densenet_engine.detach(net)
    DC.check_against_fixture(out, data, 1e-4, bound, "densenet121_small, plan")
    # a slice accumulated twice or missed breaks this at full size, whatever tolerance depth may excuse
    resid = DC.completeness_residual(x, out, meta["logit_bias"])
    print("completeness", resid.tolist())
    assert float(resid.max()) <= 1e-4
    assert DC.rel(tg["dynamic_linear_weights"][:, 0], data["weights"]) <= bound          # (both images predict the same class)
    other = dict(out, dynamic_linear_weights=tg["dynamic_linear_weights"][:, 1], explained_class_idx=torch.full((2,), 3, device=DEV))
    assert float(DC.completeness_residual(x, other, meta["logit_bias"]).max()) <= 1e-4


def test_tiny_plan_batch_of_64_equals_its_halves(tiny):
    """64 images of 64 x 64 run as two sub-batches on side streams: the explanation of the batch carries the bits of the explanations of
    its two halves (each one pass on the caller's stream), and of a second call"""
    from bcos_hip import densenet_engine, synth
    net, meta, data, _ = tiny
    x = synth.synthetic_images(64, seed=9, size=64).to(DEV)
    eng = densenet_engine.attach(net)
    try:
        assert eng.n_streams(x) == 2 and eng.n_streams(x[:32]) == 1
        whole, again = net.explain_batch(x), net.explain_batch(x)
        lo, hi = net.explain_batch(x[:32]), net.explain_batch(x[32:])
        with torch.no_grad():
            fwd = net(x)
    finally:
        densenet_engine.detach(net)
    assert torch.equal(fwd, whole["logits"])
    for k in ("logits", "prediction", "dynamic_linear_weights", "contribution_map"):
        assert torch.equal(whole[k], again[k]), k
        assert torch.equal(whole[k], torch.cat([lo[k], hi[k]])), k
    module = net.explain_batch(x[:4])
    assert DC.rel(whole["dynamic_linear_weights"][:4], module["dynamic_linear_weights"]) <= 1e-4
