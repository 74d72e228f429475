"""`-m gpu`: the native B-cos ConvNeXt against the fixtures recorded from the reference (tests/golden/make_golden_convnext.py), through
the module path and through the fused plan (bcos_hip/convnext_engine.py), in every contraction mode; DetachablePositionNorm2d against
fp64 under the bounds of tests/token_cases.py; the refusals of the depthwise layer and of attach().

Network bounds: logits within 1e-4 of the fp64 record (absolute: the logits are O(1)), class indices exact for every image, W(x) and the
contribution maps within 1e-4 of their per-image maximum; engine against module path at the same tolerances."""
import json
import os

import numpy as np
import pytest
import torch

import token_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("f32", "bf16x3", "f16x2")
FIXTURES = ("convnext_small_cfg", "convnext_two")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOL = 1e-4


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module", params=FIXTURES)
def recorded(request, lib):
    from bcos_hip import synth
    with open(os.path.join(GOLDEN, request.param + ".json")) as f:
        meta = json.load(f)
    ref = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, request.param + "_fp64.npz")).items()}
    net = synth.build_bcos_convnext(meta["block_setting"], meta["num_classes"], seed=meta["weight_seed"]).to(DEV)
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"]).to(DEV)
    return request.param, meta, ref, net, x


def _per_image(a, b):
    """worst image of max |a - b| / max |b|"""
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


def _check(out, ref, what, logits=None):
    dl = float((out["logits"].double().cpu() - ref["logits"]).abs().max())
    dw = _per_image(out["dynamic_linear_weights"], ref["weights"])
    dm = _per_image(out["contribution_map"], ref["contribution_map"])
    print(f"{what}: logits {dl:.2e}, W(x) {dw:.2e}, maps {dm:.2e} (bound {TOL:g})")
    assert out["prediction"].cpu().tolist() == ref["prediction"].tolist(), what
    assert dl <= TOL and dw <= TOL and dm <= TOL, (what, dl, dw, dm)
    if logits is not None:
        assert float((logits.double().cpu() - ref["logits"]).abs().max()) <= TOL, what


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from bcos_hip import lib as blib
        self.prev = blib.get_contraction_mode()
        blib.set_contraction_mode(self.mode)

    def __exit__(self, *exc):
        from bcos_hip import lib as blib
        blib.set_contraction_mode(self.prev)
        return False


@pytest.mark.parametrize("mode", MODES)
def test_module_path(recorded, mode):
    name, meta, ref, net, x = recorded
    with _mode(mode):
        with torch.no_grad():
            logits = net(x)
        out = net.explain_batch(x)
    _check(out, ref, f"{name}, module path, {mode}", logits)


@pytest.mark.parametrize("mode", MODES)
def test_engine(recorded, mode):
    from bcos_hip import convnext_engine
    name, meta, ref, net, x = recorded
    with _mode(mode):
        module_out = net.explain_batch(x)
        eng = convnext_engine.attach(net)
        try:
            with torch.no_grad():
                logits = net(x)
            out = net.explain_batch(x)
            assert net._bcos_engine is eng
        finally:
            convnext_engine.detach(net)
    assert torch.equal(logits, out["logits"]), mode
    _check(out, ref, f"{name}, engine, {mode}", logits)
    dl = float((out["logits"] - module_out["logits"]).abs().max())
    dw = _per_image(out["dynamic_linear_weights"], module_out["dynamic_linear_weights"])
    dm = _per_image(out["contribution_map"], module_out["contribution_map"])
    print(f"{name}, engine against module path, {mode}: logits {dl:.2e}, W(x) {dw:.2e}, maps {dm:.2e}")
    assert out["prediction"].tolist() == module_out["prediction"].tolist()
    assert dl <= TOL and dw <= TOL and dm <= TOL, (mode, dl, dw, dm)


def test_engine_launch_list_and_targets(recorded):
    """four launches per block forward, none of them elementwise; explain(targets=...) explains the asked class"""
    from bcos_hip import convnext_engine
    name, meta, ref, net, x = recorded
    eng = convnext_engine.attach(net)
    try:
        convnext_engine.PLAN_LOG = []
        eng.forward(x[:1])
        log, convnext_engine.PLAN_LOG = convnext_engine.PLAN_LOG, None
        blocks = sum(s[2] for s in meta["block_setting"])
        downs = sum(1 for s in meta["block_setting"] if s[1] is not None)
        kinds = [k for k, _ in log]
        assert kinds.count("dw") == blocks and kinds.count("pn") == blocks + downs + 2 and kinds.count("conv") == 2 * blocks + downs + 2
        i = kinds.index("dw")
        assert kinds[i:i + 4] == ["dw", "pn", "conv", "conv"]
        tg = torch.tensor([(p + 1) % meta["num_classes"] for p in ref["prediction"].tolist()], device=DEV)
        out = eng.explain(x, targets=tg)
        assert out["explained_class_idx"].tolist() == tg.tolist()
    finally:
        convnext_engine.detach(net)
    mod = net.explain_batch(x, targets=tg)
    assert _per_image(out["dynamic_linear_weights"], mod["dynamic_linear_weights"]) <= TOL


@pytest.mark.parametrize("affine", [True, False])
def test_position_norm_against_fp64(lib, affine):
    """forward and explanation-mode input gradient at (2, 40, 5, 9): the LayerNorm forms of tests/token_cases.py over the rows of the
    NHWC image (K_y on the output, K_det on the detached gradient)"""
    from bcos.modules import norms
    g = torch.Generator().manual_seed(40)
    x = torch.randn(2, 40, 5, 9, generator=g) * 2 + 0.5
    gy = torch.randn(2, 40, 5, 9, generator=g)
    pn = norms.DetachablePositionNorm2d(40, eps=1e-6, affine=affine).to(DEV)
    if affine:
        with torch.no_grad():
            pn.weight.copy_(torch.rand(40, generator=g) + 0.5)
            pn.bias.copy_(torch.randn(40, generator=g) * 0.1)
    pn.set_explanation_mode(True)
    xd = x.to(DEV).requires_grad_(True)
    y = pn(xd)
    (gx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 40)      # noqa: E731
    w = pn.weight.detach().cpu() if affine else None
    b = pn.bias.detach().cpu() if affine else None
    eps = float(np.float32(1e-6))
    x2, g2 = rows(x), rows(gy)
    ref_f = TC._ln_eval(x2, w, b, None, None, None, None, eps, torch.float64, fwd_only=True)
    rstd32 = TC._ln_eval(x2, w, b, None, None, None, None, eps, torch.float32, fwd_only=True)["rstd"]
    zeros = torch.zeros_like(x2)
    ref = TC._ln_eval(x2, w, b, g2, rstd32, zeros, zeros, eps, torch.float64)
    forms = TC._ln_forms(x2, w, g2, rstd32, zeros, zeros, eps, ref)
    ey = (rows(y.detach().cpu()).double() - ref_f["y"]).abs()
    by = TC.K["y"] * forms["y"][1]
    # the backward's rstd is the kernel's own (within K_rstd of the fp32 formula's): its relative error moves h = gy w rstd, so the
    # detached form is widened by K_rstd u (1 + A / sd) |h| -- the rstd bound of token_cases carried through the product and the mean
    h = ((g2.double() * (w.double() if w is not None else 1.0)) * rstd32.double().view(-1, 1)).abs()
    q = forms["rstd"][1].view(-1, 1) / ref["rstd"].view(-1, 1)
    eg = (rows(gx.cpu()).double() - ref["out/--"]).abs()
    bg = TC.K["det"] * forms["out/--"][1] + TC.K["rstd"] * q * (h + h.mean(1, keepdim=True))
    print(f"position norm affine={affine}: y {float((ey / by).max()):.3f} of its bound, gx {float((eg / bg).max()):.3f}")
    assert bool((ey <= by).all()) and bool((eg <= bg).all())


def test_depthwise_layer_refuses_training_gradients(lib):
    from bcos.modules import BcosConv2d
    from bcos_hip.lib import BcosHipError
    conv = BcosConv2d(8, 8, kernel_size=7, padding=3, groups=8).to(DEV)
    x = torch.randn(2, 8, 9, 9, device=DEV, requires_grad=True)
    y = conv(x)                                        # the forward runs in any mode
    with pytest.raises(BcosHipError, match="do not train yet"):
        y.sum().backward()
    conv.eval()
    with pytest.raises(BcosHipError, match="do not train yet"):
        conv(x).sum().backward()                       # eval mode, outside explanation mode: the scale would need its derivative
    conv.set_explanation_mode(True)
    (gx,) = torch.autograd.grad(conv(x).sum(), x)      # explanation mode: the input gradient
    assert gx.shape == x.shape and bool(torch.isfinite(gx).all())
    norms = conv.calc_patch_norms(x.detach())
    want = (torch.nn.functional.avg_pool2d(x.detach() ** 2, 7, stride=1, padding=3, divisor_override=1) + 1e-6).sqrt()
    assert norms.shape == want.shape and float((norms / want - 1).abs().max()) <= 1e-5
    # every other grouped geometry behaves as before, today's error included
    other = BcosConv2d(8, 8, kernel_size=3, padding=1, groups=8).to(DEV)
    with pytest.raises(BcosHipError, match=r"grouped B-cos conv needs in_channels/groups % 4 == 0"):
        other(x.detach())


def test_attach_refuses_what_the_plan_does_not_cover(lib):
    from bcos.models import convnext
    from bcos.modules import norms
    from bcos_hip import convnext_engine
    from bcos_hip.lib import BcosHipError
    stages = [convnext.CNBlockConfig(8, None, 2)]          # (one block in all divides by zero in the drop-rate schedule, as the reference does)
    bnu = convnext.BcosConvNeXt(stages, num_classes=4, norm_layer=norms.NoBias(norms.BatchNormUncentered2d)).to(DEV).eval()
    with pytest.raises(BcosHipError, match="position-norm"):
        convnext_engine.attach(bnu)
    assert not hasattr(bnu, "_bcos_engine")
    with torch.no_grad():
        assert bnu(torch.rand(1, 6, 8, 8, device=DEV)).shape == (1, 4)          # the module path keeps working
    net = convnext.BcosConvNeXt(stages, num_classes=4).to(DEV)
    with pytest.raises(BcosHipError, match="eval mode"):
        convnext_engine.attach(net.train())
    from functools import partial
    from bcos.modules import BcosConv2d
    with pytest.raises(BcosHipError, match="B = "):
        convnext_engine.attach(convnext.BcosConvNeXt(stages, num_classes=4, conv_layer=partial(BcosConv2d, b=1.5)).to(DEV).eval())
    eng = convnext_engine.attach(net.eval())
    with pytest.raises(BcosHipError, match="gates"):
        eng.explain(torch.rand(1, 6, 8, 8, device=DEV), gates=[torch.ones(1, device=DEV)])
    convnext_engine.detach(net)
