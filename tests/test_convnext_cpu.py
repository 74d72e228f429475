"""CPU side of the B-cos ConvNeXt: the model's state dict and execution order against the record of the reference
(tests/golden/make_golden_convnext.py), the fp64 launch-list restatement (tests/convnext_emulation.py) against the recorded fp64 results,
the depthwise reference and bounds of tests/dwconv_cases.py against F.conv2d and against mutations, the header / binding / argument checks
of the two depthwise entry points (no device needed) and the geometry the depthwise route accepts."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_emulation as CE
import dwconv_cases as DW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FIXTURES = ("convnext_small_cfg", "convnext_two")
SYMBOLS = ("bcos_dwconv7_fwd", "bcos_dwconv7_bwd")


def _record(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    return meta, {tag: np.load(os.path.join(GOLDEN, f"{name}_{tag}.npz")) for tag in ("fp32", "fp64")}


@pytest.fixture(scope="module", params=FIXTURES)
def recorded(request):
    from bcos_hip import synth
    meta, arrays = _record(request.param)
    net = synth.build_bcos_convnext(meta["block_setting"], meta["num_classes"], seed=meta["weight_seed"])
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"])
    return meta, arrays, net, x


def test_state_dict_is_the_references(recorded):
    meta, _, net, _ = recorded
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state_keys"]
    for k, (s, a) in meta["state_checksum"].items():          # the seeded weights are the recorded ones
        assert abs(float(sd[k].double().sum()) - s) <= 1e-9 * max(1.0, a) and abs(float(sd[k].double().abs().sum()) - a) <= 1e-9 * a, k
    assert abs(float(net.logit_layer.logit_bias) - meta["logit_bias"]) <= 1e-12


def test_convnext_tiny_keys_are_the_references():
    from bcos.models import convnext
    with open(os.path.join(GOLDEN, "convnext_tiny_keys.json")) as f:
        want = json.load(f)["state_keys"]
    net = convnext.convnext_tiny()
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == want
    for name in ("BcosConvNeXt", "CNBlock", "CNBlockConfig", "convnext_atto", "convnext_tiny", "convnext_small", "convnext_base",
                 "convnext_large"):
        assert name in convnext.__all__ and hasattr(convnext, name), name
    assert net.features[2][1].stochastic_depth.p > 0 and convnext.convnext_tiny(stochastic_depth_prob=0.0).features[2][1].stochastic_depth.p == 0
    assert net.features[1].bias is None and net.features[1].eps == 1e-6


def test_execution_order_is_the_recorded_one(recorded):
    """the leaf modules in the order one forward calls them, with their input and output shapes; the HIP-backed leaves are replaced by
    shape-only stand-ins (there is no device here), the others run as they are"""
    from bcos_hip import ops
    meta, _, net, x = recorded
    names = {m: n for n, m in net.named_modules()}
    trace = []
    leaves = ("BcosConv2d", "DetachablePositionNorm2d", "StochasticDepth", "AdaptiveAvgPool2d", "LogitLayer")
    for m in net.modules():
        kind = type(m).__name__
        if kind == "BcosConv2d":
            lin = m.linear
            m.forward = (lambda t, lin=lin: torch.zeros(t.shape[0], lin.out_channels,
                                                        ops.conv_out_size(t.shape[2], lin.kernel_size[0], lin.stride[0], lin.padding[0]),
                                                        ops.conv_out_size(t.shape[3], lin.kernel_size[1], lin.stride[1], lin.padding[1])))
        elif kind == "DetachablePositionNorm2d":
            m.forward = lambda t: torch.zeros_like(t)
        if kind in leaves:
            m.register_forward_hook(lambda mod, inp, res: trace.append([names[mod], type(mod).__name__, list(inp[0].shape), list(res.shape)]))
    with torch.no_grad():
        net(x[:1])
    assert trace == meta["exec_order"]


def test_emulation_reproduces_the_recorded_fp64_results(recorded):
    meta, arrays, net, x = recorded
    plan = CE.Plan(net.state_dict(), meta["block_setting"], meta["logit_bias"])
    out = plan.explain(x)
    ref = arrays["fp64"]
    assert out["prediction"].tolist() == ref["prediction"].tolist()
    for key in ("logits", "weights", "contribution_map"):
        want = torch.from_numpy(ref[key])
        err = float((out[key] - want).abs().max())
        print(meta["block_setting"], key, "max |emulation - record| =", err)
        assert err <= 1e-10, (key, err)
    assert min(meta["margins_fp64"]) >= 1e-2                   # every image decides its class: no test leaves one out


@pytest.mark.parametrize("shape,kind", DW.CASES, ids=[DW.case_id(s, k) for s, k in DW.CASES])
def test_depthwise_reference_is_conv2d_with_per_channel_norms(shape, kind):
    inp = DW.make_inputs(shape, kind)
    N, H, W, Cc = shape
    x = inp["x"].double().permute(0, 3, 1, 2)
    w = inp["w"].double().permute(2, 0, 1).unsqueeze(1)                    # [C,1,7,7]
    lin = F.conv2d(x, w, padding=3, groups=Cc)
    norm = (F.conv2d(x * x, torch.ones_like(w), padding=3, groups=Cc) + DW.EPS32).sqrt()
    ref = DW.reference_fwd(inp, 2.0)
    tol = 1e-13 * max(1.0, float(lin.abs().max()))
    assert float((ref["lin"].permute(0, 3, 1, 2) - lin).abs().max()) <= tol
    assert float((ref["norm"].permute(0, 3, 1, 2) / norm - 1).abs().max()) <= 1e-13
    assert float((ref["y"].permute(0, 3, 1, 2) - lin * lin.abs() / norm).abs().max()) <= tol * max(1.0, float(lin.abs().max()))
    z = (inp["gy"].double() * inp["mul"].double()).permute(0, 3, 1, 2)
    gx = F.conv_transpose2d(z, w, padding=3, groups=Cc) + inp["addend"].double().permute(0, 3, 1, 2)
    refb = DW.reference_bwd(inp, True, True)
    assert float((refb["gx"].permute(0, 3, 1, 2) - gx).abs().max()) <= 1e-13 * max(1.0, float(gx.abs().max()))


@pytest.mark.parametrize("shape", [s for s in DW.SHAPES if s[1] * s[2] > 1], ids=lambda s: "n%dh%dw%dc%d" % s)
def test_bound_notices_a_dropped_or_misplaced_tap(shape):
    """a plain fp32 evaluation sits inside the bounds; the same evaluation with one tap left out, or reading its neighbour's pixel, is
    orders of magnitude outside them (the centre tap and the one next to it: every image of the table has them in range)"""
    inp = DW.make_inputs(shape, "normal")
    ref, refb = DW.reference_fwd(inp, 2.0), DW.reference_bwd(inp, True, True)
    bnd, bndb = DW.bounds_fwd(ref, 2.0), DW.bounds_bwd(refb)
    x32 = inp["x"].permute(0, 3, 1, 2)
    w32 = inp["w"].permute(2, 0, 1).unsqueeze(1)
    lin = F.conv2d(x32, w32, padding=3, groups=shape[3])
    y32 = (lin * (lin.abs() / (F.conv2d(x32 * x32, torch.ones_like(w32), padding=3, groups=shape[3]) + 1e-6).sqrt())).permute(0, 2, 3, 1)
    assert DW.worst_ratio(y32, ref["y"], bnd["y"]) <= 1.0
    for mut in (dict(drop=(3, 3)), dict(shift=((3, 3), (3, 4)))):
        bad = DW.reference_fwd(inp, 2.0, **mut)
        assert DW.worst_ratio(bad["y"], ref["y"], bnd["y"]) > 1e3, mut
        badb = DW.reference_bwd(inp, True, True, **mut)
        assert DW.worst_ratio(badb["gx"], refb["gx"], bndb["gx"]) > 1e3, mut


def test_header_and_binding_declare_the_entry_points(hip_lib):
    from bcos_hip import lib
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
        assert hasattr(hip_lib, name), name                                   # the built library exports it
    assert "bcos_dwconv.hip" in lib.SOURCES and os.path.exists(os.path.join(str(lib.CSRC), "bcos_dwconv.hip"))
    assert "#define BCOS_ABI_VERSION 12" in header and lib.ABI_VERSION == 12 and hip_lib.bcos_version() == 12


def test_argument_validation_needs_no_device(hip_lib):
    """every refusal comes back as BCOS_E_INVAL before any HIP call (this machine has no device)"""
    from bcos_hip import lib
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)

    def fwd(x=p, w=p, y=p, scale=None, norm=None, N=1, H=2, W=2, Cc=4, b=2.0):
        return hip_lib.bcos_dwconv7_fwd(x, w, y, scale, norm, N, H, W, Cc, b, None)

    def bwd(gy=p, w=p, mul=None, addend=None, gx=p, N=1, H=2, W=2, Cc=4):
        return hip_lib.bcos_dwconv7_bwd(gy, w, mul, addend, gx, N, H, W, Cc, None)
    bad_f = [dict(x=None), dict(w=None), dict(y=None), dict(N=0), dict(H=0), dict(W=-1), dict(Cc=0), dict(Cc=6), dict(x=odd), dict(w=odd),
             dict(y=odd), dict(scale=odd), dict(norm=odd), dict(b=1.0, scale=p), dict(N=1 << 30, H=1 << 10, W=1 << 10)]
    for kw in bad_f:
        assert fwd(**kw) == lib.BCOS_E_INVAL, kw
        assert b"bcos_dwconv7_fwd" in hip_lib.bcos_last_error_string(), kw
    bad_b = [dict(gy=None), dict(w=None), dict(gx=None), dict(N=0), dict(H=-3), dict(W=0), dict(Cc=0), dict(Cc=10), dict(gy=odd), dict(w=odd),
             dict(gx=odd), dict(mul=odd), dict(addend=odd), dict(N=1 << 30, H=1 << 10, W=1 << 10)]
    for kw in bad_b:
        assert bwd(**kw) == lib.BCOS_E_INVAL, kw
        assert b"bcos_dwconv7_bwd" in hip_lib.bcos_last_error_string(), kw


def test_depthwise_route_accepts_exactly_its_geometry():
    from bcos.modules import BcosConv2d, _hipfn
    ok = dict(in_channels=8, out_channels=8, kernel_size=7, stride=1, padding=3, dilation=1, groups=8, max_out=1)
    assert _hipfn.is_depthwise7(**ok)
    assert _hipfn.is_depthwise7(**dict(ok, kernel_size=(7, 7), padding=(3, 3), stride=(1, 1), dilation=(1, 1)))
    others = [dict(groups=1), dict(groups=4), dict(groups=2), dict(out_channels=16), dict(kernel_size=5, padding=2), dict(kernel_size=3, padding=1),
              dict(kernel_size=(7, 5)), dict(stride=2), dict(padding=2), dict(padding=(3, 2)), dict(dilation=2), dict(max_out=2),
              dict(in_channels=16, out_channels=16)]
    for kw in others:
        assert not _hipfn.is_depthwise7(**dict(ok, **kw)), kw
    assert _hipfn.conv_is_depthwise7(BcosConv2d(8, 8, kernel_size=7, padding=3, groups=8).linear)
    assert not _hipfn.conv_is_depthwise7(BcosConv2d(8, 8, kernel_size=7, padding=3, groups=2).linear)
    assert not _hipfn.conv_is_depthwise7(BcosConv2d(8, 8, kernel_size=3, padding=1, groups=8).linear)
    assert not _hipfn.conv_is_depthwise7(BcosConv2d(8, 8, kernel_size=7, padding=3, groups=8, max_out=2).linear, 2)


def test_position_norm_module():
    from bcos.modules import norms
    pn = norms.DetachablePositionNorm2d(12)
    assert pn.eps == 1e-5 and pn.weight.shape == (12,) and pn.bias is not None and pn.features == 12 and pn.detach is False
    assert norms.DetachablePositionNorm2d(12, affine=False).weight is None
    nb = norms.NoBias(norms.DetachablePositionNorm2d)(12, eps=1e-6)
    assert nb.bias is None and nb.weight is not None and nb.eps == 1e-6
    assert "DetachablePositionNorm2d" in norms.centered_norms.__all__
    pn.set_explanation_mode(True)
    assert pn.detach is True
