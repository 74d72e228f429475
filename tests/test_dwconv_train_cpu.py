"""CPU side of the depthwise 7x7 training-mode gradients (csrc/bcos_dwconv_train.hip): the fp64 reference of tests/dwconv_train_cases.py
against torch's float64 autograd and against mutations, the header / binding / exported symbols, every argument check of the two launch
entry points and the workspace formula (no device needed), the integrity of the recorded training step
(tests/golden/make_golden_convnext_train.py) and which layers are opted in."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_train_cases as DT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SYMBOLS = ("bcos_dwconv7_train_bwd", "bcos_dwconv7_wgrad", "bcos_dwconv7_wgrad_workspace")
STEM = "convnext_two_train_step"
IDS = [DT.case_id(s, k) for s, k in DT.CASES]


@pytest.mark.parametrize("shape,kind", DT.CASES, ids=IDS)
def test_reference_is_float64_autograd(shape, kind):
    """gx and gw of the case module, fed the unrounded fp64 forward, equal autograd of lin |lin| / sqrt(box7(x^2) + eps)"""
    inp = DT.make_inputs(shape, kind)
    Cc = shape[3]
    x = inp["x"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = inp["w"].double().permute(2, 0, 1).unsqueeze(1).contiguous().requires_grad_(True)          # [C,1,7,7]
    lin = F.conv2d(x, w, padding=3, groups=Cc)
    y = lin * lin.abs() / (F.conv2d(x * x, torch.ones_like(w), padding=3, groups=Cc) + DT.EPS32).sqrt()
    gx, gw = torch.autograd.grad(y, (x, w), inp["gy"].double().permute(0, 3, 1, 2))
    given = DT.forward_given(inp, rounded=False)
    ref = DT.reference_gx(inp, given, False)
    refw = DT.reference_gw(inp, given["scale"], 2.0)
    for got, want in ((ref["gx"].permute(0, 3, 1, 2), gx), (refw["gw"].permute(2, 0, 1).unsqueeze(1), gw)):
        assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
    with_add = DT.reference_gx(inp, given, True)
    assert torch.equal(with_add["gx"], ref["gx"] + inp["addend"].double())
    # the scale held constant: the gradient of sum(gy * scale.detach() * lin) with respect to the filters
    lin2 = F.conv2d(x.detach(), w, padding=3, groups=Cc)
    (gw_c,) = torch.autograd.grad(lin2, w, (inp["gy"].double() * given["scale"]).permute(0, 3, 1, 2))
    refc = DT.reference_gw(inp, given["scale"], 1.0)
    assert float((refc["gw"].permute(2, 0, 1).unsqueeze(1) - gw_c).abs().max()) <= 1e-11 * max(1.0, float(gw_c.abs().max()))


@pytest.mark.parametrize("shape", DT.SHAPES, ids=lambda s: "n%dh%dw%dc%d" % s)
def test_bounds_notice_the_mutations(shape):
    """a plain fp32 evaluation of the header's expressions sits inside the bounds; a dropped tap, a dropped norm term, a missing factor
    2 and a weight gradient with a shifted tap are each at least 100 x outside them"""
    inp = DT.make_inputs(shape, "normal")
    given = DT.forward_given(inp)
    ref = DT.reference_gx(inp, given, True)
    bnd = DT.bounds_gx(ref)
    refw = DT.reference_gw(inp, given["scale"], 2.0)
    bndw = DT.bounds_gw(refw, shape)
    Cc = shape[3]
    nchw = lambda t: t.permute(0, 3, 1, 2)      # noqa: E731
    g, x = inp["gy"], inp["x"]
    y32, s32, n32 = (given[k].float() for k in ("y", "scale", "norm"))
    w4 = inp["w"].permute(2, 0, 1).unsqueeze(1)
    glin = 2.0 * (s32 * g)
    r = -(g * y32) / (n32 * n32)
    acc = F.conv_transpose2d(nchw(glin), w4, padding=3, groups=Cc)
    box = F.conv_transpose2d(nchw(r), torch.ones_like(w4), padding=3, groups=Cc)
    gx32 = (acc + nchw(x) * box + nchw(inp["addend"])).permute(0, 2, 3, 1)
    assert DT.worst_ratio(gx32, ref["gx"], bnd["gx"]) <= 1.0
    gw32 = torch.nn.grad.conv2d_weight(nchw(x), w4.shape, nchw(glin), padding=3, groups=Cc)[:, 0].permute(1, 2, 0)
    assert DT.worst_ratio(gw32, refw["gw"], bndw["gw"]) <= 1.0
    for mut in (dict(drop=(3, 3)), dict(no_r=True), dict(factor=1.0)):
        bad = DT.reference_gx(inp, given, True, **mut)
        assert DT.worst_ratio(bad["gx"], ref["gx"], bnd["gx"]) >= 100.0, mut
    badw = DT.reference_gw(inp, given["scale"], 2.0, shift=((3, 3), (3, 4)))
    assert DT.worst_ratio(badw["gw"], refw["gw"], bndw["gw"]) >= 100.0
    halfw = DT.reference_gw(inp, given["scale"], 1.0)
    assert DT.worst_ratio(halfw["gw"], refw["gw"], bndw["gw"]) >= 100.0


def test_header_binding_and_library_carry_the_symbols(hip_lib):
    from bcos_hip import lib, ops
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    for name in SYMBOLS:
        m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*)\);", header)
        assert m and name in lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
        assert hasattr(hip_lib, name) and re.search(r" T " + name + r"$", exported, re.M), name
    assert "bcos_dwconv_train.hip" in lib.SOURCES and os.path.exists(os.path.join(str(lib.CSRC), "bcos_dwconv_train.hip"))
    assert "#define BCOS_ABI_VERSION 12" in header and lib.ABI_VERSION == 12 and hip_lib.bcos_version() == 12
    for name in ("dwconv7_train_bwd", "dwconv7_wgrad"):
        assert callable(getattr(ops, name)), name


def test_argument_validation_needs_no_device(hip_lib):
    """every refusal comes back as BCOS_E_INVAL, under the entry point's name, before any HIP call (this machine has no device)"""
    from bcos_hip import lib
    buf = (C.c_float * 65536)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd = C.c_void_p(base), C.c_void_p(base + 4)

    def bwd(gy=p, x=p, y=p, scale=p, norm=p, w=p, addend=None, gx=p, N=1, H=2, W=2, Cc=4, b=2.0):
        return hip_lib.bcos_dwconv7_train_bwd(gy, x, y, scale, norm, w, addend, gx, N, H, W, Cc, b, None)

    def wgrad(gy=p, mul=None, gain=1.0, x=p, gw=p, ws=p, ws_bytes=1 << 17, N=1, H=2, W=2, Cc=4):
        return hip_lib.bcos_dwconv7_wgrad(gy, mul, gain, x, gw, ws, ws_bytes, N, H, W, Cc, None)
    bad_b = [dict(gy=None), dict(w=None), dict(gx=None), dict(x=None), dict(y=None), dict(scale=None), dict(norm=None), dict(N=0),
             dict(H=-3), dict(W=0), dict(Cc=0), dict(Cc=10), dict(gy=odd), dict(x=odd), dict(y=odd), dict(scale=odd), dict(norm=odd),
             dict(w=odd), dict(addend=odd), dict(gx=odd), dict(b=1.5), dict(b=3.0), dict(b=float("nan")),
             dict(b=1.0, x=odd), dict(N=1 << 30, H=1 << 10, W=1 << 10)]
    for kw in bad_b:
        assert bwd(**kw) == lib.BCOS_E_INVAL, kw
        assert b"bcos_dwconv7_train_bwd" in hip_lib.bcos_last_error_string(), kw
    need = hip_lib.bcos_dwconv7_wgrad_workspace(1, 2, 2, 4)
    bad_w = [dict(gy=None), dict(x=None), dict(gw=None), dict(ws=None), dict(N=0), dict(H=0), dict(W=-1), dict(Cc=0), dict(Cc=6),
             dict(gy=odd), dict(mul=odd), dict(x=odd), dict(gw=odd), dict(ws=odd), dict(gain=float("inf")), dict(gain=float("nan")),
             dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1)]
    for kw in bad_w:
        assert wgrad(**kw) == lib.BCOS_E_INVAL, kw
        assert b"bcos_dwconv7_wgrad" in hip_lib.bcos_last_error_string(), kw
    for bad in ((0, 2, 2, 4), (1, 0, 2, 4), (1, 2, -1, 4), (1, 2, 2, 0), (1, 2, 2, 6)):
        assert hip_lib.bcos_dwconv7_wgrad_workspace(*bad) == lib.BCOS_E_INVAL, bad
        assert b"bcos_dwconv7_wgrad_workspace" in hip_lib.bcos_last_error_string(), bad


def test_workspace_is_the_headers_formula(hip_lib):
    """bytes = 4 * 49 * C * 2 * G, G = ceil(P / ceil(P / 256)), P = N ceil(H / 6) ceil(W / 8)"""
    from bcos_hip import ops
    for shape in DT.SHAPES + [(64, 56, 56, 96), (64, 7, 7, 768), (1, 6, 8, 4), (1, 7, 9, 4), (256, 6, 8, 64), (257, 6, 8, 64)]:
        N, H, W, Cc = shape
        P = N * ((H + 5) // 6) * ((W + 7) // 8)
        L = (P + 255) // 256
        G = (P + L - 1) // L
        assert DT.wgrad_plan(shape) == (P, L, G) and G <= 256
        assert hip_lib.bcos_dwconv7_wgrad_workspace(N, H, W, Cc) == 4 * 49 * Cc * 2 * G == DT.workspace_bytes(shape), shape
        assert ops.dwconv7_wgrad_workspace(N, H, W, Cc) == DT.workspace_bytes(shape)
    assert DT.wgrad_plan((9, 33, 41, 4))[1] == 2 and all(DT.wgrad_plan(s)[1] == 1 for s in DT.SHAPES[:-1])


def test_recorded_training_step_is_whole():
    with open(os.path.join(GOLDEN, STEM + ".json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(GOLDEN, STEM + ".npz"))
    for ext in (".json", ".npz"):
        assert os.path.getsize(os.path.join(GOLDEN, STEM + ext)) < 1 << 20
    assert os.path.getsize(os.path.join(GOLDEN, "make_golden_convnext_train.py")) < 1 << 20
    assert meta["block_setting"] == [[16, 32, 1], [32, None, 2]] and meta["num_classes"] == 10 and meta["layer_scale"] == 1.0
    assert meta["stochastic_depth_prob"] == 0.0 and meta["n_images"] == 4 and meta["size"] == 36 and meta["loss"] == "bce_with_logits"
    names = meta["param_names"]
    assert set(data.files) == {"output", "loss", "gx", "grad_norms"} | {"grad/" + n for n in names}
    assert data["output"].shape == (4, 10) and data["gx"].shape == (4, 6, 36, 36) and data["grad_norms"].shape == (len(names),)
    floor = meta["reference_self_floor"]["fp32_vs_fp64"]
    assert max(floor["output"], floor["gx"], floor["worst_param"]) <= 2e-5
    # the null set as recorded: the 1e-2-of-median rule applied to the recorded fp64 norms, empty, and no depthwise weight in it
    norms = meta["grad_norms_fp64"]
    median = float(np.median([norms[n] for n in names]))
    assert abs(median - meta["median_grad_norm_fp64"]) <= 1e-12 * median
    null = [n for n in names if norms[n] < meta["null_fraction_of_median"] * median]
    assert null == meta["null_gradient_params"] == [] and meta["null_fraction_of_median"] == 1e-2
    dw = meta["depthwise_params"]
    assert dw == ["features.2.0.block.0.linear.weight", "features.4.0.block.0.linear.weight", "features.4.1.block.0.linear.weight"]
    assert all(data["grad/" + n].shape == (c, 1, 7, 7) for n, c in zip(dw, (16, 32, 32)))
    for n in names:
        g = data["grad/" + n]
        assert np.isfinite(g).all() and abs(float(np.linalg.norm(g.astype(np.float64))) - norms[n]) <= 1e-4 * norms[n], n
    # the network of this package has the recorded parameters
    from bcos_hip import synth
    net = synth.build_bcos_convnext(meta["block_setting"], meta["num_classes"], seed=meta["weight_seed"])
    assert [n for n, _ in net.named_parameters()] == names
    assert all(tuple(p.shape) == data["grad/" + n].shape for n, p in net.named_parameters())


def test_blocks_opt_in_and_bare_layers_do_not():
    from bcos.models import convnext
    from bcos.modules import BcosConv2d, _hipfn
    assert hasattr(_hipfn, "BcosDwConv7TrainFn") and "do not train yet" in _hipfn.DEPTHWISE_NO_TRAINING
    assert "enable_depthwise_training" in _hipfn.DEPTHWISE_NO_TRAINING
    bare = BcosConv2d(8, 8, kernel_size=7, padding=3, groups=8)
    assert bare._depthwise_training is False
    assert bare.enable_depthwise_training()._depthwise_training is True and bare.enable_depthwise_training(False)._depthwise_training is False
    with pytest.raises(ValueError, match="not a depthwise 7x7 layer"):
        BcosConv2d(8, 8, kernel_size=3, padding=1, groups=8).enable_depthwise_training()
    block = convnext.CNBlock(8, 1.0, 0.0)
    assert block.block[0]._depthwise_training is True
    assert not any(m._depthwise_training for m in block.block[1:] if isinstance(m, BcosConv2d))
    net = convnext.BcosConvNeXt([convnext.CNBlockConfig(8, 16, 1), convnext.CNBlockConfig(16, None, 2)], num_classes=4)
    flags = [m._depthwise_training for m in net.modules() if isinstance(m, BcosConv2d)]
    assert sum(flags) == 3 and len(flags) == 2 + 3 * 3 + 1
    # a block built from another convolution (its first layer is no depthwise 7x7 B-cos layer of this package) is left alone
    from functools import partial
    other = convnext.CNBlock(8, 1.0, 0.0, conv_layer=partial(BcosConv2d, max_out=2))
    assert other.block[0]._depthwise_training is False
