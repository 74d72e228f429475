"""`-m gpu`: training a native B-cos ConvNeXt per layer.  A depthwise 7x7 layer that opted in (BcosConv2d.enable_depthwise_training, which
every CNBlock calls) against float64 autograd of the same expressions; its explanation mode against the bare layer's, bit for bit; one
train()-mode step of the BcosConvNeXt of tests/golden/convnext_two_train_step.* (recorded from the reference by
tests/golden/make_golden_convnext_train.py) against the record; a second step's depthwise weight gradients against the first's.

Bounds, in relative L2 (densenet_cases.rel, the measure of densenet_train_cases.check_same_step): a single layer 1e-5; the recorded step
1e-5 for the logits and the loss, 1e-4 for the input gradient and every parameter gradient outside the fixture's null set (which is
empty) -- what the project holds a shallow fixture to once the reference's own fp32-vs-fp64 distance is <= 2e-5."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from densenet_cases import GOLDEN, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEM = "convnext_two_train_step"
LAYER_TOL, OUT_TOL, GRAD_TOL = 1e-5, 1e-5, 1e-4


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _layer(channels, opted_in):
    from bcos.modules import BcosConv2d
    torch.manual_seed(channels)
    conv = BcosConv2d(channels, channels, kernel_size=7, padding=3, groups=channels)
    return (conv.enable_depthwise_training() if opted_in else conv).to(DEV)


@pytest.mark.parametrize("shape", [(2, 8, 9, 9), (2, 40, 7, 7)], ids=lambda s: "n%dc%dh%dw%d" % s)
def test_opted_in_layer_against_float64_autograd(lib, shape):
    """the input gradient and the gradient of the RAW weight (through the unit-norm projection) of y = lin |lin| / sqrt(box7(x^2) + eps)"""
    Cc = shape[1]
    conv = _layer(Cc, True).train()
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    gy = torch.randn(*shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = conv(xd)
    assert type(y.grad_fn).__name__ == "BcosDwConv7TrainFnBackward"
    gx, gw = torch.autograd.grad(y, (xd, conv.linear.weight), gy.to(DEV))
    x64 = x.double().requires_grad_(True)
    w64 = conv.linear.weight.detach().cpu().double().requires_grad_(True)
    w_hat = w64 / w64.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    lin = F.conv2d(x64, w_hat, padding=3, groups=Cc)
    y64 = lin * lin.abs() / (F.conv2d(x64 * x64, torch.ones_like(w64), padding=3, groups=Cc) + float(np.float32(1e-6))).sqrt()
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), gy.double())
    fig = dict(y=rel(y.detach().cpu(), y64.detach()), gx=rel(gx.cpu(), gx64), gw=rel(gw.cpu(), gw64))
    print(shape, fig)
    assert gw.shape == conv.linear.weight.shape and max(fig.values()) <= LAYER_TOL, fig
    # the weight gradient alone (a frozen input), and the input gradient alone (a frozen weight)
    (gw_only,) = torch.autograd.grad(conv(x.to(DEV)), conv.linear.weight, gy.to(DEV))
    assert torch.equal(gw_only, gw)
    conv.linear.weight.requires_grad_(False)
    (gx_only,) = torch.autograd.grad(conv(xd), xd, gy.to(DEV))
    assert rel(gx_only.cpu(), gx64) <= LAYER_TOL


def test_explanation_mode_is_the_bare_layers(lib):
    bare, opted = _layer(8, False), _layer(8, True)
    opted.load_state_dict(bare.state_dict())
    x = torch.randn(2, 8, 9, 9, device=DEV, requires_grad=True)
    gy = torch.randn(2, 8, 9, 9, device=DEV)
    res = []
    for conv in (bare, opted):
        conv.eval().set_explanation_mode(True)
        y = conv(x)
        (gx,) = torch.autograd.grad(y, x, gy)
        res.append((y.detach(), gx))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isfinite(res[1][1]).all()) and float(res[1][1].abs().max()) > 0


@pytest.fixture(scope="module")
def recorded_step(lib):
    """the fixture's network, one train()-mode step and a second identical one: shared by the tests below"""
    from bcos_hip import synth
    with open(os.path.join(GOLDEN, STEM + ".json")) as f:
        meta = json.load(f)
    data = dict(np.load(os.path.join(GOLDEN, STEM + ".npz")))
    net = synth.build_bcos_convnext(meta["block_setting"], meta["num_classes"], seed=meta["weight_seed"]).to(DEV)
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"]).to(DEV)
    target = F.one_hot(torch.tensor(meta["labels"]), meta["num_classes"]).float().to(DEV)

    def step():
        net.train()
        xr = x.clone().requires_grad_(True)
        out = net(xr)
        loss = F.binary_cross_entropy_with_logits(out, target)
        named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
        gs = torch.autograd.grad(loss, [xr] + [p for _, p in named])
        return dict(out=out.detach(), loss=float(loss.detach()), gx=gs[0], grads={n: g for (n, _), g in zip(named, gs[1:])})
    return meta, data, step(), step()


def test_recorded_training_step(recorded_step):
    meta, data, res, _ = recorded_step
    names = list(res["grads"])
    assert names == meta["param_names"] and meta["null_gradient_params"] == []
    fig = dict(output=rel(res["out"], data["output"]), loss=abs(res["loss"] - float(data["loss"])) / abs(float(data["loss"])),
               gx=rel(res["gx"], data["gx"]))
    per = {n: rel(res["grads"][n], data["grad/" + n]) for n in names}
    worst = max(per, key=per.get)
    worst_dw = max(meta["depthwise_params"], key=per.get)
    print("recorded step:", fig, "worst parameter", worst, per[worst], "worst depthwise", worst_dw, per[worst_dw],
          "reference's own fp32-vs-fp64", meta["reference_self_floor"]["fp32_vs_fp64"])
    assert fig["output"] <= OUT_TOL and fig["loss"] <= OUT_TOL, fig
    assert fig["gx"] <= GRAD_TOL, fig
    assert all(v <= GRAD_TOL for v in per.values()), {n: v for n, v in per.items() if v > GRAD_TOL}
    assert set(meta["depthwise_params"]) <= set(per)


def test_second_step_gives_the_same_depthwise_bits(recorded_step):
    meta, _, first, second = recorded_step
    for n in meta["depthwise_params"]:
        a, b = first["grads"][n], second["grads"][n]
        assert a.shape[1:] == (1, 7, 7) and torch.equal(a.view(torch.int32), b.view(torch.int32)), n
