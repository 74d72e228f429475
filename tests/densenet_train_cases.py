"""Shared by test_densenet_train_cpu.py and test_densenet_train_gpu.py (TEST INFRASTRUCTURE): the network and the step of the
densenet_tiny_train_step fixture (recorded from the reference's train()-mode step, tests/golden/make_golden_densenet_train.py) and the
measures it is held to -- output and running_var <= 1e-5, loss <= 1e-5 relative, the input gradient, every parameter gradient and its
norm <= 1e-4 in relative L2, and for the parameters of `null_gradient_params` (mathematically zero gradient: norm0's weight, whose
channels every reader renormalises) an ABSOLUTE distance <= 1e-4 of the median parameter gradient norm."""
import json
import os

import numpy as np
import torch

from densenet_cases import GOLDEN, rel

STEM = "densenet_tiny_train_step"
OUT_TOL, GRAD_TOL, RV_TOL = 1e-5, 1e-4, 1e-5
_cache = {}


def fixture():
    if "f" not in _cache:
        meta = json.load(open(os.path.join(GOLDEN, STEM + ".json")))
        _cache["f"] = (meta, dict(np.load(os.path.join(GOLDEN, STEM + ".npz"))))
    return _cache["f"]


def tiny_net(device="cpu"):
    """-> (net in eval() with the fixture's weights, images, BCE target)"""
    from bcos_hip import synth
    meta, data = fixture()
    net = synth.build_bcosified_densenet(meta["growth"], tuple(meta["block_config"]), meta["init_features"], meta["bn_size"],
                                         meta["num_classes"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"])
    target = torch.nn.functional.one_hot(torch.tensor(meta["labels"]), meta["num_classes"]).float()
    return net.to(device).eval(), x.to(device), target.to(device)


def step(net, x, target):
    """one train()-mode step -> dict(out, loss, gx, grads {name: tensor}, node = name of the output's autograd node)"""
    net.train()
    return step_in_current_mode(net, x, target)


def step_in_current_mode(net, x, target):
    """... with every module left in the mode it is in (norms put in eval() under net.train())"""
    xr = x.clone().requires_grad_(True)
    out = net(xr)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    gs = torch.autograd.grad(loss, [xr] + [p for _, p in named])
    return dict(out=out.detach(), loss=float(loss.detach()), gx=gs[0], grads={n: g for (n, _), g in zip(named, gs[1:])},
                node=type(out.grad_fn).__name__)


def check_against_fixture(res, net, what=""):
    meta, data = fixture()
    names = list(res["grads"])
    assert names == meta["param_names"] and len(names) == 46
    null = meta["null_gradient_params"]
    ref_norms = dict(zip(names, data["grad_norms"].astype(np.float64)))
    median = float(np.median(data["grad_norms"]))
    fig = dict(output=rel(res["out"], data["output"]), loss=abs(res["loss"] - float(data["loss"])) / abs(float(data["loss"])),
               gx=rel(res["gx"], data["gx"]))
    worst = dict(grad=("", 0.0), norm=("", 0.0), null=("", 0.0), running_var=("", 0.0))

    def note(kind, name, v):
        if v >= worst[kind][1]:
            worst[kind] = (name, v)
    for n in names:
        g = res["grads"][n].detach().cpu()
        key = "grad/" + n if "grad/" + n in data else "gradrows/" + n
        ref = torch.from_numpy(data[key])
        got = g[:ref.shape[0]] if key.startswith("gradrows/") else g
        if n in null:
            assert key.startswith("grad/")
            note("null", n, float((got.double() - ref.double()).norm()) / median)
        else:
            note("grad", n, rel(got, ref))
            note("norm", n, abs(float(g.double().norm()) - ref_norms[n]) / ref_norms[n])
    bufs = dict(net.named_buffers())
    rv_keys = [k for k in data if k.startswith("running_var/")]
    assert len(rv_keys) == sum(1 for k in bufs if k.endswith(".running_var"))
    for k in rv_keys:
        note("running_var", k, rel(bufs[k[12:] + ".running_var"], data[k]))
    print(what, fig, worst)
    assert fig["output"] <= OUT_TOL and fig["loss"] <= OUT_TOL, (what, fig)
    assert fig["gx"] <= GRAD_TOL, (what, fig)
    assert worst["grad"][1] <= GRAD_TOL and worst["norm"][1] <= GRAD_TOL, (what, worst)
    assert worst["null"][1] <= GRAD_TOL, (what, worst)
    assert worst["running_var"][1] <= RV_TOL, (what, worst)
    return fig, worst


def check_same_step(a, b, tol_out, tol, what=""):
    """two steps of the same network and batch through different paths: every gradient within `tol`, the null rule for the null set"""
    meta, data = fixture()
    median = float(np.median(data["grad_norms"]))
    assert rel(a["out"], b["out"]) <= tol_out, (what, rel(a["out"], b["out"]))
    assert rel(a["gx"], b["gx"]) <= tol, (what, "gx", rel(a["gx"], b["gx"]))
    assert list(a["grads"]) == list(b["grads"])
    for n, g in a["grads"].items():
        if n in meta["null_gradient_params"]:
            dist = float((g.double() - b["grads"][n].double()).norm()) / median
        else:
            dist = rel(g, b["grads"][n])
        assert dist <= tol, (what, n, dist)


def scale_running_var(net, factor=1.7):
    """move every running_var away from the batch variance (the fixture's network was calibrated on the fixture's own images, so the
    update (1 - m) rv + m var would otherwise be a no-op that a plan without any update reproduces) -> the buffers before the step"""
    with torch.no_grad():
        for m in net.modules():
            if getattr(m, "running_var", None) is not None:
                m.running_var.mul_(factor)
    return {k: b.clone() for k, b in net.named_buffers()}


def check_buffers(net_a, net_b, before, frozen=(), tol=1e-5, what=""):
    """every buffer of two networks after the same step through different paths: running_var within `tol` AND moved by the step (by
    more than 1e-3, relative) unless its norm is in `frozen` (then bit-equal to before); counts equal"""
    names_frozen = {k for k, m in net_a.named_modules() if any(m is f for f in frozen)}
    bufs_b = dict(net_b.named_buffers())
    n_moved = 0
    for k, a in net_a.named_buffers():
        b = bufs_b[k]
        if k.endswith("running_var"):
            assert rel(a, b) <= tol, (what, k, rel(a, b))
            if k[:-len(".running_var")] in names_frozen:
                assert torch.equal(a, before[k]), (what, k)
            else:
                assert rel(a, before[k]) > 1e-3, (what, k, "not moved")
                n_moved += 1
        elif k.endswith("num_batches_tracked"):
            assert torch.equal(a, b), (what, k)
    return n_moved
