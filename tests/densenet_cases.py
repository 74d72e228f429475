"""Shared by test_densenet_cpu.py and test_densenet_gpu.py (TEST INFRASTRUCTURE): the networks of the DenseNet fixtures rebuilt from
their recorded seeds and calibration, the recorded outputs, and the measures the issue's bounds are stated in."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def worst_over_peak(a, b):
    """largest |a - b| of an image over that image's largest |b|, maximised over the images"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    n = b.shape[0]
    return float(((a - b).abs().reshape(n, -1).amax(1) / b.abs().reshape(n, -1).amax(1)).max())


def load(stem):
    meta = json.load(open(os.path.join(GOLDEN, stem + ".json")))
    data = dict(np.load(os.path.join(GOLDEN, stem + ".npz")))
    if "weights" not in data:           # W(x) of the 224 x 224 case: one file per image and channel half
        data["weights"] = np.stack([np.concatenate([np.load(os.path.join(GOLDEN, f"{stem}_w{i}{h}.npz"))["weights"] for h in "ab"])
                                    for i in range(meta["n_images"])])
    return meta, data


def golden_net(stem):
    """-> (net on the CPU, meta, data, images): this package's modules with the fixture's weights"""
    from bcos_hip import synth
    meta, data = load(stem)
    net = synth.build_bcosified_densenet(meta["growth"], tuple(meta["block_config"]), meta["init_features"], meta["bn_size"],
                                         meta["num_classes"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"])
    return net, meta, data, x


def state_checksum(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items() if v.dtype.is_floating_point}


def check_against_fixture(out, data, bound_logits, bound_maps, what=""):
    """the issue's bounds: logits and classes; W(x) and maps in relative L2 AND in the worst element per image over the map's peak"""
    figures = dict(logits=rel(out["logits"], data["logits"]),
                   weights=rel(out["dynamic_linear_weights"], data["weights"]),
                   weights_worst=worst_over_peak(out["dynamic_linear_weights"], data["weights"]),
                   maps=rel(out["contribution_map"], data["contribution_map"]),
                   maps_worst=worst_over_peak(out["contribution_map"], data["contribution_map"]))
    print(what, figures)
    assert figures["logits"] <= bound_logits, (what, figures)
    assert np.array_equal(out["prediction"].cpu().numpy(), data["prediction"]), what
    for k in ("weights", "weights_worst", "maps", "maps_worst"):
        assert figures[k] <= bound_maps, (what, k, figures)
    return figures


def completeness_residual(x, out, logit_bias):
    """per image |sum m - (logit - logit_bias)| / sum |m| with m = sum_c (x - mean_c) W(x)_c: the network is linear in the NORMALISED
    input (bcosify.py: Normalize in front), so the map that sums to the bias-free logit is the one of x - mean"""
    from bcosify import IMAGENET_MEAN_ADDINVERSE
    mean = torch.tensor(IMAGENET_MEAN_ADDINVERSE, device=x.device).view(1, 6, 1, 1)
    m = ((x - mean) * out["dynamic_linear_weights"]).double().sum(1)
    n = x.shape[0]
    logit = out["logits"][torch.arange(n), out["explained_class_idx"]].double()
    return ((m.sum((1, 2)) - (logit - logit_bias)).abs() / m.abs().sum((1, 2))).cpu()
