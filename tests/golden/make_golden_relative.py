"""Generate the fixtures of the mean-corrected and the contrastive explanation under tests/golden/ by RUNNING THE REFERENCE's network on
CPU.  Build container only:   python tests/golden/make_golden_relative.py

  relative.json, relative_fp32.npz, relative_mean64.npz, relative_contrast64.npz
        on the resnet18_e2e fixture network (the weights and calibration record of make_golden.py) and images 0 and 1 of that fixture,
        each explained alone as make_golden.py explains them, under the reference's `explanation_mode()`:
            mean      x * d(y_t - mean_k y_k) / dx     t = the arg-max class of the image
            contrast  x * d(y_a - y_b) / dx            a = the arg-max class, b chosen as described below
        summed over the six channels ([2, 224, 224] per functional), once in float32 and once with network and image in float64, and the
        fp32-vs-fp64 distance of every map (relative L2 and worst element over the map's peak).  One .npz per float64 functional keeps
        every file under 1 MiB.

The maps come from plain torch.autograd.  The reference's own OursRelative (interpretability/explanation_methods/explainers/ours.py:16-71)
wraps the network in captum's InputXGradient, and captum is not installed here; what it differentiates -- its
`model_forward_with_mean_subtracted` -- is three lines: run the model, assert a 2-D output, return `out - out.mean(dim=1, keepdim=True)`.
They are restated in `mean_subtracted` below; Input x Gradient of a selected output is `x * autograd.grad(out[0, t], x)`.

Contrast classes: y_a - y_b cancels when the two logits are close, and the map then sits on the rounding of the two passes.  The pair is the
first of (top-1, top-2), (top-1, the class of median logit), (top-1, the class of lowest logit) whose fp32-vs-fp64 relative L2 distance is at
most 3e-5; every pair after the first has a logit gap above the image's median gap between consecutive sorted logits.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference import: oracle/refimport.py)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bcos_hip import synth  # noqa: E402

MAX_SELF_DISTANCE = 3e-5


def mean_subtracted(net, x):
    out = net(x)
    assert out.dim() == 2
    return out - out.mean(dim=1, keepdim=True)


def ixg_map(net, x, fn):
    """channel-summed Input x Gradient of the scalar fn(net, x) under explanation_mode(), [H, W]"""
    xi = x.clone().requires_grad_(True)
    with torch.enable_grad(), net.explanation_mode():
        (g,) = torch.autograd.grad(fn(net, xi), xi)
    return (x * g).sum(1)[0].detach()


def distance(m32, m64):
    d = m32.double() - m64
    return float(d.norm() / m64.norm()), float(d.abs().max() / m64.abs().max())


def main():
    base = json.load(open(os.path.join(HERE, "resnet18_e2e.json")))
    gold = np.load(os.path.join(HERE, "resnet18_e2e.npz"))
    net = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(gold["calib/" + k]) for k in base["calib_order"]})
    net64 = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    net64.load_state_dict(net.state_dict())
    net, net64 = net.eval(), net64.double().eval()
    x = synth.synthetic_images(base["n_images"], seed=base["image_seed"])[:2]
    maps = {k: [] for k in ("mean32", "mean64", "contrast32", "contrast64")}
    meta = dict(net_fixture="resnet18_e2e", arch=base["arch"], images=[0, 1], cases=[], torch_version=torch.__version__,
                max_self_distance=MAX_SELF_DISTANCE)
    for i in range(2):
        xi = x[i:i + 1]
        with torch.no_grad():
            logits = net(xi)[0]
        assert torch.equal(logits, torch.from_numpy(gold["logits"][i]))
        order = torch.argsort(logits, descending=True)
        t = int(order[0])
        mean = lambda n, xx: mean_subtracted(n, xx)[0, t]                    # noqa: E731
        m32, m64 = ixg_map(net, xi, mean), ixg_map(net64, xi.double(), mean)
        gaps = (logits[order][:-1] - logits[order][1:])
        median_gap = float(gaps.median())
        tried = []
        for b in (int(order[1]), int(order[len(order) // 2]), int(order[-1])):
            con = lambda n, xx: n(xx)[0, t] - n(xx)[0, b]                    # noqa: E731
            c32, c64 = ixg_map(net, xi, con), ixg_map(net64, xi.double(), con)
            d = distance(c32, c64)
            tried.append(dict(b=b, logit_gap=float(logits[t] - logits[b]), rel_l2=d[0], worst_over_peak=d[1]))
            if d[0] <= MAX_SELF_DISTANCE:
                break
        else:
            raise SystemExit(f"image {i}: no contrast pair within {MAX_SELF_DISTANCE}: {tried}")
        assert len(tried) == 1 or tried[-1]["logit_gap"] > median_gap
        for k, v in (("mean32", m32), ("mean64", m64), ("contrast32", c32), ("contrast64", c64)):
            assert torch.isfinite(v).all()
            maps[k].append(v)
        dm = distance(m32, m64)
        meta["cases"].append(dict(image=i, target=t, contrast=[t, b], median_logit_gap=median_gap, contrast_pairs_tried=tried,
                                  mean_fp32_vs_fp64=dict(rel_l2=dm[0], worst_over_peak=dm[1]),
                                  contrast_fp32_vs_fp64=dict(rel_l2=tried[-1]["rel_l2"], worst_over_peak=tried[-1]["worst_over_peak"])))
        print("image", i, "target", t, "contrast", (t, b), "mean fp32-vs-fp64", dm, "contrast", tried)
    stack = {k: torch.stack(v) for k, v in maps.items()}
    files = dict(relative_fp32=dict(mean=stack["mean32"], contrast=stack["contrast32"]), relative_mean64=dict(mean=stack["mean64"]),
                 relative_contrast64=dict(contrast=stack["contrast64"]))
    for name, arrays in files.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **MG.t2n(arrays))
        print(name + ".npz:", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)
    with open(os.path.join(HERE, "relative.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
