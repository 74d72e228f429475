"""Generate the DenseNet training-step fixture under tests/golden/ by RUNNING THE REFERENCE on CPU (beside make_golden_densenet.py, whose
`reference_densenet` / `TINY` it imports and which stays as it is).

Run in the build container only:   python tests/golden/make_golden_densenet_train.py [first image seed, default 40]

One train()-mode step of the reference's DenseNetBcos inside the reference's BcosifyNetwork (TINY spec, weight seed 0) on 4 images of
64 x 64 (synth.synthetic_images), calibrated on those images (synth.calibrate), labels [1, 5, 11, 0] of 12 classes, BCE with logits:
output, loss, input gradient, the fp64 norm and the values of EVERY parameter gradient (leading rows where a gradient is large: every
committed file stays under 1 MiB), every running_var after the step, and the reference's distance from itself (one thread against
eight, fp32 against fp64).

An image seed is accepted only if
  * fp32_vs_fp64 <= 2e-5 for the output, the input gradient and every parameter gradient outside the null set (the project's condition
    for holding a shallow fixture to 1e-4), and
  * the null set -- parameters whose fp64 gradient norm is below 1e-2 of the median parameter gradient norm -- is exactly
    ["model.features.1.weight"]: norm0's weight.  Every reader of slice 0 of the first block normalises each channel by its own batch
    standard deviation, so the loss does not depend on that channel's scale; the exact gradient is zero and what is recorded is
    cancellation noise.
Files: densenet_tiny_train_step.{json,npz}.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_densenet as MG  # noqa: E402  (sets the reference up, replaces the torchvision DenseNet stand-in)

synth = MG.synth
STEM = "densenet_tiny_train_step"
LABELS = [1, 5, 11, 0]
FLOOR_MAX = 2e-5
NULL_FRACTION = 1e-2
NULL_EXPECTED = ["model.features.1.weight"]
ROWS_ABOVE = 1 << 14          # gradients of this many elements or more: leading rows of <= ROWS_KEEP elements
ROWS_KEEP = 1 << 12


def _step(net, x, target):
    net.train()
    xr = x.clone().requires_grad_(True)
    out = net(xr)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(loss, [xr] + [p for _, p in named])
    net.eval()
    return out.detach(), loss.detach(), grads[0], [n for n, _ in named], list(grads[1:])


def _dist(a, b, names, null):
    """(output, gx, parameter gradients) of two steps -> relative L2 distances; the worst parameter outside the null set"""
    per = {n: MG.rel(u, v) for n, u, v in zip(names, a[4], b[4])}
    return dict(output=MG.rel(a[0], b[0]), gx=MG.rel(a[2], b[2]), worst_param=max(v for n, v in per.items() if n not in null),
                null_params={n: per[n] for n in null})


def record(first_seed=40):
    base = MG.reference_densenet(MG.TINY, seed=0)
    target = torch.nn.functional.one_hot(torch.tensor(LABELS), MG.TINY["num_classes"]).float()
    for image_seed in range(first_seed, first_seed + 20):
        x = synth.synthetic_images(4, seed=image_seed, size=64)
        net = copy.deepcopy(base)
        calib = synth.calibrate(net, x)
        sd = copy.deepcopy(net.state_dict())
        f64 = _step(copy.deepcopy(net).double(), x.double(), target.double())
        norms64 = torch.stack([g.norm() for g in f64[4]])
        names = f64[3]
        null = [n for n, v in zip(names, norms64) if float(v) < NULL_FRACTION * float(norms64.median())]
        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        one = _step(copy.deepcopy(net), x, target)
        torch.set_num_threads(nt)
        step = _step(net, x, target)               # (this one moves net's running_var: recorded below)
        floors = dict(one_thread_vs_eight=_dist(one, step, names, null), fp32_vs_fp64=_dist(step, f64, names, null))
        f = floors["fp32_vs_fp64"]
        ok = null == NULL_EXPECTED and max(f["output"], f["gx"], f["worst_param"]) <= FLOOR_MAX
        print("image seed", image_seed, "null set", null, "floors", floors, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit("no image seed met the conditions")
    out_t, loss, gx, names, grads = step
    arrays = dict(output=out_t.numpy(), loss=loss.numpy(), gx=gx.numpy(),
                  grad_norms=torch.stack([g.double().norm() for g in grads]).numpy())
    for n, g in zip(names, grads):
        if g.numel() >= ROWS_ABOVE:
            arrays["gradrows/" + n] = g[:max(1, ROWS_KEEP // g[0].numel())].numpy()
        else:
            arrays["grad/" + n] = g.numpy()
    for n, b in net.named_buffers():
        if n.endswith(".running_var"):
            arrays["running_var/" + n[:-len(".running_var")]] = b.detach().numpy()
    moved = {n: MG.rel(b, sd[n]) for n, b in net.named_buffers() if n.endswith(".running_var")}
    # (how far the step moved each buffer from its calibrated value: norm0 was calibrated on these very images, its update is a no-op;
    #  behind the first train()-mode norm the activations differ from the calibration pass)
    print("running_var moved by", {n: f"{v:.1e}" for n, v in moved.items()})
    arrays.update({f"calib/{k}": v.numpy() for k, v in calib.items()})
    np.savez_compressed(os.path.join(HERE, STEM + ".npz"), **arrays)
    with open(os.path.join(HERE, STEM + ".json"), "w") as fh:
        json.dump(dict(arch="densenet", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in MG.TINY.items()}, weight_seed=0,
                       image_seed=image_seed, n_images=4, size=64, labels=LABELS, loss="bce_with_logits", param_names=names,
                       calib_order=list(calib.keys()), null_gradient_params=null, null_fraction_of_median=NULL_FRACTION,
                       grad_norms_fp64={n: float(v) for n, v in zip(names, norms64)}, median_grad_norm_fp64=float(norms64.median()),
                       reference_self_floor=floors,
                       reference_self_floor_note="relative L2 distance of the reference's own train()-mode step from itself; worst_param "
                                                 "is over the parameters outside null_gradient_params",
                       torch_version=torch.__version__), fh, indent=1)
    size = os.path.getsize(os.path.join(HERE, STEM + ".npz"))
    assert size < (1 << 20), size
    print("written", STEM, size, "bytes")


if __name__ == "__main__":
    record(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
