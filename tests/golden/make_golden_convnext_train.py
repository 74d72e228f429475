"""Generate the ConvNeXt training-step fixture under tests/golden/ by RUNNING THE REFERENCE on CPU (beside make_golden_convnext.py, which
stays as it is and is not imported: its stand-in StochasticDepth refuses training mode).

Run in the build container only:   python tests/golden/make_golden_convnext_train.py [first image seed, default 300]

The reference's bcos/models/convnext.py imports `torchvision.ops.StochasticDepth`; torchvision is not installed, so after
refimport.setup() this generator registers a stand-in `torchvision.ops` of its own whose StochasticDepth is the identity at p == 0 and
asserts otherwise.  Then one train()-mode step of the reference's own BcosConvNeXt runs: block_setting [[16, 32, 1], [32, None, 2]], 10
classes, stochastic_depth_prob 0, layer_scale 1.0 in the constructor (at the default 1e-6 the block branch, and with it every depthwise
gradient, sits below the fp32 noise of the residual), weights from synth.seed_convnext (seed 0; it redraws layer_scale in [0.25, 1]), 4
images of 36 x 36 (synth.synthetic_images), labels [1, 5, 9, 0], BCE with logits.  Recorded: output, loss, input gradient, EVERY
parameter gradient, the fp64 gradient norms, and the reference's distance from itself (one thread against eight, fp32 against fp64).

An image seed is accepted only if
  * fp32_vs_fp64 <= 2e-5 for the output, the input gradient and every parameter gradient outside the null set (the project's condition
    for holding a shallow fixture to 1e-4), and
  * the null set -- parameters whose fp64 gradient norm is below 1e-2 of the median parameter gradient norm -- is exactly NULL_EXPECTED
    below and contains no depthwise weight.  It is EMPTY: a ConvNeXt has no batch statistics that would cancel a parameter's scale (the
    position norms normalise over channels, their weights are read by the next layer as they are), and although every B-cos filter's
    raw gradient is the projection of the effective filter's onto the complement of the filter (unit-norm layers do not see their own
    length), that projection leaves gradients of ordinary size.
Files: convnext_two_train_step.{json,npz}.
"""
import copy
import importlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import refimport  # noqa: E402

refimport.setup()


class StochasticDepth(torch.nn.Module):
    def __init__(self, p, mode):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x):
        assert self.p == 0.0, "the stand-in is the identity of p == 0 only"
        return x


_ops = types.ModuleType("torchvision.ops")
_ops.StochasticDepth = StochasticDepth
sys.modules["torchvision.ops"] = _ops
sys.modules["torchvision"].ops = _ops
sys.path.append(os.path.join(REPO, "b-cosification_amd"))   # AFTER the reference: only `bcos_hip.synth` is used

from bcos_hip import synth  # noqa: E402

ref_convnext = importlib.import_module("bcos.models.convnext")
assert ref_convnext.__file__.startswith(refimport.REFERENCE_ROOT), ref_convnext.__file__
torch.set_num_threads(8)

STEM = "convnext_two_train_step"
SPEC = dict(block_setting=[[16, 32, 1], [32, None, 2]], num_classes=10, stochastic_depth_prob=0.0, layer_scale=1.0)
LABELS = [1, 5, 9, 0]
N_IMAGES, SIZE = 4, 36
FLOOR_MAX = 2e-5
NULL_FRACTION = 1e-2
NULL_EXPECTED = []


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def reference_convnext():
    stages = [ref_convnext.CNBlockConfig(*s) for s in SPEC["block_setting"]]
    torch.manual_seed(0)
    net = ref_convnext.BcosConvNeXt(stages, num_classes=SPEC["num_classes"], stochastic_depth_prob=SPEC["stochastic_depth_prob"],
                                    layer_scale=SPEC["layer_scale"])
    assert type(net).__module__ == "bcos.models.convnext"
    return synth.seed_convnext(net, 0)


def is_depthwise(net, name):
    mod = net.get_submodule(name.rsplit(".", 1)[0])
    return isinstance(mod, torch.nn.Conv2d) and mod.groups > 1


def _step(net, x, target):
    net.train()
    xr = x.clone().requires_grad_(True)
    out = net(xr)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(loss, [xr] + [p for _, p in named])
    return out.detach(), loss.detach(), grads[0], [n for n, _ in named], list(grads[1:])


def _dist(a, b, names, null):
    per = {n: rel(u, v) for n, u, v in zip(names, a[4], b[4])}
    return dict(output=rel(a[0], b[0]), gx=rel(a[2], b[2]), worst_param=max(v for n, v in per.items() if n not in null),
                worst_depthwise=max(v for n, v in per.items() if n in DEPTHWISE), null_params={n: per[n] for n in null})


DEPTHWISE = []


def record(first_seed=300):
    base = reference_convnext()
    DEPTHWISE[:] = [n for n, _ in base.named_parameters() if is_depthwise(base, n)]
    assert len(DEPTHWISE) == sum(s[2] for s in SPEC["block_setting"]), DEPTHWISE
    target = torch.nn.functional.one_hot(torch.tensor(LABELS), SPEC["num_classes"]).float()
    for image_seed in range(first_seed, first_seed + 20):
        x = synth.synthetic_images(N_IMAGES, seed=image_seed, size=SIZE)
        f64 = _step(copy.deepcopy(base).double(), x.double(), target.double())
        norms64 = torch.stack([g.norm() for g in f64[4]])
        names = f64[3]
        null = [n for n, v in zip(names, norms64) if float(v) < NULL_FRACTION * float(norms64.median())]
        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        one = _step(copy.deepcopy(base), x, target)
        torch.set_num_threads(nt)
        step = _step(copy.deepcopy(base), x, target)
        floors = dict(one_thread_vs_eight=_dist(one, step, names, null), fp32_vs_fp64=_dist(step, f64, names, null))
        f = floors["fp32_vs_fp64"]
        ok = (null == NULL_EXPECTED and not set(null) & set(DEPTHWISE)
              and max(f["output"], f["gx"], f["worst_param"]) <= FLOOR_MAX)
        print("image seed", image_seed, "null set", null, "floors", floors, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit("no image seed met the conditions")
    out_t, loss, gx, names, grads = step
    arrays = dict(output=out_t.numpy(), loss=loss.numpy(), gx=gx.numpy(),
                  grad_norms=torch.stack([g.double().norm() for g in grads]).numpy())
    arrays.update({"grad/" + n: g.numpy() for n, g in zip(names, grads)})
    np.savez_compressed(os.path.join(HERE, STEM + ".npz"), **arrays)
    with open(os.path.join(HERE, STEM + ".json"), "w") as fh:
        json.dump(dict(arch="convnext", **SPEC, weight_seed=0, image_seed=image_seed, n_images=N_IMAGES, size=SIZE, labels=LABELS,
                       loss="bce_with_logits", param_names=names, depthwise_params=list(DEPTHWISE), null_gradient_params=null,
                       null_fraction_of_median=NULL_FRACTION, grad_norms_fp64={n: float(v) for n, v in zip(names, norms64)},
                       median_grad_norm_fp64=float(norms64.median()), reference_self_floor=floors,
                       reference_self_floor_note="relative L2 distance of the reference's own train()-mode step from itself; worst_param "
                                                 "is over the parameters outside null_gradient_params",
                       torch_version=torch.__version__), fh, indent=1)
    for ext in (".npz", ".json"):
        size = os.path.getsize(os.path.join(HERE, STEM + ext))
        assert size < (1 << 20), (ext, size)
        print("written", STEM + ext, size, "bytes")


if __name__ == "__main__":
    record(int(sys.argv[1]) if len(sys.argv) > 1 else 300)
