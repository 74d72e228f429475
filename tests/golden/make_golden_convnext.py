"""Generate the ConvNeXt fixtures under tests/golden/ by RUNNING THE REFERENCE on CPU (beside the other generators, which stay as they are).

Run in the build container only:   python tests/golden/make_golden_convnext.py

The reference's bcos/models/convnext.py imports `torchvision.ops.StochasticDepth`; torchvision is not installed, so after
refimport.setup() this generator registers a stand-in `torchvision.ops` whose StochasticDepth is the identity outside training (all the
fixtures run in eval mode) and refuses to run in training mode.  Then the reference's own BcosConvNeXt is what runs, `forward` and
`explain`, in fp32 and in fp64.  Weights are seeded (synth.seed_convnext); recorded are the seed and a state checksum, not the weights.

Files per network: NAME.json (configuration, seeds, state-dict keys and shapes, checksum, execution order of the leaf modules, the
reference's own fp32-vs-fp64 spread d_ref, the top-2 margins), NAME_fp32.npz and NAME_fp64.npz (logits, prediction, weights = W(x),
contribution_map).  Every file stays under 1 MiB.
"""
import copy
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
if "torchvision.ops" not in sys.modules:
    class StochasticDepth(torch.nn.Module):
        def __init__(self, p, mode):
            super().__init__()
            self.p, self.mode = p, mode

        def forward(self, x):
            assert not self.training or self.p == 0.0, "the stand-in is the identity of eval mode only"
            return x

    _ops = types.ModuleType("torchvision.ops")
    _ops.StochasticDepth = StochasticDepth
    sys.modules["torchvision.ops"] = _ops
    sys.modules["torchvision"].ops = _ops
sys.path.append(os.path.join(REPO, "b-cosification_amd"))   # AFTER the reference: only `bcos_hip.synth` is used

import importlib  # noqa: E402

from bcos_hip import synth  # noqa: E402

ref_convnext = importlib.import_module("bcos.models.convnext")
assert ref_convnext.__file__.startswith(refimport.REFERENCE_ROOT), ref_convnext.__file__
torch.set_num_threads(8)

CASES = {
    "convnext_small_cfg": dict(block_setting=[[40, 80, 1], [80, 160, 1], [160, 320, 2], [320, None, 1]], num_classes=12, n_images=3,
                               size=64, first_seed=123),
    "convnext_two": dict(block_setting=[[16, 32, 1], [32, None, 2]], num_classes=10, n_images=3, size=36, first_seed=200),
}
MIN_MARGIN = 1e-2
LEAVES = ("BcosConv2d", "DetachablePositionNorm2d", "StochasticDepth", "AdaptiveAvgPool2d", "LogitLayer")


def state_checksum(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items() if v.dtype.is_floating_point}


def explain_all(net, x):
    """the reference's explanation, one image at a time exactly like BcosUtilMixin.explain"""
    logits, wts, maps, preds = [], [], [], []
    for i in range(x.shape[0]):
        with torch.no_grad():
            logits.append(net(x[i:i + 1]))
        res = net.explain(x[i:i + 1].clone().requires_grad_(True))
        wts.append(res["dynamic_linear_weights"].detach())
        maps.append(res["contribution_map"].detach())
        preds.append(int(res["prediction"]))
    return torch.cat(logits), torch.cat(wts), torch.cat(maps), preds


def exec_order(net, x):
    names = {m: n for n, m in net.named_modules()}
    trace, hooks = [], []
    for m in net.modules():
        if type(m).__name__ in LEAVES:
            hooks.append(m.register_forward_hook(
                lambda mod, inp, res: trace.append([names[mod], type(mod).__name__, list(inp[0].shape), list(res.shape)])))
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return trace


def spread(a, b):
    """max |a - b| per image over the image's max |b|, worst image"""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


def record_case(name, spec):
    net = synth.build_bcos_convnext(spec["block_setting"], spec["num_classes"], seed=0, convnext_module=ref_convnext)
    assert type(net).__module__ == "bcos.models.convnext" and all(m.training is False for m in net.modules())
    net64 = copy.deepcopy(net).double()
    for image_seed in range(spec["first_seed"], spec["first_seed"] + 40):
        x = synth.synthetic_images(spec["n_images"], seed=image_seed, size=spec["size"])
        l32, w32, m32, p32 = explain_all(net, x)
        l64, w64, m64, p64 = explain_all(net64, x.double())
        top2 = l64.topk(2, dim=1).values
        margins = (top2[:, 0] - top2[:, 1]).tolist()
        ok = p32 == p64 == l64.argmax(1).tolist() and min(margins) >= MIN_MARGIN
        print(name, "image seed", image_seed, "classes", p64, "margins", [f"{m:.3f}" for m in margins], "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no image seed met the conditions")
    assert min(margins) >= MIN_MARGIN
    d_ref = dict(logits=float((l32.double() - l64).abs().max()), weights=spread(w32, w64), maps=spread(m32, m64))
    sd = net.state_dict()
    for tag, (lg, w, m, p) in (("fp32", (l32, w32, m32, p32)), ("fp64", (l64, w64, m64, p64))):
        path = os.path.join(HERE, f"{name}_{tag}.npz")
        np.savez_compressed(path, logits=lg.numpy(), prediction=np.array(p), weights=w.numpy(), contribution_map=m.numpy())
        assert os.path.getsize(path) < 1 << 20, path
    with open(os.path.join(HERE, f"{name}.json"), "w") as f:
        json.dump(dict(arch="convnext", block_setting=spec["block_setting"], num_classes=spec["num_classes"], weight_seed=0,
                       image_seed=image_seed, n_images=spec["n_images"], size=spec["size"],
                       state_keys=[[k, list(v.shape)] for k, v in sd.items()], state_checksum=state_checksum(sd),
                       exec_order=exec_order(net, x[:1]),
                       exec_order_note="(module name, class, input shape, output shape) of every leaf module call of one forward of the "
                                       "imported reference on image 0, in execution order",
                       d_ref=d_ref, d_ref_note="the reference in fp32 against the reference in fp64 (same weights): max |logit difference|; "
                                               "W(x) and maps as max |difference| over the image's max |value|, worst image",
                       margins_fp64=margins, min_margin=MIN_MARGIN, logit_bias=float(net.logit_layer.logit_bias),
                       torch_version=torch.__version__), f, indent=1)
    print(name, "d_ref", d_ref)


def tiny_keys():
    net = ref_convnext.convnext_tiny()
    with open(os.path.join(HERE, "convnext_tiny_keys.json"), "w") as f:
        json.dump(dict(note="state-dict keys and shapes of the reference's convnext_tiny()",
                       state_keys=[[k, list(v.shape)] for k, v in net.state_dict().items()]), f)


if __name__ == "__main__":
    for case_name, case_spec in CASES.items():
        record_case(case_name, case_spec)
    tiny_keys()
