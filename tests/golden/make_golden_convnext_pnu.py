"""Generate the fixtures of the B-cos ConvNeXt with UNCENTERED position norms under tests/golden/ by RUNNING THE REFERENCE on CPU (beside
make_golden_convnext.py and make_golden_convnext_train.py, which stay as they are and are not imported).

Run in the build container only:   python tests/golden/make_golden_convnext_pnu.py

The `convnext_two` configuration -- block_setting [[16, 32, 1], [32, None, 2]], 10 classes -- built by the reference's own BcosConvNeXt with
norm_layer = NoBias(PositionNormUncentered2d), weights from synth.seed_convnext (seed 0).  torchvision is not installed: as in the other
two generators a stand-in `torchvision.ops.StochasticDepth` (the identity at p == 0, an assertion otherwise) is registered first.
  convnext_two_pnu.json, _fp32.npz, _fp64.npz     eval mode, 3 images of 36 x 36: logits, prediction, W(x) and contribution maps of
                                                  `explain`, one image at a time, in fp32 and fp64 (as make_golden_convnext.py records them)
  convnext_two_pnu_train_step.{json,npz}          one train()-mode BCE step, layer_scale 1.0 in the constructor, 4 images, labels
                                                  [1, 5, 9, 0]: output, loss, input gradient, every parameter gradient (as
                                                  make_golden_convnext_train.py records them)
Each JSON carries the reference's own fp32-vs-fp64 distance in the measure the GPU test uses, and a fixture whose distance exceeds a TENTH
of the tolerance the GPU test applies is refused (the next image seed is tried): eval 1e-4 on logits (absolute), W(x) and maps (per image,
of the image's maximum) -> 1e-5; training step 1e-5 on output and loss, 1e-4 on the gradients (relative L2) -> 1e-6 and 1e-5.
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
ref_norms = importlib.import_module("bcos.modules.norms")
assert ref_convnext.__file__.startswith(refimport.REFERENCE_ROOT) and ref_norms.__file__.startswith(refimport.REFERENCE_ROOT)
torch.set_num_threads(8)

STEM = "convnext_two_pnu"
SPEC = dict(block_setting=[[16, 32, 1], [32, None, 2]], num_classes=10)
NORM = "NoBias(PositionNormUncentered2d)"
EVAL_TOL, OUT_TOL, GRAD_TOL = 1e-4, 1e-5, 1e-4
MIN_MARGIN = 1e-2
LABELS = [1, 5, 9, 0]


def build(**kw):
    stages = [ref_convnext.CNBlockConfig(*s) for s in SPEC["block_setting"]]
    torch.manual_seed(0)
    net = ref_convnext.BcosConvNeXt(stages, num_classes=SPEC["num_classes"],
                                    norm_layer=ref_norms.NoBias(ref_norms.PositionNormUncentered2d), **kw)
    assert type(net).__module__ == "bcos.models.convnext"
    norms = [m for m in net.modules() if isinstance(m, torch.nn.LayerNorm)]
    assert norms and all(type(m).__name__ == "PositionNormUncentered2d" and m.bias is None for m in norms)
    return synth.seed_convnext(net, 0)


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


def spread(a, b):
    """max |a - b| per image over the image's max |b|, worst image"""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def record_eval(n_images=3, size=36, first_seed=200):
    net = build().eval()
    net64 = copy.deepcopy(net).double()
    for image_seed in range(first_seed, first_seed + 40):
        x = synth.synthetic_images(n_images, seed=image_seed, size=size)
        l32, w32, m32, p32 = explain_all(net, x)
        l64, w64, m64, p64 = explain_all(net64, x.double())
        top2 = l64.topk(2, dim=1).values
        margins = (top2[:, 0] - top2[:, 1]).tolist()
        d_ref = dict(logits=float((l32.double() - l64).abs().max()), weights=spread(w32, w64), maps=spread(m32, m64))
        ok = p32 == p64 == l64.argmax(1).tolist() and min(margins) >= MIN_MARGIN and max(d_ref.values()) <= EVAL_TOL / 10
        print("eval: image seed", image_seed, "classes", p64, "margins", [f"{m:.3f}" for m in margins], d_ref, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit("eval: no image seed met the conditions")
    for tag, (lg, w, m, p) in (("fp32", (l32, w32, m32, p32)), ("fp64", (l64, w64, m64, p64))):
        path = os.path.join(HERE, f"{STEM}_{tag}.npz")
        np.savez_compressed(path, logits=lg.numpy(), prediction=np.array(p), weights=w.numpy(), contribution_map=m.numpy())
        assert os.path.getsize(path) < 1 << 20, path
    sd = net.state_dict()
    with open(os.path.join(HERE, STEM + ".json"), "w") as f:
        json.dump(dict(arch="convnext", norm_layer=NORM, **SPEC, weight_seed=0, image_seed=image_seed, n_images=n_images, size=size,
                       state_keys=[[k, list(v.shape)] for k, v in sd.items()], tolerance=EVAL_TOL, d_ref=d_ref,
                       d_ref_note="the reference in fp32 against the reference in fp64 (same weights): max |logit difference|; W(x) and "
                                  "maps as max |difference| over the image's max |value|, worst image; at most a tenth of `tolerance`",
                       margins_fp64=margins, min_margin=MIN_MARGIN, torch_version=torch.__version__), f, indent=1)


def _step(net, x, target):
    net.train()
    xr = x.clone().requires_grad_(True)
    out = net(xr)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(loss, [xr] + [p for _, p in named])
    return out.detach(), loss.detach(), grads[0], [n for n, _ in named], list(grads[1:])


def record_train(n_images=4, size=36, first_seed=300):
    base = build(stochastic_depth_prob=0.0, layer_scale=1.0)
    target = torch.nn.functional.one_hot(torch.tensor(LABELS), SPEC["num_classes"]).float()
    for image_seed in range(first_seed, first_seed + 40):
        x = synth.synthetic_images(n_images, seed=image_seed, size=size)
        f64 = _step(copy.deepcopy(base).double(), x.double(), target.double())
        f32 = _step(copy.deepcopy(base), x, target)
        names = f64[3]
        per = {n: rel(a, b) for n, a, b in zip(names, f32[4], f64[4])}
        floor = dict(output=rel(f32[0], f64[0]), loss=abs(float(f32[1]) - float(f64[1])) / abs(float(f64[1])), gx=rel(f32[2], f64[2]),
                     worst_param=max(per.values()))
        ok = max(floor["output"], floor["loss"]) <= OUT_TOL / 10 and max(floor["gx"], floor["worst_param"]) <= GRAD_TOL / 10
        print("train: image seed", image_seed, floor, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit("train: no image seed met the conditions")
    out_t, loss, gx, names, grads = f64
    arrays = dict(output=out_t.numpy(), loss=loss.numpy(), gx=gx.float().numpy())
    arrays.update({"grad/" + n: g.float().numpy() for n, g in zip(names, grads)})
    path = os.path.join(HERE, STEM + "_train_step.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 1 << 20
    with open(os.path.join(HERE, STEM + "_train_step.json"), "w") as f:
        json.dump(dict(arch="convnext", norm_layer=NORM, **SPEC, stochastic_depth_prob=0.0, layer_scale=1.0, weight_seed=0,
                       image_seed=image_seed, n_images=n_images, size=size, labels=LABELS, loss="bce_with_logits", param_names=names,
                       precision="the fp64 step (gradients stored rounded to fp32)", out_tolerance=OUT_TOL, grad_tolerance=GRAD_TOL,
                       reference_self_floor=floor, per_param_fp32_vs_fp64=per,
                       reference_self_floor_note="relative L2 distance of the reference's fp32 step from its fp64 step; at most a tenth "
                                                 "of the tolerances", torch_version=torch.__version__), f, indent=1)


if __name__ == "__main__":
    record_eval()
    record_train()
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith(STEM):
            print("written", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
