"""Generate the DenseNet fixtures under tests/golden/ by RUNNING THE REFERENCE on CPU (beside make_golden.py, which stays as it is).

Run in the build container only:   python tests/golden/make_golden_densenet.py [tiny] [d121] [trace]

oracle/refimport.py stubs `torchvision.models.DenseNet` with an empty class (the reference only subclasses it at import time).  Here the
stub is replaced, after refimport.setup() and BEFORE the first import of the reference's bcos.models.standard_models, by the torchvision
topology restated in b-cosification_amd/bcos/models/_tv_densenet.py, so that the reference's own DenseNetBcos (standard_models.py:56-63)
inside the reference's own BcosifyNetwork is what runs; the pool swap and the removal of every bias are the reference's
(bcosification/model.py:45-55, through synth.finish_conversion).  Weights are seeded and calibrated (synth.calibrate); recorded in the
resnet50_small style: weight seed, calibration record and state checksum, not the weights.

Files: densenet_tiny.{json,npz}, densenet121_small.{json,npz} + densenet121_small_w{image}{a,b}.npz (W(x) of one image, channels 0-2 /
3-5: every file stays under 1 MiB), densenet_exec_trace.json.
"""
import copy
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import refimport  # noqa: E402

refimport.setup()
if getattr(sys.modules.get("torchvision"), "_bcos_standin", False):
    _spec = importlib.util.spec_from_file_location(
        "_tv_densenet_standin", os.path.join(REPO, "b-cosification_amd", "bcos", "models", "_tv_densenet.py"))
    _tvd = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(_tvd)
    assert "bcos.models.standard_models" not in sys.modules, "the reference's standard_models was imported before the DenseNet stand-in"
    sys.modules["torchvision.models"].DenseNet = _tvd.DenseNet
sys.path.append(os.path.join(REPO, "b-cosification_amd"))   # AFTER the reference: only `bcos_hip.synth` is used

from bcos_hip import synth  # noqa: E402

R = refimport.modules()
torch.set_num_threads(8)

TINY = dict(growth=32, block_config=(2, 3, 2, 2), init_features=64, bn_size=2, num_classes=12)
D121 = dict(growth=32, block_config=(6, 12, 24, 16), init_features=64, bn_size=4, num_classes=1000)
D_REF_TINY_MAX = 3e-5


def reference_densenet(spec, seed=0):
    cfg = synth.densenet_model_config(spec["num_classes"])
    std = synth.standard_densenet(spec["growth"], spec["block_config"], spec["init_features"], spec["bn_size"], spec["num_classes"], seed,
                                  densenet_cls=R.standard_models.DenseNetBcos)
    net = R.bcosify.BcosifyNetwork(std, cfg, add_channels=True, logit_layer=True)
    synth.finish_conversion(net, cfg, hip_pools=False)
    assert type(net.model.features[3]).__name__ == "AvgPool2d"
    assert all(getattr(m, "bias", None) is None for m in net.modules())
    return net.eval()


def state_checksum(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items() if v.dtype.is_floating_point}


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


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


def record_case(name, spec, n_images, size, first_seed, d_ref_max=None, split_weights=False):
    net = reference_densenet(spec)
    for image_seed in range(first_seed, first_seed + 20):
        x = synth.synthetic_images(n_images, seed=image_seed, size=size)
        cand = copy.deepcopy(net)
        record = synth.calibrate(cand, x)
        logits, wts, maps, preds = explain_all(cand, x)
        l64, w64, m64, p64 = explain_all(copy.deepcopy(cand).double(), x.double())
        d_ref = dict(logits=rel(logits, l64), weights=rel(wts, w64), maps=rel(maps, m64))
        ok = preds == p64 and preds == logits.argmax(1).tolist() and all(np.isfinite(v) for v in d_ref.values())
        if ok and d_ref_max is not None:
            ok = max(d_ref.values()) <= d_ref_max
        print(name, "image seed", image_seed, "classes", preds, p64, "d_ref", d_ref, "ok" if ok else "rejected")
        if ok:
            break
    else:
        raise SystemExit(f"{name}: no image seed met the conditions")
    sd = {k: v.detach().clone() for k, v in cand.state_dict().items()}
    arrays = dict(logits=logits.numpy(), prediction=np.array(preds), contribution_map=maps.numpy(),
                  **{f"calib/{k}": v.numpy() for k, v in record.items()})
    if split_weights:
        for i in range(n_images):
            np.savez_compressed(os.path.join(HERE, f"{name}_w{i}a.npz"), weights=wts[i, :3].numpy())
            np.savez_compressed(os.path.join(HERE, f"{name}_w{i}b.npz"), weights=wts[i, 3:].numpy())
    else:
        arrays["weights"] = wts.numpy()
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **arrays)
    with open(os.path.join(HERE, f"{name}.json"), "w") as f:
        json.dump(dict(arch="densenet", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in spec.items()}, weight_seed=0,
                       image_seed=image_seed, n_images=n_images, size=size, calib_images=n_images, calib_order=list(record.keys()),
                       state_keys=[[k, list(v.shape)] for k, v in sd.items()], state_checksum=state_checksum(sd),
                       d_ref=d_ref, d_ref_note="relative L2 distance of the reference in fp32 from the reference in fp64 (same weights)",
                       logit_bias=float(cand.logit_layer.logit_bias), torch_version=torch.__version__), f, indent=1)


def exec_trace():
    net = reference_densenet(D121)
    names = {m: n for n, m in net.named_modules()}
    trace, hooks = [], []

    def hook(m, inp, res):
        trace.append([names[m], type(m).__name__, list(inp[0].shape), list(res.shape)])

    for m in net.modules():
        if type(m).__name__ in ("BcosifyConv2d", "BatchNormUncentered2d", "AvgPool2d", "ReLU", "LogitLayer", "Normalize"):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net(synth.synthetic_images(1, seed=5))
    for h in hooks:
        h.remove()
    with open(os.path.join(HERE, "densenet_exec_trace.json"), "w") as f:
        json.dump(dict(note="(module name, class, input shape, output shape) of every B-cos conv / norm / pool / ReLU module call of ONE forward "
                            "of the imported reference DenseNet-121 on a [1, 6, 224, 224] image, in execution order; the ReLU behind norm5 and the "
                            "global pool are functional calls and leave no entry (make_golden_densenet.py: exec_trace)",
                       densenet121=trace), f)
    print("trace:", len(trace), "calls")


if __name__ == "__main__":
    which = sys.argv[1:] or ["tiny", "d121", "trace"]
    if "tiny" in which:
        record_case("densenet_tiny", TINY, 3, 64, first_seed=123, d_ref_max=D_REF_TINY_MAX)
    if "d121" in which:
        record_case("densenet121_small", D121, 2, 224, first_seed=123, split_weights=True)
    if "trace" in which:
        exec_trace()
