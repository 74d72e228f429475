"""Generate the uncentered-norm fixtures under tests/golden/ by RUNNING THE REFERENCE's own classes on the CPU, in fp32 and in fp64.

Run in the build container only:   python tests/golden/make_golden_unorms.py

Modules (bcos/modules/norms/uncentered_norms of the reference): PositionNormUncentered2d at a vector width and at a ragged one (the
latter through NoBias), GroupNormUncentered2d with an intermediate group count, GNInstanceNormUncentered2d, GNLayerNormUncentered2d
(through Unaffine), AllNormUncentered2d in train() (momentum 0.1), in train() with momentum=None (two steps: the cumulative average) and
in eval().  Inputs have a mean of the size of their spread, so the centred norm would give other numbers.  Recorded per module:
    y            output
    gx_expl      input gradient of sum(y * cot) under set_explanation_mode(True)
    gx, gw, gb   training-mode gradients (nothing detached) of input, weight and bias
    running_var  after the step(s)                                                          (AllNorm)
Every array is kept in fp64 (what the GPU test compares with) and the reference's own fp32-vs-fp64 distance, max |a32 - a64| / max |a64|,
goes into the JSON.  The GPU test holds a layer to TOL = 1e-5 of the tensor's maximum; a fixture whose own distance exceeds TOL / 10 is
refused here, so the reference alone stays well within the tolerance.
The second file, unorms_surface.json, records what the classes look like from outside: bases, constructor signatures, `__all__`, parameter
shapes, state-dict keys and the names NoBias / Unaffine give -- the list tests/test_norms_uncentered_cpu.py compares ours with.
Files: unorms.{json,npz}, unorms_surface.json.
"""
import copy
import importlib
import inspect
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
norms = importlib.import_module("bcos.modules.norms")
unc = importlib.import_module("bcos.modules.norms.uncentered_norms")
assert norms.__file__.startswith(refimport.REFERENCE_ROOT), norms.__file__

STEM = "unorms"
TOL = 1e-5

# name -> (factory, input shape, mode, steps)
SPECS = {
    "pnu_c20": (lambda: norms.PositionNormUncentered2d(20), (2, 20, 5, 7), "train", 1),
    "pnu_c6_nobias": (lambda: norms.NoBias(norms.PositionNormUncentered2d)(6, eps=1e-6), (2, 6, 5, 7), "train", 1),
    "gnu_g4_c12": (lambda: norms.GroupNormUncentered2d(4, 12), (2, 12, 5, 7), "train", 1),
    "gnu_instance_c12": (lambda: norms.GNInstanceNormUncentered2d(12), (2, 12, 5, 7), "train", 1),
    "gnu_layer_c12_unaffine": (lambda: norms.Unaffine(norms.GNLayerNormUncentered2d)(12), (2, 12, 5, 7), "train", 1),
    "allnorm_train": (lambda: norms.AllNormUncentered2d(8), (3, 8, 5, 7), "train", 1),
    "allnorm_train_cma": (lambda: norms.AllNormUncentered2d(8, momentum=None), (3, 8, 5, 7), "train", 2),
    "allnorm_eval": (lambda: norms.AllNormUncentered2d(8), (3, 8, 5, 7), "eval", 1),
}


def build(name):
    make, shape, mode, steps = SPECS[name]
    g = torch.Generator().manual_seed(sum(name.encode()))
    m = make()
    with torch.no_grad():
        for p in (m.weight, m.bias):
            if p is not None:
                p.copy_(torch.randn(p.shape, generator=g) * 0.5 + (1.0 if p is m.weight else 0.0))
        if getattr(m, "running_var", None) is not None:
            m.running_var.fill_(0.7)
    x = torch.randn(shape, generator=g) * 1.3 + 0.8
    cot = torch.randn(shape, generator=g)
    m.train(mode == "train")
    return m, x, cot


def run(m, x, cot, steps):
    """-> dict of results of the LAST step; the steps before it see x * 1.5 + 0.3, x * 2.0 + 0.6, ... and only move the statistics"""
    m = copy.deepcopy(m)
    for s in range(steps - 1, 0, -1):
        with torch.no_grad():
            m(x * (1 + 0.5 * s) + 0.3 * s)
    r = {}
    params = [p for p in (m.weight, m.bias) if p is not None]
    stats = copy.deepcopy(m.state_dict())
    m.set_explanation_mode(True)
    xe = x.clone().requires_grad_(True)
    r["gx_expl"] = torch.autograd.grad((m(xe) * cot).sum(), xe)[0]
    m.set_explanation_mode(False)
    m.load_state_dict(stats)                                  # (the explanation pass of a train()-mode AllNorm moved the statistics)
    xt = x.clone().requires_grad_(True)
    y = m(xt)
    grads = torch.autograd.grad((y * cot).sum(), [xt] + params)
    r["y"], r["gx"] = y.detach(), grads[0]
    rest = list(grads[1:])
    if m.weight is not None:
        r["gw"] = rest.pop(0)
    if m.bias is not None:
        r["gb"] = rest.pop(0)
    if getattr(m, "running_var", None) is not None:
        r["running_var"] = m.running_var.detach().clone()
        r["num_batches_tracked"] = m.num_batches_tracked.detach().clone().double()
    return r


def dist(a32, a64):
    return float((a32.double() - a64).abs().max() / a64.abs().max().clamp_min(1e-300))


def surface():
    out = {"uncentered_norms.__all__": {}}
    for mod in ("posnorm_uncentered", "groupnorm_uncentered", "allnorm_uncentered"):
        out["uncentered_norms.__all__"][mod] = list(importlib.import_module("bcos.modules.norms.uncentered_norms." + mod).__all__)
    makers = {"PositionNormUncentered2d": (16,), "GroupNormUncentered2d": (4, 16), "GNInstanceNormUncentered2d": (16,),
              "GNLayerNormUncentered2d": (16,), "AllNormUncentered2d": (16,)}
    for cls_name, args in makers.items():
        cls = getattr(norms, cls_name)
        m = cls(*args)
        sig = inspect.signature(cls.__init__)
        entry = dict(
            bases=[b.__name__ for b in cls.__mro__[1:] if b.__name__ in ("LayerNorm", "GroupNorm", "BatchNorm2d", "DetachableModule",
                                                                         "GroupNormUncentered2d")],
            init=[[n, str(p.kind), None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in sig.parameters.items()],
            args=list(args), eps=m.eps,
            parameters={n: list(p.shape) for n, p in m.named_parameters()},
            state_dict={k: list(v.shape) for k, v in m.state_dict().items()},
            detach_default=bool(m.detach),
            nobias=dict(name=norms.NoBias(cls)(*args)._get_name(), factory=norms.NoBias(cls).__name__,
                        state_dict=list(norms.NoBias(cls)(*args).state_dict().keys())),
            unaffine=dict(name=norms.Unaffine(cls)(*args)._get_name(), factory=norms.Unaffine(cls).__name__,
                          state_dict=list(norms.Unaffine(cls)(*args).state_dict().keys())))
        for attr in ("normalized_shape", "num_groups", "num_channels", "num_features", "momentum", "affine", "elementwise_affine",
                     "track_running_stats", "features"):
            if hasattr(m, attr):
                v = getattr(m, attr)
                entry[attr] = list(v) if isinstance(v, tuple) else v
        out[cls_name] = entry
    fn = unc.group_norm_uncentered
    out["group_norm_uncentered"] = [[n, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                    for n, p in inspect.signature(fn).parameters.items()]
    fa = importlib.import_module("bcos.modules.norms.uncentered_norms.allnorm_uncentered").all_norm_uncentered_2d
    out["all_norm_uncentered_2d"] = [[n, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                     for n, p in inspect.signature(fa).parameters.items()]
    return out


def record():
    arrays, meta = {}, {}
    for name, (_, shape, mode, steps) in SPECS.items():
        m, x, cot = build(name)
        r32 = run(m, x, cot, steps)
        r64 = run(copy.deepcopy(m).double(), x.double(), cot.double(), steps)
        floors = {k: dist(r32[k], r64[k]) for k in r64}
        bad = {k: v for k, v in floors.items() if v > TOL / 10}
        if bad:
            raise SystemExit(f"{name}: the reference's own fp32-vs-fp64 distance exceeds a tenth of the tolerance {TOL}: {bad}")
        arrays[name + "/x"], arrays[name + "/cot"] = x.numpy(), cot.numpy()
        for k, p in (("weight", m.weight), ("bias", m.bias), ("running_var", getattr(m, "running_var", None))):
            if p is not None:
                arrays[f"{name}/{k}"] = p.detach().numpy()
        for k in r64:
            arrays[f"{name}/f64/{k}"] = r64[k].numpy()
            arrays[f"{name}/f32/{k}"] = r32[k].numpy()
        meta[name] = dict(cls=type(m).__name__, shape=list(shape), mode=mode, steps=steps, eps=m.eps, outputs=sorted(r64),
                          fp32_vs_fp64=floors)
        print(name, floors)
    np.savez_compressed(os.path.join(HERE, STEM + ".npz"), **arrays)
    with open(os.path.join(HERE, STEM + ".json"), "w") as fh:
        json.dump(dict(tolerance=TOL, distance="max |a - b| / max |b|", modules=meta, torch_version=torch.__version__), fh, indent=1)
    with open(os.path.join(HERE, STEM + "_surface.json"), "w") as fh:
        json.dump(surface(), fh, indent=1)
    for fn in (STEM + ".npz", STEM + ".json", STEM + "_surface.json"):
        size = os.path.getsize(os.path.join(HERE, fn))
        assert size < (1 << 20), (fn, size)
        print("written", fn, size, "bytes")


if __name__ == "__main__":
    record()
