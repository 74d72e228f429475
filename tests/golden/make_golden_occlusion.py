"""Generate the Occlusion fixtures under tests/golden/ by RUNNING THE REFERENCE (its
interpretability/explanation_methods/explainers/occlusion.py) on CPU.  Build container only:   python tests/golden/make_golden_occlusion.py

  occlusion.{json,npz}   four cases on the resnet18_e2e fixture network (the weights and calibration record of make_golden.py):
                           d64       64 x 64,  "default"  (stride 32, ks 32:   4 masks)
                           occ9_32   32 x 32,  "Occ9"     (stride 2,  ks 9:  256 masks)
                           occ5p_32  32 x 32,  "Occ5" with only_positive=True (256 masks)
                           occ9ti_48 48 x 48,  "Occ9-TI"  (stride 4,  ks 9:  144 masks; the reference's [n_masks, 1000, H, W]
                                                          intermediate is 2.7 GB in float64 at this size)
                         per case: the rectangles read back from the reference's `masks` (every mask is checked to BE one rectangle), n_part,
                         the logits the reference's model calls returned (org_out, pert_out), three targets, the map of `attribute` for the
                         first and of `attribute_selection` for all three -- each once in float32 and once with network and image in float64
                         -- and the reference's own fp32-vs-fp64 spread of the maps.  The logits are recorded for CLASSES of the 1000 (the
                         targets and a seeded draw), which keeps the file under 1 MiB; the maps of a class depend on that class's logits only.

The reference's occlusion.py is loaded by file path (its package __init__ imports captum); its `attribute` ends in `.cuda()`, which this process
makes an identity.
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference import: oracle/refimport.py)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import refimport  # noqa: E402

from bcos_hip import synth  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self          # (this process only: the reference's attribute() ends in .cuda())

CASES = [  # name, size, image seed, config name, constructor arguments
    ("d64", 64, 501, "default", {}),
    ("occ9_32", 32, 502, "Occ9", dict(ks=9, stride=2)),
    ("occ5p_32", 32, 503, "Occ5", dict(ks=5, stride=2, only_positive=True)),
    ("occ9ti_48", 48, 504, "Occ9-TI", dict(ks=9, stride=4, batch_size=1)),
]
N_CLASSES_KEPT = 64
SEED = 2025


def reference_occlusion():
    path = os.path.join(refimport.REFERENCE_ROOT, "interpretability", "explanation_methods", "explainers", "occlusion.py")
    spec = importlib.util.spec_from_file_location("_reference_occlusion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Occlusion


class Recorder(torch.nn.Module):
    """the model under the explainer, keeping what every call returned"""

    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, []

    def forward(self, x):
        out = self.net(x)
        self.calls.append(out.detach().clone())
        return out


def rects_of(masks):
    """[n, 1, H, W] 0/1 masks -> int32 [n, 4] (r0, r1, c0, c1); asserts that the zeros of every mask are exactly one rectangle"""
    out = []
    for m in masks[:, 0]:
        zr = torch.nonzero((m == 0).any(1)).flatten()
        zc = torch.nonzero((m == 0).any(0)).flatten()
        r0, r1, c0, c1 = int(zr[0]), int(zr[-1]) + 1, int(zc[0]), int(zc[-1]) + 1
        rebuilt = torch.ones_like(m)
        rebuilt[r0:r1, c0:c1] = 0
        assert torch.equal(rebuilt, m)
        out.append((r0, r1, c0, c1))
    return torch.tensor(out, dtype=torch.int32)


def run(Occ, net, img, kwargs, targets):
    rec = Recorder(net)
    ex = Occ(rec, **kwargs)
    one = ex.attribute(img, targets[0])
    org, pert = rec.calls[0], torch.cat(rec.calls[1:])
    sel = ex.attribute_selection(img, targets)
    return ex, dict(org_out=org, pert_out=pert, map=one, selection=sel)


def main():
    Occ = reference_occlusion()
    base = json.load(open(os.path.join(HERE, "resnet18_e2e.json")))
    gold = np.load(os.path.join(HERE, "resnet18_e2e.npz"))
    net = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(gold["calib/" + k]) for k in base["calib_order"]})
    net64 = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    net64.load_state_dict(net.state_dict())
    net64 = net64.double().eval()
    rng = np.random.default_rng(SEED)
    out, meta = {}, dict(net_fixture="resnet18_e2e", arch=base["arch"], cases=[], torch_version=torch.__version__)
    for name, size, seed, config, kwargs in CASES:
        img = synth.synthetic_images(1, seed=seed, size=size)
        with torch.no_grad():
            logits = net(img)[0]
        order = torch.argsort(logits, descending=True)
        targets = [int(order[0]), int(order[1]), int((int(order[0]) + 333) % 1000)]
        assert len(set(targets)) == 3
        ex, r32 = run(Occ, net, img, kwargs, targets)
        _, r64 = run(Occ, net64, img.double(), kwargs, targets)
        rects = rects_of(ex.masks)
        n_part = ex.n_part.reshape(-1)
        assert torch.equal(n_part, ((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])).to(n_part.dtype))
        assert all(torch.isfinite(v).all() for v in list(r32.values()) + list(r64.values()))
        assert r32["map"].shape == (1, 1, size, size) and r32["selection"].shape == (3, 1, size, size)
        assert torch.equal(r32["selection"][:1], r32["map"])
        extra = [int(c) for c in rng.permutation(1000) if int(c) not in targets][:N_CLASSES_KEPT - 3]
        classes = torch.tensor(sorted(targets + extra))
        out[f"{name}/rects"], out[f"{name}/n_part"], out[f"{name}/classes"] = rects, n_part.to(torch.int64), classes
        out[f"{name}/targets"] = torch.tensor(targets)
        for tag, r in (("", r32), ("64", r64)):
            out[f"{name}/org_out{tag}"] = r["org_out"][:, classes]
            out[f"{name}/pert_out{tag}"] = r["pert_out"][:, classes]
            out[f"{name}/map{tag}"] = r["map"]
            out[f"{name}/selection{tag}"] = r["selection"]
        peak = float(r64["selection"].abs().max())
        spread = float((r32["selection"].double() - r64["selection"]).abs().max()) / peak
        logit_spread = float((r32["pert_out"].double() - r64["pert_out"]).norm() / r64["pert_out"].norm())
        meta["cases"].append(dict(name=name, size=size, image_seed=seed, config=config, kwargs=kwargs, n_masks=int(rects.shape[0]),
                                  targets=targets, n_classes=1000, classes_kept=int(classes.numel()),
                                  reference_self_floor=dict(map_fp32_vs_fp64_over_peak=spread, logits_fp32_vs_fp64_rel_l2=logit_spread),
                                  map_peak=peak))
        print(name, "masks", int(rects.shape[0]), "targets", targets, "map spread / peak", spread, "logit spread", logit_spread)
    np.savez_compressed(os.path.join(HERE, "occlusion.npz"), **MG.t2n(out))
    with open(os.path.join(HERE, "occlusion.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("occlusion.npz:", os.path.getsize(os.path.join(HERE, "occlusion.npz")), "bytes")


if __name__ == "__main__":
    main()
