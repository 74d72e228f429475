"""Generate the RISE fixtures under tests/golden/ by RUNNING THE REFERENCE (its
interpretability/explanation_methods/explainers/rise.py) on CPU.  Build container only:   python tests/golden/make_golden_rise.py

  rise.{json,npz}   two cases on the resnet18_e2e fixture network (the weights and calibration record of make_golden.py):
                      r32   32 x 32,  n = 64, s = 4, p1 = 0.1
                      r48   48 x 48,  n = 96, s = 6, p1 = 0.5 (as the constructor argument)
                    per case: the masks the reference's own generate_masks / load_masks produced (float32, as load_masks keeps them),
                    the logits its model calls returned and the probabilities it made of them -- for CLASSES of the 1000 (the targets
                    and a seeded draw; a B-cos network's probability of a class is the sigmoid of that class's logit alone) -- the map
                    of `attribute` for the first of three targets and of `attribute_selection` for all three, each once in float32 and
                    once with network, image and masks in float64, and the reference's own fp32-vs-fp64 spread of the maps over the map
                    peak (`d_ref`).  Square images only: the reference reloads its masks when W != H.

The reference's rise.py is loaded by file path (its package __init__ imports captum).  The one thing it takes from skimage is
`resize(grid, up_size, order=1, mode="reflect", anti_aliasing=False)`; skimage is not installed, so a stand-in `skimage.transform` is
registered first whose `resize` checks those arguments and calls `scipy.ndimage.zoom(grid, up / s, order=1, mode="mirror",
grid_mode=True)` -- the call current skimage makes for them.  Equality with skimage's own bits is therefore unverified.  The reference
writes its masks under ./target/rise_masks: the process works in a temporary directory.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference import: oracle/refimport.py)
import numpy as np  # noqa: E402
import scipy.ndimage  # noqa: E402
import torch  # noqa: E402
from oracle import refimport  # noqa: E402

from bcos_hip import synth  # noqa: E402

CASES = [  # name, size, image seed, constructor arguments
    ("r32", 32, 601, dict(n=64, s=4, p1=0.1, batch_size=8)),
    ("r48", 48, 602, dict(n=96, s=6, p1=0.5, batch_size=8)),
]
N_CLASSES_KEPT = 64
SEED = 2026


def install_skimage_standin():
    def resize(image, output_shape, order=None, mode="reflect", anti_aliasing=None, **rest):
        assert order == 1 and mode == "reflect" and anti_aliasing is False and not rest, (order, mode, anti_aliasing, rest)
        image = np.asarray(image)
        out_shape = tuple(int(v) for v in output_shape)
        assert image.ndim == 2 and all(float(v) == int(v) for v in output_shape)
        zoom = tuple(o / i for o, i in zip(out_shape, image.shape))
        out = scipy.ndimage.zoom(image.astype(np.float64), zoom, order=1, mode="mirror", grid_mode=True)
        assert out.shape == out_shape
        return out
    sk, tr = types.ModuleType("skimage"), types.ModuleType("skimage.transform")
    sk.__path__ = []
    tr.resize = resize
    sk.transform = tr
    sys.modules.update({"skimage": sk, "skimage.transform": tr})


def reference_rise():
    install_skimage_standin()
    path = os.path.join(refimport.REFERENCE_ROOT, "interpretability", "explanation_methods", "explainers", "rise.py")
    spec = importlib.util.spec_from_file_location("_reference_rise", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RISE


class Recorder(torch.nn.Module):
    """the model under the explainer, keeping what every call returned"""

    def __init__(self, net):
        super().__init__()
        self.net, self.calls = net, []
        if hasattr(net, "to_probabilities"):
            self.to_probabilities = net.to_probabilities

    def forward(self, x):
        out = self.net(x)
        self.calls.append(out.detach().clone())
        return out


def run(Rise, net, img, kwargs, targets, double):
    rec = Recorder(net)
    ex = Rise(rec, **kwargs)
    H = img.shape[-1]
    path = ex.PATH_TEMPLATE.format(H=int(H), n=ex.N, s=ex.s)
    masks32 = ex.load_masks(path)                                   # the reference's generate_masks + load_masks: float32 [n, 1, H, W]
    if double:
        ex.masks = torch.from_numpy(np.load(path))                  # what generate_masks saved, before load_masks' .float()
        assert ex.masks.dtype == torch.float64 and torch.equal(ex.masks.float(), masks32)
    one = ex.attribute(img, [targets[0]])
    logits = torch.cat(rec.calls)
    assert logits.shape[0] == ex.N
    sel = ex.attribute_selection(img, targets)
    return dict(masks=masks32[:, 0], logits=logits, scores=rec.to_probabilities(logits), map=one, selection=sel)


def main():
    work = tempfile.mkdtemp(prefix="rise_golden_")
    os.chdir(work)
    Rise = reference_rise()
    base = json.load(open(os.path.join(HERE, "resnet18_e2e.json")))
    gold = np.load(os.path.join(HERE, "resnet18_e2e.npz"))
    net = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(gold["calib/" + k]) for k in base["calib_order"]})
    assert net.to_probabilities is torch.sigmoid                    # (the recorded class subset relies on it)
    net64 = MG.reference_resnet(base["arch"], seed=base["weight_seed"])
    net64.load_state_dict(net.state_dict())
    net64 = net64.double().eval()
    rng = np.random.default_rng(SEED)
    out, meta = {}, dict(net_fixture="resnet18_e2e", arch=base["arch"], score_mode="sigmoid", cases=[], torch_version=torch.__version__,
                         numpy_version=np.__version__, scipy_version=scipy.__version__,
                         resize="scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) standing in for skimage.transform.resize")
    for name, size, seed, kwargs in CASES:
        img = synth.synthetic_images(1, seed=seed, size=size)
        with torch.no_grad():
            logits = net(img)[0]
        order = torch.argsort(logits, descending=True)
        targets = [int(order[0]), int(order[1]), int((int(order[0]) + 333) % 1000)]
        assert len(set(targets)) == 3
        r32 = run(Rise, net, img, kwargs, targets, False)
        r64 = run(Rise, net64, img.double(), kwargs, targets, True)
        assert all(torch.isfinite(v).all() for v in list(r32.values()) + list(r64.values()))
        assert r32["map"].shape == (1, 1, size, size) and r32["selection"].shape == (3, 1, size, size)
        assert r32["masks"].dtype == torch.float32 and torch.equal(r32["masks"], r64["masks"])
        extra = [int(c) for c in rng.permutation(1000) if int(c) not in targets][:N_CLASSES_KEPT - 3]
        classes = torch.tensor(sorted(targets + extra))
        out[f"{name}/masks"], out[f"{name}/classes"], out[f"{name}/targets"] = r32["masks"], classes, torch.tensor(targets)
        for tag, r in (("", r32), ("64", r64)):
            out[f"{name}/logits{tag}"] = r["logits"][:, classes]
            out[f"{name}/scores{tag}"] = r["scores"][:, classes]
            out[f"{name}/map{tag}"] = r["map"]
            out[f"{name}/selection{tag}"] = r["selection"]
        peak = float(r64["selection"].abs().max())
        d_ref = float((r32["selection"].double() - r64["selection"]).abs().max()) / peak
        score_spread = float((r32["scores"].double() - r64["scores"]).norm() / r64["scores"].norm())
        meta["cases"].append(dict(name=name, size=size, image_seed=seed, kwargs=kwargs, n_masks=int(r32["masks"].shape[0]), targets=targets,
                                  n_classes=1000, classes_kept=int(classes.numel()), d_ref=d_ref, scores_fp32_vs_fp64_rel_l2=score_spread,
                                  map_peak=peak))
        print(name, "masks", tuple(r32["masks"].shape), "targets", targets, "d_ref", d_ref, "score spread", score_spread)
    np.savez_compressed(os.path.join(HERE, "rise.npz"), **MG.t2n(out))
    with open(os.path.join(HERE, "rise.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("rise.npz:", os.path.getsize(os.path.join(HERE, "rise.npz")), "bytes")


if __name__ == "__main__":
    main()
