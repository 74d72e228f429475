"""The Occlusion explainer without a device: the registry, the rectangle rule, the explainer's host logic on emulated kernels
(tests/occlusion_emulation.py) against a plain float64 evaluation of the formula on the logits the reference recorded
(tests/golden/make_golden_occlusion.py), and the argument checks of the two entry points (ABI v12)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import occlusion_emulation as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CONFIGS = {"default": dict(stride=(32, 32), ks=32, batch_size=8), "Occ5": dict(stride=(2, 2), ks=5, batch_size=8),
           "Occ9": dict(stride=(2, 2), ks=9, batch_size=8), "Occ9-TI": dict(stride=(4, 4), ks=9, batch_size=1),
           "Occ13-TI": dict(stride=(4, 4), ks=13, batch_size=1)}


def fixture():
    return json.load(open(os.path.join(GOLDEN, "occlusion.json"))), np.load(os.path.join(GOLDEN, "occlusion.npz"))


class RecordedModel(torch.nn.Module):
    """stands in for the network: the first call returns the recorded logits of the image, the later ones those of the occluded copies
    in mask order, whatever the chunking; it also checks that every copy IS `img * mask_i`"""

    def __init__(self, img, org, pert, rects):
        super().__init__()
        self.img, self.org, self.pert, self.rects, self.next, self.batches = img, org, pert, rects, None, []

    def forward(self, x):
        if self.next is None:
            assert torch.equal(x, self.img)
            self.next = 0
            return self.org.clone()
        lo, hi = self.next, self.next + x.shape[0]
        H, W = x.shape[-2:]
        assert torch.equal(x, self.img * E.keep_masks(self.rects[lo:hi], H, W))
        self.next = hi
        self.batches.append(x.shape[0])
        return self.pert[lo:hi].clone()


def emulated(monkeypatch):
    from bcos_hip import ops
    monkeypatch.setattr(ops, "occlusion_accumulate", E.occlusion_accumulate)
    monkeypatch.setattr(ops, "prep_input_occluded", E.prep_input_occluded)


def case_setup(case, data, batch_size=None):
    from bcos_hip import synth
    from interpretability.explanation_methods.explainers.occlusion import Occlusion
    name = case["name"]
    img = synth.synthetic_images(1, seed=case["image_seed"], size=case["size"])
    rects = torch.from_numpy(data[f"{name}/rects"])
    org, pert = torch.from_numpy(data[f"{name}/org_out"]), torch.from_numpy(data[f"{name}/pert_out"])
    kw = dict(case["kwargs"])
    if batch_size is not None:
        kw["batch_size"] = batch_size

    def make():
        model = RecordedModel(img, org, pert, rects)
        return Occlusion(model, **kw), model
    classes = data[f"{name}/classes"].tolist()
    local = [classes.index(t) for t in case["targets"]]          # the targets as indices into the recorded class subset
    return img, rects, org, pert, make, local


# ---------------------------------------------------------------------------------------------------------------------- registry
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_registry_builds_every_named_configuration(name, capsys):
    from interpretability.explanation_methods.explainers import OUT_OF_SCOPE, get_explainer
    from interpretability.explanation_methods.explainers.occlusion import Occlusion
    net = torch.nn.Identity()
    occ = get_explainer(net, "Occlusion", name)
    assert isinstance(occ, Occlusion) and occ.model is net
    assert (occ.stride, occ.ks, occ.batch_size, occ.only_positive) == (CONFIGS[name]["stride"], CONFIGS[name]["ks"], CONFIGS[name]["batch_size"], False)
    assert occ.max_imgs_bs == 1
    assert capsys.readouterr().out == ""                          # (the reference prints its batch size from __init__)
    assert "Occlusion" not in OUT_OF_SCOPE and "RISE" in OUT_OF_SCOPE
    assert get_explainer(net, "Occlusion", name, only_positive=True).only_positive is True


def test_the_other_baselines_stay_out_of_scope():
    from interpretability.explanation_methods.explainers import get_explainer
    for name in ("RISE", "LIME", "GCam", "IntGrad", "GB", "DeepLIFT"):
        with pytest.raises(KeyError, match="out of scope"):
            get_explainer(torch.nn.Identity(), name, "default")
    with pytest.raises(KeyError):
        get_explainer(torch.nn.Identity(), "Occlusion", "Occ7")


# ---------------------------------------------------------------------------------------------------------------------- masks
def test_make_masks_reproduces_the_recorded_rectangles():
    from interpretability.explanation_methods.explainers.occlusion import Occlusion
    meta, data = fixture()
    assert [c["name"] for c in meta["cases"]] == ["d64", "occ9_32", "occ5p_32", "occ9ti_48"]
    for case in meta["cases"]:
        kw = {k: v for k, v in case["kwargs"].items()}
        occ = Occlusion(None, **kw)
        occ.make_masks(torch.empty(1, 6, case["size"], case["size"]))
        assert occ.masks.dtype == torch.int32 and occ.masks.shape == (case["n_masks"], 4)
        assert np.array_equal(occ.masks.numpy(), data[f"{case['name']}/rects"]), case["name"]
        assert np.array_equal(occ.n_part.numpy(), data[f"{case['name']}/n_part"]), case["name"]


def test_make_masks_keeps_the_quirks_of_the_rule():
    from interpretability.explanation_methods.explainers.occlusion import Occlusion
    occ = Occlusion(None, stride=4, ks=9)                          # odd ks: a window of ks - 1 = 8, centred on the grid point
    occ.make_masks(torch.empty(1, 6, 16, 16))
    assert occ.masks.tolist()[0] == [0, 4, 0, 4] and occ.masks.tolist()[5] == [0, 8, 0, 8]
    # the slow index of the position grid selects the COLUMNS: mask 1 moves down, mask 4 moves right
    assert occ.masks.tolist()[1] == [0, 8, 0, 4] and occ.masks.tolist()[4] == [0, 4, 0, 8]
    assert int(occ.n_part.max()) == 64
    occ = Occlusion(None, stride=8, ks=10)                         # even ks: rows [(h + 1) s - ks, h s + ks), clipped to the image
    occ.make_masks(torch.empty(1, 6, 16, 16))
    assert occ.masks.tolist() == [[0, 10, 0, 10], [6, 16, 0, 10], [0, 10, 6, 16], [6, 16, 6, 16]]
    with pytest.raises(ValueError, match="empty"):                  # an even ks under the stride: rows [s - ks, ks) of the first mask
        Occlusion(None, stride=8, ks=4).make_masks(torch.empty(1, 6, 16, 16))


def test_make_masks_refuses_what_the_reference_cannot_attribute():
    from interpretability.explanation_methods.explainers.occlusion import Occlusion
    with pytest.raises(ValueError, match="multiple of the stride"):
        Occlusion(None, stride=32, ks=32).make_masks(torch.empty(1, 6, 48, 64))
    with pytest.raises(ValueError, match="multiple of the stride"):
        Occlusion(None, stride=(2, 4), ks=5).make_masks(torch.empty(1, 6, 32, 30))
    with pytest.raises(ValueError, match="empty"):                  # non-square: the column index runs over the rows' grid
        Occlusion(None, stride=32, ks=32).make_masks(torch.empty(1, 6, 128, 64))
    with pytest.raises(ValueError, match="empty"):
        Occlusion(None, stride=2, ks=1).make_masks(torch.empty(1, 6, 8, 8))


# ---------------------------------------------------------------------------------------------------------------------- explainer
@pytest.mark.parametrize("index", range(4))
def test_explainer_equals_the_float64_formula_on_the_recorded_logits(index, monkeypatch):
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][index]
    img, rects, org, pert, make, local = case_setup(case, data)
    H = W = case["size"]
    pos = bool(case["kwargs"].get("only_positive", False))
    ref_all, mag, cover = E.formula64(org, pert, rects, H, W, None, pos)
    bound = E.chain_bound(mag, cover)
    assert int(cover.min()) >= 1 and float(bound.max()) > 0

    occ, model = make()
    one = occ.attribute(img, local[0])
    assert one.shape == (1, 1, H, W) and one.dtype == torch.float32 and one.device == img.device
    assert model.next == case["n_masks"] and max(model.batches) <= occ.batch_size
    assert bool(((one[0, 0].double() - ref_all[local[0]]).abs() <= bound[local[0]]).all())

    occ, _ = make()
    sel = occ.attribute_selection(img, local)
    assert sel.shape == (3, 1, H, W)
    assert bool(((sel[:, 0].double() - ref_all[local]).abs() <= bound[local]).all())
    assert torch.equal(sel[:1], one)                                # a class's map does not depend on which other classes are asked for
    occ, _ = make()
    assert torch.equal(occ.attribute_selection(img, torch.tensor(local)), sel)

    occ, _ = make()
    full = occ.attribute(img, None, return_all=True)
    assert full.shape == (1, org.shape[1], H, W)
    assert bool(((full[0].double() - ref_all).abs() <= bound).all())
    assert torch.equal(full[0, local][:, None], sel)

    # the map the reference recorded for the same logits (its own fp32 sum, in torch's order): twice the chain bound
    rec = torch.from_numpy(data[f"{case['name']}/selection"])[:, 0].double()
    assert bool(((sel[:, 0].double() - rec).abs() <= 2 * bound[local]).all())
    if pos:
        assert float(sel.min()) >= 0.0


def test_result_does_not_depend_on_the_chunk_size(monkeypatch):
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][1]
    outs, batches = [], []
    for bs in (1, 8, 100, 1000):
        img, _, _, _, make, local = case_setup(case, data, batch_size=bs)
        occ, model = make()
        outs.append(occ.attribute_selection(img, local))
        batches.append(max(model.batches))
    assert batches == [1, 8, 100, 256]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


def test_images_are_processed_one_at_a_time(monkeypatch):
    emulated(monkeypatch)
    from interpretability.explanation_methods.explainers.occlusion import Occlusion

    class Net(torch.nn.Module):
        def forward(self, x):
            assert x.shape[0] <= 4
            return torch.stack([x[:, 0].mean((1, 2)), x[:, 1, :8].sum((1, 2)), -x[:, 2].amax((1, 2))], dim=1)
    x = torch.rand(3, 6, 16, 16, generator=torch.Generator().manual_seed(3))
    occ = Occlusion(Net(), stride=8, ks=8, batch_size=4)
    out = occ.attribute(x, [0, 1, 2])
    assert out.shape == (3, 1, 16, 16)
    for i, t in enumerate((0, 1, 2)):
        assert torch.equal(out[i:i + 1], occ.attribute(x[i:i + 1], t))
    assert torch.equal(occ.attribute(x, torch.tensor([0, 1, 2])), out)
    assert occ.attribute(x, 1).shape == (3, 1, 16, 16)              # one class for every image
    assert occ.attribute(x, None, return_all=True).shape == (3, 3, 16, 16)
    with pytest.raises(ValueError):
        occ.attribute(x, [0, 1])
    with pytest.raises(ValueError):
        occ.attribute_selection(x, [0, 1])                          # the reference reads image 0 only: one image here


def test_engine_path_asks_for_occluded_forwards(monkeypatch):
    """with a fused engine attached nothing is masked on the host: every chunk is one engine.forward(img, occlude=bank[lo:hi])"""
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][1]
    img, rects, org, pert, make, local = case_setup(case, data)
    occ, model = make()
    want = occ.attribute_selection(img, local)

    class Engine:
        calls = []

        def forward(self, x, occlude=None):
            assert torch.equal(x, img)
            if occlude is None:
                return org.clone()
            lo = sum(self.calls)
            assert torch.equal(occlude, rects[lo:lo + occlude.shape[0]]) and occlude.dtype == torch.int32
            self.calls.append(occlude.shape[0])
            return pert[lo:lo + occlude.shape[0]].clone()

    class Net(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the module path must not run")
    for chunk, calls in ((None, [256]), (100, [100, 100, 56])):
        net = Net().eval()
        object.__setattr__(net, "_bcos_engine", Engine())
        Engine.calls = []
        from interpretability.explanation_methods.explainers.occlusion import Occlusion
        occ = Occlusion(net, **case["kwargs"])
        assert occ.engine_batch_size == 256
        if chunk:
            occ.engine_batch_size = chunk
        assert torch.equal(occ.attribute_selection(img, local), want)
        assert Engine.calls == calls


def test_harness_takes_an_explainer(monkeypatch):
    from bcos_hip import localisation, ops

    class Expl:
        def attribute_selection(self, img, tgts):
            assert img.shape[0] == 1 and list(tgts) == [3, 1, 2, 0]
            return torch.stack([img[0] * (t + 1) for t in tgts])    # [T, C, H, W]
    monkeypatch.setattr(ops, "localisation_fractions", lambda att, ch, cw, neg=False: torch.eye(4)[None].repeat(att.shape[0] // 4, 1, 1).view(-1, 4))
    x = torch.rand(2, 6, 8, 8)
    tg = torch.tensor([[3, 1, 2, 0], [3, 1, 2, 0]])
    a = localisation.grid_pointing_game(None, x, tg, 4, explainer=Expl())
    assert a["attributions"].shape == (2, 4, 8, 8)
    assert torch.equal(a["attributions"][1, 0], x[1].sum(0) * 4)
    b = localisation.grid_pointing_game(None, x, tg, 4, attributions=a["attributions"])
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------- emulation
def test_emulated_prepared_input_is_the_prepared_masked_copy():
    x = torch.rand(1, 6, 9, 7, generator=torch.Generator().manual_seed(1))
    mean, std = torch.rand(6), torch.rand(6) + 0.5
    rects = torch.tensor([[0, 3, 0, 2], [2, 9, 1, 7], [4, 5, 6, 7], [0, 9, 0, 7]], dtype=torch.int32)
    out = E.prep_input_occluded(x, rects, mean, std, first=1, n=2)
    assert out.shape == (2, 9, 7, 8) and torch.equal(out[..., 6:], torch.zeros(2, 9, 7, 2))
    assert torch.equal(out, E.prep_input(x * E.keep_masks(rects[1:3], 9, 7), mean, std))
    inside = out[0, 2:9, 1:7, :6]
    assert torch.equal(inside, ((0 - mean) / std).expand_as(inside))


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_library_agree_on_abi_12(hip_lib):
    from bcos_hip import lib
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header)
    for name in ("bcos_prep_input_occluded", "bcos_occlusion_accumulate"):
        assert re.search(r"\bint " + name + r"\(", header) and name in lib.SIGNATURES
        assert getattr(hip_lib, name) is not None
    assert lib.ABI_VERSION == 12 and hip_lib.bcos_version() == 12
    assert "bcos_occlusion.hip" in lib.SOURCES


def test_abi_refuses_malformed_arguments(hip_lib):
    fake = C.c_void_p(1 << 20)
    bank = (C.c_int32 * 8)(0, 4, 0, 4, 2, 6, 1, 5)
    host = C.cast(bank, C.c_void_p)
    prep = lambda **k: hip_lib.bcos_prep_input_occluded(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", fake), ("rects", fake), ("out", fake), ("mean", fake), ("std", fake), ("am", None), ("n", 2), ("Cx", 6), ("H", 8), ("W", 8),
        ("Cpad", 8), ("add_inverse", 0), ("stream", None))])
    for bad in (dict(x=None), dict(rects=None), dict(out=None), dict(mean=None), dict(std=None), dict(n=0), dict(n=-1), dict(H=0), dict(W=-2),
                dict(Cpad=5), dict(Cx=3, add_inverse=1), dict(Cx=3), dict(add_inverse=1), dict(rects=C.c_void_p((1 << 20) + 4))):
        assert prep(**bad) == -22, bad
        assert b"bcos_prep_input_occluded" in hip_lib.bcos_last_error_string()
    acc = lambda **k: hip_lib.bcos_occlusion_accumulate(*[k.get(a, d) for a, d in (  # noqa: E731
        ("org", fake), ("pert", fake), ("rects", fake), ("host", host), ("targets", fake), ("out", fake), ("n", 2), ("CL", 10), ("T", 3),
        ("H", 8), ("W", 8), ("pos", 0), ("stream", None))])
    for bad in (dict(org=None), dict(pert=None), dict(rects=None), dict(out=None), dict(n=0), dict(CL=0), dict(T=0), dict(T=-1), dict(H=0),
                dict(W=0), dict(targets=None), dict(rects=C.c_void_p((1 << 20) + 8)), dict(H=5), dict(W=4)):       # (the bank leaves a 5 x 8 / 8 x 4 image)
        assert acc(**bad) == -22, bad
        assert b"bcos_occlusion_accumulate" in hip_lib.bcos_last_error_string()
    for rect in ((3, 3, 0, 4), (0, 4, 2, 2), (5, 2, 0, 4), (-1, 4, 0, 4)):
        bank[4:8] = rect
        assert acc() == -22 and acc(targets=None, T=10) == -22, rect


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    x = torch.zeros(1, 6, 8, 8)
    with pytest.raises(BcosHipError, match="int32"):
        ops.prep_input_occluded(x, torch.zeros(3, 4), torch.zeros(6), torch.ones(6))
    with pytest.raises(BcosHipError, match="one image"):
        ops.prep_input_occluded(torch.zeros(2, 6, 8, 8), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(6), torch.ones(6))
    with pytest.raises(BcosHipError, match="bank of 3"):
        ops.prep_input_occluded(x, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(6), torch.ones(6), first=2, n=2)
    with pytest.raises(BcosHipError):                               # no CPU path: the bank and the image live on the device
        ops.prep_input_occluded(x, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(6), torch.ones(6))
    with pytest.raises(IndexError):
        ops.occlusion_accumulate(torch.zeros(5), torch.zeros(3, 5), torch.ones(3, 4, dtype=torch.int32), 8, 8, targets=[5])


def test_occlusion_abi_validation_under_address_sanitizer():
    """tests/asan/occlusion_abi_validation.c against the ASan host build (scripts/asan_host_check.sh), as the AGC file"""
    import subprocess
    proc = subprocess.run(["bash", os.path.join(REPO, "scripts", "asan_host_check.sh")], capture_output=True, text=True, timeout=1500)
    assert proc.returncode == 0 and "bcos_prep_input_occluded, bcos_occlusion_accumulate: all refusals ok" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
