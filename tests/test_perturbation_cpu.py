"""Pixel perturbation without a device: the emulation (tests/perturbation_emulation.py) against a brute-force sort, the harness's host
logic on emulated kernels with a toy model, and the argument checks of the four entry points (additive to ABI v12)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import perturbation_emulation as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bcos_perturb_select_ws_bytes", "bcos_perturb_select", "bcos_prep_input_perturbed", "bcos_class_scores")


def special_scores(n, seed):
    """ties, both zeros, infinities, subnormals and one NaN among normal values"""
    s = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    s[::5] = s[1]
    vals = [0.0, -0.0, float("inf"), float("-inf"), 1e-42, -1e-42, float("nan"), 0.0, -0.0]
    s[2:2 + len(vals)] = torch.tensor(vals)
    return s


# ---------------------------------------------------------------------------------------------------------------------- emulation
def brute_force_removed(scores_row, k, descending):
    """the first k of the ranking by the definition itself: sort the (key32, p) pairs as Python integers"""
    keys = E.key32(scores_row[None], descending)[0].tolist()
    order = sorted(range(len(keys)), key=lambda p: (keys[p] << 32) | p)
    gone = np.zeros(len(keys), dtype=bool)
    gone[order[:k]] = True
    return gone


@pytest.mark.parametrize("descending", [False, True])
def test_emulated_select_against_a_brute_force_sort(descending):
    HW = 13 * 11
    scores = torch.stack([special_scores(HW, 1), torch.zeros(HW), torch.randn(HW, generator=torch.Generator().manual_seed(2)).round()])
    counts = [0, 1, 7, 7, HW - 1, HW, 40]
    thr = E.perturb_select(scores, counts, descending)
    assert thr.dtype == torch.int64 and thr.shape == (3, len(counts))
    gone = E.removed(scores, thr, descending)
    for b in range(3):
        for j, k in enumerate(counts):
            assert int(gone[b, j].sum()) == k
            assert np.array_equal(gone[b, j], brute_force_removed(scores[b], k, descending)), (b, k)
    assert thr[0, counts.index(HW)].item() == -1                       # UINT64_MAX
    assert np.array_equal(gone[1, 2], np.arange(HW) < 7)               # all scores equal: ascending pixel index in EITHER order


def test_key32_orders_like_the_header_says():
    s = torch.tensor([float("-inf"), -1.0, -1e-42, -0.0, 0.0, 1e-42, 1.0, float("inf"), float("nan")])
    k = E.key32(s[None])[0].astype(np.int64)
    assert bool((np.diff(k) > 0).all())                                # -0.0 < +0.0; the (positive) NaN above +inf
    assert bool((np.diff(E.key32(s[None], True)[0].astype(np.int64)) < 0).all())


def test_emulated_prepared_input_and_host_mask_agree():
    from bcos_hip import perturbation as P
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 6, 5, 7, generator=g) - 0.25
    scores = torch.stack([special_scores(35, 4), torch.randn(35, generator=g)])
    mean, std = torch.rand(6, generator=g), torch.rand(6, generator=g) + 0.5
    for desc in (False, True):
        thr = E.perturb_select(scores, [0, 3, 35], desc)
        assert np.array_equal(P.removed_pixels(scores, thr, desc).numpy(), E.removed(scores, thr, desc))
        copies = E.materialise(x, scores, thr, desc)
        assert torch.equal(P.materialise(x, scores, thr, desc), copies)
        assert torch.equal(copies[0], x[0]) and torch.equal(copies[5], torch.zeros(6, 5, 7))
        out = E.prep_input_perturbed(x, scores, thr, mean, std, desc, first=1, n=4)
        assert out.shape == (4, 5, 7, 8) and torch.equal(out[..., 6:], torch.zeros(4, 5, 7, 2))
        assert torch.equal(out[1, ..., :6], ((0 - mean) / std).expand(5, 7, 6))        # copy 2: everything removed


# ---------------------------------------------------------------------------------------------------------------------- harness
class ToyNet(torch.nn.Module):
    def forward(self, x):
        return torch.stack([x[:, 0].sum((1, 2)), x[:, 1, :3].sum((1, 2)) - x[:, 4].sum((1, 2)), -x[:, 2].amax((1, 2)) + x[:, 5].mean((1, 2))], dim=1)


class ToyExplainer:
    def __init__(self, maps):
        self.maps, self.calls = maps, []

    def attribute(self, img, target):
        b = len(self.calls)
        self.calls.append(int(target))
        out = torch.zeros((1, 6) + tuple(img.shape[-2:]))
        out[0, 2] = self.maps[b]                                    # [1, 6, H, W]: sum(1) is the map
        return out


def emulated(monkeypatch):
    from bcos_hip import ops
    monkeypatch.setattr(ops, "perturb_select", E.perturb_select)
    monkeypatch.setattr(ops, "class_scores", E.class_scores)


def test_harness_on_emulated_kernels(monkeypatch):
    from bcos_hip import perturbation as P
    emulated(monkeypatch)
    g = torch.Generator().manual_seed(5)
    B, H, W = 5, 6, 7
    HW = H * W
    x = torch.rand(B, 6, H, W, generator=g)
    maps = torch.randn(B, H, W, generator=g).round() + 0.0            # ties; no -0.0 (a sum over channels would turn it into +0.0)
    net = ToyNet().eval()
    fractions = (0, 0.1, 0.5, 1.0)
    res = P.pixel_perturbation(net, x, attributions=maps, fractions=fractions)
    assert res["counts"] == [0, 4, 21, 42] and res["fractions"] == [0.0, 0.1, 0.5, 1.0]
    logits = net(x)
    assert torch.equal(res["targets"], logits.argmax(1))              # the predicted classes
    assert res["curves"].shape == (B, 4) and res["thresholds"].shape == (B, 4)
    assert torch.equal(res["curves"][:, 0], logits.gather(1, res["targets"][:, None])[:, 0])              # k = 0: the unperturbed score
    zero = net(torch.zeros(1, 6, H, W))[0]
    assert torch.equal(res["curves"][:, 3], zero[res["targets"]])                                          # k = HW: nothing is left
    assert torch.equal(res["thresholds"], E.perturb_select(maps.reshape(B, HW), res["counts"]))
    # every column is the model on the materialised copies
    copies = E.materialise(x, maps.reshape(B, HW), res["thresholds"])
    assert torch.equal(res["curves"].reshape(-1), net(copies).gather(1, res["targets"].repeat_interleave(4)[:, None])[:, 0])
    # chunking by copies_per_call does not change the result
    for cpc in (1, 4, 9, 1000):
        again = P.pixel_perturbation(net, x, attributions=maps, fractions=fractions, copies_per_call=cpc)
        assert torch.equal(again["curves"], res["curves"]) and torch.equal(again["thresholds"], res["thresholds"])
    # [B, C, H, W] attributions are summed over the channels; the explainer route gives the same ranking
    four = torch.stack([maps * 0.25, maps * 0.75], dim=1)
    assert torch.equal(P.pixel_perturbation(net, x, attributions=four, fractions=fractions)["curves"], res["curves"])
    expl = ToyExplainer(maps)
    via = P.pixel_perturbation(net, x, explainer=expl, fractions=fractions)
    assert expl.calls == res["targets"].tolist()
    assert torch.equal(via["curves"], res["curves"]) and torch.equal(via["thresholds"], res["thresholds"])
    # given targets (negative ones wrap), the other order, the other scores
    tg = [0, -1, 1, 2, 0]
    most = P.pixel_perturbation(net, x, tg, attributions=maps, fractions=fractions, order="most", score="softmax")
    assert most["targets"].tolist() == [0, 2, 1, 2, 0]
    assert torch.equal(most["thresholds"], E.perturb_select(maps.reshape(B, HW), res["counts"], True))
    want = torch.softmax(net(E.materialise(x, maps.reshape(B, HW), most["thresholds"], True)).double(), 1)
    assert torch.allclose(most["curves"].double().reshape(-1), want.gather(1, most["targets"].repeat_interleave(4)[:, None])[:, 0], rtol=1e-6, atol=0)
    with pytest.raises(IndexError):
        P.pixel_perturbation(net, x, [0, 1, 2, 3, 0], attributions=maps)
    # an explainer is handed validated classes only: negative ones wrapped, a class the logits do not have refused before its first call
    expl = ToyExplainer(maps)
    via = P.pixel_perturbation(net, x, tg, explainer=expl, fractions=fractions, order="most", score="softmax")
    assert expl.calls == [0, 2, 1, 2, 0] and via["targets"].tolist() == expl.calls
    assert torch.equal(via["curves"], most["curves"]) and torch.equal(via["thresholds"], most["thresholds"])
    for bad in ([0, 1, 2, 3, 0], [0, 1, -4, 2, 0]):
        expl = ToyExplainer(maps)
        with pytest.raises(IndexError):
            P.pixel_perturbation(net, x, bad, explainer=expl)
        assert expl.calls == []
    with pytest.raises(ValueError, match="one target per image"):
        P.pixel_perturbation(net, x, [0, 1], attributions=maps)
    with pytest.raises(ValueError, match="order"):
        P.pixel_perturbation(net, x, attributions=maps, order="random")
    with pytest.raises(ValueError, match="score"):
        P.pixel_perturbation(net, x, attributions=maps, score="prob")
    with pytest.raises(ValueError, match="fractions"):
        P.pixel_perturbation(net, x, attributions=maps, fractions=(0.5, 1.5))
    with pytest.raises(ValueError, match="attributions"):
        P.pixel_perturbation(net, x, attributions=maps[:, :3])
    with pytest.raises(ValueError, match="6-channel"):
        P.pixel_perturbation(net, x[:, :3], attributions=maps)
    with pytest.raises(ValueError, match="explainer"):
        P.pixel_perturbation(net, x)                                  # no engine: nothing to take the scores from


def test_harness_asks_an_attached_engine_for_perturbed_forwards(monkeypatch):
    """with a fused engine attached nothing is materialised on the host: every chunk is one engine.forward(x[lo:hi], perturb=plan)"""
    from bcos_hip import perturbation as P
    emulated(monkeypatch)
    g = torch.Generator().manual_seed(6)
    B, H, W = 5, 4, 5
    x = torch.rand(B, 6, H, W, generator=g)
    maps = torch.randn(B, H, W, generator=g)
    toy = ToyNet()

    class Engine:
        calls = []

        def forward(self, xs, occlude=None, perturb=None):
            if perturb is None:
                return toy(xs)
            assert occlude is None and perturb.K == 3 and perturb.descending is False
            self.calls.append(xs.shape[0])
            return toy(E.materialise(xs, perturb.scores, perturb.thr, perturb.descending))

        def explain(self, xs, targets, want_weights=True):
            assert want_weights is False and targets is None
            return dict(contribution_map=maps, explained_class_idx=toy(xs).argmax(1))

    class Net(torch.nn.Module):
        def forward(self, xs):
            raise AssertionError("the module path must not run")
    net = Net().eval()
    object.__setattr__(net, "_bcos_engine", Engine())
    want = P.pixel_perturbation(toy, x, attributions=maps, fractions=(0, 0.25, 0.5))
    for first in (net, net._bcos_engine):
        Engine.calls = []
        got = P.pixel_perturbation(first, x, fractions=(0, 0.25, 0.5), copies_per_call=6)       # the default scores: engine.explain
        assert Engine.calls == [2, 2, 1]
        assert torch.equal(got["curves"], want["curves"]) and torch.equal(got["targets"], want["targets"])
    net.train()                                                      # train() mode: the module path
    with pytest.raises(AssertionError, match="module path"):
        P.pixel_perturbation(net, x, attributions=maps)


def test_forward_refuses_perturb_together_with_occlude():
    from bcos_hip import engine, perturbation as P, vit_engine
    from bcos_hip.plan import input_source
    x = torch.zeros(1, 6, 4, 4)
    plan = P.PerturbPlan(torch.zeros(1, 16), torch.zeros(1, 2, dtype=torch.int64))
    bank = torch.tensor([[0, 2, 0, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="one of the two"):
        input_source(x, occlude=bank, perturb=plan)
    for cls in (engine.ResNetEngine, vit_engine.ViTEngine):
        with pytest.raises(ValueError, match="one of the two"):
            cls.forward(object.__new__(cls), x, occlude=bank, perturb=plan)
    from bcos_hip.lib import BcosHipError
    with pytest.raises(ValueError, match="6-channel"):
        input_source(x[:, :3], perturb=plan)
    with pytest.raises(BcosHipError):                                  # no CPU path
        input_source(x, perturb=plan)


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_header_signatures_and_library_agree(hip_lib):
    from bcos_hip import lib
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header) and re.search(r"#define BCOS_PERTURB_MAX_COUNTS 64\b", header)
    for name in NAMES:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m and name in lib.SIGNATURES
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name         # as many parameters as the binding types
        assert getattr(hip_lib, name) is not None
    assert lib.ABI_VERSION == 12 and hip_lib.bcos_version() == 12
    assert "bcos_perturb.hip" in lib.SOURCES and os.path.exists(os.path.join(str(lib.CSRC), "bcos_perturb.hip"))
    exported = subprocess.run(["nm", "-D", "--defined-only", str(lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert all(re.search(r"\bT " + name + r"\b", exported) for name in NAMES)


def test_abi_refuses_malformed_arguments(hip_lib):
    fake = C.c_void_p(1 << 20)
    odd = C.c_void_p((1 << 20) + 4)
    counts = (C.c_int32 * 4)(0, 3, 64, 64)
    host = C.cast(counts, C.c_void_p)
    nbytes = C.c_int64(-1)
    size = lambda **k: hip_lib.bcos_perturb_select_ws_bytes(*[k.get(a, d) for a, d in (("B", 2), ("HW", 64), ("K", 4), ("bytes", C.byref(nbytes)))])  # noqa: E731
    assert size() == 0 and nbytes.value >= 4 * (2 * 256 + 2 * 4 * 256)
    for bad in (dict(bytes=None), dict(B=0), dict(B=-1), dict(HW=0), dict(HW=1 << 31), dict(K=0), dict(K=65)):
        assert size(**bad) == -22, bad
        assert b"bcos_perturb_select_ws_bytes" in hip_lib.bcos_last_error_string()
    sel = lambda **k: hip_lib.bcos_perturb_select(*[k.get(a, d) for a, d in (  # noqa: E731
        ("scores", fake), ("counts", host), ("desc", 0), ("thr", fake), ("ws", fake), ("ws_bytes", nbytes.value), ("B", 2), ("HW", 64), ("K", 4),
        ("stream", None))])
    for bad in (dict(scores=None), dict(counts=None), dict(thr=None), dict(ws=None), dict(B=0), dict(HW=0), dict(HW=1 << 31), dict(K=0), dict(K=65),
                dict(HW=63), dict(ws_bytes=nbytes.value - 1), dict(ws_bytes=0), dict(thr=odd), dict(ws=odd)):      # (HW = 63: the counts of 64 leave it)
        assert sel(**bad) == -22, bad
        assert b"bcos_perturb_select:" in hip_lib.bcos_last_error_string()
    for k in (-1, 65):
        counts[1] = k
        assert sel() == -22 and sel(desc=1) == -22 and b"count outside" in hip_lib.bcos_last_error_string()
    prep = lambda **k: hip_lib.bcos_prep_input_perturbed(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", fake), ("scores", fake), ("thr", fake), ("desc", 0), ("out", fake), ("mean", fake), ("std", fake), ("am", None), ("B", 3), ("K", 5),
        ("first", 2), ("n", 13), ("Cx", 6), ("H", 8), ("W", 8), ("Cpad", 8), ("add_inverse", 0), ("stream", None))])
    for bad in (dict(x=None), dict(scores=None), dict(thr=None), dict(out=None), dict(mean=None), dict(std=None), dict(B=0), dict(K=0), dict(H=0),
                dict(W=-2), dict(Cpad=5), dict(Cx=3, add_inverse=1), dict(Cx=3), dict(add_inverse=1), dict(first=-1), dict(n=0), dict(n=-3),
                dict(n=14), dict(first=15, n=1), dict(thr=odd), dict(H=1 << 16, W=1 << 16)):
        assert prep(**bad) == -22, bad
        assert b"bcos_prep_input_perturbed" in hip_lib.bcos_last_error_string()
    cls = lambda **k: hip_lib.bcos_class_scores(*[k.get(a, d) for a, d in (  # noqa: E731
        ("logits", fake), ("targets", fake), ("group", 5), ("mode", 0), ("out", fake), ("R", 15), ("CL", 10), ("stream", None))])
    for bad in (dict(logits=None), dict(targets=None), dict(out=None), dict(group=0), dict(group=-1), dict(group=4), dict(R=0), dict(R=-5),
                dict(CL=0), dict(mode=3), dict(mode=-1)):
        assert cls(**bad) == -22, bad
        assert b"bcos_class_scores" in hip_lib.bcos_last_error_string()


def test_ops_wrappers_refuse_what_the_kernels_cannot_take(hip_lib):
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    s = torch.zeros(2, 64)
    with pytest.raises(BcosHipError, match="perturb_select.*float32"):
        ops.perturb_select(s.double(), [1])
    with pytest.raises(BcosHipError, match="perturb_select.*float32"):
        ops.perturb_select(torch.zeros(64), [1])
    with pytest.raises(BcosHipError, match="perturb_select: between 1 and 64"):
        ops.perturb_select(s, [])
    with pytest.raises(BcosHipError, match="perturb_select: between 1 and 64"):
        ops.perturb_select(s, list(range(65)))
    with pytest.raises(BcosHipError, match="perturb_select: a removal count outside"):
        ops.perturb_select(s, [0, 65])
    with pytest.raises(BcosHipError, match="perturb_select: a removal count outside"):
        ops.perturb_select(s, [-1])
    with pytest.raises(BcosHipError, match="perturb_select: the counts"):
        ops.perturb_select(s, [0.5])
    with pytest.raises(BcosHipError, match="perturb_select"):                 # no CPU path
        ops.perturb_select(s, [0, 64])
    x, thr, mean, std = torch.zeros(2, 6, 8, 8), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(6), torch.ones(6)
    with pytest.raises(BcosHipError, match="prep_input_perturbed: 6-channel"):
        ops.prep_input_perturbed(x[:, :3], s, thr, mean, std)
    with pytest.raises(BcosHipError, match="prep_input_perturbed: scores"):
        ops.prep_input_perturbed(x, s[:1], thr, mean, std)
    with pytest.raises(BcosHipError, match="prep_input_perturbed: the thresholds"):
        ops.prep_input_perturbed(x, s, thr.int(), mean, std)
    with pytest.raises(BcosHipError, match="prep_input_perturbed: the thresholds"):
        ops.prep_input_perturbed(x, s, thr[:1], mean, std)
    with pytest.raises(BcosHipError, match=r"prep_input_perturbed: copies \[4, 7\) of 2 x 3"):
        ops.prep_input_perturbed(x, s, thr, mean, std, first=4, n=3)
    with pytest.raises(BcosHipError, match="prep_input_perturbed: copies"):
        ops.prep_input_perturbed(x, s, thr, mean, std, first=0, n=0)
    with pytest.raises(BcosHipError, match="prep_input_perturbed"):           # no CPU path
        ops.prep_input_perturbed(x, s, thr, mean, std)
    logits = torch.zeros(6, 10)
    with pytest.raises(BcosHipError, match="class_scores: mode"):
        ops.class_scores(logits, [1, 2], group=3, mode="prob")
    with pytest.raises(BcosHipError, match="class_scores: 6 rows"):
        ops.class_scores(logits, [1, 2], group=4)
    with pytest.raises(BcosHipError, match="class_scores: 3 targets"):
        ops.class_scores(logits, [1, 2, 3], group=3)
    with pytest.raises(IndexError):
        ops.class_scores(logits, [1, 10], group=3)
    with pytest.raises(BcosHipError):                                          # no CPU path
        ops.class_scores(logits, [1, 2], group=3)


def test_perturbation_abi_validation_is_listed_for_the_sanitizer_build():
    """tests/asan/perturbation_abi_validation.c runs with its siblings in scripts/asan_host_check.sh (which the occlusion suite runs)"""
    script = open(os.path.join(REPO, "scripts", "asan_host_check.sh")).read()
    assert re.search(r"^for t in .*\bperturbation_abi_validation\b", script, re.M)
    assert os.path.exists(os.path.join(REPO, "tests", "asan", "perturbation_abi_validation.c"))
