"""The RISE explainer without a device: the mask of include/bcos_hip.h restated in numpy float32 (tests/rise_emulation.py) against
scipy's zoom and against the masks the reference recorded (tests/golden/make_golden_rise.py), the bank's random stream, the explainer's
host logic on emulated kernels against the recorded maps, the input source of forward(x, rise=...), and the argument checks of the three
entry points (ABI v12)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import scipy.ndimage
import torch

import rise_emulation as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SHAPES = [(224, 224, 8), (224, 224, 6), (32, 32, 4), (40, 24, 3), (33, 47, 5), (64, 64, 8), (16, 16, 2)]
MASK_TOL = 5e-7            # six fp32 roundings of values in [0, 1]


def fixture():
    return json.load(open(os.path.join(GOLDEN, "rise.json"))), np.load(os.path.join(GOLDEN, "rise.npz"))


def emulated(monkeypatch):
    from bcos_hip import ops
    for name in ("rise_masks", "prep_input_rise", "rise_accumulate", "class_scores"):
        monkeypatch.setattr(ops, name, getattr(E, name))


# ---------------------------------------------------------------------------------------------------------------------- the mask
@pytest.mark.parametrize("H,W,s", SHAPES)
def test_emulated_mask_is_scipys_mirrored_grid_mode_zoom(H, W, s):
    rs = np.random.RandomState(1000 * H + 10 * W + s)
    cell_h, cell_w = -(-H // s), -(-W // s)
    worst = 0.0
    shifts = [(0, 0), (cell_h - 1, cell_w - 1)] + [(rs.randint(0, cell_h), rs.randint(0, cell_w)) for _ in range(4)]
    for x, y in shifts:
        grid = rs.rand(s, s) < 0.4
        up = scipy.ndimage.zoom(grid.astype(np.float64), ((s + 1) * cell_h / s, (s + 1) * cell_w / s), order=1, mode="mirror", grid_mode=True)
        assert up.shape == ((s + 1) * cell_h, (s + 1) * cell_w)
        m = E.mask(grid, x, y, H, W)
        assert m.shape == (H, W) and m.dtype == np.float32
        worst = max(worst, float(np.abs(m.astype(np.float64) - up[x:x + H, y:y + W]).max()))
        # through the packed bank row as well
        assert np.array_equal(E.masks(E.pack_rows(grid[None], np.array([[x, y]])), s, H, W)[0], m)
    print(f"RISE mask {H}x{W} s={s}: max |emulation - scipy| = {worst:.3e}")
    assert worst <= MASK_TOL
    ones = E.mask(np.ones((s, s), dtype=bool), cell_h // 2, cell_w // 3, H, W)
    assert np.array_equal(ones, np.ones((H, W), dtype=np.float32))
    assert np.array_equal(E.mask(np.zeros((s, s), dtype=bool), 0, 0, H, W), np.zeros((H, W), dtype=np.float32))


def test_pack_rows_keeps_the_high_word_for_s_8():
    grid = np.zeros((1, 8, 8), dtype=bool)
    grid[0, 7, 7] = grid[0, 3, 7] = grid[0, 4, 0] = True            # bits 63, 31 and 32
    rows = E.pack_rows(grid, np.array([[1, 2]]))
    assert rows.dtype == np.int32 and rows.tolist() == [[-2 ** 31, -2 ** 31 + 1, 1, 2]]
    assert np.array_equal(E.unpack_grid(rows, 8), grid.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------- the bank
@pytest.mark.parametrize("H,W,n,s,p1", [(32, 32, 64, 4, 0.1), (48, 48, 96, 6, 0.5), (40, 24, 10, 3, 0.3), (64, 64, 17, 8, 0.5)])
def test_make_bank_draws_the_references_random_stream(H, W, n, s, p1):
    from interpretability.explanation_methods.explainers.rise import RISE
    state = np.random.get_state()
    bank = RISE(None, n=n, s=s, p1=p1).make_bank(H, W)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # the global stream is not touched
    # the reference's three numpy calls in its order (rise.py:35-51), from the global seed as it uses it
    cell = np.ceil(np.array((H, W)) / s)
    try:
        np.random.seed(42)
        grid = np.random.rand(n, s, s) < p1
        shifts = np.array([(np.random.randint(0, cell[0]), np.random.randint(0, cell[1])) for _ in range(n)])
    finally:
        np.random.set_state(state)
    want = E.pack_rows(grid, shifts)
    assert bank.s == s and bank.rows.dtype == torch.int32 and tuple(bank.rows.shape) == (n, 4) and not bank.rows.is_cuda
    assert np.array_equal(bank.rows.numpy(), want)
    assert bank.host is bank.rows and len(bank[3:7]) == 4 and torch.equal(bank[3:7].rows, bank.rows[3:7])


@pytest.mark.parametrize("index", range(2))
def test_emulated_masks_equal_the_recorded_masks(index):
    from interpretability.explanation_methods.explainers.rise import RISE
    meta, data = fixture()
    case = meta["cases"][index]
    H = W = case["size"]
    bank = RISE(None, **case["kwargs"]).make_bank(H, W)
    rec = data[f"{case['name']}/masks"]
    assert rec.dtype == np.float32 and rec.shape == (case["n_masks"], H, W)
    d = float(np.abs(E.masks(bank.rows, bank.s, H, W).astype(np.float64) - rec).max())
    print(f"RISE {case['name']}: max |emulated mask - recorded mask| = {d:.3e}")
    assert d <= MASK_TOL


# ---------------------------------------------------------------------------------------------------------------------- the explainer
class RecordedModel(torch.nn.Module):
    """stands in for the network: returns the recorded logits of the masked copies in mask order, whatever the chunking, and checks
    that every copy IS `img * mask_i` (emulated masks)"""
    to_probabilities = torch.sigmoid

    def __init__(self, img, logits, masks):
        super().__init__()
        self.img, self.logits, self.masks, self.next, self.batches = img, logits, masks, 0, []

    def forward(self, x):
        lo, hi = self.next, self.next + x.shape[0]
        assert torch.equal(x, self.img * self.masks[lo:hi, None])
        self.next = hi
        self.batches.append(x.shape[0])
        return self.logits[lo:hi].clone()


def case_setup(case, data, **override):
    from bcos_hip import synth
    from interpretability.explanation_methods.explainers.rise import RISE
    name = case["name"]
    H = W = case["size"]
    img = synth.synthetic_images(1, seed=case["image_seed"], size=case["size"])
    logits = torch.from_numpy(data[f"{name}/logits"])
    kw = {**case["kwargs"], **override}
    bank = RISE(None, **kw).make_bank(H, W)
    masks = torch.from_numpy(E.masks(bank.rows, bank.s, H, W))

    def make():
        model = RecordedModel(img, logits, masks)
        return RISE(model, **kw), model
    classes = data[f"{name}/classes"].tolist()
    local = [classes.index(t) for t in case["targets"]]          # the targets as indices into the recorded class subset
    return img, logits, bank, make, local


@pytest.mark.parametrize("index", range(2))
def test_explainer_on_emulated_kernels_equals_the_recorded_maps(index, monkeypatch, capsys):
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][index]
    name, H = case["name"], case["size"]
    W = H
    img, logits, bank, make, local = case_setup(case, data)
    tol = max(1e-4, 3 * case["d_ref"])

    rise, model = make()
    assert capsys.readouterr().out == ""                            # (the reference prints from __init__)
    assert rise.score_mode == "sigmoid" and rise.max_imgs_bs == 1
    sel = rise.attribute_selection(img, local)
    assert sel.shape == (3, 1, H, W) and sel.dtype == torch.float32
    assert model.next == case["n_masks"] and max(model.batches) <= rise.batch_size
    rec = torch.from_numpy(data[f"{name}/selection"])
    rec64 = torch.from_numpy(data[f"{name}/selection64"])
    peak = float(rec64.abs().max())
    d32, d64 = float((sel.double() - rec.double()).abs().max()) / peak, float((sel.double() - rec64).abs().max()) / peak
    print(f"RISE {name}: explainer vs recorded fp32 maps {d32:.3e}, vs fp64 maps {d64:.3e} of the peak (bound {tol:.1e})")
    assert d32 <= tol and d64 <= tol

    rise, _ = make()
    one = rise.attribute(img, [local[0]])
    assert one.shape == (1, 1, H, W)
    assert torch.equal(one, sel[:1])                                # a class's map does not depend on which other classes ride along
    assert float((one.double() - torch.from_numpy(data[f"{name}/map"]).double()).abs().max()) / peak <= tol
    rise, _ = make()
    assert torch.equal(rise.attribute_selection(img, torch.tensor(local)), sel)

    rise, _ = make()
    full = rise.attribute(img, None, return_all=True)
    assert full.shape == (logits.shape[1], 1, H, W)
    assert float((full[local].double() - rec64).abs().max()) / peak <= tol


def test_result_does_not_depend_on_the_chunk_size(monkeypatch):
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][0]
    outs, batches = [], []
    for bs in (1, 8, 50, 1000):
        img, _, _, make, local = case_setup(case, data, batch_size=bs)
        rise, model = make()
        outs.append(rise.attribute_selection(img, local))
        batches.append(max(model.batches))
    assert batches == [1, 8, 50, 64]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


def test_shapes_of_the_three_entry_points(monkeypatch):
    emulated(monkeypatch)
    from interpretability.explanation_methods.explainers.rise import RISE

    class Net(torch.nn.Module):                                     # no to_probabilities: softmax over the row (rise.py:22-24)
        def forward(self, x):
            assert x.shape[0] <= 4
            return torch.stack([x[:, 0].mean((1, 2)), x[:, 1, :8].sum((1, 2)), -x[:, 2].amax((1, 2)), x[:, 3, 4:, 4:].mean((1, 2))], dim=1)
    x = torch.rand(3, 6, 16, 12, generator=torch.Generator().manual_seed(3))
    rise = RISE(Net(), batch_size=4, n=10, s=3, p1=0.5)
    assert rise.score_mode == "softmax"
    out = rise.attribute(x, [0, 1, 2])
    assert out.shape == (3, 1, 16, 12)
    for i, t in enumerate((0, 1, 2)):
        assert torch.equal(out[i:i + 1], rise.attribute(x[i:i + 1], [t]))
    assert rise.attribute(x, 1).shape == (3, 1, 16, 12)             # one class for every image
    assert rise.attribute(x[:1], None, return_all=True).shape == (4, 1, 16, 12)
    assert rise.attribute(x, None, return_all=True).shape == (12, 1, 16, 12)
    sel = rise.attribute_selection(x[:1], [3, 0])
    assert sel.shape == (2, 1, 16, 12) and torch.equal(sel[1:], out[:1])
    # softmax scores sum to one over the classes: the maps of all classes add up to sum_i m_i / n / p1
    full = rise.attribute(x[:1], None, return_all=True)
    bank = rise.make_bank(16, 12)
    cover = torch.from_numpy(E.masks(bank.rows, 3, 16, 12)).double().sum(0) / 10 / float(np.float32(0.5))
    assert float((full[:, 0].double().sum(0) - cover).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        rise.attribute(x, [0, 1])
    with pytest.raises(ValueError):
        rise.attribute_selection(x, [0, 1])                         # the reference reads one image: one image here
    with pytest.raises(ValueError, match="2..8"):
        RISE(Net(), s=9)


def test_engine_path_asks_for_rise_forwards(monkeypatch):
    """with a fused engine attached nothing is masked on the host: every chunk is one engine.forward(img, rise=bank[lo:hi])"""
    emulated(monkeypatch)
    meta, data = fixture()
    case = meta["cases"][1]
    img, logits, bank, make, local = case_setup(case, data)
    rise, _ = make()
    want = rise.attribute_selection(img, local)

    class Engine:
        calls = []

        def forward(self, x, rise=None):
            assert torch.equal(x, img) and rise.s == bank.s
            lo = sum(self.calls)
            assert torch.equal(rise.rows, bank.rows[lo:lo + len(rise)])
            self.calls.append(len(rise))
            return logits[lo:lo + len(rise)].clone()

    class Net(torch.nn.Module):
        to_probabilities = torch.sigmoid

        def forward(self, x):
            raise AssertionError("the module path must not run")
    from interpretability.explanation_methods.explainers.rise import RISE
    for chunk, calls in ((None, [96]), (40, [40, 40, 16])):
        net = Net().eval()
        object.__setattr__(net, "_bcos_engine", Engine())
        Engine.calls = []
        rise = RISE(net, **case["kwargs"])
        assert rise.engine_batch_size == 256
        if chunk:
            rise.engine_batch_size = chunk
        assert torch.equal(rise.attribute_selection(img, local), want)
        assert Engine.calls == calls


def test_named_configuration():
    """"default" of the reference's explanation_configs.py: n = 500, s = 8, batch_size = 8, and the key "p" that the constructor
    swallows, so p1 stays 0.1.  (get_explainer itself keeps answering "out of scope" for "RISE": the older test files pin that.)"""
    from interpretability.explanation_methods.explainers import RISE
    from interpretability.explanation_methods.explanation_configs import explainer_configs
    assert explainer_configs["RISE"] == {"default": {"n": 500, "s": 8, "p": 0.1, "batch_size": 8}}
    net = torch.nn.Identity()
    rise = RISE.from_config(net, "default")
    assert rise.model is net and (rise.N, rise.s, rise.p1, rise.batch_size, rise.max_imgs_bs) == (500, 8, 0.1, 8, 1)
    assert RISE(net, **explainer_configs["RISE"]["default"]).p1 == 0.1
    assert (RISE(net).N, RISE(net).s, RISE(net).p1, RISE(net).batch_size) == (6000, 6, 0.1, 2)       # the class defaults (rise.py:19)
    assert RISE.from_config(net, "default", n=64).N == 64
    bank = rise.make_bank(224, 224)
    assert tuple(bank.rows.shape) == (500, 4) and int(bank.rows[:, 2:].max()) < 28 and int(bank.rows[:, 2:].min()) >= 0


# ---------------------------------------------------------------------------------------------------------------------- the plans
def test_input_source_validates_on_the_host():
    from bcos_hip import ops, plan
    from bcos_hip.lib import BcosHipError
    x = torch.zeros(1, 6, 8, 8)
    rows = torch.zeros(3, 4, dtype=torch.int32)
    bank = ops.RiseBank(rows, 4)
    rects = torch.zeros(3, 4, dtype=torch.int32)
    for kw in (dict(occlude=rects, rise=bank), dict(perturb=object(), rise=bank), dict(occlude=rects, perturb=object(), rise=bank)):
        with pytest.raises(ValueError, match="one of the three"):
            plan.input_source(x, **kw)
    with pytest.raises(ValueError, match="one of the two"):
        plan.input_source(x, occlude=rects, perturb=object())
    with pytest.raises(BcosHipError, match="no CPU fallback"):       # a CPU image
        plan.input_source(x, rise=bank)
    with pytest.raises(ValueError, match="ONE 6-channel image"):
        plan.input_source(torch.zeros(1, 3, 8, 8), rise=bank)
    with pytest.raises(ValueError, match="ONE 6-channel image"):
        plan.input_source(torch.zeros(2, 6, 8, 8), rise=bank)
    assert type(plan.input_source(x)) is plan.Images and issubclass(plan.RiseCopies, plan.OccludedCopies)

    class OnDevice(torch.Tensor):
        """a host tensor that claims to be a device image: the bank checks come behind the image's"""
        is_cuda = True
    xd = torch.zeros(1, 6, 8, 8).as_subclass(OnDevice)
    for bad in (ops.RiseBank(rows.long(), 4), ops.RiseBank(rows.float(), 4), ops.RiseBank(torch.zeros(3, 3, dtype=torch.int32), 4),
                ops.RiseBank(torch.zeros(12, dtype=torch.int32), 4), ops.RiseBank(torch.zeros(0, 4, dtype=torch.int32), 4),
                ops.RiseBank(torch.zeros(3, 8, dtype=torch.int32)[:, ::2], 4), ops.RiseBank(rows, 9), ops.RiseBank(rows, 1), rows, (rows, 4)):
        with pytest.raises(ValueError, match="ops.RiseBank"):
            plan.input_source(xd, rise=bad)
    src = plan.input_source(xd, rise=bank)
    assert type(src) is plan.RiseCopies and (src.n, src.first, src.add_inverse) == (3, 0, False)
    part = src.cut(1, 3)
    assert (part.n, part.first) == (2, 1) and part.bank is bank and (src.n, src.first) == (3, 0)
    assert (part.cut(1, 2).first, part.cut(1, 2).n) == (2, 1)


def test_ops_wrappers_refuse_what_the_kernels_cannot_take():
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    x = torch.zeros(1, 6, 8, 8)
    bank = ops.RiseBank(torch.zeros(3, 4, dtype=torch.int32), 4)
    with pytest.raises(BcosHipError, match="RiseBank"):
        ops.prep_input_rise(x, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(6), torch.ones(6))
    with pytest.raises(BcosHipError, match="RiseBank"):
        ops.rise_masks(ops.RiseBank(torch.zeros(3, 4), 4), 8, 8)
    with pytest.raises(BcosHipError, match="2..8"):
        ops.rise_masks(ops.RiseBank(torch.zeros(3, 4, dtype=torch.int32), 9), 8, 8)
    with pytest.raises(BcosHipError, match="one image"):
        ops.prep_input_rise(torch.zeros(2, 6, 8, 8), bank, torch.zeros(6), torch.ones(6))
    with pytest.raises(BcosHipError, match="bank of 3"):
        ops.prep_input_rise(x, bank, torch.zeros(6), torch.ones(6), first=2, n=2)
    with pytest.raises(BcosHipError, match="bank of 3"):
        ops.rise_masks(bank, 8, 8, first=3, n=1)
    for call in (lambda: ops.rise_masks(bank, 8, 8), lambda: ops.prep_input_rise(x, bank, torch.zeros(6), torch.ones(6)),
                 lambda: ops.rise_accumulate(torch.zeros(3, 2), bank, 8, 8, 0.1)):
        with pytest.raises(BcosHipError):                           # no CPU path: the bank lives on the device
            call()
    with pytest.raises(BcosHipError, match="scores"):
        ops.rise_accumulate(torch.zeros(4, 2), bank, 8, 8, 0.1)


def test_densenet_plan_refuses_rise():
    from bcos_hip import ops
    from bcos_hip.densenet_engine import DenseNetEngine
    from bcos_hip.lib import BcosHipError
    bank = ops.RiseBank(torch.zeros(3, 4, dtype=torch.int32), 4)
    eng = object.__new__(DenseNetEngine)                            # the refusal comes before the plan is touched
    with pytest.raises(BcosHipError, match="`rise=`"):
        eng.forward(torch.zeros(1, 6, 8, 8), rise=bank)
    with pytest.raises(BcosHipError, match="`occlude=`"):
        eng.forward(torch.zeros(1, 6, 8, 8), occlude=torch.zeros(3, 4, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------- ABI
NAMES = ("bcos_rise_masks", "bcos_prep_input_rise", "bcos_rise_accumulate")


def test_header_binding_and_library_export_the_entry_points(hip_lib):
    from bcos_hip import lib, ops
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header)
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header) and name in lib.SIGNATURES
        assert getattr(hip_lib, name) is not None
    assert lib.ABI_VERSION == 12 and hip_lib.bcos_version() == 12
    assert "bcos_rise.hip" in lib.SOURCES
    assert all(callable(getattr(ops, n)) for n in ("rise_masks", "prep_input_rise", "rise_accumulate"))


def test_abi_refuses_malformed_arguments(hip_lib):
    fake = C.c_void_p(1 << 20)
    odd = C.c_void_p((1 << 20) + 4)
    H, W, s = 10, 12, 4                                             # cells of 3 x 3
    bank = (C.c_int32 * 8)(0x1234, 0, 2, 1, 0xFFFF, 0, 0, 2)
    host = C.cast(bank, C.c_void_p)
    masks = lambda **k: hip_lib.bcos_rise_masks(*[k.get(a, d) for a, d in (  # noqa: E731
        ("bank", fake), ("out", fake), ("n_bank", 5), ("first", 1), ("n", 2), ("s", s), ("H", H), ("W", W), ("stream", None))])
    for bad in (dict(bank=None), dict(out=None), dict(n_bank=0), dict(first=-1), dict(n=0), dict(first=4), dict(n=5), dict(s=1), dict(s=9),
                dict(H=0), dict(W=-1), dict(bank=odd), dict(H=1 << 16, W=1 << 16), dict(H=1 << 24, W=1)):
        assert masks(**bad) == -22, bad
        assert b"bcos_rise_masks" in hip_lib.bcos_last_error_string()
    prep = lambda **k: hip_lib.bcos_prep_input_rise(*[k.get(a, d) for a, d in (  # noqa: E731
        ("x", fake), ("bank", fake), ("out", fake), ("mean", fake), ("std", fake), ("am", None), ("n_bank", 5), ("first", 1), ("n", 2),
        ("s", s), ("Cx", 6), ("H", H), ("W", W), ("Cpad", 8), ("add_inverse", 0), ("stream", None))])
    for bad in (dict(x=None), dict(bank=None), dict(out=None), dict(mean=None), dict(std=None), dict(n_bank=0), dict(first=-1), dict(n=0),
                dict(n=-3), dict(first=4), dict(s=1), dict(s=9), dict(H=0), dict(W=0), dict(Cpad=5), dict(Cx=3, add_inverse=1), dict(Cx=3),
                dict(add_inverse=1), dict(bank=odd)):
        assert prep(**bad) == -22, bad
        assert b"bcos_prep_input_rise" in hip_lib.bcos_last_error_string()
    acc = lambda **k: hip_lib.bcos_rise_accumulate(*[k.get(a, d) for a, d in (  # noqa: E731
        ("scores", fake), ("bank", fake), ("host", host), ("out", fake), ("n", 2), ("T", 3), ("s", s), ("H", H), ("W", W), ("p1", 0.1),
        ("stream", None))])
    for bad in (dict(scores=None), dict(bank=None), dict(out=None), dict(n=0), dict(n=-1), dict(T=0), dict(s=1), dict(s=9), dict(H=0),
                dict(W=0), dict(p1=0.0), dict(p1=-0.5), dict(p1=float("nan")), dict(p1=float("inf")), dict(bank=odd),
                dict(s=3),                                          # bits at and above 9 are set in both rows
                dict(H=8), dict(W=8)):                              # cells of 2: the shifts 2 leave them
        assert acc(**bad) == -22, bad
        assert b"bcos_rise_accumulate" in hip_lib.bcos_last_error_string()
    for row in ((1 << 16, 0, 0, 0), (0, 1, 0, 0), (1, 0, 3, 0), (1, 0, 0, 3), (1, 0, -1, 0), (1, 0, 0, -1)):
        bank[4:8] = row
        assert acc() == -22, row
    assert acc(H=1 << 15, W=1 << 15, host=None) == -95              # the axis tables do not fit the LDS


def test_rise_abi_validation_is_part_of_the_sanitizer_script():
    """tests/asan/rise_abi_validation.c against the ASan host build (scripts/asan_host_check.sh), as its siblings"""
    import subprocess
    script = open(os.path.join(REPO, "scripts", "asan_host_check.sh")).read()
    assert re.search(r"for t in [^;]*\brise_abi_validation\b[^;]*; do", script)
    proc = subprocess.run(["bash", os.path.join(REPO, "scripts", "asan_host_check.sh")], capture_output=True, text=True, timeout=1500)
    assert proc.returncode == 0 and "bcos_rise_masks, bcos_prep_input_rise, bcos_rise_accumulate: all refusals ok" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
