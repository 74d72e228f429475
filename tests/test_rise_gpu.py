"""`-m gpu`: the three RISE kernels, the engines' `rise=` forward, the explainer and the harness on the device, against the numpy float32
restatement (tests/rise_emulation.py), float64 evaluations and the fixtures the reference recorded (tests/golden/make_golden_rise.py).

Bounds (none taken from what the kernels return):
  * masks: bit-equality with the emulation (the same operations, each rounded once);
  * prepared input: bit-equality with bcos_prep_input on the materialised `img * masks`, per-pixel maxima included;
  * accumulate: |out - out64| <= (2 * 64 + ceil(n / 64) + 4) 2^-24 sum_i |score m| / (n p1) per element against float64 over the SAME fp32
    mask values and fp32 scores -- two roundings per term of a chunk, one per chunk sum, two divisions and second order;
  * `rise=` logits: bit-equality with the engine's forward on the materialised batch;
  * end-to-end maps: max(1e-4, 3 d_ref) of the map peak against the recorded maps, d_ref the reference's own fp32-vs-fp64 spread.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rise_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN = (0.485, 0.456, 0.406, 0.515, 0.544, 0.594)
STD = (0.229, 0.224, 0.225, 0.229, 0.224, 0.225)
SMALL = [(32, 32, 4), (40, 24, 3), (33, 47, 5), (16, 16, 2), (64, 64, 8)]
WINDOWS = ((0, 37), (5, 1), (36, 1))


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "rise.json"))), np.load(os.path.join(golden_dir, "rise.npz"))


def golden_net(golden_dir):
    from bcos_hip import synth
    meta = json.load(open(os.path.join(golden_dir, "resnet18_e2e.json")))
    data = np.load(os.path.join(golden_dir, "resnet18_e2e.npz"))
    net = synth.build_bcosified_resnet(meta["arch"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    return net.to(DEV).eval()


def random_bank(n, H, W, s, seed, p=0.4):
    """host RiseBank of n rows: random grids, shifts over the whole cell (first row: the largest shifts, second: none), one grid of
    ones and one of zeros"""
    from bcos_hip import ops
    rs = np.random.RandomState(seed)
    cell_h, cell_w = -(-H // s), -(-W // s)
    grid = rs.rand(n, s, s) < p
    shifts = np.stack([rs.randint(0, cell_h, n), rs.randint(0, cell_w, n)], 1)
    shifts[0] = (cell_h - 1, cell_w - 1)
    if n > 1:
        shifts[1] = (0, 0)
    if n > 3:
        grid[2], grid[3] = True, False
    rows = torch.from_numpy(E.pack_rows(grid, shifts))
    return ops.RiseBank(rows, s, rows)


_MASKS = {}


def emulated_masks(H, W, s):
    """(host bank of 37 rows, its emulated masks [37, H, W]) -- computed once per shape and shared, never modified"""
    if (H, W, s) not in _MASKS:
        bank = random_bank(37, H, W, s, seed=100 * H + W + s)
        _MASKS[(H, W, s)] = (bank, torch.from_numpy(E.masks(bank.rows, s, H, W)))
    return _MASKS[(H, W, s)]


def consts():
    return torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- 1. dense masks
@pytest.mark.parametrize("H,W,s", SMALL)
def test_masks_equal_the_emulation_bit_for_bit(lib, H, W, s):
    from bcos_hip import ops
    bank, want = emulated_masks(H, W, s)
    dev = bank.to(DEV)
    for first, n in WINDOWS:
        got = ops.rise_masks(dev, H, W, first=first, n=n)
        assert got.shape == (n, H, W) and torch.equal(got.cpu(), want[first:first + n]), (first, n)
    assert torch.equal(ops.rise_masks(dev[5:9], H, W).cpu(), want[5:9])                  # a slice of the bank is a bank
    assert torch.equal(got.new_ones(H, W).cpu(), want[2]) and not bool(want[3].any())    # a grid of ones is 1.0 exactly, of zeros 0.0
    # a NaN-filled guard around `out` stays NaN
    pad, n, first = 64, 3, 7
    buf = torch.full((pad + n * H * W + pad,), float("nan"), device=DEV)
    code = lib.bcos_rise_masks(ctypes.c_void_p(dev.rows.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4 * pad), 37, first, n, s, H, W, stream())
    assert code == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n * H * W:]).all())
    assert torch.equal(buf[pad:pad + n * H * W].view(n, H, W).cpu(), want[first:first + n])


# ---------------------------------------------------------------------------------------------------------------- 2. prepared input
@pytest.mark.parametrize("H,W,s", SMALL)
def test_prepared_input_equals_prep_of_the_masked_copies(lib, H, W, s):
    from bcos_hip import lib as blib
    from bcos_hip import ops
    bank, masks = emulated_masks(H, W, s)
    dev = bank.to(DEV)
    mean, std = consts()
    img = (torch.rand(1, 6, H, W, generator=torch.Generator().manual_seed(H + W)) - 0.25).to(DEV)
    prev = blib.get_contraction_mode()
    try:
        for mode in ("f16x2", "bf16x3"):                   # with and without the fused per-pixel maxima
            blib.set_contraction_mode(mode)
            for first, n in WINDOWS:
                a = ops.prep_input_rise(img, dev, mean, std, first=first, n=n, want_absmax=True)
                b = ops.prep_input((img * masks[first:first + n, None].to(DEV)).contiguous(), mean, std, want_absmax=True)
                assert a.shape == (n, H, W, 8) and torch.equal(a, b), (mode, first, n)
                am_a, am_b = ops.absmax_of(a), ops.absmax_of(b)
                assert (am_a is None) == (am_b is None) == (mode != "f16x2")
                if am_a is not None:
                    assert torch.equal(am_a, am_b), (mode, first, n)
    finally:
        blib.set_contraction_mode(prev)
    # the raw entry point: a window, Cpad 8 and 12, guards around both outputs
    pad, n, first = 64, 5, 30
    for cpad in (8, 12):
        size = n * H * W * cpad
        buf = torch.full((pad + size + pad,), float("nan"), device=DEV)
        am = torch.full((pad + n * H * W + pad,), -1, device=DEV, dtype=torch.int32)
        code = lib.bcos_prep_input_rise(ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(dev.rows.data_ptr()),
                                        ctypes.c_void_p(buf.data_ptr() + 4 * pad), ctypes.c_void_p(mean.data_ptr()),
                                        ctypes.c_void_p(std.data_ptr()), ctypes.c_void_p(am.data_ptr() + 4 * pad), 37, first, n, s, 6, H, W,
                                        cpad, 0, stream())
        assert code == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + size:]).all())
        assert bool((am[:pad] == -1).all()) and bool((am[pad + n * H * W:] == -1).all())
        want = ops.prep_input((img * masks[first:first + n, None].to(DEV)).contiguous(), mean, std, cpad=cpad)
        got = buf[pad:pad + size].view(n, H, W, cpad)
        assert torch.equal(got, want)
        assert torch.equal(am[pad:pad + n * H * W].view(n, H, W), (got.abs().amax(-1)).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 3. accumulate
_ACC = {}


def accumulate_case(H, W, s, n):
    """(host bank, fp32 masks, signed fp32 scores [n, 9]) per (shape, n): shared by the accumulate tests, never modified"""
    key = (H, W, s, n)
    if key not in _ACC:
        bank = random_bank(n, H, W, s, seed=7 * n + H)
        scores = torch.randn(n, 9, generator=torch.Generator().manual_seed(n + W)) * torch.tensor([1, 10, 0.1, 1, 1, 100, 1, 1e-3, 1.0])
        _ACC[key] = (bank, E.masks(bank.rows, s, H, W), scores.float().contiguous())
    return _ACC[key]


@pytest.mark.parametrize("H,W,s", [(33, 47, 5), (64, 64, 8)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_accumulate_against_float64_and_the_emulation(lib, H, W, s, n):
    from bcos_hip import ops
    bank, masks, scores = accumulate_case(H, W, s, n)
    dev = bank.to(DEV)
    p1 = 0.1 if n % 2 else 0.5
    nine = ops.rise_accumulate(scores.to(DEV), dev, H, W, p1)
    assert nine.shape == (9, H, W)
    worst = 0.0
    for T in (1, 3, 9):
        sc = scores[:, :T].contiguous()
        out = nine if T == 9 else ops.rise_accumulate(sc.to(DEV), dev, H, W, p1)
        assert out.shape == (T, H, W)
        out64, mag = E.accumulate64(sc.numpy(), masks, p1)
        err = np.abs(out.double().cpu().numpy() - out64)
        bound = E.accumulate_bound(mag, n)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (T, ratio)
        assert torch.equal(out.cpu(), torch.from_numpy(E.accumulate(sc.numpy(), masks, p1))), T      # the documented order, bit for bit
        assert torch.equal(out, nine[:T]), T               # a target's map does not depend on T or on which targets ride along
    print(f"rise_accumulate {H}x{W} s={s} n={n}: worst error / bound {worst:.3f}")
    for t in (4, 8):                                       # alone (one target per workgroup) or among nine (eight per workgroup)
        assert torch.equal(ops.rise_accumulate(scores[:, t:t + 1].contiguous().to(DEV), dev, H, W, p1)[0], nine[t])


def test_accumulate_propagates_a_nan_score_over_the_whole_map_of_its_target(lib):
    """the rule of include/bcos_hip.h: no term is skipped, so a NaN score makes every pixel of ITS target's map NaN (0 * NaN), an
    infinite one wherever its mask is 0 (and +-inf elsewhere); the other targets keep their bits"""
    from bcos_hip import ops
    H, W, s, n = 33, 47, 5, 65
    bank, masks, scores = accumulate_case(H, W, s, n)
    dev = bank.to(DEV)
    clean = ops.rise_accumulate(scores[:, :3].contiguous().to(DEV), dev, H, W, 0.1)
    bad = scores[:, :3].clone()
    bad[64, 1] = float("nan")                              # the last mask: a chunk of its own
    bad[3, 2] = float("inf")                               # mask 3 of the bank is the grid of zeros: inf * 0 everywhere
    out = ops.rise_accumulate(bad.contiguous().to(DEV), dev, H, W, 0.1)
    assert torch.equal(out[0], clean[0])
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[2]).all())
    bad = scores[:, :3].clone()
    bad[2, 0] = float("inf")                               # mask 2 is the grid of ones: +inf everywhere, no NaN
    out = ops.rise_accumulate(bad.contiguous().to(DEV), dev, H, W, 0.1)
    assert bool(torch.isposinf(out[0]).all()) and torch.equal(out[1:], clean[1:])
    # guards around `out` stay NaN; the bank's host copy is what is validated
    pad, T = 64, 3
    buf = torch.full((pad + T * H * W + pad,), float("nan"), device=DEV)
    sc = scores[:, :3].contiguous().to(DEV)
    code = lib.bcos_rise_accumulate(ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(dev.rows.data_ptr()), ctypes.c_void_p(bank.rows.data_ptr()),
                                    ctypes.c_void_p(buf.data_ptr() + 4 * pad), n, T, s, H, W, ctypes.c_float(0.1), stream())
    assert code == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + T * H * W:]).all())
    assert torch.equal(buf[pad:pad + T * H * W].view(T, H, W), clean)


# ---------------------------------------------------------------------------------------------------------------- 4. rise= forward
def _chunked(forward, n, chunk):
    return torch.cat([forward(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)])


def test_rise_forward_resnet18_equals_the_materialised_batch(lib, golden_dir):
    from bcos_hip import engine, ops, synth
    net = golden_net(golden_dir)
    eng = engine.attach(net)
    H = W = 32
    n = 70                                                 # two sub-batch streams, cut along the copy index
    img = synth.synthetic_images(1, seed=21, size=H).to(DEV)
    bank = random_bank(n, H, W, 4, seed=5).to(DEV)
    masked = (img * ops.rise_masks(bank, H, W)[:, None]).contiguous()
    assert eng.n_streams(masked) >= 2
    out = eng.forward(img, rise=bank)
    assert out.shape == (n, 1000) and bool(torch.isfinite(out).all())
    assert torch.equal(out, eng.forward(masked))
    for chunk in (8, 64):
        assert torch.equal(_chunked(lambda lo, hi: eng.forward(img, rise=bank[lo:hi]), n, chunk), out), chunk
    rects = torch.tensor([[0, 4, 0, 4]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="one of the three"):
        eng.forward(img, rise=bank, occlude=rects)
    with pytest.raises(ValueError):
        eng.forward(img[:, :3], rise=bank)                 # masking before AddInverse is another operator
    with pytest.raises(ValueError):
        eng.forward(torch.cat([img, img]), rise=bank)
    with pytest.raises(ValueError):
        eng.forward(img, rise=ops.RiseBank(bank.rows.cpu(), 4))
    with pytest.raises(ValueError):
        eng.forward(img, rise=bank.rows)


def test_rise_forward_simple_vit_equals_the_materialised_batch(lib):
    from bcos_hip import ops, synth, vit_engine
    vnet = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV).eval()
    x = synth.synthetic_images(1, seed=11).to(DEV)
    veng = vit_engine.attach(vnet)
    bank = random_bank(12, 224, 224, 8, seed=9).to(DEV)
    masked = (x * ops.rise_masks(bank, 224, 224)[:, None]).contiguous()
    out = veng.forward(x, rise=bank)
    assert out.shape == (12, 1000) and bool(torch.isfinite(out).all())
    assert torch.equal(out, veng.forward(masked))
    assert torch.equal(_chunked(lambda lo, hi: veng.forward(x, rise=bank[lo:hi]), 12, 5), out)


# ---------------------------------------------------------------------------------------------------------------- 5. end-to-end maps
def _check_maps(case, data, sel, what):
    name = case["name"]
    rec64 = torch.from_numpy(data[f"{name}/selection64"])
    peak = float(rec64.abs().max())
    tol = max(1e-4, 3 * case["d_ref"])
    d64 = float((sel.double().cpu() - rec64).abs().max()) / peak
    d32 = float((sel.double().cpu() - torch.from_numpy(data[f"{name}/selection"]).double()).abs().max()) / peak
    print(f"RISE map {name} ({what}): max |ours - recorded| / peak: {d64:.2e} (float64 maps), {d32:.2e} (float32 maps); bound {tol:.1e}, "
          f"the reference's own spread {case['d_ref']:.2e}")
    assert d64 <= tol and d32 <= tol, (name, what)
    return peak, tol


def test_end_to_end_maps_engine_and_module_path(lib, fixture, golden_dir):
    from bcos_hip import engine, synth
    from interpretability.explanation_methods.explainers.rise import RISE
    meta, data = fixture
    net = golden_net(golden_dir)
    for case in meta["cases"]:
        name, H = case["name"], case["size"]
        img = synth.synthetic_images(1, seed=case["image_seed"], size=H).to(DEV)
        engine.detach(net)
        rise = RISE(net, **case["kwargs"])
        mod = rise.attribute_selection(img, case["targets"])                    # the nn.Module path: img * ops.rise_masks(...)
        assert mod.shape == (3, 1, H, H) and mod.is_cuda
        _check_maps(case, data, mod, "module path")
        engine.attach(net)
        rise = RISE(net, **case["kwargs"])
        sel = rise.attribute_selection(img, case["targets"])
        peak, tol = _check_maps(case, data, sel, "engine")
        d = float((sel.double() - mod.double()).abs().max()) / peak
        print(f"RISE map {name}: engine path vs module path {d:.2e} of the peak")
        assert d <= tol
        # the scores behind the maps: sigmoid of the engine's logits against the recorded float64 probabilities
        bank = rise._bank(img)
        classes = torch.from_numpy(data[f"{name}/classes"]).to(DEV)
        prob = torch.sigmoid(net._bcos_engine.forward(img, rise=bank))[:, classes]
        ref = torch.from_numpy(data[f"{name}/scores64"])
        assert float((prob.double().cpu() - ref).norm() / ref.norm()) <= 1e-4
        one = rise.attribute(img, case["targets"][:1])
        assert one.shape == (1, 1, H, H) and torch.equal(one, sel[:1])
        rise.engine_batch_size = 8                                               # results do not depend on the chunk size
        assert torch.equal(rise.attribute_selection(img, torch.tensor(case["targets"])), sel)
    full = rise.attribute(img, None, return_all=True)
    assert full.shape == (1000, 1, H, H)
    assert float((full[case["targets"]].double() - sel.double()).abs().max()) / peak <= tol      # (torch's sigmoid against bcos_class_scores')


# ---------------------------------------------------------------------------------------------------------------- 6. harness
def test_grid_pointing_game_with_the_rise_explainer(lib, golden_dir):
    from bcos_hip import engine, localisation, synth
    from interpretability.explanation_methods.explainers.rise import RISE
    net = golden_net(golden_dir)
    singles = synth.synthetic_images(4, seed=31, size=32).to(DEV)
    multi = localisation.make_multi_image(singles)
    assert multi.shape == (1, 6, 64, 64)
    engine.attach(net)
    tgts = net._bcos_engine.forward(singles).argmax(1).view(1, -1).cpu()
    rise = RISE(net, n=64, s=4, p1=0.5, batch_size=8)
    res = localisation.grid_pointing_game(None, multi, tgts, 32, explainer=rise)
    assert res["attributions"].shape == (1, 4, 64, 64) and res["fractions"].shape == (1, 4, 4) and res["metric"].shape == (1, 4)
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    assert float((res["fractions"].sum(-1) - 1).abs().max()) <= 1e-5
    own = torch.stack([rise.attribute_selection(multi, tgts[0].tolist()).sum(1)])
    assert torch.equal(own, res["attributions"])
