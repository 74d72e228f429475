"""`-m gpu`: the two Occlusion kernels, the engines' occluded forward, the explainer and the harness on the device, against the fixtures
the reference recorded (tests/golden/make_golden_occlusion.py) and against float64 evaluations of the documented formula.

Bounds (none taken from what the kernels return):
  * prepared input: bit-equality with bcos_prep_input on the materialised `img * mask_i`;
  * accumulate: the fp32 chain over the k covering masks is within (k + 2) 2^-24 sum |d / n_part| of the exact sum
    (occlusion_emulation.chain_bound); the reference's own fp32 map, summed in torch's order, within twice that;
  * occluded logits: relative L2 <= 1e-4 against the recorded float64 logits (the bound of test_resnet18_config1_against_reference_golden),
    here per row as well, which makes tau_row = 1e-4 ||row||_2 a bound on every logit's error;
  * end-to-end map: the map is linear in the logits, so its error is at most sum over the covering masks of (tau_org + tau_m) / n_part,
    plus the chain bound.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import occlusion_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN = (0.485, 0.456, 0.406, 0.515, 0.544, 0.594)
STD = (0.229, 0.224, 0.225, 0.229, 0.224, 0.225)
LOGIT_TOL = 1e-4


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "occlusion.json"))), np.load(os.path.join(golden_dir, "occlusion.npz"))


def golden_net(golden_dir):
    from bcos_hip import synth
    meta = json.load(open(os.path.join(golden_dir, "resnet18_e2e.json")))
    data = np.load(os.path.join(golden_dir, "resnet18_e2e.npz"))
    net = synth.build_bcosified_resnet(meta["arch"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    return net.to(DEV).eval()


def case_image(case):
    from bcos_hip import synth
    return synth.synthetic_images(1, seed=case["image_seed"], size=case["size"]).to(DEV)


def consts():
    return torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)


def random_bank(n, H, W, seed, full_every=0):
    g = torch.Generator().manual_seed(seed)
    r0 = torch.randint(0, H, (n,), generator=g)
    c0 = torch.randint(0, W, (n,), generator=g)
    r1 = (r0 + 1 + torch.randint(0, H, (n,), generator=g)).clamp(max=H)
    c1 = (c0 + 1 + torch.randint(0, W, (n,), generator=g)).clamp(max=W)
    bank = torch.stack([r0, r1, c0, c1], 1).to(torch.int32)
    if full_every:
        bank[::full_every] = torch.tensor([0, H, 0, W], dtype=torch.int32)
    return bank.contiguous()


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------- 1. prepared input
def _prep_pair(img, bank, first, n):
    """(occluded prep, prep of the materialised copies), each with the per-pixel maxima its launch emitted"""
    from bcos_hip import ops
    mean, std = consts()
    H, W = img.shape[-2:]
    a = ops.prep_input_occluded(img, bank.to(DEV), mean, std, first=first, n=n, want_absmax=True)
    masked = (img * E.keep_masks(bank[first:first + n], H, W).to(DEV)).contiguous()
    b = ops.prep_input(masked, mean, std, want_absmax=True)
    return a, ops.absmax_of(a), b, ops.absmax_of(b)


def test_prepared_input_equals_prep_of_the_masked_copies(lib, fixture):
    from bcos_hip import lib as blib
    meta, data = fixture
    prev = blib.get_contraction_mode()
    try:
        for mode in ("f16x2", "bf16x3"):                   # with and without the fused per-pixel maxima
            blib.set_contraction_mode(mode)
            for case in meta["cases"]:
                bank = torch.from_numpy(data[f"{case['name']}/rects"])
                a, am_a, b, am_b = _prep_pair(case_image(case), bank, 0, bank.shape[0])
                assert a.shape == (bank.shape[0], case["size"], case["size"], 8)
                assert torch.equal(a, b), (mode, case["name"])
                assert (am_a is None) == (am_b is None) == (mode != "f16x2")
                if am_a is not None:
                    assert torch.equal(am_a, am_b), case["name"]
            # a ragged size and an offset into the bank
            img = torch.rand(1, 6, 13, 11, generator=torch.Generator().manual_seed(5)).to(DEV) - 0.25
            bank = random_bank(37, 13, 11, seed=6, full_every=9)
            for first, n in ((0, 37), (5, 17), (36, 1)):
                a, am_a, b, am_b = _prep_pair(img, bank, first, n)
                assert torch.equal(a, b), (first, n)
                if am_a is not None:
                    assert torch.equal(am_a, am_b)
    finally:
        blib.set_contraction_mode(prev)
    # inside a rectangle every channel is (0 - mean) / std
    mean, std = consts()
    assert torch.equal(a[0, bank[36, 0], bank[36, 2], :6], (0 - mean) / std)


def test_prepared_input_writes_nothing_outside_its_tensors(lib):
    from bcos_hip import ops
    H, W, n, pad = 13, 11, 7, 64
    img = torch.rand(1, 6, H, W, generator=torch.Generator().manual_seed(8)).to(DEV)
    bank = random_bank(20, H, W, seed=9).to(DEV)
    mean, std = consts()
    for cpad in (8, 12):
        size = n * H * W * cpad
        buf = torch.full((pad + size + pad,), float("nan"), device=DEV)
        am = torch.full((pad + n * H * W + pad,), -1, device=DEV, dtype=torch.int32)
        code = lib.bcos_prep_input_occluded(ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(bank.data_ptr() + 16 * 3),
                                            ctypes.c_void_p(buf.data_ptr() + 4 * pad), ctypes.c_void_p(mean.data_ptr()),
                                            ctypes.c_void_p(std.data_ptr()), ctypes.c_void_p(am.data_ptr() + 4 * pad), n, 6, H, W, cpad, 0,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + size:]).all())
        assert bool((am[:pad] == -1).all()) and bool((am[pad + n * H * W:] == -1).all())
        want = ops.prep_input((img * E.keep_masks(bank[3:3 + n].cpu(), H, W).to(DEV)).contiguous(), mean, std, cpad=cpad)
        got = buf[pad:pad + size].view(n, H, W, cpad)
        assert torch.equal(got, want)
        assert torch.equal(am[pad:pad + n * H * W].view(n, H, W), (got.abs().amax(-1)).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 2.-4. accumulate
def _recorded(case, data):
    name = case["name"]
    return (torch.from_numpy(data[f"{name}/org_out"]), torch.from_numpy(data[f"{name}/pert_out"]), torch.from_numpy(data[f"{name}/rects"]),
            [data[f"{name}/classes"].tolist().index(t) for t in case["targets"]])


def _accumulate(org, pert, bank, H, W, targets=None, only_positive=False):
    from bcos_hip import ops
    return ops.occlusion_accumulate(org.reshape(-1).to(DEV), pert.to(DEV).contiguous(), bank.to(DEV), H, W, targets=targets,
                                    only_positive=only_positive, rects_host=bank).cpu()


def test_accumulate_against_float64_and_the_reference_map(lib, fixture):
    meta, data = fixture
    for case in meta["cases"]:
        org, pert, bank, local = _recorded(case, data)
        H = W = case["size"]
        pos = bool(case["kwargs"].get("only_positive", False))
        exact, mag, cover = E.formula64(org, pert, bank, H, W, None, pos)
        bound = E.chain_bound(mag, cover)
        out = _accumulate(org, pert, bank, H, W, None, pos)
        assert out.shape == (org.shape[1], H, W)
        err = (out.double() - exact).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"occlusion accumulate {case['name']}: {bank.shape[0]} masks, cover {int(cover.min())}..{int(cover.max())}, "
              f"worst |fp32 - fp64| / bound {worst:.3f}")
        assert bool((err <= bound).all()), (case["name"], worst)
        # the map the reference built from the same fp32 logits, in torch's summation order
        rec = torch.from_numpy(data[f"{case['name']}/selection"])[:, 0].double()
        err_ref = (out[local].double() - rec).abs()
        worst_ref = float((err_ref / (2 * bound[local]).clamp_min(1e-300)).max())
        print(f"occlusion accumulate {case['name']}: worst |ours - reference fp32 map| / (2 x bound) {worst_ref:.3f}")
        assert bool((err_ref <= 2 * bound[local]).all()), (case["name"], worst_ref)
        # the explicit-target form: the matching rows of the all-class form, bit for bit; two runs agree bit for bit
        sel = _accumulate(org, pert, bank, H, W, local, pos)
        assert torch.equal(sel, out[local])
        assert torch.equal(_accumulate(org, pert, bank, H, W, None, pos), out)
        assert torch.equal(_accumulate(org, pert, bank, H, W, [local[1]], pos)[0], out[local[1]])
        # both signs of the clamp on every case
        flip = _accumulate(org, pert, bank, H, W, local, not pos)
        e2, m2, _ = E.formula64(org, pert, bank, H, W, local, not pos)
        assert bool(((flip.double() - e2).abs() <= E.chain_bound(m2, cover)).all())
        if pos:
            assert float(out.min()) >= 0.0 and not torch.equal(flip, sel)
        # the chain is the documented one: subtraction, division, additions in ascending m -- the numpy restatement gives the same bits
        assert torch.equal(out, E.occlusion_accumulate(org, pert, bank, H, W, None, pos))


@pytest.mark.parametrize("n,H,W,CL,full_every", [(1500, 70, 45, 100, 0), (2100, 40, 33, 70, 1), (300, 9, 200, 33, 7)])
def test_accumulate_on_general_banks(lib, n, H, W, CL, full_every):
    """banks no named configuration produces: rectangles of every size in random order, ragged tiles, class counts that are no multiple
    of the register chunk, and (full_every = 1) every rectangle covering the whole image, which overfills the tile list"""
    g = torch.Generator().manual_seed(n)
    bank = random_bank(n, H, W, seed=n + 1, full_every=full_every)
    org = torch.randn(1, CL, generator=g)
    pert = org + torch.randn(n, CL, generator=g) * 0.1
    exact, mag, cover = E.formula64(org, pert, bank, H, W)
    out = _accumulate(org, pert, bank, H, W)
    err = (out.double() - exact).abs()
    bound = E.chain_bound(mag, cover)
    print(f"occlusion accumulate n={n} {H}x{W} CL={CL}: cover {int(cover.min())}..{int(cover.max())}, worst / bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((out[:, cover == 0] == 0).all())                    # pixels no mask covers
    assert torch.equal(out, E.occlusion_accumulate(org, pert, bank, H, W))
    targets = [CL - 1, 0, 0, -1, 5]                                 # repeated and negative (wrapped on the host) classes
    sel = _accumulate(org, pert, bank, H, W, targets)
    assert torch.equal(sel, out[[CL - 1, 0, 0, CL - 1, 5]])
    pos = _accumulate(org, pert, bank, H, W, None, True)
    assert torch.equal(pos, E.occlusion_accumulate(org, pert, bank, H, W, None, True)) and float(pos.min()) >= 0.0


def test_accumulate_leaves_its_surroundings_alone(lib):
    n, H, W, CL, T, pad = 40, 13, 11, 9, 4, 64
    bank = random_bank(n, H, W, seed=3)
    g = torch.Generator().manual_seed(4)
    org, pert = torch.randn(CL, generator=g).to(DEV), torch.randn(n, CL, generator=g).to(DEV)
    tg = torch.tensor([8, 0, 3, 3], dtype=torch.int32, device=DEV)
    dev_bank = bank.to(DEV)
    buf = torch.full((pad + T * H * W + pad,), float("nan"), device=DEV)
    code = lib.bcos_occlusion_accumulate(ctypes.c_void_p(org.data_ptr()), ctypes.c_void_p(pert.data_ptr()), ctypes.c_void_p(dev_bank.data_ptr()),
                                         ctypes.c_void_p(bank.data_ptr()), ctypes.c_void_p(tg.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 4 * pad),
                                         n, CL, T, H, W, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + T * H * W:]).all())
    assert torch.equal(buf[pad:pad + T * H * W].view(T, H, W).cpu(), E.occlusion_accumulate(org, pert, bank, H, W, [8, 0, 3, 3]))


# ---------------------------------------------------------------------------------------------------------------- 5. occluded logits
def _chunked(forward, n, chunk):
    return torch.cat([forward(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)])


def test_occluded_logits_resnet18(lib, fixture, golden_dir):
    from bcos_hip import engine
    meta, data = fixture
    net = golden_net(golden_dir)
    eng = engine.attach(net)
    for case in meta["cases"]:
        name = case["name"]
        img = case_image(case)
        bank = torch.from_numpy(data[f"{name}/rects"]).to(DEV)
        n, H = bank.shape[0], case["size"]
        classes = torch.from_numpy(data[f"{name}/classes"]).to(DEV)
        out = eng.forward(img, occlude=bank)
        assert out.shape == (n, 1000)
        ref64 = torch.from_numpy(data[f"{name}/pert_out64"])
        r = rel(out[:, classes], ref64)
        rows = ((out[:, classes].double().cpu() - ref64).norm(dim=1) / ref64.norm(dim=1))
        print(f"occluded logits {name}: relL2 {r:.2e} against the recorded float64 logits, worst row {float(rows.max()):.2e}")
        assert r <= LOGIT_TOL and float(rows.max()) <= LOGIT_TOL
        assert rel(eng.forward(img)[:, classes], data[f"{name}/org_out64"]) <= LOGIT_TOL
        masked = (img * E.keep_masks(bank.cpu(), H, H).to(DEV)).contiguous()
        for chunk in (8, 256):
            a = _chunked(lambda lo, hi: eng.forward(img, occlude=bank[lo:hi]), n, chunk)
            b = _chunked(lambda lo, hi: eng.forward(masked[lo:hi]), n, chunk)
            assert torch.equal(a, b), (name, chunk)
            assert torch.equal(a, out), (name, chunk)
    with pytest.raises(ValueError):
        eng.forward(img[:, :3], occlude=bank)                       # masking before AddInverse is another operator
    with pytest.raises(ValueError):
        eng.forward(torch.cat([img, img]), occlude=bank)
    with pytest.raises(ValueError):
        eng.forward(img, occlude=bank.cpu())


def test_occluded_logits_vit_and_module_path(lib, fixture, golden_dir):
    from bcos_hip import synth, vit_engine
    from interpretability.explanation_methods.explainers import get_explainer
    vnet = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV).eval()
    x = synth.synthetic_images(1, seed=11).to(DEV)
    veng = vit_engine.attach(vnet)
    occ = get_explainer(vnet, "Occlusion", "default", stride=16, ks=16)        # 196 masks: three sub-batch streams
    occ.make_masks(x)
    bank = occ.masks.to(DEV)
    assert bank.shape == (196, 4)
    masked = (x * E.keep_masks(occ.masks, 224, 224).to(DEV)).contiguous()
    out = veng.forward(x, occlude=bank)
    assert out.shape == (196, 1000) and bool(torch.isfinite(out).all())
    assert torch.equal(out, veng.forward(masked))
    assert torch.equal(_chunked(lambda lo, hi: veng.forward(x, occlude=bank[lo:hi]), 196, 8), out)
    sel = occ.attribute_selection(x, [3, 500])
    exact, mag, cover = E.formula64(veng.forward(x), out, occ.masks, 224, 224, [3, 500])
    assert sel.shape == (2, 1, 224, 224) and sel.device == x.device
    assert bool(((sel[:, 0].double().cpu() - exact).abs() <= E.chain_bound(mag, cover)).all())

    # the nn.Module path: no engine, the chunks masked with torch ops; the same accumulate kernel
    meta, data = fixture
    net = golden_net(golden_dir)
    case = meta["cases"][0]
    img = case_image(case)
    occ = get_explainer(net, "Occlusion", case["config"], **{k: v for k, v in case["kwargs"].items()})
    sel = occ.attribute_selection(img, case["targets"])
    _check_map(case, data, sel, None, "module path")


# ---------------------------------------------------------------------------------------------------------------- 6. end-to-end map
def _check_map(case, data, sel, logits, what):
    """sel [3, 1, H, W] from our logits against the reference's float64 map of the same targets.  `logits` = (org, pert) of ours restricted
    to the recorded classes, or None: the per-logit tolerance tau_row is then taken as met (checked where logits are at hand)."""
    name, H = case["name"], case["size"]
    classes = data[f"{name}/classes"].tolist()
    local = [classes.index(t) for t in case["targets"]]
    org64, pert64 = torch.from_numpy(data[f"{name}/org_out64"]), torch.from_numpy(data[f"{name}/pert_out64"])
    bank = torch.from_numpy(data[f"{name}/rects"])
    pos = bool(case["kwargs"].get("only_positive", False))
    tau_o, tau_m = LOGIT_TOL * float(org64.norm()), LOGIT_TOL * pert64.norm(dim=1)
    if logits is not None:
        assert float((logits[0].double().cpu() - org64).abs().max()) <= tau_o
        assert bool(((logits[1].double().cpu() - pert64).abs().amax(1) <= tau_m).all())
    env = torch.zeros(H, H, dtype=torch.float64)
    for m, (r0, r1, c0, c1) in enumerate(bank.tolist()):
        env[r0:r1, c0:c1] += (tau_o + float(tau_m[m])) / ((r1 - r0) * (c1 - c0))
    _, mag, cover = E.formula64(org64, pert64, bank, H, H, local, pos)
    ref = torch.from_numpy(data[f"{name}/selection64"])[:, 0]
    assert sel.shape == (3, 1, H, H) and sel.is_cuda
    err = (sel[:, 0].double().cpu() - ref).abs()
    allowed = env[None] + E.chain_bound(mag, cover)
    assert bool((err <= allowed).all()), (name, what, float((err / allowed).max()))
    floor = case["reference_self_floor"]["map_fp32_vs_fp64_over_peak"]
    dev = float(err.max()) / case["map_peak"]
    print(f"occlusion map {name} ({what}): max |ours - reference float64 map| / peak {dev:.2e} = {dev / floor:.2f} x the reference's own "
          f"fp32-vs-fp64 spread ({floor:.2e}); worst error / envelope {float((err / allowed).max()):.2e}")


def test_end_to_end_maps_on_the_engine(lib, fixture, golden_dir):
    from bcos_hip import engine
    from interpretability.explanation_methods.explainers import get_explainer
    meta, data = fixture
    net = golden_net(golden_dir)
    eng = engine.attach(net)
    for case in meta["cases"]:
        name = case["name"]
        img = case_image(case)
        occ = get_explainer(net, "Occlusion", case["config"], **{k: v for k, v in case["kwargs"].items()})
        sel = occ.attribute_selection(img, case["targets"])
        classes = torch.from_numpy(data[f"{name}/classes"]).to(DEV)
        bank = torch.from_numpy(data[f"{name}/rects"]).to(DEV)
        assert torch.equal(occ.masks, bank.cpu())
        _check_map(case, data, sel, (eng.forward(img)[:, classes], eng.forward(img, occlude=bank)[:, classes]), "engine")
        one = occ.attribute(img, case["targets"][0])
        assert one.shape == (1, 1, case["size"], case["size"]) and torch.equal(one, sel[:1])
        assert torch.equal(occ.attribute(img, torch.tensor(case["targets"][:1])), one)
        occ.engine_batch_size = 8                                    # results do not depend on the chunk size
        assert torch.equal(occ.attribute_selection(img, case["targets"]), sel)
    full = occ.attribute(img, None, return_all=True)
    assert full.shape == (1, 1000, case["size"], case["size"]) and torch.equal(full[0, case["targets"]][:, None], sel)


# ---------------------------------------------------------------------------------------------------------------- 7. harness
def test_grid_pointing_game_with_the_occlusion_explainer(lib, golden_dir):
    from bcos_hip import engine, localisation, synth
    from interpretability.explanation_methods.explainers import get_explainer
    net = golden_net(golden_dir)
    loc = json.load(open(os.path.join(golden_dir, "localisation.json")))
    data = np.load(os.path.join(golden_dir, "localisation.npz"))
    singles = synth.synthetic_images(loc["n_imgs"], seed=loc["image_seed"], size=loc["single_shape"]).to(DEV)
    multi = localisation.make_multi_image(singles)
    tgts = torch.from_numpy(data["targets"]).view(1, -1)
    engine.attach(net)
    occ = get_explainer(net, "Occlusion", "default")               # 49 masks of 32 x 32 on the 224 x 224 multi-image
    res = localisation.grid_pointing_game(None, multi, tgts, loc["single_shape"], smooth=15, explainer=occ)
    T = tgts.shape[1]
    assert res["attributions"].shape == (1, T, 224, 224) and res["fractions"].shape == (1, T, T) and res["metric"].shape == (1, T)
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    assert float((res["fractions"].sum(-1) - 1).abs().max()) <= 1e-5
    own = torch.stack([occ.attribute_selection(multi, tgts[0].tolist()).sum(1)])
    assert torch.equal(own, res["attributions"])
    again = localisation.grid_pointing_game(None, multi, tgts, loc["single_shape"], smooth=15, attributions=own)
    assert all(torch.equal(res[k], again[k]) for k in res)
