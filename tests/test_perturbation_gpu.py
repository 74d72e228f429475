"""`-m gpu`: the pixel-perturbation kernels, the engines' perturbed forward and the harness on the device.

Bounds (none taken from what the kernels return):
  * select: the thresholds are integers -- torch.equal with the stable numpy sort of tests/perturbation_emulation.py;
  * prepared input: bit-equality with bcos_prep_input on the materialised copies, per-pixel maxima included;
  * class scores: the logit is an exact copy; sigmoid and softmax are held against float64 within the bounds include/bcos_hip.h states,
    evaluated from the inputs (perturbation_emulation.sigmoid_bound / softmax_bound);
  * perturbed forward: bit-equality with forward() on the materialised copies (an image's result does not depend on its batch);
  * harness, k = 0 column: relative L2 <= 1e-4 against engine.forward(x), the logit bound of test_resnet18_config1_against_reference_golden.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import perturbation_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN = (0.485, 0.456, 0.406, 0.515, 0.544, 0.594)
STD = (0.229, 0.224, 0.225, 0.229, 0.224, 0.225)
SHAPES = [(13, 11), (97, 89), (300, 231)]          # below one workgroup; several with a ragged tail; pixel indices past 2^16
KINDS = ["normal", "equal", "quant4", "special"]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def consts():
    return torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)


def golden_net(golden_dir):
    from bcos_hip import synth
    meta = json.load(open(os.path.join(golden_dir, "resnet18_e2e.json")))
    data = np.load(os.path.join(golden_dir, "resnet18_e2e.npz"))
    net = synth.build_bcosified_resnet(meta["arch"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    return net.to(DEV).eval()


def scores_of(kind, HW, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(HW, generator=g)
    if kind == "equal":
        return torch.full((HW,), 0.375)                               # a pure index tie-break
    if kind == "quant4":
        return torch.randint(0, 4, (HW,), generator=g).float() - 1.0  # long tie runs that straddle workgroups
    s = torch.randn(HW, generator=g)
    s[::7] = s[3]
    vals = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-42, -1e-42, 3e-39, float("nan"), -0.0, 0.0, float("inf")])
    s[torch.randperm(HW, generator=g)[:vals.numel()]] = vals
    return s


def batch_scores(kind, B, HW, seed):
    """B images; 'mixed': a different distribution per image"""
    kinds = [KINDS[(b + 1) % len(KINDS)] for b in range(B)] if kind == "mixed" else [kind] * B
    return torch.stack([scores_of(k, HW, seed + b) for b, k in enumerate(kinds)]).contiguous()


# ---------------------------------------------------------------------------------------------------------------- 1. select
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind,B", [("normal", 1), ("equal", 1), ("quant4", 2), ("special", 1), ("mixed", 3)])
def test_select_equals_the_stable_sort(lib, shape, kind, B):
    from bcos_hip import ops
    HW = shape[0] * shape[1]
    scores = batch_scores(kind, B, HW, seed=HW + B)
    counts = [HW // 3, 0, HW, 1, HW - 1, HW // 3, 5, HW // 2]          # unsorted, with a duplicate and both ends
    dev = scores.to(DEV)
    for desc in (False, True):
        want = E.perturb_select(scores, counts, desc)
        got = ops.perturb_select(dev, counts, descending=desc)
        assert got.dtype == torch.int64 and got.shape == (B, len(counts)) and got.is_cuda
        assert torch.equal(got.cpu(), want), (shape, kind, desc)
        assert torch.equal(ops.perturb_select(dev, counts, descending=desc), got)              # two calls: identical
        for j in (1, 4):                                                  # a single count gives the same threshold as among others
            assert torch.equal(ops.perturb_select(dev, counts[j:j + 1], descending=desc), got[:, j:j + 1])


def test_select_with_one_and_with_sixty_four_counts(lib):
    from bcos_hip import ops
    H, W = SHAPES[1]
    HW = H * W
    scores = batch_scores("mixed", 3, HW, seed=7)
    g = torch.Generator().manual_seed(8)
    counts = torch.randint(0, HW + 1, (64,), generator=g).tolist()
    counts[10], counts[63], counts[40] = HW, 0, counts[41]
    for desc in (False, True):
        assert torch.equal(ops.perturb_select(scores.to(DEV), counts, descending=desc).cpu(), E.perturb_select(scores, counts, desc))
        assert torch.equal(ops.perturb_select(scores.to(DEV), [HW // 2], descending=desc).cpu(), E.perturb_select(scores, [HW // 2], desc))


def test_select_above_the_histogram_grid_cap(lib):
    """the pixel workgroups of the histogram passes are capped at 128 x 1024 pixels: at 401 x 331 = 132 731 pixels every one of them takes
    its grid-stride loop, the last with a ragged tail; counts on either side of the cap"""
    from bcos_hip import ops
    HW = 401 * 331
    assert HW > 128 * 1024
    scores = batch_scores("mixed", 4, HW, seed=41)
    counts = [128 * 1024, 0, HW, 1, HW - 1, 128 * 1024 + 1, HW // 2, 70000]
    dev = scores.to(DEV)
    for desc in (False, True):
        got = ops.perturb_select(dev, counts, descending=desc)
        assert torch.equal(got.cpu(), E.perturb_select(scores, counts, desc)), desc
        assert torch.equal(ops.perturb_select(dev, counts, descending=desc), got)


@pytest.mark.parametrize("shape,B,K", [(SHAPES[1], 3, 5), (SHAPES[0], 64, 64)])
def test_select_leaves_its_surroundings_alone(lib, shape, B, K):
    """the words of ws and thr_out beyond their sizes keep a canary; a workspace full of garbage does not change the result.
    B = K = 64: the 64 x 65 x 256 words the call clears exceed its clearing launch of 4096 x 256 threads, which takes its grid-stride loop"""
    HW, pad = shape[0] * shape[1], 64
    scores = batch_scores("mixed", B, HW, seed=9)
    if K == 5:
        counts = [0, 17, HW, 4000, 17]
    else:
        assert B * 256 * (K + 1) > 4096 * 256
        counts = torch.randint(0, HW + 1, (K,), generator=torch.Generator().manual_seed(10)).tolist()
        counts[0], counts[1], counts[2] = HW, 0, counts[3]
    need = ctypes.c_int64(0)
    assert lib.bcos_perturb_select_ws_bytes(B, HW, K, ctypes.byref(need)) == 0 and need.value % 8 == 0
    words = need.value // 8
    ws = torch.full((pad + words + pad,), 0x5A5A5A5A5A5A5A5A, device=DEV, dtype=torch.int64)
    thr = torch.full((pad + B * K + pad,), -7, device=DEV, dtype=torch.int64)
    host = (ctypes.c_int32 * K)(*counts)
    dev = scores.to(DEV)
    code = lib.bcos_perturb_select(ctypes.c_void_p(dev.data_ptr()), ctypes.cast(host, ctypes.c_void_p), 0, ctypes.c_void_p(thr.data_ptr() + 8 * pad),
                                   ctypes.c_void_p(ws.data_ptr() + 8 * pad), need.value, B, HW, K,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0x5A5A5A5A5A5A5A5A).all()) and bool((ws[pad + words:] == 0x5A5A5A5A5A5A5A5A).all())
    assert bool((thr[:pad] == -7).all()) and bool((thr[pad + B * K:] == -7).all())
    assert torch.equal(thr[pad:pad + B * K].view(B, K).cpu(), E.perturb_select(scores, counts, False))


# ---------------------------------------------------------------------------------------------------------------- 2. prepared input
def _case(shape, B=3, K=5, seed=0, desc=False):
    H, W = shape
    HW = H * W
    g = torch.Generator().manual_seed(1000 + seed + HW)
    x = torch.rand(B, 6, H, W, generator=g) * 0.98 + 0.01            # (no pixel is zero in every channel)
    scores = batch_scores("mixed", B, HW, seed=seed + 11)
    counts = [0, HW // 4, 7, HW, HW - 1][:K]
    thr = E.perturb_select(scores, counts, desc)
    return x, scores, thr, counts


@pytest.mark.parametrize("shape", SHAPES)
def test_prepared_input_equals_prep_of_the_materialised_copies(lib, shape):
    from bcos_hip import lib as blib, ops
    H, W = shape
    B, K = 3, 5
    mean, std = consts()
    removed_value = (0 - mean) / std
    prev = blib.get_contraction_mode()
    try:
        for mode, desc in (("f16x2", False), ("bf16x3", True)):          # with and without the fused per-pixel maxima
            blib.set_contraction_mode(mode)
            x, scores, thr, counts = _case(shape, B, K, seed=3, desc=desc)
            copies = E.materialise(x, scores, thr, desc).to(DEV)
            xd, sd, td = x.to(DEV), scores.to(DEV), thr.to(DEV)
            for first, n in ((0, B * K), (4, 7), (B * K - 1, 1), (5, 5)):
                a = ops.prep_input_perturbed(xd, sd, td, mean, std, descending=desc, first=first, n=n, want_absmax=True)
                b = ops.prep_input(copies[first:first + n].contiguous(), mean, std, want_absmax=True)
                assert a.shape == (n, H, W, 8) and torch.equal(a, b), (mode, first, n)
                am_a, am_b = ops.absmax_of(a), ops.absmax_of(b)
                assert (am_a is None) == (am_b is None) == (mode != "f16x2")
                if am_a is not None:
                    assert torch.equal(am_a, am_b), (first, n)
                gone = (a[..., :6] == removed_value).all(-1).flatten(1).sum(1).tolist()
                assert gone == [counts[c % K] for c in range(first, first + n)]      # exactly k_j removed pixels per copy
    finally:
        blib.set_contraction_mode(prev)


def _prep_perturbed_raw(lib, xd, sd, td, desc, mean, std, B, K, first, n, H, W, cpad, pad, absmax):
    """bcos_prep_input_perturbed through ctypes into buffers with `pad` canary words on either side -> (out [n,H,W,cpad], absmax or None);
    asserts that the canaries survived"""
    size, px = n * H * W * cpad, n * H * W
    buf = torch.full((pad + size + pad,), float("nan"), device=DEV)
    am = torch.full((pad + px + pad,), -1, device=DEV, dtype=torch.int32)
    code = lib.bcos_prep_input_perturbed(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(sd.data_ptr()), ctypes.c_void_p(td.data_ptr()), int(desc),
                                         ctypes.c_void_p(buf.data_ptr() + 4 * pad), ctypes.c_void_p(mean.data_ptr()),
                                         ctypes.c_void_p(std.data_ptr()), ctypes.c_void_p(am.data_ptr() + 4 * pad) if absmax else None,
                                         B, K, first, n, 6, H, W, cpad, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + size:]).all()), (first, n, cpad, pad)
    assert bool((am[:pad] == -1).all()) and bool((am[pad + px:] == -1).all()), (first, n, cpad, pad)
    if not absmax:
        assert bool((am == -1).all())
    return buf[pad:pad + size].view(n, H, W, cpad), (am[pad:pad + px].view(n, H, W) if absmax else None)


@pytest.mark.parametrize("shape", SHAPES)
def test_prepared_input_writes_nothing_outside_its_tensors(lib, shape):
    """NaN canaries around `out` (and -1 around the per-pixel maxima) at every shape, for the full range of copies and for sub-ranges,
    in both contraction modes (f16x2: with the fused maxima; bf16x3: without).  Also a 12-channel padding and an `out` that is only
    4-byte aligned (65 canary words in front of it): the paths without 16-byte stores."""
    from bcos_hip import lib as blib, ops
    H, W = shape
    B, K = 3, 5
    mean, std = consts()
    prev = blib.get_contraction_mode()
    try:
        for mode, desc in (("f16x2", False), ("bf16x3", True)):
            blib.set_contraction_mode(mode)
            x, scores, thr, counts = _case(shape, B, K, seed=5, desc=desc)
            xd, sd, td = x.to(DEV), scores.to(DEV), thr.to(DEV)
            copies = E.materialise(x, scores, thr, desc).to(DEV)
            for first, n, cpad, pad in ((0, B * K, 8, 64), (4, 7, 8, 64), (B * K - 1, 1, 8, 64), (5, 5, 12, 64), (3, 8, 8, 65)):
                got, am = _prep_perturbed_raw(lib, xd, sd, td, desc, mean, std, B, K, first, n, H, W, cpad, pad, absmax=mode == "f16x2")
                want = ops.prep_input(copies[first:first + n].contiguous(), mean, std, cpad=cpad, want_absmax=True)
                assert torch.equal(got, want), (mode, first, n, cpad, pad)
                want_am = ops.absmax_of(want)
                assert (am is None) == (want_am is None)
                if am is not None:
                    assert torch.equal(am.reshape(-1), want_am.reshape(-1).view(torch.int32)), (first, n, cpad)
                    assert torch.equal(am, got.abs().amax(-1).view(torch.int32))
    finally:
        blib.set_contraction_mode(prev)


def test_prepared_input_above_the_grid_cap(lib):
    """the launch is capped at 16384 workgroups of 256 pixels: 64 copies of 300 x 231 are 4 435 200 pixels, so threads take the grid-stride
    loop a second time.  Held against the same copies prepared in two halves, each below the cap -- launches of the kind the tests above
    pin to bcos_prep_input -- with canaries around the large output and exactly k_j removed pixels per copy."""
    from bcos_hip import ops
    H, W = SHAPES[2]
    B, K, HW = 2, 32, H * W
    assert B * K * HW > 16384 * 256 >= (B * K // 2) * HW
    g = torch.Generator().manual_seed(77)
    x = torch.rand(B, 6, H, W, generator=g) * 0.98 + 0.01
    scores = batch_scores("mixed", B, HW, seed=78)
    counts = [(HW * j) // (K - 1) for j in range(K)]                     # 0 ... HW
    thr = E.perturb_select(scores, counts, True)
    xd, sd, td = x.to(DEV), scores.to(DEV), thr.to(DEV)
    mean, std = consts()
    got, am = _prep_perturbed_raw(lib, xd, sd, td, True, mean, std, B, K, 0, B * K, H, W, 8, 64, absmax=True)
    half = B * K // 2
    for first in (0, half):
        part, part_am = _prep_perturbed_raw(lib, xd, sd, td, True, mean, std, B, K, first, half, H, W, 8, 64, absmax=True)
        assert torch.equal(got[first:first + half], part) and torch.equal(am[first:first + half], part_am), first
    assert torch.equal(got[:1], ops.prep_input(xd[:1], mean, std))         # copy 0 removes nothing
    gone = (got[..., :6] == (0 - mean) / std).all(-1).flatten(1).sum(1).tolist()
    assert gone == counts * B


# ---------------------------------------------------------------------------------------------------------------- 3. class scores
def _check_scores(logits, targets, group):
    from bcos_hip import ops
    dev = logits.to(DEV).contiguous()
    tg = torch.as_tensor(targets)
    rows = tg.repeat_interleave(group)
    assert torch.equal(ops.class_scores(dev, tg, group=group, mode="logit").cpu(), logits.gather(1, rows[:, None])[:, 0])
    for mode, bound in (("sigmoid", E.sigmoid_bound), ("softmax", E.softmax_bound)):
        got = ops.class_scores(dev, tg, group=group, mode=mode).cpu().double()
        want, allowed = E.class_scores64(logits, tg, group, mode), bound(logits, tg, group)
        err = (got - want).abs()
        print(f"class scores {mode} [{logits.shape[0]} x {logits.shape[1]}]: worst |fp32 - fp64| / bound {float((err / allowed).max()):.3f}")
        assert bool((err <= allowed).all()), (mode, float((err / allowed).max()))


def test_class_scores(lib, golden_dir):
    from bcos_hip import ops
    data = np.load(os.path.join(golden_dir, "resnet18_e2e.npz"))
    logits = torch.from_numpy(data["logits"])                              # [8, 1000]
    pred = torch.from_numpy(data["prediction"])
    _check_scores(logits, pred, 1)
    _check_scores(logits, [int(pred[0]), 3, 999, 0], 2)
    g = torch.Generator().manual_seed(12)
    wide = torch.randn(6, 1000, generator=g)
    wide[:, 5], wide[:, 700] = 30.0, -30.0                                 # a 60-unit spread; the smallest and the largest class explained
    _check_scores(wide, [5, 700, 1, 700, 5, 999], 1)
    ragged = torch.randn(9, 77, generator=g) * 4                           # CL no multiple of 64, rows no multiple of the 4 per workgroup
    _check_scores(ragged, [0, 76, 64], 3)
    _check_scores(torch.randn(5, 3, generator=g), [2, 0, 1, 1, 2], 1)      # fewer classes than lanes
    # a target outside the logits: NaN for its rows only (an int32 device tensor is taken as it is)
    tg = torch.tensor([3, 77, -1], dtype=torch.int32, device=DEV)
    for mode in ("logit", "sigmoid", "softmax"):
        out = ops.class_scores(ragged.to(DEV), tg, group=3, mode=mode).cpu()
        assert bool(torch.isfinite(out[:3]).all()) and bool(torch.isnan(out[3:]).all())


# ---------------------------------------------------------------------------------------------------------------- 4. engines
def _perturbed_forward_equals_materialised(eng, x, seed):
    from bcos_hip import ops, passes, perturbation as P
    B, _, H, W = x.shape
    HW = H * W
    scores = batch_scores("mixed", B, HW, seed=seed)
    seen = set()
    for K, counts, desc in ((5, [0, HW // 10, HW, 3, HW // 2], False), (24, None, True)):
        n_img = 3 if K == 5 else B
        if counts is None:
            counts = [(HW * j) // 40 for j in range(K)]
        sd = scores[:n_img].to(DEV)
        thr = ops.perturb_select(sd, counts, descending=desc)
        assert torch.equal(thr.cpu(), E.perturb_select(scores[:n_img], counts, desc))
        plan = P.PerturbPlan(sd, thr, desc)
        out = eng.forward(x[:n_img], perturb=plan)
        n = n_img * K
        seen.add(passes.n_streams(n, eng.subbatch_streams, x.device))
        copies = E.materialise(x[:n_img], scores[:n_img], thr, desc).to(DEV)
        assert out.shape[0] == n and bool(torch.isfinite(out).all())
        assert torch.equal(out, eng.forward(copies)), (K, desc)
        if counts[0] == 0:                                                # nothing removed: the image's own row
            assert torch.equal(out[:1], eng.forward(x[:1]))
    assert seen == {1, 2}                                                 # 15 copies on one stream, 72 on two sub-batch streams
    with pytest.raises(ValueError):
        eng.forward(x[:2], perturb=plan)                                  # a plan for another number of images
    with pytest.raises(ValueError):
        eng.forward(x[:, :3], perturb=plan)                               # masking before AddInverse is another operator
    with pytest.raises(ValueError):
        eng.forward(x[:1], perturb=plan, occlude=torch.tensor([[0, 2, 0, 2]], dtype=torch.int32, device=DEV))


def test_perturbed_forward_resnet18(lib, golden_dir):
    from bcos_hip import engine, synth
    eng = engine.attach(golden_net(golden_dir))
    _perturbed_forward_equals_materialised(eng, synth.synthetic_images(3, seed=21, size=32).to(DEV), seed=31)


def test_perturbed_forward_vit(lib):
    from bcos_hip import synth, vit_engine
    vnet = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV).eval()
    _perturbed_forward_equals_materialised(vit_engine.attach(vnet), synth.synthetic_images(3, seed=22).to(DEV), seed=32)


# ---------------------------------------------------------------------------------------------------------------- 5. harness
def test_pixel_perturbation_on_the_engine(lib, golden_dir):
    from bcos_hip import engine, perturbation as P, synth
    net = golden_net(golden_dir)
    eng = engine.attach(net)
    x = synth.synthetic_images(4, seed=23, size=32).to(DEV)
    HW = 32 * 32
    res0 = eng.explain(x, want_weights=False)
    maps, tg = res0["contribution_map"], res0["explained_class_idx"].reshape(-1)
    for order, score in (("least", "logit"), ("most", "softmax")):
        desc = order == "most"
        res = P.pixel_perturbation(net, x, attributions=maps, order=order, score=score, copies_per_call=16)
        counts = [int(np.floor(f * HW + 0.5)) for f in P.DEFAULT_FRACTIONS]
        assert res["counts"] == counts and res["curves"].shape == (4, 11) and res["curves"].is_cuda
        assert torch.equal(res["targets"], tg)
        thr = E.perturb_select(maps.reshape(4, HW).cpu(), counts, desc)
        assert torch.equal(res["thresholds"].cpu(), thr)
        logits = eng.forward(E.materialise(x, maps.reshape(4, HW), thr, desc).to(DEV))
        rows = tg.repeat_interleave(11)
        if score == "logit":
            assert torch.equal(res["curves"].reshape(-1), logits.gather(1, rows[:, None])[:, 0])
            base = eng.forward(x).gather(1, tg[:, None])[:, 0].double()
            r = float((res["curves"][:, 0].double() - base).norm() / base.norm())
            print(f"pixel perturbation: k = 0 column against engine.forward(x): relL2 {r:.2e}")
            assert r <= 1e-4
            whole = P.pixel_perturbation(eng, x, attributions=maps, copies_per_call=256)      # the engine itself; one call for all 44 copies
            assert torch.equal(whole["curves"], res["curves"])
            default = P.pixel_perturbation(net, x)                         # scores from engine.explain, predicted classes
            assert torch.equal(default["curves"], res["curves"]) and torch.equal(default["targets"], tg)
        else:
            want = E.class_scores64(logits.cpu(), tg.cpu(), 11, "softmax")
            assert bool(((res["curves"].reshape(-1).cpu().double() - want).abs() <= E.softmax_bound(logits.cpu(), tg.cpu(), 11)).all())
    # the module path: no engine attached, the copies materialised with torch ops from the same thresholds
    bare = golden_net(golden_dir)
    assert getattr(bare, "_bcos_engine", None) is None
    mod = P.pixel_perturbation(bare, x, tg, attributions=maps, fractions=(0, 0.1, 1.0))
    assert torch.equal(mod["thresholds"].cpu(), E.perturb_select(maps.reshape(4, HW).cpu(), mod["counts"], False))
    assert torch.equal(mod["curves"].reshape(-1), bare(P.materialise(x, maps.reshape(4, HW), mod["thresholds"])).gather(1, tg.repeat_interleave(3)[:, None])[:, 0])
