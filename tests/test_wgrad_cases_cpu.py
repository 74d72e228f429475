"""The case table, the reference and the bounds of tests/wgrad_cases.py and tests/patch_norm_bwd_cases.py, without a device:

  * bcos_conv2d_wgrad_plan_query (host only) answers every case with the plan the table states, the table covers every route, and the
    query refuses what the launch refuses;
  * the constants are what the module says: K_fam = max(4 x the worst use of the form by PyTorch's fp32 weight gradient, 16), and the
    measurement is the one the constants were set from;
  * the three ways to the fp64 reference agree (gathered columns, F.unfold, autograd of conv2d);
  * the bound is sharp enough to matter: the documented arithmetic (exact bf16 planes, six products), evaluated in fp64, stays within
    8 u of every element, while a seventh dropped product, a dropped last pixel, swapped paddings, a tap decoded with kh, and a skipped
    hot pixel each exceed K_fam;
  * cpu_emulation.conv2d_wgrad, the stand-in of the CPU tier, computes the reference;
  * patch-norm backward: the derived bound holds for an fp32 evaluation and rejects swapped paddings and mixed-up strides.
"""
import ctypes as C

import pytest
import torch

import patch_norm_bwd_cases as pc
import wgrad_cases as wc

MEASURED = {}        # family -> (worst fp32 use of the form, case id)
_DONE = set()        # the (case id, family) pairs that went into MEASURED
_INPUTS = {}


def inputs(case, family):
    """(x, glin, reference) of a case and family; computed once, never written to"""
    key = (case.geom, family)
    if key not in _INPUTS:
        x, gl = wc.make_inputs(case, family)
        _INPUTS[key] = (x, gl, wc.reference(x, gl, case))
    return _INPUTS[key]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _INPUTS.clear()
    if MEASURED:
        print("\nworst |fp32 PyTorch weight gradient - fp64| / form over the case table, in units of u (K = max(4 x FP32_WORST, 16)):")
        for fam, (v, cid) in MEASURED.items():
            print(f"  {fam:9s} {v:7.3f}  ({cid})   FP32_WORST {wc.FP32_WORST[fam]}   K {wc.K[fam]}")


BOTH = [(c, f) for c in wc.CASES for f in wc.FAMILIES]
IDS = [f"{c.id}-{f}" for c, f in BOTH]


# ---- the plan query ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.id)
def test_query_answers_the_plan_the_table_states(hip_lib, case):
    from bcos_hip import lib
    assert lib.get_option("wgrad_wgs") == 768
    if case.wgs:
        lib.set_option("wgrad_wgs", case.wgs)
    got = lib.wgrad_plan_query(*case.ints())
    assert got == case.plan, (case.id, got)
    ws = C.c_int64(-1)
    lib.check(hip_lib.bcos_conv2d_wgrad_ws_floats(*case.ints(), C.byref(ws)), "bcos_conv2d_wgrad_ws_floats")
    assert ws.value == got["ws_floats"] == (got["split"] * case.Cout * case.taps * case.C if got["split"] > 1 else 0)
    assert got["chunk"] % 16 == 0 and (got["split"] - 1) * got["chunk"] + got["last"] == case.M and 1 <= got["last"] <= got["chunk"]
    assert got["grid_y"] == (1 if got["fused_taps"] else case.taps)
    assert (got["combine"] == 0) == (got["split"] == 1)


def test_table_covers_every_route():
    """(the module asserts the same when it is imported; spelled out here with what each property reaches in csrc/bcos_train.hip)"""
    kinds = {(wc.kind(c), c.plan["direct"]) for c in wc.CASES}
    assert kinds == {("fused", 0), ("pertap", 0), ("1x1", 1), ("1x1", 0)}
    assert {c.plan["combine"] for c in wc.CASES} == {0, 1, 2}
    thin = [c for c in wc.CASES if c.plan["combine"] == 1]
    wide = [c for c in wc.CASES if c.plan["combine"] == 2]
    assert any(c.plan["split"] > 4 and (c.plan["split"] - 1) % 4 for c in thin)       # the by-4 loop of the thin combine and its remainder
    assert any(c.plan["split"] > 64 and c.plan["split"] % 16 for c in wide)           # the by-64 loop of the wide combine and its remainder
    assert any(c.plan["last"] < c.plan["chunk"] and c.plan["split"] > 1 for c in wc.CASES)
    assert any(wc.dead_wave(c) for c in wc.CASES)
    assert any(c.C % 4 == 0 for c in wc.CASES) and any(c.C % 4 and c.C >= 128 for c in wc.CASES)        # 16-byte and scalar stores
    assert any(c.Cout % 4 for c in wc.CASES)                                          # the scalar tail of the gradient loads
    assert any(c.P * c.Q < 16 and c.N > 16 for c in wc.CASES)                         # a stage advance that wraps rows and images
    assert wc.empty_taps(wc.by_id("pad_only_taps")) == [0, 1, 2, 3, 5, 6, 7, 8]
    a, b = wc.by_id("wide_combine"), wc.by_id("wide_combine_wgs64")
    assert a.geom == b.geom and (a.plan["split"], a.plan["chunk"]) != (b.plan["split"], b.plan["chunk"])
    assert wc.K == {f: max(4 * wc.FP32_WORST[f], 16.0) for f in wc.FAMILIES}
    # the matrix pipe's term: one family, and small next to every mutant on the short chains
    assert wc.PIPE_TERM_FAMILIES == ("full",) and wc.chain(16, 1) == 6 and wc.chain(256, 67) == 162
    assert all(wc.bound_k("full", wc.by_id(i).steps) <= 28 and wc.bound_k("normal", wc.by_id(i).steps) == wc.K["normal"] for i in wc.SHORT_CHAIN)


def test_query_refusals(hip_lib):
    from bcos_hip import lib
    case = wc.by_id("fused3x3_c36")
    plan = lib.WgradPlan()
    assert hip_lib.bcos_conv2d_wgrad_plan_query(*case.ints(), None) == lib.BCOS_E_INVAL
    assert b"NULL" in hip_lib.bcos_last_error_string()

    def code(**change):
        names = ("N", "H", "W", "C", "x_pitch", "P", "Q", "Cout", "g_pitch", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "gw_cin")
        v = dict(zip(names, case.ints()))
        v.update(change)
        plan.split = -7
        rc = hip_lib.bcos_conv2d_wgrad_plan_query(*[v[n] for n in names], C.byref(plan))
        assert rc == 0 or (plan.split == -7 and hip_lib.bcos_last_error_string())        # a refusal writes nothing and says why
        return rc

    assert code() == 0 and code(gw_cin=case.C) == 0
    for change in (dict(N=0), dict(Cout=0), dict(kh=0), dict(sw=0), dict(dh=0), dict(x_pitch=case.C - 4), dict(x_pitch=case.C + 2),
                   dict(g_pitch=case.Cout + 1), dict(g_pitch=case.Cout - 4)):
        assert code(**change) == lib.BCOS_E_INVAL, change
    assert code(gw_cin=case.C - 4) == lib.BCOS_E_INVAL
    assert code(gw_cin=case.C + 4) == lib.BCOS_E_NOSUP                 # the ordered launch wants a dense gw ...
    assert code(C=3, x_pitch=4, Cout=3, g_pitch=4, kh=1, kw=1) == lib.BCOS_E_NOSUP       # ... of a multiple of 4 floats (here 9)


# ---- the constants ----------------------------------------------------------------------------------------------------------------------
def _measure(case, family):
    v = wc.fp32_ratio(case, family)
    _DONE.add((case.id, family))
    if family not in MEASURED or v > MEASURED[family][0]:
        MEASURED[family] = (v, case.id)
    return v


@pytest.mark.parametrize("case,family", BOTH, ids=IDS)
def test_fp32_weight_gradient_stays_within_a_quarter_of_the_bound(case, family):
    v = _measure(case, family)
    print(case.id, family, f"{v:.3f} u")
    assert v <= wc.FP32_WORST[family] <= wc.K[family] / 4, (case.id, family, v)


def test_constants_are_four_times_the_measured_worst():
    """(runs behind the parametrised measurement above: the constants are not looser than the table makes them either)"""
    for case, family in BOTH:
        if (case.id, family) not in _DONE:
            _measure(case, family)
    for family, want in wc.FP32_WORST.items():
        got = MEASURED[family][0]
        assert want - wc.fp32_tolerance(want) < got <= want, (family, got, want, MEASURED[family][1])


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.id)
def test_three_ways_to_the_reference_agree(case):
    x, gl, ref = inputs(case, "normal")
    xd = x.double()
    assert torch.equal(wc.xcol(xd, case), wc.xcol_unfold(xd, case))
    # fp64 against fp64 in another summation order: a few 2^-53 of the form, i.e. far below 1e-6 u
    assert wc.ratio(wc.conv_weight_grad(x, gl, case, torch.float64), ref) <= 1e-6
    empty = ref[1] == 0
    assert bool((ref[0][empty] == 0).all())
    taps = wc.empty_taps(case)
    assert bool(empty[:, taps].all()) and int(empty.sum()) == len(taps) * case.Cout * case.C


def test_input_families_are_what_they_are_in_the_table_for():
    for case in wc.CASES:
        for fam in wc.FAMILIES:
            x, gl = wc.make_inputs(case, fam)
            x2, gl2 = wc.make_inputs(case, fam)
            assert torch.equal(x[..., :case.C], x2[..., :case.C]) and torch.equal(gl[..., :case.Cout], gl2[..., :case.Cout])
            assert bool(torch.isnan(x[..., case.C:]).all()) and bool(torch.isnan(gl[..., case.Cout:]).all())
            assert bool(torch.isfinite(x[..., :case.C]).all()) and bool(torch.isfinite(gl[..., :case.Cout]).all())
            if fam == "full":
                for t in (x[..., :case.C], gl[..., :case.Cout]):
                    h, m, l = wc.planes(t.contiguous())
                    assert bool((h > 0).all() and (m > 0).all() and (l > 0).all())
    case = wc.by_id("stem7x7_c6")
    x, gl = wc.make_inputs(case, "imgrange")
    scale = [float(x[n, ..., :case.C].abs().max()) * float(gl[n, ..., :case.Cout].abs().max()) for n in range(case.N)]
    assert max(scale) / min(scale) > 2.0 ** 20 and len({round(torch.tensor(s).log2().item() / 3) for s in scale}) == case.N
    xh, gh = wc.make_inputs(case, "hot")
    hx, hg = wc.hot_pixels(case)
    assert hx[0] == 0 and hg[0] == case.N - 1
    assert float(xh[hx][:case.C].abs().min()) > 0 and float(xh[hx][:case.C].abs().max()) > 1000


@pytest.mark.parametrize("cid,family", [("pertap_rect_c132", "normal"), ("stem7x7_c6", "imgrange"), ("pad_only_taps", "hot")])
def test_cpu_emulation_computes_the_reference(cid, family):
    import cpu_emulation as E
    case = wc.by_id(cid)
    x, gl, ref = inputs(case, family)
    gw = E.conv2d_wgrad(gl, x, case.C, case.Cout, (case.kh, case.kw), (case.sh, case.sw), (case.ph, case.pw), (case.dh, case.dw))
    assert gw.dtype == torch.float32 and tuple(gw.shape) == (case.Cout, case.kh, case.kw, case.C)
    # fp64 rounded once to fp32: half an ulp of the element, i.e. <= 2^-24 |element| = u |element|, and |element| <= form -- reached
    # where the sum has one term or one sign; under 1 / 16 of the smallest bound, K = 16
    assert wc.ratio(gw, ref) <= 1.0


# ---- the bound is sharp enough to matter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,family", BOTH, ids=IDS)
def test_documented_arithmetic_stays_within_8u(case, family):
    x, gl, ref = inputs(case, family)
    v = wc.ratio(wc.six_products(x, gl, case), ref)
    print(case.id, family, f"six products in fp64: {v:.3f} u")
    assert v <= 8.0 and v <= wc.K[family] / 2


# a seventh dropped product is 2^-16 of |a b| where the planes are full ("full": 256 u on every element, whatever the shape); in
# "normal" the planes are full on average only, and the excess over K shows where few pixels are summed: the short-chain cases
MUTANT_A = [(c, "full") for c in wc.CASES] + [(wc.by_id(i), "normal") for i in wc.SHORT_CHAIN]


@pytest.mark.parametrize("case,family", MUTANT_A, ids=[f"{c.id}-{f}" for c, f in MUTANT_A])
@pytest.mark.parametrize("drop", [("l", "h"), ("h", "l"), ("m", "m")], ids=lambda d: f"a_{d[0]}b_{d[1]}")
def test_bound_notices_a_seventh_dropped_product(case, family, drop):
    x, gl, ref = inputs(case, family)
    v = wc.ratio(wc.six_products(x, gl, case, also_drop=(drop,)), ref)
    k = wc.bound_k(family, case.steps)                      # (with the matrix pipe's term of `full`: 16 + 164 at most)
    print(case.id, family, drop, f"{v:.1f} u   K {k}")
    assert v > k
    if family == "full":
        assert 250 <= v <= 260


# (imgrange is left out: its last image may lie 2^24 below the largest one BY DESIGN -- tinyQ_multiwrap's does -- and then no L1 form
# can see that image at all)
MUTANT_B = [(c, f) for c, f in BOTH if f != "imgrange"]


@pytest.mark.parametrize("case,family", MUTANT_B, ids=[f"{c.id}-{f}" for c, f in MUTANT_B])
def test_bound_notices_a_dropped_last_pixel(case, family):
    x, gl, ref = inputs(case, family)
    g2 = gl[..., :case.Cout].double().reshape(case.M, case.Cout).clone()
    g2[-1] = 0                                           # the last pixel of the last chunk never reaches the matrix pipe
    v = wc.ratio(wc.contract(g2, wc.xcol(x.double(), case)), ref)
    k = wc.bound_k(family, case.steps)
    print(case.id, family, f"{v:.1f} u   K {k}")
    assert v > k


@pytest.mark.parametrize("family", wc.FAMILIES)
def test_bound_notices_swapped_paddings_and_a_tap_decoded_with_kh(family):
    case = wc.by_id("pertap_rect_c132")
    assert case.ph != case.pw and case.kh != case.kw
    x, gl, ref = inputs(case, family)
    g2 = gl[..., :case.Cout].double().reshape(case.M, case.Cout)
    assert wc.ratio(wc.contract(g2, wc.xcol(x.double(), case)), ref) == 0.0
    swapped = wc.ratio(wc.contract(g2, wc.xcol(x.double(), case, ph=case.pw, pw=case.ph)), ref)
    decoded = wc.ratio(wc.contract(g2, wc.xcol(x.double(), case, decode_kw=case.kh)), ref)
    k = wc.bound_k(family, case.steps)
    print(family, f"ph/pw swapped {swapped:.3g} u, th = tap / kh {decoded:.3g} u   K {k}")
    assert swapped > k and decoded > k


@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.id)
def test_bound_notices_a_skipped_hot_pixel(case):
    x, gl, ref = inputs(case, "hot")
    hx, _ = wc.hot_pixels(case)
    x2 = x.clone()
    x2[hx] = 0
    g2 = gl[..., :case.Cout].double().reshape(case.M, case.Cout)
    v = wc.ratio(wc.contract(g2, wc.xcol(x2.double(), case)), ref)
    print(case.id, f"{v:.3g} u   K {wc.K['hot']}")
    assert v > wc.K["hot"]


# ---- patch-norm backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_patch_norm_bound_holds_in_fp32_and_rejects_index_mutants(case):
    x, r, addend = pc.make_inputs(case)
    for ad in (addend, None):
        ref = pc.reference(x, r, ad, case)
        exact, bound, covered = ref
        T64 = pc.patch_sum_gather(r.double(), case)
        assert torch.allclose(T64, pc.patch_sum_scatter(r.double(), case)[0], rtol=1e-13, atol=0)
        T32 = pc.patch_sum_gather(r, case)                  # fp32, tap order: the kernels' own arithmetic up to the order of the additions
        out32 = x[..., :case.C] * T32[..., None]
        if ad is not None:
            out32 = out32 + ad
        v = pc.worst(out32, ref)
        assert v <= 1.0, (case.id, v)
        want = ad if ad is not None else torch.zeros_like(out32)
        assert torch.equal(out32[:, ~covered], want[:, ~covered])
        if "gaps" in case.variant:
            assert int((~covered).sum()) > covered.numel() // 2
            continue                                        # (a 1 x 1 unpadded kernel has no paddings to swap)
        xs = x[..., :case.C].double()
        for name, kw in (("ph/pw swapped", dict(swap_pad=True)), ("strides mixed up", dict(mix_strides=True))):
            wrong = xs * pc.patch_sum_gather(r.double(), case, **kw)[..., None] + (ad.double() if ad is not None else 0)
            assert pc.worst(wrong, ref) > 1.0, (case.id, name)
