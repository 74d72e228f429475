"""The reference and the bounds of tests/token_cases.py, without a device:

  * the case tables are the ones the constants were measured on, and the input families have the properties they are there for;
  * the constants are what the module says they are: for every case the plain fp32 PyTorch evaluation of the documented expressions
    stays within K / 4 of each bound form, and the worst use over the tables is the measurement the constants were set from;
  * the Abramowitz-Stegun polynomial of bcos_gelu_gate, in fp64, stays within 1.5e-7 of erf: E_AS is the right additive term;
  * the bounds are sharp enough to matter: ten deliberate mistakes, each applied to the fp32 evaluation, break their bound on a named
    case (most of them on plain `normal` data);
  * the stand-ins of the CPU tier (tests/cpu_emulation.py) compute the reference within the bounds.
"""
import math

import pytest
import torch

import token_cases as tc

MEASURED = {}        # constant's name -> (worst fp32 use of the form, case id, output)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst |fp32 PyTorch - fp64| / bound form over the case tables, in units of u (K = 4 x FP32_WORST):")
        for kind, (v, cid, name) in sorted(MEASURED.items()):
            print(f"  {kind:8s} {v:6.3f}  ({cid}: {name})   FP32_WORST {tc.FP32_WORST[kind]}   K {tc.K[kind]:.1f}")


def _measure(case, inp=None):
    r = tc.fp32_uses(case, inp)
    for kind, (v, name) in r.items():
        if kind not in MEASURED or not v <= MEASURED[kind][0]:
            MEASURED[kind] = (v, case.id, name)
    return r


def test_case_table_is_the_one_the_bounds_were_measured_on():
    ids = [c.id for c in tc.CASES]
    assert len(ids) == len(set(ids))
    assert (len(tc.LN_CASES), len(tc.GN_CASES), len(tc.GELU_CASES), len(tc.ADD_CASES), len(tc.FIN_CASES)) == (52, 22, 4, 4, 8)
    ln = tc.LN_CASES
    assert {c.D for c in ln if c.rows <= 333} == set(tc.VEC_WIDTHS) | set(tc.STRIDED_WIDTHS)
    assert {c.rows for c in ln if c.rows <= 333} == {1, 3, 5, 17, 50, 333}
    for D in tc.VEC_WIDTHS + tc.STRIDED_WIDTHS:
        assert any(c.D == D and c.rows % 4 for c in ln), D
    for D in (4, 68, 192, 256):                              # NV = 1 .. 4 of layernorm_stats16_kernel, a lone row and a lone row behind a full group
        assert {1, 5} <= {c.rows for c in ln if c.D == D and "stats" in c.ops}, D
    assert {(c.D + 63) // 64 for c in ln if c.D in tc.VEC_WIDTHS} == {1, 2, 3, 4}
    big = {(c.rows, c.D, c.ops) for c in ln if c.rows > 333}
    assert big == {(8229, 8, tc.LN_OPS), (8229, 5, tc.LN_OPS), (131093, 4, ("stats",)), (131093, 68, ("stats",))}
    assert {c.family for c in ln} == set(tc.LN_FAMILIES) and {c.affine for c in ln} == set(tc.AFFINES)
    assert {c.eps for c in ln} == {1e-5, 1e-6}
    for fam in tc.LN_FAMILIES:                               # every family on both kernel forms
        assert {c.D in tc.VEC_WIDTHS for c in ln if c.family == fam and c.D > 1} == {True, False}, fam
    assert any(c.family == "constant" and c.D == 1 for c in ln)
    geoms = {(c.N, c.HW, c.C, c.G) for c in tc.GN_CASES if c.family == "normal"}
    assert geoms == {(1, 1, 2, 1), (2, 1, 4, 4), (2, 49, 12, 4), (3, 196, 48, 8), (2, 196, 64, 1), (2, 37, 32, 32), (1, 3136, 24, 4),
                     (2, 85, 3, 1), (2, 64, 4, 1), (2, 257, 1, 1)}
    assert {c.family for c in tc.GN_CASES} == set(tc.GN_FAMILIES) and {c.affine for c in tc.GN_CASES} == {"wb", "none"}
    assert {(c.op, c.n) for c in tc.GELU_CASES} == {("gate", 77), ("gate", 2048 * 256 + 77), ("bwd", 77), ("bwd", 8192 * 256 + 77)}
    assert {(c.B, c.T, c.D) for c in tc.ADD_CASES} == {(1, 1, 4), (3, 5, 8), (2, 197, 192), (512, 1, 4104)}
    assert 512 * 4104 // 4 > 2048 * 256
    fin = {(c.N, c.H, c.W, c.ps, c.Cpad, c.add_inverse, c.gp_offset) for c in tc.FIN_CASES}
    assert fin == {(1, 4, 4, 1, 8, 1, 0), (2, 8, 12, 2, 8, 0, 0), (2, 12, 8, 4, 8, 1, 0), (1, 32, 48, 16, 8, 1, 0), (2, 8, 12, 2, 6, 1, 0),
                   (2, 8, 12, 2, 12, 0, 0), (2, 8, 12, 2, 8, 1, 1), (65, 256, 256, 16, 8, 1, 0)}
    assert 65 * 256 * 256 > 16384 * 256 and len(set(tc.STD6)) == 6
    assert tc.K == {k: 4 * v for k, v in tc.FP32_WORST.items()} and tc.E_AS == 0.75e-7


def test_families_have_the_properties_they_are_in_the_table_for():
    for case in tc.LN_CASES:
        if case.rows > 333:
            continue
        inp = tc.make_inputs(case)
        x = inp["x"].double()
        again = tc.make_inputs(case)
        assert all(torch.equal(inp[k], again[k]) for k in inp if inp[k] is not None), case.id
        if inp["w"] is not None:
            assert bool((inp["w"] < 0).any()) and (case.D == 1 or int((inp["w"] == 0).sum()) == 1), case.id
        assert (inp["w"] is None) == (case.affine == "none") and (inp["b"] is None) == (case.affine != "wb")
        if case.family == "offset":
            ratio = x.mean(1).abs() / x.std(1, unbiased=False)
            assert float(ratio.min()) >= 100 and bool((x.mean(1) > 0).any()) and bool((x.mean(1) < 0).any()), (case.id, float(ratio.min()))
        if case.family == "rowrange":
            mag = x.abs().amax(1)
            assert float(mag.max() / mag.min()) > (1e3 if case.rows >= 17 else 10), case.id
        if case.family == "constant":
            rows = tc.constant_rows(case)
            assert rows and (case.D > 1 or len(rows) == case.rows)
            var = ((x - x.mean(1, keepdim=True)) ** 2).mean(1)
            assert bool((var[rows] == 0).all()), case.id                    # exactly zero: sd = sqrt(eps)
            assert -1000.0 in {float(x[r, 0]) for r in rows} <= {0.0, 1.0, -1000.0}, case.id
    for case in tc.GN_CASES:
        if case.family == "grouprange":
            x = tc.make_inputs(case)["x"].reshape(case.N, case.HW, case.G, -1)
            mag = x.abs().amax(dim=(1, 3)).reshape(-1)
            assert float(mag.max() / mag.min()) >= 1e4, (case.id, float(mag.max() / mag.min()))
    x = tc.make_inputs(tc.by_id("gelu-gate-n524365"))["x"].double()
    Phi = 0.5 * torch.erfc(-x / math.sqrt(2))
    assert int((Phi < tc.E_AS).sum()) > 1000                            # the negative tail: the gate is below the approximation's error
    assert int(((x - tc.GELU_DERIV_ZERO).abs() < 1e-3).sum()) >= 100 and abs(tc.GELU_DERIV_ZERO + 0.7518) < 1e-4
    assert bool(torch.isfinite(x).all()) and float(x.min()) == -14 and float(x.max()) == 14
    assert float(torch.exp(-(x.float().abs() * 0.70710678118654752) ** 2).min()) < 2.0 ** -126    # exp(-z^2) leaves fp32's normal range
    short = tc.make_inputs(tc.by_id("gelu-gate-n77"))["x"]
    assert torch.equal(short, x[:77].float()) and bool((short == 0).sum() == 3) and bool(torch.signbit(short[1]))
    fin = tc.make_inputs(tc.by_id("fin-n2h8w12p2c8-inv0"))
    assert bool(torch.isnan(fin["gp"][..., 6:]).all()) and bool(torch.isfinite(fin["gp"][..., :6]).all())
    mag = fin["gp"][..., :6].abs().amax(-1)
    assert float(mag.max() / mag.min()) > 1e4


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_fp32_reference_stays_within_a_quarter_of_every_bound(case):
    inp = tc.make_inputs(case)
    r = _measure(case, inp)
    print(case.id, {k: f"{v:.3f} ({n})" for k, (v, n) in r.items()})
    bad = {kind: v for kind, (v, _) in r.items() if not v <= tc.K[kind] / 4}
    assert not bad, (case.id, "fp32 error / form beyond K / 4", bad)
    if case.kind == "gelu":              # ... and against erf itself, with E_AS: a quarter of K on top of the additive term
        ref = tc.reference(case, inp)
        r32 = tc.evaluate(case, inp, torch.float32)
        for name, (key, form, add) in tc.forms(case, inp, ref).items():
            v, i = tc.use(r32[name], ref[name], form, add)
            assert v <= tc.K[key] / 4, (case.id, name, v, i)
    if case.kind == "add":
        assert torch.equal(tc.evaluate(case, inp, torch.float32)["x"], inp["x"] + inp["pe"])


def test_constants_are_four_times_the_measured_worst():
    """(runs behind the parametrised measurement above: the constants are not looser than the tables make them either)"""
    if len(MEASURED) < len(tc.FP32_WORST):
        for case in tc.CASES:
            _measure(case)
    assert set(MEASURED) == set(tc.FP32_WORST)
    for kind, want in tc.FP32_WORST.items():
        got = MEASURED[kind][0]
        assert want - 0.3 < got <= want, (kind, got, want, MEASURED[kind][1:])


def test_the_polynomial_is_within_its_stated_error_of_erf():
    """Abramowitz-Stegun 7.1.26 in fp64 over the whole GELU vector: |erf error| <= 1.5e-7, i.e. E_AS on the gate"""
    x = tc.make_inputs(tc.by_id("gelu-bwd-n2097229"))["x"]
    gate = tc.gate_poly(x, torch.float64)
    erf_err = (2 * gate - 1 - torch.erf(x.double() / math.sqrt(2))).abs()
    gate_err = (gate - 0.5 * torch.erfc(-x.double() / math.sqrt(2))).abs()
    print("polynomial vs erf", float(erf_err.max()), "gate vs Phi", float(gate_err.max()))
    assert float(erf_err.max()) <= 1.5e-7 and float(gate_err.max()) <= tc.E_AS
    assert float(gate_err.max()) > 0.5 * tc.E_AS           # and E_AS is not generous: the formula uses most of it


MUTATIONS = [            # (deliberate mistake, the case it must show on, the output judged)
    ("onepass", "ln-offset-r50d192-w-e5", "rstd"),           # E[x^2] - mean^2
    ("padded", "ln-normal-r50d68-w-e6", "y"),                # the variance divided by the padded width
    ("droplast", "ln-normal-r333d65-w-e5", "y"),             # the 65th column never read
    ("maskedlane", "ln-normal-r5d68-wb-e5", "rstd"),         # lanes past the row contribute (0 - mean)^2
    ("det_nomean", "ln-normal-r50d192-none-e6", "out/--"),   # gx = h
    ("full_nomhx", "ln-normal-r17d64-w-e5", "gx/-"),         # gx = rstd (h - mean h)
    ("gn_goffset", "gn-grouprange-n2hw49c12g4-none", "y"),   # group g starts at channel g, not g cg
    ("gn_whole", "gn-normal-n3hw196c48g8-none", "y"),        # one mean and variance per image
    ("tanh", "gelu-gate-n77", "gate"),                       # the tanh form of GELU
    ("gw_from_h", "fin-n2h8w12p2c8-inv0", "weights"),        # patch row pitch H / ps on a rectangular image
]


@pytest.mark.parametrize("mut,cid,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_bound_notices_the_mistake(mut, cid, name):
    case = tc.by_id(cid)
    inp = tc.make_inputs(case)
    ref = tc.reference(case, inp)
    key, form, add = tc.forms(case, inp, ref)[name]
    good, _ = tc.use(tc.evaluate(case, inp, torch.float32)[name], ref[name], form, add)
    wrong, i = tc.use(tc.evaluate(case, inp, torch.float32, mut=mut)[name], ref[name], form, add)
    print(f"{mut} on {cid}: {name} error / form {wrong:.3g} at element {i} (unmutated {good:.3g}), K {tc.K[key]}")
    assert good <= tc.K[key] / 4 and wrong > tc.K[key], (mut, cid, good, wrong)


def test_mutations_do_not_need_the_extreme_families():
    fams = [tc.by_id(cid).family for _, cid, _ in MUTATIONS if tc.by_id(cid).kind in ("ln", "gn")]
    assert fams.count("normal") >= 5


def _held(case, inp, ref, outs):
    """every element of the outputs given within its bound"""
    f = tc.forms(case, inp, ref)
    for name, t in outs.items():
        key, form, add = f[name]
        v, i = tc.use(t, ref[name], form, add)
        assert v <= tc.K[key], (case.id, name, key, v, i)


@pytest.mark.parametrize("cid", ["ln-normal-r50d192-none-e6", "ln-offset-r17d65-none-e5", "ln-constant-r17d68-wb-e6", "ln-outlier-r5d1000-w-e5"])
def test_cpu_emulation_computes_the_layernorm_reference(cid):
    import cpu_emulation as E
    case = tc.by_id(cid)
    inp = tc.make_inputs(case)
    ref = tc.reference(case, inp)
    x, w, b, gy, rstd, addend, mul2 = (inp[k] for k in ("x", "w", "b", "gy", "rstd", "addend", "mul2"))
    y, rs = E.layernorm_fwd(x, w, b, tc.eps32(case), want_rstd=True)
    rs2, zss = E.layernorm_stats(x, w, b, tc.eps32(case), want_zsumsq=True)
    out, out2 = E.layernorm_bwd_detached(gy, w, rstd, addend=addend, mul2=mul2, want_out=True, want_out2=True)
    gx, xhat = E.layernorm_bwd(gy, x, w, rstd, want_xhat=True, addend=addend)
    gx0, _ = E.layernorm_bwd(gy, x, w, rstd)
    _held(case, inp, ref, {"y": y, "rstd": rs, "zss": zss, "out/am": out, "out2/am": out2, "gx/a": gx, "gx/-": gx0, "xhat": xhat})
    assert torch.equal(rs, rs2)


@pytest.mark.parametrize("cid", ["gn-normal-n2hw49c12g4-wb", "gn-grouprange-n2hw37c32g32-none", "gn-offset-n2hw85c3g1-wb"])
def test_cpu_emulation_computes_the_groupnorm_reference(cid):
    import cpu_emulation as E
    case = tc.by_id(cid)
    inp = tc.make_inputs(case)
    ref = tc.reference(case, inp)
    nhwc = lambda t: t.reshape(case.N, case.HW, 1, case.C)          # noqa: E731
    y, rs = E.groupnorm_fwd(nhwc(inp["x"]), case.G, inp["w"], inp["b"], tc.eps32(case), want_rstd=True)
    gd = E.groupnorm_bwd_detached(nhwc(inp["gy"]), case.G, inp["w"], inp["rstd"])
    gx, xhat = E.groupnorm_bwd(nhwc(inp["gy"]), nhwc(inp["x"]), case.G, inp["w"], inp["rstd"], want_xhat=True)
    flat = lambda t: t.reshape(case.N, case.HW, case.C)             # noqa: E731
    _held(case, inp, ref, {"y": flat(y), "rstd": rs, "gx_det": flat(gd), "gx": flat(gx), "xhat": flat(xhat)})


def test_cpu_emulation_computes_the_elementwise_references():
    import cpu_emulation as E
    for cid in ("gelu-gate-n77", "gelu-gate-n524365"):
        case = tc.by_id(cid)
        inp = tc.make_inputs(case)
        y, gate = E.gelu_gate(inp["x"], want_gate=True)
        _held(case, inp, tc.reference(case, inp), {"y": y, "gate": gate})
    for cid in ("gelu-bwd-n77", "gelu-bwd-n2097229"):
        case = tc.by_id(cid)
        inp = tc.make_inputs(case)
        _held(case, inp, tc.reference(case, inp), {"gx": E.gelu_bwd(inp["gy"], inp["x"])})
    for cid in ("add-b3t5d8", "add-b2t197d192"):
        case = tc.by_id(cid)
        inp = tc.make_inputs(case)
        assert torch.equal(E.add_rows_bcast(inp["x"].clone(), inp["pe"]), tc.reference(case, inp)["x"])
    for cid in ("fin-n2h12w8p4c8-inv1", "fin-n2h8w12p2c12-inv0"):
        case = tc.by_id(cid)
        inp = tc.make_inputs(case)
        gp = inp["gp"].reshape(-1, case.ps * case.ps * case.Cpad)
        wo, co = E.finalize_explanation_patches(gp, inp["x"], inp["std6"], case.ps, add_inverse=bool(case.add_inverse))
        _held(case, inp, tc.reference(case, inp), {"weights": wo, "contrib": co})
