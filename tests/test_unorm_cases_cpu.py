"""The reference and the bounds of tests/unorm_cases.py, without a device:

  * the case table is the one the constants were measured on, and it reaches every uncentered code path of csrc/bcos_norms.hip;
  * the constants are what the module says they are: for every case the plain fp32 PyTorch evaluation of the documented expressions
    stays within K / 4 of each bound form, and the worst use over the table is the measurement the constants were set from;
  * the bounds are sharp enough to matter: three deliberate mistakes, each applied to the fp32 evaluation, break their bound on a named
    case of plain `normal` data -- the mean subtracted from the value that is divided (the CENTRED norm), the mean term dropped from
    the full gradient, and n wrong by one.
"""
import pytest
import torch

import unorm_cases as uc

MEASURED = {}        # constant's name -> (worst fp32 use of the form, case id, output)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst |fp32 PyTorch - fp64| / bound form over the case table, in units of u (K = 4 x FP32_WORST):")
        for kind, (v, cid, name) in sorted(MEASURED.items()):
            print(f"  {kind:8s} {v:6.3f}  ({cid}: {name})   FP32_WORST {uc.FP32_WORST[kind]}   K {uc.K[kind]:.1f}")


def _measure(case):
    r = uc.fp32_uses(case)
    for kind, (v, name) in r.items():
        if kind not in MEASURED or not v <= MEASURED[kind][0]:
            MEASURED[kind] = (v, case.id, name)
    return r


def test_case_table_reaches_every_code_path():
    ids = [c.id for c in uc.CASES]
    assert len(ids) == len(set(ids))
    assert (len(uc.ROW_CASES), len(uc.GRP_CASES)) == (36, 20)
    rows = uc.ROW_CASES
    small = [c for c in rows if c.rows <= 333 and not c.misaligned]
    assert {c.D for c in small} == set(uc.VEC_WIDTHS) | set(uc.STRIDED_WIDTHS)
    assert all(D % 4 == 0 and D <= 256 for D in uc.VEC_WIDTHS) and all(D % 4 or D > 256 for D in uc.STRIDED_WIDTHS)
    for D in uc.VEC_WIDTHS + uc.STRIDED_WIDTHS:                # a wavefront group of four left partly empty, at every width
        assert any(c.D == D and c.rows % 4 for c in rows), D
    # a width divisible by 4 on the strided kernels; the second pass of the grid-stride loop on both kernel forms
    assert {(c.D, c.family) for c in rows if c.misaligned} == {(68, "normal"), (256, "offset")}
    assert {(c.rows, c.D) for c in rows if c.rows > 333} == {(uc.FIRST_PASS_ROWS + 37, 8), (uc.FIRST_PASS_ROWS + 37, 5)}
    assert {c.family for c in rows} == set(uc.ROW_FAMILIES) and {c.affine for c in rows} == set(uc.AFFINES)
    assert {c.eps for c in rows} == {1e-5, 1e-6}
    for fam in uc.ROW_FAMILIES:                                # every family on both kernel forms
        assert {c.D in uc.VEC_WIDTHS for c in rows if c.family == fam and c.D > 1 and not c.misaligned} == {True, False}, fam
    assert any(c.family == "constant" and c.D == 1 for c in rows)
    grp = uc.GRP_CASES
    sizes = {c.HW * c.C // c.G for c in grp}
    assert min(sizes) == 1 and max(sizes) == 18816 and {255, 256, 257} & sizes
    assert any(c.G == 1 for c in grp) and any(c.G == c.C > 1 for c in grp) and any(1 < c.G < c.C for c in grp)
    assert {c.family for c in grp} == set(uc.GRP_FAMILIES) and {c.affine for c in grp} == set(uc.AFFINES)
    assert uc.K == {k: 4 * v for k, v in uc.FP32_WORST.items()}


def test_inputs_are_reproducible_and_families_have_their_properties():
    for case in uc.ROW_CASES:
        if case.rows > 333:
            continue
        inp, again = uc.make_inputs(case), uc.make_inputs(case)
        assert all(torch.equal(inp[k], again[k]) for k in inp if inp[k] is not None), case.id
        assert (inp["w"] is None) == (case.affine == "none") and (inp["b"] is None) == (case.affine != "wb")
        x = inp["x"].double()
        if case.family == "offset":
            assert float((x.mean(1).abs() / x.std(1, unbiased=False)).min()) >= 100, case.id
        if case.family == "constant":
            var = ((x - x.mean(1, keepdim=True)) ** 2).mean(1)
            assert bool((var == 0).any()), case.id


@pytest.mark.parametrize("case", uc.CASES, ids=lambda c: c.id)
def test_fp32_reference_stays_within_a_quarter_of_every_bound(case):
    r = _measure(case)
    print(case.id, {k: f"{v:.3f} ({n})" for k, (v, n) in r.items()})
    bad = {kind: v for kind, (v, _) in r.items() if not v <= uc.K[kind] / 4}
    assert not bad, (case.id, "fp32 error / form beyond K / 4", bad)


def test_constants_are_four_times_the_measured_worst():
    """(runs behind the parametrised measurement above: the constants are not looser than the table makes them either)"""
    if len(MEASURED) < len(uc.FP32_WORST):
        for case in uc.CASES:
            _measure(case)
    assert set(MEASURED) == set(uc.FP32_WORST)
    for kind, want in uc.FP32_WORST.items():
        got = MEASURED[kind][0]
        assert want - 0.3 < got <= want, (kind, got, want, MEASURED[kind][1:])


MUTATIONS = [            # (deliberate mistake, the case it must show on, the output judged)
    ("centred", "row-normal-r50d96-none-e6", "y"),               # y = w (x - mean) / sd: the centred norm
    ("centred", "grp-normal-n2hw49c12g4-none", "y"),
    ("full_nomean", "row-normal-r17d64-none-e5", "gx/-"),        # gx = r h - r^3 x (sum h x) / n
    ("full_nomean", "grp-normal-n3hw196c48g8-wb", "gx"),
    ("n_off", "row-normal-r333d256-none-e5", "y"),               # n + 1 in the mean and the variance ...
    ("n_off", "row-normal-r3d1000-none-e5", "gx/-"),             # ... and under sum h x, at the widest row
    ("n_off", "grp-normal-n1hw3136c24g4-wb", "rstd"),            # 18 816 values: 1 / n is still 3 x 10^-5, far above u
]
assert {m[0] for m in MUTATIONS} == set(uc.MUTATIONS)


@pytest.mark.parametrize("mut,cid,name", MUTATIONS, ids=[f"{m[0]}-{m[1]}" for m in MUTATIONS])
def test_bound_notices_the_mistake(mut, cid, name):
    case = uc.by_id(cid)
    inp = uc.make_inputs(case)
    ref = uc.reference(case, inp)
    key, form = uc.forms(case, inp, ref)[name]
    good, _ = uc.use(uc.evaluate(case, inp, torch.float32)[name], ref[name], form)
    wrong, i = uc.use(uc.evaluate(case, inp, torch.float32, mut=mut)[name], ref[name], form)
    print(f"{mut} on {cid}: {name} error / form {wrong:.3g} at element {i} (unmutated {good:.3g}), K {uc.K[key]}")
    assert good <= uc.K[key] / 4 and wrong > uc.K[key], (mut, cid, good, wrong)
