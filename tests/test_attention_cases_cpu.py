"""The reference and the bounds of tests/attention_cases.py, without a device:

  * the constants are what the module says they are: for every case the plain fp32 PyTorch evaluation of the reference expression stays
    within K / 4 of each bound form, and the worst use over the table is the measurement the constants were set from;
  * the bound is sharp enough to matter: a forward that drops the low plane of q's two-way fp16 split, and one that lets a zero-padded
    key into the softmax, exceed K_OUT;
  * cpu_emulation.attention_fwd / attention_bwd_v, the stand-ins of the CPU tier, compute the reference.
"""
import pytest
import torch

import attention_cases as ac

MEASURED = {}        # output kind -> (worst fp32 use of the form, case id)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nworst |fp32 PyTorch - fp64| / bound form over the case table, in units of u (K = 4 x FP32_WORST):")
        for kind, (v, cid) in sorted(MEASURED.items()):
            print(f"  {kind:5s} {v:6.3f}  ({cid})   FP32_WORST {ac.FP32_WORST[kind]}   K {ac.K[kind]}")


def test_case_table_is_the_one_the_bounds_were_measured_on():
    ids = [c.id for c in ac.CASES]
    assert len(ids) == len(set(ids))
    normal = {(c.B, c.H, c.T) for c in ac.CASES if c.family == "normal"}
    assert normal == {(2, 3, T) for T in (1, 31, 32, 33, 64, 65, 197, 256, 257, 288)} | {(1, 32, 50), (3, 1, 17)}
    for fam in ac.FAMILIES:
        assert {c.T for c in ac.CASES if c.family == fam} >= {33, 197, 288}, fam
    assert {c.family for c in ac.CASES} == set(ac.FAMILIES)
    assert ac.K == {k: 4 * v for k, v in ac.FP32_WORST.items()}
    assert (ac.K_OUT, ac.K_GV, ac.K_MAX, ac.K_RSUM) == (ac.K["out"], ac.K["gv"], ac.K["max"], ac.K["rsum"])


def test_families_have_the_properties_they_are_in_the_table_for():
    for T in (33, 197, 288):
        qkv, gout = ac.make_inputs(ac.Case("hot", T))
        ref = ac.reference(qkv, gout, 3)
        assert float(ref["max"][0].max()) > 2 * 88          # exp(s) overflows fp32 unless the row maximum is subtracted first
        qkv, gout = ac.make_inputs(ac.Case("negscore", T))
        q, k, _ = ac.split_qkv(qkv.double(), 3)
        assert float((q @ k.transpose(-1, -2) * ac.SCALE).max()) <= -50      # a zero-padded key (raw score 0) would win every row
        qkv, gout = ac.make_inputs(ac.Case("tokrange", T))
        rowmax = ac.split_qkv(qkv, 3)[1].abs().amax(-1)
        assert float(rowmax.max() / rowmax.min()) > 100
        qkv, gout = ac.make_inputs(ac.Case("colrange", T))
        colmax = ac.split_qkv(qkv, 3)[2].abs().amax(-2)
        assert float(colmax.max() / colmax.min()) > 1e5
    a, b = ac.make_inputs(ac.Case("normal", 33))
    a2, b2 = ac.make_inputs(ac.Case("normal", 33))
    assert torch.equal(a, a2) and torch.equal(b, b2)
    q = ac.split_qkv(a, 3)[0]
    assert not torch.equal(q[0, 0], q[0, 1]) and not torch.equal(q[0, 0], q[1, 0])       # batches and heads carry different data


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_fp32_reference_stays_within_a_quarter_of_every_bound(case):
    r = ac.fp32_ratios(case)
    print(case.id, {k: f"{v:.3f}" for k, v in r.items()})
    for kind, v in r.items():
        if kind not in MEASURED or v > MEASURED[kind][0]:
            MEASURED[kind] = (v, case.id)
    bad = {kind: v for kind, v in r.items() if not v <= ac.K[kind] / 4}
    assert not bad, (case.id, "fp32 error / form beyond K / 4", bad)


def test_constants_are_four_times_the_measured_worst():
    """(runs behind the parametrised measurement above: the constants are not looser than the table makes them either)"""
    if len(MEASURED) < 4:
        for case in ac.CASES:
            for kind, v in ac.fp32_ratios(case).items():
                if kind not in MEASURED or v > MEASURED[kind][0]:
                    MEASURED[kind] = (v, case.id)
    for kind, want in ac.FP32_WORST.items():
        got = MEASURED[kind][0]
        assert want - 0.3 < got <= want, (kind, got, want, MEASURED[kind][1])


def _high_plane(x):
    """x rounded ONCE to fp16 behind the per-row power of two of the kernels (row maximum in [2^14, 2^15)): the high plane of the
    two-way split alone"""
    e = x.abs().amax(-1, keepdim=True).frexp().exponent          # max = f 2^e, f in [0.5, 1)
    sc = torch.ldexp(torch.ones_like(x[..., :1]), 15 - e)
    return (x * sc).half().float() / sc


def test_bound_notices_a_dropped_low_plane():
    case = ac.by_id("normal-b2h3t197")
    qkv, gout = ac.make_inputs(case)
    ref = ac.reference(qkv, gout, case.H)
    q = ac.split_qkv(qkv, case.H)[0]
    qh = _high_plane(q)
    assert float((qh - q).abs().max()) > 0 and float(((qh - q).abs() / q.abs().amax(-1, keepdim=True)).max()) <= 2.0 ** -11
    wrong = ac.evaluate(qkv, gout, case.H, torch.float64, q_override=qh)
    r = ac.ratios(ref, out=wrong["out"])["out"]
    print("high plane of q only: error / form", r, "K_OUT", ac.K_OUT)
    assert r > ac.K_OUT
    exact = ac.evaluate(qkv, gout, case.H, torch.float64)
    assert ac.ratios(ref, out=exact["out"])["out"] == 0.0


def test_bound_notices_a_padded_key_in_the_softmax():
    case = ac.by_id("negscore-b2h3t33")
    qkv, gout = ac.make_inputs(case)
    ref = ac.reference(qkv, gout, case.H)
    B, T, _ = qkv.shape
    padded = torch.cat([qkv, torch.zeros(B, 1, qkv.shape[-1])], dim=1)           # one zero key (and value) behind the last token
    wrong = ac.evaluate(padded, torch.cat([gout, torch.zeros(B, 1, gout.shape[-1])], dim=1), case.H, torch.float64)
    r = ac.ratios(ref, out=wrong["out"][:, :T])["out"]
    print("one zero-padded key in the softmax: error / form", r, "K_OUT", ac.K_OUT)
    assert r > ac.K_OUT


@pytest.mark.parametrize("cid", ["normal-b2h3t33", "colrange-b2h3t197"])
def test_cpu_emulation_computes_the_reference(cid):
    import cpu_emulation as E
    case = ac.by_id(cid)
    qkv, gout = ac.make_inputs(case)
    ref = ac.reference(qkv, gout, case.H)
    out, _ = E.attention_fwd(qkv, case.H, ac.SCALE, want_stats=True)
    gv = E.attention_bwd_v(qkv, None, gout, case.H, ac.SCALE)
    r = ac.ratios(ref, out=out, gv=gv)
    # (fp64 rounded once to fp32: half an ulp of the element, |out| <= p |v| -- far inside a form that starts at 4 u p |v|)
    assert r["out"] <= 0.25 and r["gv"] <= 0.25, r
