"""`-m gpu`: every case of tests/attention_cases.py through bcos_attention_fwd / bcos_attention_bwd_v, on BOTH kernel families -- the
default attention_h2_kernel (f16 matrix pipe, two-way splits) and attention_mfma_kernel (fp32 matrix pipe, option attention_f32) --
launched through the C ABI and judged PER ELEMENT against the same operation in fp64 (the reference, the four bound forms and their
constants: tests/attention_cases.py; stated in include/bcos_hip.h).

For a case and a family:
  * out, stats[..., 0] (row max), stats[..., 1] (1 / row sum) and gv are held to their bounds, every element; gv is computed from the
    family's OWN forward statistics;
  * out_absmax / gv_absmax are bit-equal to the row maxima, over all H 64 columns, of the tensor actually written;
  * nothing else is written: every output lies inside a larger buffer with guard bands of 64 rows (tensors: NaN; maxima: a NaN
    bit pattern around the zeroed words) that must be untouched;
  * a second call gives the same bits.
Refusals (T = 289, head dim 32, the full gradient at T = 257) return non-zero, set the error string and write nothing.
The full gradient bcos_attention_bwd runs the interior and the end of its scalar kernel's range and the misaligned-pointer route to it,
under the criterion of test_gpu_parity.py::test_attention_gradient_on_the_matrix_pipe against cpu_emulation.attention_bwd (fp64).

The module prints, per family and direction, the worst error / bound and the case that produced it; BCOS_ATTENTION_REPORT=<path>
writes the same as JSON.
"""
import ctypes as C
import json
import os

import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = ("h2", "f32")          # attention_h2_kernel (default) / attention_mfma_kernel (option attention_f32 = 1)
GUARD_ROWS = 64
NAN_WORD = 0x7FC00000

WORST = {}          # "family/direction" -> {output kind: (worst error / (K form), case id)}
_REF = {}           # the one case whose inputs and fp64 reference are on the device (shared by the two families, never written to)


@pytest.fixture(scope="module")
def blib(hip_lib):
    from bcos_hip import lib
    yield lib
    rows = {r: {k: (round(v, 4), cid) for k, (v, cid) in d.items()} for r, d in sorted(WORST.items())}
    if rows:
        print("\nworst error / bound per kernel family, direction and output:")
        for r, d in rows.items():
            print(f"  {r:8s} " + "  ".join(f"{k}={v[0]:.3f} ({v[1]})" for k, v in sorted(d.items())))
    path = os.environ.get("BCOS_ATTENTION_REPORT")
    if path and rows:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def family_option(blib, family):
    return blib.option("attention_f32", 1 if family == "f32" else 0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """a tensor inside a larger buffer: `guard` elements on either side that nobody may write.  Float tensors are NaN throughout;
    the int32 words of a row-maximum buffer are zero (the heads meet in an atomic max) between guards of a NaN bit pattern."""

    def __init__(self, shape, guard, maxima=False, offset=0):
        n = 1
        for s in shape:
            n *= s
        self.guard, self.n, self.maxima, self.offset = guard, n, maxima, offset
        if maxima:
            self.buf = torch.full((2 * guard + n,), NAN_WORD, dtype=torch.int32, device=DEV)
            self.buf[guard:guard + n] = 0
        else:
            self.buf = torch.full((2 * guard + n + offset,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[guard + offset:guard + offset + n].view(shape)
        assert self.t.data_ptr() % 16 == (4 * offset) % 16

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def guards_untouched(self):
        lo, hi = self.buf[:self.guard + self.offset], self.buf[self.guard + self.offset + self.n:]
        if self.maxima:
            return bool((lo == NAN_WORD).all() and (hi == NAN_WORD).all())
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())

    def untouched(self):
        assert not self.maxima
        return bool(torch.isnan(self.buf).all())


def ptr(t):
    return C.c_void_p(t.data_ptr())


def device_reference(case):
    """inputs and fp64 reference of the case on the device; computed once per case"""
    if _REF.get("id") != case.id:
        qkv, gout = (t.to(DEV) for t in ac.make_inputs(case))
        _REF.clear()
        _REF.update(id=case.id, qkv=qkv, gout=gout, ref=ac.reference(qkv, gout, case.H))
    return _REF["qkv"], _REF["gout"], _REF["ref"]


def launch_fwd(lib, blib, qkv, case):
    B, T, H = case.B, case.T, case.H
    inner = H * ac.DH
    g = GUARD_ROWS * inner
    out, stats, am = Guarded((B, T, inner), g), Guarded((B, H, T, 2), g), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True)
    blib.check(lib.bcos_attention_fwd(ptr(qkv), out.ptr, stats.ptr, am.ptr, B, T, H, ac.DH, ac.SCALE, stream()), "bcos_attention_fwd")
    torch.cuda.synchronize()
    return out, stats, am


def launch_bwd_v(lib, blib, qkv, stats, gout, case):
    B, T, H = case.B, case.T, case.H
    inner = H * ac.DH
    gv, am = Guarded((B, T, inner), GUARD_ROWS * inner), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True)
    blib.check(lib.bcos_attention_bwd_v(ptr(qkv), ptr(stats), ptr(gout), gv.ptr, am.ptr, B, T, H, ac.DH, ac.SCALE, stream()),
               "bcos_attention_bwd_v")
    torch.cuda.synchronize()
    return gv, am


def row_maxima_bits(t):
    return t.reshape(-1, t.shape[-1]).abs().amax(dim=1).view(torch.int32)


def record(family, direction, kind, value, cid):
    slot = WORST.setdefault(f"{family}/{direction}", {})
    if kind not in slot or not value <= slot[kind][0]:
        slot[kind] = (value, cid)


@pytest.mark.parametrize("case,family", [(c, f) for c in ac.CASES for f in FAMILIES], ids=lambda v: v if isinstance(v, str) else v.id)
def test_case_against_fp64_per_element(blib, case, family):
    lib = blib.load()
    qkv, gout, ref = device_reference(case)
    with family_option(blib, family):
        out, stats, am = launch_fwd(lib, blib, qkv, case)
        gv, gam = launch_bwd_v(lib, blib, qkv, stats.t, gout, case)
        out2, stats2, am2 = launch_fwd(lib, blib, qkv, case)
        gv2, gam2 = launch_bwd_v(lib, blib, qkv, stats.t, gout, case)
    for name, gd in (("out", out), ("stats", stats), ("out_absmax", am), ("gv", gv), ("gv_absmax", gam)):
        assert gd.guards_untouched(), (case.id, family, name, "write outside the tensor")
    r = ac.ratios(ref, out=out.t, stats=stats.t, gv=gv.t)
    used = {kind: v / ac.K[kind] for kind, v in r.items()}          # error / bound: <= 1 passes
    print(case.id, family, {k: f"{v:.3f}" for k, v in used.items()})
    for kind, v in used.items():
        record(family, "bwd" if kind == "gv" else "fwd", kind, v, case.id)
    bad = {k: v for k, v in used.items() if not v <= 1.0}
    assert not bad, (case.id, family, "worst error / bound", used)
    assert torch.equal(am.t, row_maxima_bits(out.t)), (case.id, family, "out_absmax")
    assert torch.equal(gam.t, row_maxima_bits(gv.t)), (case.id, family, "gv_absmax")
    for name, a, b in (("out", out, out2), ("stats", stats, stats2), ("out_absmax", am, am2), ("gv", gv, gv2), ("gv_absmax", gam, gam2)):
        assert torch.equal(a.t, b.t), (case.id, family, name, "differs from call to call")


def test_the_option_selects_the_fp32_kernels(blib):
    """attention_mfma_kernel<fwd> and <bwd> are launched by the option: with the same inputs (and the SAME statistics for the backward)
    their results differ in bits from the default family's, and both were held to fp64 above"""
    lib = blib.load()
    case = ac.by_id("normal-b2h3t197")
    qkv, gout, _ = device_reference(case)
    res = {}
    for family in FAMILIES:
        with family_option(blib, family):
            assert blib.get_option("attention_f32") == (1 if family == "f32" else 0)
            out, stats, _ = launch_fwd(lib, blib, qkv, case)
            res.setdefault("stats", stats.t)                 # (the default family's, for both backward launches)
            gv, _ = launch_bwd_v(lib, blib, qkv, res["stats"], gout, case)
            res[family] = (out.t, gv.t)
    assert not torch.equal(res["h2"][0], res["f32"][0]), "the forward result does not depend on the attention_f32 option"
    assert not torch.equal(res["h2"][1], res["f32"][1]), "the backward result does not depend on the attention_f32 option"


def _error_set(lib):
    msg = lib.bcos_last_error_string()
    return bool(msg) and b"attention" in msg


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_beyond_the_lds_are_refused(blib, family):
    lib = blib.load()
    case = ac.Case("normal", 289)
    qkv, gout = (t.to(DEV) for t in ac.make_inputs(case))
    B, T, H = case.B, case.T, case.H
    inner = H * ac.DH
    g = GUARD_ROWS * inner
    stats_in = torch.zeros(B, H, T, 2, device=DEV)
    with family_option(blib, family):
        out, stats, am = Guarded((B, T, inner), g), Guarded((B, H, T, 2), g), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True)
        rc = lib.bcos_attention_fwd(ptr(qkv), out.ptr, stats.ptr, am.ptr, B, T, H, ac.DH, ac.SCALE, stream())
        assert rc == blib.BCOS_E_NOSUP and _error_set(lib), (rc, lib.bcos_last_error_string())
        gv, gam = Guarded((B, T, inner), g), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True)
        rc = lib.bcos_attention_bwd_v(ptr(qkv), ptr(stats_in), ptr(gout), gv.ptr, gam.ptr, B, T, H, ac.DH, ac.SCALE, stream())
        assert rc == blib.BCOS_E_NOSUP and _error_set(lib), (rc, lib.bcos_last_error_string())
    torch.cuda.synchronize()
    assert out.untouched() and stats.untouched() and gv.untouched()
    assert am.guards_untouched() and gam.guards_untouched() and not bool(am.t.any()) and not bool(gam.t.any())


def test_other_head_dimensions_and_long_full_gradients_are_refused(blib):
    lib = blib.load()
    B, T, H, Dh = 2, 33, 3, 32
    inner = H * Dh
    g = GUARD_ROWS * inner
    gen = torch.Generator().manual_seed(5)
    qkv, gout = torch.randn(B, T, 3 * inner, generator=gen).to(DEV), torch.randn(B, T, inner, generator=gen).to(DEV)
    stats_in, out_in = torch.zeros(B, H, T, 2, device=DEV), torch.zeros(B, T, inner, device=DEV)
    out, stats, am = Guarded((B, T, inner), g), Guarded((B, H, T, 2), g), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True)
    gv, gam, gqkv = Guarded((B, T, inner), g), Guarded((B * T,), 4 * GUARD_ROWS, maxima=True), Guarded((B, T, 3 * inner), 3 * g)
    rc = lib.bcos_attention_fwd(ptr(qkv), out.ptr, stats.ptr, am.ptr, B, T, H, Dh, ac.SCALE, stream())
    assert rc == blib.BCOS_E_NOSUP and _error_set(lib), rc
    rc = lib.bcos_attention_bwd_v(ptr(qkv), ptr(stats_in), ptr(gout), gv.ptr, gam.ptr, B, T, H, Dh, ac.SCALE, stream())
    assert rc == blib.BCOS_E_NOSUP and _error_set(lib), rc
    rc = lib.bcos_attention_bwd(ptr(qkv), ptr(stats_in), ptr(out_in), ptr(gout), gqkv.ptr, B, T, H, Dh, ac.SCALE, stream())
    assert rc == blib.BCOS_E_NOSUP and _error_set(lib), rc
    # the full gradient holds one key per thread of a 256-thread workgroup: 257 tokens are refused
    case = ac.Case("normal", 257, B=1, H=2)
    qkv, gout = (t.to(DEV) for t in ac.make_inputs(case))
    inner = case.H * ac.DH
    stats_in, out_in = torch.zeros(1, case.H, 257, 2, device=DEV), torch.zeros(1, 257, inner, device=DEV)
    gq257 = Guarded((1, 257, 3 * inner), GUARD_ROWS * 3 * inner)
    rc = lib.bcos_attention_bwd(ptr(qkv), ptr(stats_in), ptr(out_in), ptr(gout), gq257.ptr, 1, 257, case.H, ac.DH, ac.SCALE, stream())
    assert rc == blib.BCOS_E_NOSUP and _error_set(lib), rc
    torch.cuda.synchronize()
    for gd in (out, stats, gv, gqkv, gq257):
        assert gd.untouched()
    assert am.guards_untouched() and gam.guards_untouched() and not bool(am.t.any()) and not bool(gam.t.any())


def _full_gradient(lib, blib, qkv, stats, out, gout, case, offset):
    """bcos_attention_bwd with qkv, out, gout and gqkv each `offset` floats behind a 16-byte boundary; returns the guarded gradient"""
    B, T, H = case.B, case.T, case.H
    inner = H * ac.DH

    def placed(t):
        gd = Guarded(tuple(t.shape), 4, offset=offset)
        gd.t.copy_(t)
        return gd
    q_, o_, g_ = placed(qkv), placed(out), placed(gout)
    gq = Guarded((B, T, 3 * inner), GUARD_ROWS * 3 * inner, offset=offset)
    blib.check(lib.bcos_attention_bwd(q_.ptr, ptr(stats), o_.ptr, g_.ptr, gq.ptr, B, T, H, ac.DH, ac.SCALE, stream()), "bcos_attention_bwd")
    torch.cuda.synchronize()
    assert gq.guards_untouched(), (case.id, offset, "write outside gqkv")
    return gq


def _full_gradient_errors(g, ref, inner):
    """the criterion of test_attention_gradient_on_the_matrix_pipe: per part, (L2 error, tolerance)"""
    scale_all = float(ref.double().norm())
    res = {}
    for name, sl in (("q", slice(0, inner)), ("k", slice(inner, 2 * inner)), ("v", slice(2 * inner, 3 * inner))):
        err = float((g[..., sl].double().cpu() - ref[..., sl].double()).norm())
        res[name] = (err, max(2e-5 * float(ref[..., sl].double().norm()), 1e-6 * scale_all))
    return res


@pytest.mark.parametrize("T,offset", [(209, 0), (255, 0), (256, 0), (33, 1)], ids=["t209", "t255", "t256", "t33-misaligned"])
def test_full_gradient_on_the_scalar_kernel(blib, T, offset):
    """bcos_attention_bwd beyond the 207 tokens of its matrix-pipe kernel (the interior and the end of the scalar kernel's range), and
    at T = 33 with every vector-accessed pointer one float off a 16-byte boundary: the alignment gate sends that call to the scalar
    kernel too.  Against fp64; the misaligned call also agrees with the aligned one (matrix pipe) within twice the tolerance."""
    import cpu_emulation as E
    from bcos_hip import ops
    lib = blib.load()
    case = ac.Case("normal", T, B=2, H=2)
    qkv, gout = (t.to(DEV) for t in ac.make_inputs(case))
    inner = case.H * ac.DH
    out, stats = ops.attention_fwd(qkv, case.H, ac.SCALE, want_stats=True)
    ref = E.attention_bwd(qkv.cpu(), None, None, gout.cpu(), case.H, ac.SCALE)
    gq = _full_gradient(lib, blib, qkv, stats, out, gout, case, offset)
    again = _full_gradient(lib, blib, qkv, stats, out, gout, case, offset)
    assert torch.equal(gq.t, again.t), (T, offset, "differs from call to call")
    assert bool(torch.isfinite(gq.t).all())
    errs = _full_gradient_errors(gq.t, ref, inner)
    print(T, offset, {k: f"{e:.3e} / {t:.3e}" for k, (e, t) in errs.items()})
    assert all(e <= t for e, t in errs.values()), (T, offset, errs)
    if offset:
        aligned = _full_gradient(lib, blib, qkv, stats, out, gout, case, 0)
        assert all(e <= t for e, t in _full_gradient_errors(aligned.t, ref, inner).values())
        assert not torch.equal(aligned.t, gq.t), "the misaligned call took the same kernel as the aligned one"
        for name, sl in (("q", slice(0, inner)), ("k", slice(inner, 2 * inner)), ("v", slice(2 * inner, 3 * inner))):
            diff = float((gq.t[..., sl].double() - aligned.t[..., sl].double()).norm())
            assert diff <= 2 * errs[name][1], (name, diff, errs[name][1])
