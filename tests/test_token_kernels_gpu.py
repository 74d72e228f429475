"""`-m gpu`: every case of tests/token_cases.py through the token-path entry points of csrc/bcos_vit.hip and the centred norms of
csrc/bcos_norms.hip, launched through the C ABI (raw pointers: the misaligned cases are views that bcos_hip.ops would not pass) and
judged PER ELEMENT against the same operation in fp64 (the reference, the bound forms and their constants:
tests/token_cases.py; stated in include/bcos_hip.h).

Which case reaches which kernel:
  norm_rows_fwd / _bwd_detached_kernel<VEC, CENTERED>             ln-* with D in {4, 64, 68, 192, 252, 256} (D = 8 for the second pass)
  norm_rows_fwd / _bwd_detached_kernel<!VEC, CENTERED>            ln-* with D in {1, 3, 50, 65, 260, 384, 768, 1000} (D = 5 for the second
                                                                  pass), and every D % 4 == 0 case again with x, y or w one float off a
                                                                  16-byte boundary (test_misaligned_operands_take_the_strided_kernels)
  layernorm_stats16_kernel<1> .. <4>                              `stats` of D = 4 and 64 / 68 / 192 / 252 and 256, each with rows 1 and 5;
                                                                  the second pass (131072 rows) at ln-*-r131093d4 and -r131093d68
  layernorm_stats_kernel                                          `stats` of the strided widths; second pass at ln-offset-r8229d5
  norm_rows_bwd_full_kernel<!VEC, CENTERED>                       `bwd` of every ln-* case (bcos_layernorm_bwd and bcos_layernorm_bwd_add)
  norm_group_fwd / _bwd_detached / _bwd_full_kernel<CENTERED>     gn-*: m = HW C / G of 1, 2, 255, 256, 257 and beyond; cg of 1, 2, 3, 4, 6, 64; G = 1
  gelu_gate_kernel, gelu_bwd_full_kernel                          gelu-gate-*, gelu-bwd-*; the long ones run 77 elements of a second pass
  add_rows_bcast_kernel                                           add-*; add-b512t1d4104 goes past the grid cap
  finalize_patches_kernel, 16-byte record loads                   fin-*c8-* (fin-n65h256w256p16c8-inv1 goes past the grid cap)
  finalize_patches_kernel, scalar record loads                    fin-*c6-*, fin-*c12-*, fin-*-mis (gp one float into its buffer)

For a case and an entry point:
  * every element of every output is held to its bound; a failure names the form, the worst element and its use of the form in units of u;
  * x_absmax is bit-equal to max |x| of the row, y_absmax / out2_absmax to the row maximum of the y / out2 the same launch wrote;
  * every optional output is also left out once, and what remains has the same bits;
  * nothing else is written: every output lies between guard bands that must be untouched;
  * every call is made twice and gives the same bits (none of these kernels has atomics).
Refusals return non-zero and write nothing.

The module prints, per entry point and form, the worst error / bound and the case that produced it; BCOS_TOKEN_REPORT=<path> writes the
same as JSON.
"""
import ctypes as C
import json
import os

import pytest
import torch

import token_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256
NAN_WORD = 0x7FC00000

WORST = {}          # "entry point/form" -> (worst error / bound, case id, output)
_REF = {}           # the one case whose inputs, fp64 reference and forms are on the device (shared by its entry points, never written to)


@pytest.fixture(scope="module")
def blib(hip_lib):
    from bcos_hip import lib
    yield lib
    rows = {k: (round(v, 4), cid, name) for k, (v, cid, name) in sorted(WORST.items())}
    if rows:
        print("\nworst error / bound per entry point and form:")
        for k, (v, cid, name) in rows.items():
            print(f"  {k:24s} {v:.3f}  ({cid}: {name})")
    path = os.environ.get("BCOS_TOKEN_REPORT")
    if path and rows:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """a tensor inside a larger buffer, `offset` floats behind a 16-byte boundary, with GUARD words on either side that nobody may
    write.  Outputs start as NaN (fp32) / a NaN bit pattern (row maxima): an element the kernel skipped shows."""

    def __init__(self, shape, offset=0, maxima=False, src=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.offset, self.maxima = n, offset, maxima
        if maxima:
            self.buf = torch.full((2 * GUARD + n + offset,), NAN_WORD, dtype=torch.int32, device=DEV)
        else:
            self.buf = torch.full((2 * GUARD + n + offset,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD + offset:GUARD + offset + n].view(shape)
        assert self.t.data_ptr() % 16 == (4 * offset) % 16
        if src is not None:
            self.t.copy_(src)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def guards_untouched(self):
        lo, hi = self.buf[:GUARD + self.offset], self.buf[GUARD + self.offset + self.n:]
        if self.maxima:
            return bool((lo == NAN_WORD).all() and (hi == NAN_WORD).all())
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())

    def untouched(self):
        return bool((self.buf == NAN_WORD).all()) if self.maxima else bool(torch.isnan(self.buf).all())


def ptr(t, offset=0):
    """the device pointer of an input (None -> NULL); with an offset, of a copy that many floats behind a 16-byte boundary"""
    if t is None:
        return None, None
    if offset:
        g = Guarded(tuple(t.shape), offset=offset, src=t)
        return g.ptr, g
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr()), t


def device_case(case):
    """inputs, fp64 reference and bound forms of the case on the device; computed once per case"""
    if _REF.get("id") != case.id:
        _REF.clear()
        torch.cuda.empty_cache()
        inp = {k: (v.to(DEV) if v is not None else None) for k, v in tc.make_inputs(case).items()}
        ref = tc.reference(case, inp)
        _REF.update(id=case.id, inp=inp, ref=ref, forms=tc.forms(case, inp, ref))
    return _REF


def row_maxima_bits(t):
    return t.reshape(t.shape[0], -1).abs().amax(dim=1).view(torch.int32)


def judge(case, d, entry, outs):
    """outs: output name -> Guarded (or tensor); every element against its bound"""
    for name, g in outs.items():
        t = g.t if isinstance(g, Guarded) else g
        if isinstance(g, Guarded):
            assert g.guards_untouched(), (case.id, entry, name, "write outside the tensor")
        key, form, add = d["forms"][name]
        v, i = tc.use(t, d["ref"][name], form, add)
        slot = f"{entry}/{key}"
        if slot not in WORST or not v / tc.K[key] <= WORST[slot][0]:
            WORST[slot] = (v / tc.K[key], case.id, name)
        where = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), t.shape)) if t.dim() else ()
        assert v <= tc.K[key], (f"{case.id} {entry} {name}: form `{key}`, worst element {where} uses {v:.3f} u x form "
                                f"(K = {tc.K[key]:.1f}): got {t.reshape(-1)[i].item()!r}, fp64 {d['ref'][name].reshape(-1)[i].item()!r}")


def same_bits(case, entry, a, b, what):
    for name in a:
        ta, tb = (g.t if isinstance(g, Guarded) else g for g in (a[name], b[name]))
        assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)), (case.id, entry, name, what)


def twice(case, entry, fn):
    a, b = fn(), fn()
    same_bits(case, entry, a, b, "differs from call to call")
    return a


# ---- launches: each returns {output name: Guarded} ----------------------------------------------------------------------------------
def ln_fwd(lib, blib, case, inp, extras=True, off=None):
    off = off or {}
    rows, D = case.rows, case.D
    y = Guarded((rows, D), offset=off.get("y", 0))
    rstd, am = (Guarded((rows,)), Guarded((rows,), maxima=True)) if extras else (None, None)
    (px, kx), (pw, kw), (pb, kb) = ptr(inp["x"], off.get("x", 0)), ptr(inp["w"], off.get("w", 0)), ptr(inp["b"])
    blib.check(lib.bcos_layernorm_fwd(px, pw, pb, y.ptr, rstd.ptr if extras else None, am.ptr if extras else None, rows, D, case.eps,
                                      stream()), "bcos_layernorm_fwd")
    torch.cuda.synchronize()
    return {"y": y, "rstd": rstd, "y_absmax": am} if extras else {"y": y}


def ln_stats(lib, blib, case, inp, extras=True, off=None):
    off = off or {}
    rows, D = case.rows, case.D
    rstd = Guarded((rows,))
    zss, am = (Guarded((rows,)), Guarded((rows,), maxima=True)) if extras else (None, None)
    (px, kx), (pw, kw), (pb, kb) = ptr(inp["x"], off.get("x", 0)), ptr(inp["w"], off.get("w", 0)), ptr(inp["b"])
    blib.check(lib.bcos_layernorm_stats(px, pw, pb, rstd.ptr, zss.ptr if extras else None, am.ptr if extras else None, rows, D, case.eps,
                                        stream()), "bcos_layernorm_stats")
    torch.cuda.synchronize()
    return {"rstd": rstd, "zss": zss, "x_absmax": am} if extras else {"rstd": rstd}


DET_VARIANTS = [(outs, a, m, am) for outs in ("out", "out2", "both") for a in (False, True) for m in (False, True)
                for am in ((False,) if outs == "out" else (False, True))]


def ln_bwd_detached(lib, blib, case, inp, outs, addend, mul2, absmax, off=None):
    """one accepted combination of (out / out2 / both, addend, mul2, out2_absmax); outputs under the names of token_cases"""
    off = off or {}
    rows, D = case.rows, case.D
    key = ("a" if addend else "-") + ("m" if mul2 else "-")
    o = Guarded((rows, D), offset=off.get("y", 0)) if outs in ("out", "both") else None
    o2 = Guarded((rows, D)) if outs in ("out2", "both") else None
    am = Guarded((rows,), maxima=True) if absmax else None
    (pg, kg), (pw, kw) = ptr(inp["gy"], off.get("x", 0)), ptr(inp["w"], off.get("w", 0))
    blib.check(lib.bcos_layernorm_bwd_detached(pg, pw, ptr(inp["rstd"])[0], ptr(inp["addend"])[0] if addend else None,
                                               ptr(inp["mul2"])[0] if mul2 else None, o.ptr if o else None, o2.ptr if o2 else None,
                                               am.ptr if am else None, rows, D, stream()), "bcos_layernorm_bwd_detached")
    torch.cuda.synchronize()
    r = {}
    if o:
        r["out/" + key] = o
    if o2:
        r["out2/" + key] = o2
    if am:
        r["out2_absmax"] = am
    return r


def ln_bwd(lib, blib, case, inp, addend, xhat, via_add=False):
    rows, D = case.rows, case.D
    gx, xh = Guarded((rows, D)), (Guarded((rows, D)) if xhat else None)
    args = (ptr(inp["gy"])[0], ptr(inp["x"])[0], ptr(inp["w"])[0], ptr(inp["rstd"])[0])
    if addend or via_add:
        blib.check(lib.bcos_layernorm_bwd_add(*args, ptr(inp["addend"])[0] if addend else None, gx.ptr, xh.ptr if xh else None, rows, D,
                                              stream()), "bcos_layernorm_bwd_add")
    else:
        blib.check(lib.bcos_layernorm_bwd(*args, gx.ptr, xh.ptr if xh else None, rows, D, stream()), "bcos_layernorm_bwd")
    torch.cuda.synchronize()
    r = {"gx/a" if addend else "gx/-": gx}
    if xh:
        r["xhat"] = xh
    return r


def split_maxima(outs):
    return {k: v for k, v in outs.items() if "absmax" not in k}, {k: v for k, v in outs.items() if "absmax" in k}


def check_ln(lib, blib, case, d, op, off=None):
    inp = d["inp"]
    tag = op + ("" if not off else "[" + ",".join(f"{k}+{v}" for k, v in off.items()) + "]")
    if op == "fwd":
        full = twice(case, tag, lambda: ln_fwd(lib, blib, case, inp, True, off))
        vals, mx = split_maxima(full)
        judge(case, d, tag, vals)
        assert mx["y_absmax"].guards_untouched()
        assert torch.equal(mx["y_absmax"].t, row_maxima_bits(full["y"].t)), (case.id, tag, "y_absmax is not the row maximum of the y written")
        same_bits(case, tag, ln_fwd(lib, blib, case, inp, False, off), {"y": full["y"]}, "y depends on the optional outputs")
    elif op == "stats":
        full = twice(case, tag, lambda: ln_stats(lib, blib, case, inp, True, off))
        vals, mx = split_maxima(full)
        judge(case, d, tag, vals)
        assert mx["x_absmax"].guards_untouched()
        assert torch.equal(mx["x_absmax"].t, row_maxima_bits(inp["x"])), (case.id, tag, "x_absmax is not max |x| of the row")
        same_bits(case, tag, ln_stats(lib, blib, case, inp, False, off), {"rstd": full["rstd"]}, "rstd depends on the optional outputs")
    elif op == "bwd_detached":
        first = {}
        for outs, a, m, am in (DET_VARIANTS if not off else [("both", True, True, True)]):
            r = twice(case, tag, lambda: ln_bwd_detached(lib, blib, case, inp, outs, a, m, am, off))
            vals, mx = split_maxima(r)
            judge(case, d, f"{tag}", vals)
            if am:
                assert mx["out2_absmax"].guards_untouched()
                o2 = next(v for k, v in r.items() if k.startswith("out2/"))
                assert torch.equal(mx["out2_absmax"].t, row_maxima_bits(o2.t)), (case.id, tag, outs, a, m, "out2_absmax is not the row maximum of out2")
            for k, v in vals.items():                        # a tensor does not depend on which other outputs were asked for
                if k in first:
                    same_bits(case, tag, {k: v}, {k: first[k]}, f"depends on the outputs requested ({outs}, absmax {am})")
                first.setdefault(k, v)
    elif op == "bwd":
        plain = twice(case, tag, lambda: ln_bwd(lib, blib, case, inp, False, True))
        judge(case, d, tag, plain)
        same_bits(case, tag, ln_bwd(lib, blib, case, inp, False, False), {"gx/-": plain["gx/-"]}, "gx depends on xhat_out")
        same_bits(case, tag, ln_bwd(lib, blib, case, inp, False, True, via_add=True), plain, "bcos_layernorm_bwd_add(addend = NULL) differs")
        added = twice(case, tag + "_add", lambda: ln_bwd(lib, blib, case, inp, True, True))
        judge(case, d, tag + "_add", added)
        same_bits(case, tag, {"xhat": added["xhat"]}, {"xhat": plain["xhat"]}, "xhat depends on the addend")
    else:
        raise ValueError(op)


@pytest.mark.parametrize("case,op", [(c, op) for c in tc.LN_CASES for op in c.ops], ids=lambda v: v if isinstance(v, str) else v.id)
def test_layernorm_case_against_fp64_per_element(blib, case, op):
    check_ln(blib.load(), blib, case, device_case(case), op)


def test_misaligned_operands_take_the_strided_kernels(blib):
    """every D % 4 == 0 case of up to 333 rows again with ONE operand a view one float into its buffer -- x (gy), then y (out), then w:
    vec_ok sends the call to the strided kernels (a 16-byte access there would fault or read the neighbour), which meet the same bounds"""
    lib = blib.load()
    n = 0
    for case in tc.LN_CASES:
        if case.D % 4 or case.rows > 333:
            continue
        d = device_case(case)
        for op, operands in (("fwd", ("x", "y", "w")), ("stats", ("x", "w")), ("bwd_detached", ("x", "y", "w"))):
            for which in operands:
                if which == "w" and d["inp"]["w"] is None:
                    continue
                check_ln(lib, blib, case, d, op, off={which: 1})
                n += 1
    assert n >= 100


def gn_launch(lib, blib, case, inp, op, extra):
    N, HW, Cc, G = case.N, case.HW, case.C, case.G
    shape = (N, HW, Cc)
    pw, pb, prs = ptr(inp["w"])[0], ptr(inp["b"])[0], ptr(inp["rstd"])[0]
    if op == "fwd":
        y, rstd = Guarded(shape), (Guarded((N * G,)) if extra else None)
        blib.check(lib.bcos_groupnorm_fwd(ptr(inp["x"])[0], pw, pb, y.ptr, rstd.ptr if extra else None, N, HW, Cc, G, case.eps, stream()),
                   "bcos_groupnorm_fwd")
        r = {"y": y, "rstd": rstd} if extra else {"y": y}
    elif op == "bwd_detached":
        gx = Guarded(shape)
        blib.check(lib.bcos_groupnorm_bwd_detached(ptr(inp["gy"])[0], pw, prs, gx.ptr, N, HW, Cc, G, stream()), "bcos_groupnorm_bwd_detached")
        r = {"gx_det": gx}
    else:
        gx, xh = Guarded(shape), (Guarded(shape) if extra else None)
        blib.check(lib.bcos_groupnorm_bwd(ptr(inp["gy"])[0], ptr(inp["x"])[0], pw, prs, gx.ptr, xh.ptr if extra else None, N, HW, Cc, G,
                                          stream()), "bcos_groupnorm_bwd")
        r = {"gx": gx, "xhat": xh} if extra else {"gx": gx}
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case,op", [(c, op) for c in tc.GN_CASES for op in c.ops], ids=lambda v: v if isinstance(v, str) else v.id)
def test_groupnorm_case_against_fp64_per_element(blib, case, op):
    lib = blib.load()
    d = device_case(case)
    full = twice(case, op, lambda: gn_launch(lib, blib, case, d["inp"], op, True))
    judge(case, d, "gn_" + op, full)
    if op != "bwd_detached":             # without rstd_out / xhat_out: the same y / gx
        bare = gn_launch(lib, blib, case, d["inp"], op, False)
        same_bits(case, op, bare, {k: full[k] for k in bare}, "depends on the optional output")


def gelu_launch(lib, blib, case, inp, want_gate=True):
    n = case.n
    if case.op == "gate":
        y, gate = Guarded((n,)), (Guarded((n,)) if want_gate else None)
        blib.check(lib.bcos_gelu_gate(ptr(inp["x"])[0], y.ptr, gate.ptr if gate else None, n, stream()), "bcos_gelu_gate")
        r = {"y": y, "gate": gate} if gate else {"y": y}
    else:
        gx = Guarded((n,))
        blib.check(lib.bcos_gelu_bwd(ptr(inp["gy"])[0], ptr(inp["x"])[0], gx.ptr, n, stream()), "bcos_gelu_bwd")
        r = {"gx": gx}
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case", tc.GELU_CASES, ids=lambda c: c.id)
def test_gelu_case_against_fp64_per_element(blib, case):
    lib = blib.load()
    d = device_case(case)
    full = twice(case, case.op, lambda: gelu_launch(lib, blib, case, d["inp"]))
    judge(case, d, "gelu_" + case.op, full)
    if case.op == "gate":
        same_bits(case, "gate", gelu_launch(lib, blib, case, d["inp"], want_gate=False), {"y": full["y"]}, "y depends on gate_out")
        # in place, as the engine calls it (out = the input): the same bits
        xy = Guarded((case.n,), src=d["inp"]["x"])
        gate = Guarded((case.n,))
        blib.check(lib.bcos_gelu_gate(xy.ptr, xy.ptr, gate.ptr, case.n, stream()), "bcos_gelu_gate (in place)")
        torch.cuda.synchronize()
        same_bits(case, "gate", {"y": xy, "gate": gate}, full, "the in-place call differs from the out-of-place one")
        assert xy.guards_untouched() and gate.guards_untouched()


@pytest.mark.parametrize("case", tc.ADD_CASES, ids=lambda c: c.id)
def test_add_rows_bcast_is_exact(blib, case):
    lib = blib.load()
    d = device_case(case)
    total, period = case.B * case.T * case.D, case.T * case.D

    def run():
        x = Guarded((case.B, case.T, case.D), src=d["inp"]["x"])
        blib.check(lib.bcos_add_rows_bcast(x.ptr, ptr(d["inp"]["pe"])[0], total, period, stream()), "bcos_add_rows_bcast")
        torch.cuda.synchronize()
        assert x.guards_untouched(), (case.id, "write outside the tensor")
        return {"x": x}
    got = twice(case, "add", run)
    same_bits(case, "add", got, {"x": d["ref"]["x"]}, "is not x + pe[i % period] in fp32")


def fin_launch(lib, blib, case, inp, gp, mode):
    N, H, W = case.N, case.H, case.W
    wo = Guarded((N, 6, H, W)) if mode in ("both", "weights") else None
    co = Guarded((N, H, W)) if mode in ("both", "contrib") else None
    blib.check(lib.bcos_finalize_explanation_patches(gp, ptr(inp["x"])[0], ptr(inp["std6"])[0], wo.ptr if wo else None,
                                                     co.ptr if co else None, N, 3 if case.add_inverse else 6, H, W, case.ps, case.Cpad,
                                                     case.add_inverse, stream()), "bcos_finalize_explanation_patches")
    torch.cuda.synchronize()
    r = {}
    if wo:
        r["weights"] = wo
    if co:
        r["contrib"] = co
    return r


@pytest.mark.parametrize("case", tc.FIN_CASES, ids=lambda c: c.id)
def test_unpatchify_case_against_fp64_per_element(blib, case):
    lib = blib.load()
    d = device_case(case)
    gp, keep = ptr(d["inp"]["gp"], case.gp_offset)
    assert (gp.value % 16 == 0) == (case.gp_offset == 0)
    first = {}
    for mode in case.outputs:
        r = twice(case, mode, lambda: fin_launch(lib, blib, case, d["inp"], gp, mode))
        judge(case, d, "finalize", r)                        # (a NaN of the padding channels anywhere in an output fails here)
        for k, v in r.items():
            if k in first:
                same_bits(case, mode, {k: v}, {k: first[k]}, "depends on the outputs requested")
            first.setdefault(k, v)


def test_refusals_return_an_error_and_write_nothing(blib):
    lib = blib.load()
    gen = torch.Generator().manual_seed(11)
    src = torch.randn(4096, generator=gen).to(DEV)
    p = C.c_void_p(src.data_ptr())
    outs = [Guarded((4096,)) for _ in range(3)]
    am = Guarded((64,), maxima=True)
    a, b, c = (g.ptr for g in outs)
    st = stream()
    calls = {
        # C % G != 0
        "groupnorm_fwd C=6 G=4": lambda: lib.bcos_groupnorm_fwd(p, p, p, a, b, 2, 8, 6, 4, 1e-5, st),
        "groupnorm_bwd_detached C=6 G=4": lambda: lib.bcos_groupnorm_bwd_detached(p, p, p, a, 2, 8, 6, 4, st),
        "groupnorm_bwd C=6 G=4": lambda: lib.bcos_groupnorm_bwd(p, p, p, p, a, b, 2, 8, 6, 4, st),
        # total % 4, period % 4, total % period
        "add_rows_bcast total=6": lambda: lib.bcos_add_rows_bcast(a, p, 6, 6, st),
        "add_rows_bcast period=6": lambda: lib.bcos_add_rows_bcast(a, p, 24, 6, st),
        "add_rows_bcast total=24 period=16": lambda: lib.bcos_add_rows_bcast(a, p, 24, 16, st),
        # H % patch, W % patch, Cx against add_inverse, Cpad < 6
        "finalize H=10 patch=4": lambda: lib.bcos_finalize_explanation_patches(p, p, p, a, b, 1, 3, 10, 8, 4, 8, 1, st),
        "finalize W=10 patch=4": lambda: lib.bcos_finalize_explanation_patches(p, p, p, a, b, 1, 3, 8, 10, 4, 8, 1, st),
        "finalize Cx=6 add_inverse": lambda: lib.bcos_finalize_explanation_patches(p, p, p, a, b, 1, 6, 8, 8, 4, 8, 1, st),
        "finalize Cx=3 no add_inverse": lambda: lib.bcos_finalize_explanation_patches(p, p, p, a, b, 1, 3, 8, 8, 4, 8, 0, st),
        "finalize Cpad=5": lambda: lib.bcos_finalize_explanation_patches(p, p, p, a, b, 1, 3, 8, 8, 4, 5, 1, st),
        # out2_absmax without out2
        "layernorm_bwd_detached absmax without out2": lambda: lib.bcos_layernorm_bwd_detached(p, p, p, None, None, a, None, am.ptr, 4, 8, st),
        "layernorm_bwd_detached no output": lambda: lib.bcos_layernorm_bwd_detached(p, p, p, None, None, None, None, None, 4, 8, st),
        # rows <= 0
        "layernorm_fwd rows=0": lambda: lib.bcos_layernorm_fwd(p, p, p, a, b, am.ptr, 0, 8, 1e-5, st),
        "layernorm_stats rows=0": lambda: lib.bcos_layernorm_stats(p, p, p, a, b, am.ptr, 0, 8, 1e-5, st),
        "layernorm_bwd_detached rows=-1": lambda: lib.bcos_layernorm_bwd_detached(p, p, p, None, None, a, b, am.ptr, -1, 8, st),
        "layernorm_bwd rows=0": lambda: lib.bcos_layernorm_bwd(p, p, p, p, a, b, 0, 8, st),
        "layernorm_bwd_add rows=-3": lambda: lib.bcos_layernorm_bwd_add(p, p, p, p, p, a, b, -3, 8, st),
        "gelu_gate n=0": lambda: lib.bcos_gelu_gate(p, a, b, 0, st),
        "gelu_bwd n=0": lambda: lib.bcos_gelu_bwd(p, p, a, 0, st),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == blib.BCOS_E_INVAL and lib.bcos_last_error_string(), (what, rc)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs) and am.untouched()
    assert torch.equal(src.cpu(), torch.randn(4096, generator=torch.Generator().manual_seed(11)))
