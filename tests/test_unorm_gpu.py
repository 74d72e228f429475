"""`-m gpu`: every case of tests/unorm_cases.py through the six uncentered entry points of csrc/bcos_norms.hip, launched through the C ABI (raw
pointers: the misaligned cases are views that bcos_hip.ops would not pass) and judged PER ELEMENT against the same operation in fp64
(the reference, the bound forms and their constants: tests/unorm_cases.py; stated in include/bcos_hip.h).

Which case reaches which kernel:
  norm_rows_*_kernel<VEC, !CENTERED>    row-* with D in {4, 64, 68, 96, 252, 256} (D = 8 for the second pass of the grid-stride loop)
  norm_rows_*_kernel<!VEC, !CENTERED>   row-* with D in {1, 3, 50, 65, 260, 1000} (D = 5 for the second pass) and the `-mis` cases: D = 68 and
                                        256 with x / gy / y / out one float off a 16-byte boundary
  norm_group_*_kernel<!CENTERED>        grp-*: n = HW C / G of 1, 2, 255, 256, 257 .. 18816; cg of 1, 2, 3, 4, 6, 64; G = 1 .. C

For a case and an entry point:
  * every element of every output is held to its bound; a failure names the form, the worst element and its use of the form in units of u;
  * all four addend / mul2 combinations of the detached gradient, each with out, out2 and both;
  * every optional output is also left out once, and what remains has the same bits;
  * nothing else is written: every output lies between guard bands that must be untouched;
  * every call is made twice and gives the same bits (none of these kernels has atomics).
Refusals return BCOS_E_INVAL and write nothing.

The module prints, per entry point and form, the worst error / bound and the case that produced it; BCOS_UNORM_REPORT=<path> writes the
same as JSON.
"""
import ctypes as C
import json
import os

import pytest
import torch

import unorm_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256

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
    path = os.environ.get("BCOS_UNORM_REPORT")
    if path and rows:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """a tensor inside a larger buffer, `offset` floats behind a 16-byte boundary, with GUARD words on either side that nobody may
    write.  Outputs start as NaN: an element the kernel skipped shows."""

    def __init__(self, shape, offset=0, src=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.offset = n, offset
        self.buf = torch.full((2 * GUARD + n + offset,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD + offset:GUARD + offset + n].view(shape)
        assert self.t.data_ptr() % 16 == (4 * offset) % 16
        if src is not None:
            self.t.copy_(src)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:GUARD + self.offset]).all() and torch.isnan(self.buf[GUARD + self.offset + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


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
        inp = {k: (v.to(DEV) if v is not None else None) for k, v in uc.make_inputs(case).items()}
        ref = uc.reference(case, inp)
        _REF.update(id=case.id, inp=inp, ref=ref, forms=uc.forms(case, inp, ref))
    return _REF


def judge(case, d, entry, outs):
    """outs: output name -> Guarded; every element against its bound"""
    for name, g in outs.items():
        assert g.guards_untouched(), (case.id, entry, name, "write outside the tensor")
        key, form = d["forms"][name]
        v, i = uc.use(g.t, d["ref"][name], form)
        slot = f"{entry}/{key}"
        if slot not in WORST or not v / uc.K[key] <= WORST[slot][0]:
            WORST[slot] = (v / uc.K[key], case.id, name)
        where = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), g.t.shape)) if g.t.dim() else ()
        assert v <= uc.K[key], (f"{case.id} {entry} {name}: form `{key}`, worst element {where} uses {v:.3f} u x form "
                                f"(K = {uc.K[key]:.1f}): got {g.t.reshape(-1)[i].item()!r}, fp64 {d['ref'][name].reshape(-1)[i].item()!r}")


def same_bits(case, entry, a, b, what):
    for name in a:
        assert torch.equal(a[name].t.view(torch.int32), b[name].t.view(torch.int32)), (case.id, entry, name, what)


def twice(case, entry, fn):
    a, b = fn(), fn()
    same_bits(case, entry, a, b, "differs from call to call")
    return a


# ---- launches: each returns {output name: Guarded} ----------------------------------------------------------------------------------
def row_fwd(lib, blib, case, inp, extras=True):
    rows, D, off = case.rows, case.D, int(case.misaligned)
    y = Guarded((rows, D), offset=off)
    rstd = Guarded((rows,)) if extras else None
    (px, kx), (pw, kw), (pb, kb) = ptr(inp["x"], off), ptr(inp["w"]), ptr(inp["b"])
    blib.check(lib.bcos_layernorm_unc_fwd(px, pw, pb, y.ptr, rstd.ptr if extras else None, rows, D, case.eps, stream()),
               "bcos_layernorm_unc_fwd")
    torch.cuda.synchronize()
    return {"y": y, "rstd": rstd} if extras else {"y": y}


def row_bwd_detached(lib, blib, case, inp, outs, addend, mul2):
    rows, D, off = case.rows, case.D, int(case.misaligned)
    key = ("a" if addend else "-") + ("m" if mul2 else "-")
    o = Guarded((rows, D), offset=off) if outs in ("out", "both") else None
    o2 = Guarded((rows, D), offset=off) if outs in ("out2", "both") else None
    (pg, kg), (pw, kw) = ptr(inp["gy"], off), ptr(inp["w"])
    blib.check(lib.bcos_layernorm_unc_bwd_detached(pg, pw, ptr(inp["rstd"])[0], ptr(inp["addend"])[0] if addend else None,
                                                   ptr(inp["mul2"])[0] if mul2 else None, o.ptr if o else None, o2.ptr if o2 else None,
                                                   rows, D, stream()), "bcos_layernorm_unc_bwd_detached")
    torch.cuda.synchronize()
    r = {}
    if o:
        r["out/" + key] = o
    if o2:
        r["out2/" + key] = o2
    return r


def row_bwd(lib, blib, case, inp, addend, want_xr):
    rows, D, off = case.rows, case.D, int(case.misaligned)
    gx, xr = Guarded((rows, D), offset=off), (Guarded((rows, D)) if want_xr else None)
    (pg, kg), (px, kx) = ptr(inp["gy"]), ptr(inp["x"], off)
    blib.check(lib.bcos_layernorm_unc_bwd(pg, px, ptr(inp["w"])[0], ptr(inp["rstd"])[0], ptr(inp["addend"])[0] if addend else None,
                                          gx.ptr, xr.ptr if xr else None, rows, D, stream()), "bcos_layernorm_unc_bwd")
    torch.cuda.synchronize()
    r = {"gx/a" if addend else "gx/-": gx}
    if xr:
        r["xr"] = xr
    return r


@pytest.mark.parametrize("case,op", [(c, op) for c in uc.ROW_CASES for op in uc.OPS], ids=lambda v: v if isinstance(v, str) else v.id)
def test_row_case_against_fp64_per_element(blib, case, op):
    lib = blib.load()
    d = device_case(case)
    inp = d["inp"]
    if op == "fwd":
        full = twice(case, op, lambda: row_fwd(lib, blib, case, inp, True))
        judge(case, d, op, full)
        same_bits(case, op, row_fwd(lib, blib, case, inp, False), {"y": full["y"]}, "y depends on rstd_out")
    elif op == "bwd_detached":
        first = {}
        for outs in ("out", "out2", "both"):
            for a in (False, True):
                for m in (False, True):
                    r = twice(case, op, lambda: row_bwd_detached(lib, blib, case, inp, outs, a, m))
                    judge(case, d, op, r)
                    for k, v in r.items():                        # a tensor does not depend on which other output was asked for
                        if k in first:
                            same_bits(case, op, {k: v}, {k: first[k]}, f"depends on the outputs requested ({outs})")
                        first.setdefault(k, v)
    else:
        plain = twice(case, op, lambda: row_bwd(lib, blib, case, inp, False, True))
        judge(case, d, op, plain)
        same_bits(case, op, row_bwd(lib, blib, case, inp, False, False), {"gx/-": plain["gx/-"]}, "gx depends on xr_out")
        added = twice(case, op + "_add", lambda: row_bwd(lib, blib, case, inp, True, True))
        judge(case, d, op + "_add", added)
        same_bits(case, op, {"xr": added["xr"]}, {"xr": plain["xr"]}, "xr depends on the addend")


def grp_launch(lib, blib, case, inp, op, extra):
    N, HW, Cc, G = case.N, case.HW, case.C, case.G
    shape = (N, HW, Cc)
    pw, pb, prs = ptr(inp["w"])[0], ptr(inp["b"])[0], ptr(inp["rstd"])[0]
    if op == "fwd":
        y, rstd = Guarded(shape), (Guarded((N * G,)) if extra else None)
        blib.check(lib.bcos_groupnorm_unc_fwd(ptr(inp["x"])[0], pw, pb, y.ptr, rstd.ptr if extra else None, N, HW, Cc, G, case.eps,
                                              stream()), "bcos_groupnorm_unc_fwd")
        r = {"y": y, "rstd": rstd} if extra else {"y": y}
    elif op == "bwd_detached":
        gx = Guarded(shape)
        blib.check(lib.bcos_groupnorm_unc_bwd_detached(ptr(inp["gy"])[0], pw, prs, gx.ptr, N, HW, Cc, G, stream()),
                   "bcos_groupnorm_unc_bwd_detached")
        r = {"gx_det": gx}
    else:
        gx, xr = Guarded(shape), (Guarded(shape) if extra else None)
        blib.check(lib.bcos_groupnorm_unc_bwd(ptr(inp["gy"])[0], ptr(inp["x"])[0], pw, prs, gx.ptr, xr.ptr if extra else None, N, HW, Cc, G,
                                              stream()), "bcos_groupnorm_unc_bwd")
        r = {"gx": gx, "xr": xr} if extra else {"gx": gx}
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case,op", [(c, op) for c in uc.GRP_CASES for op in uc.OPS], ids=lambda v: v if isinstance(v, str) else v.id)
def test_group_case_against_fp64_per_element(blib, case, op):
    lib = blib.load()
    d = device_case(case)
    full = twice(case, op, lambda: grp_launch(lib, blib, case, d["inp"], op, True))
    judge(case, d, "grp_" + op, full)
    if op != "bwd_detached":             # without rstd_out / xr_out: the same y / gx
        bare = grp_launch(lib, blib, case, d["inp"], op, False)
        same_bits(case, op, bare, {k: full[k] for k in bare}, "depends on the optional output")


def test_refusals_return_an_error_and_write_nothing(blib):
    lib = blib.load()
    gen = torch.Generator().manual_seed(11)
    src = torch.randn(4096, generator=gen).to(DEV)
    p = C.c_void_p(src.data_ptr())
    outs = [Guarded((4096,)) for _ in range(2)]
    a, b = (g.ptr for g in outs)
    st = stream()
    calls = {
        "layernorm_unc_fwd rows=0": lambda: lib.bcos_layernorm_unc_fwd(p, p, p, a, b, 0, 8, 1e-5, st),
        "layernorm_unc_fwd D=0": lambda: lib.bcos_layernorm_unc_fwd(p, p, p, a, b, 4, 0, 1e-5, st),
        "layernorm_unc_fwd NULL x": lambda: lib.bcos_layernorm_unc_fwd(None, p, p, a, b, 4, 8, 1e-5, st),
        "layernorm_unc_bwd_detached no output": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, p, None, None, None, None, 4, 8, st),
        "layernorm_unc_bwd_detached NULL rstd": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, None, None, None, a, b, 4, 8, st),
        "layernorm_unc_bwd_detached rows=-1": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, p, None, None, a, b, -1, 8, st),
        "layernorm_unc_bwd rows=0": lambda: lib.bcos_layernorm_unc_bwd(p, p, p, p, None, a, b, 0, 8, st),
        "layernorm_unc_bwd NULL x": lambda: lib.bcos_layernorm_unc_bwd(p, None, p, p, None, a, b, 4, 8, st),
        "groupnorm_unc_fwd C=6 G=4": lambda: lib.bcos_groupnorm_unc_fwd(p, p, p, a, b, 2, 8, 6, 4, 1e-5, st),
        "groupnorm_unc_fwd HW=0": lambda: lib.bcos_groupnorm_unc_fwd(p, p, p, a, b, 2, 0, 8, 4, 1e-5, st),
        "groupnorm_unc_bwd_detached C=6 G=4": lambda: lib.bcos_groupnorm_unc_bwd_detached(p, p, p, a, 2, 8, 6, 4, st),
        "groupnorm_unc_bwd_detached G=0": lambda: lib.bcos_groupnorm_unc_bwd_detached(p, p, p, a, 2, 8, 8, 0, st),
        "groupnorm_unc_bwd C=6 G=4": lambda: lib.bcos_groupnorm_unc_bwd(p, p, p, p, a, b, 2, 8, 6, 4, st),
        "groupnorm_unc_bwd NULL x": lambda: lib.bcos_groupnorm_unc_bwd(p, None, p, p, a, b, 2, 8, 8, 4, st),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == blib.BCOS_E_INVAL and lib.bcos_last_error_string(), (what, rc)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs)
    assert torch.equal(src.cpu(), torch.randn(4096, generator=torch.Generator().manual_seed(11)))
