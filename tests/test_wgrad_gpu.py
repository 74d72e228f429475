"""`-m gpu`: every case of tests/wgrad_cases.py with every input family through the three weight-gradient entry points of the C ABI --
bcos_conv2d_wgrad_ordered (wgrad3_kernel + the combine kernels, workspace sized by the plan query), bcos_conv2d_wgrad in mode bf16x3
(wgrad_kernel<true>, atomics) and in mode f32 (wgrad_kernel<false>) -- judged PER ELEMENT against the same sum in fp64 (reference, bound
form and constants: tests/wgrad_cases.py; stated in include/bcos_hip.h).

For a case, a family and an entry point:
  * every element of gw is within K_fam u form -- (K_full + D) u form for the one-signed family `full` on the bf16 matrix pipe, D the
    accumulations behind an element (tests/wgrad_cases.py says why) --; an element whose sum is empty is exactly 0;
  * nothing else is written: gw and the workspace lie inside NaN-filled buffers whose guard bands must stay untouched.  The ordered entry
    point gets a NaN gw (it writes, it does not accumulate) and a NaN workspace; the pad channels of both operands hold NaN;
  * a second ordered call, over the workspace the first one left behind, gives the same bits;
  * the atomics entry point also runs with gw_cin = C + 2: the same values, the pad columns of gw left as they were;
  * where both planners cut the pixels into ONE chunk, the ordered result equals wgrad_kernel<true>'s: both issue the same six matrix
    instructions per 16 pixels, in the same order, on the same fragments (the atomics add each sum to a zero, which changes nothing but
    the sign of a zero: values are compared, not words).
Refusals return non-zero, set the error string and write nothing.
Patch-norm backward (tests/patch_norm_bwd_cases.py): bcos_patch_norm_bwd_add with and without the addend on rectangular geometry, every
kernel variant, per element against fp64 under the derived bound.

The module prints, per entry point, route and family, the worst error / bound and the case that produced it; BCOS_WGRAD_REPORT=<path>
writes the same as JSON.
"""
import ctypes as C
import json
import os

import pytest
import torch

import patch_norm_bwd_cases as pc
import wgrad_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024         # floats on either side of a tensor

WORST = {}           # "entry / route / family" -> (worst error / (K u form), case id)
_REF = {}            # the one (case, family) whose operands and fp64 reference are on the device; never written to


@pytest.fixture(scope="module")
def blib(hip_lib):
    from bcos_hip import lib
    mode = lib.get_contraction_mode()
    yield lib
    lib.set_contraction_mode(mode)
    _REF.clear()
    rows = {k: (round(v, 4), cid) for k, (v, cid) in sorted(WORST.items())}
    if rows:
        print("\nworst error / bound per entry point, route and family:")
        for k, (v, cid) in rows.items():
            print(f"  {k:55s} {v:.4f}  ({cid})")
    path = os.environ.get("BCOS_WGRAD_REPORT")
    if path and rows:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


@pytest.fixture(autouse=True)
def _contraction_mode_restored(blib):
    """the tests switch the process-wide contraction mode; whatever one leaves set -- also when it fails half way -- is put back"""
    mode = blib.get_contraction_mode()
    yield
    blib.set_contraction_mode(mode)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """a float tensor inside a larger NaN-filled buffer: GUARD elements on either side (and `offset` more in front) that nobody may write"""

    def __init__(self, shape, offset=0):
        n = 1
        for s in shape:
            n *= s
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((2 * GUARD + offset + n,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        assert self.t.data_ptr() % 16 == (4 * offset) % 16

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:self.lo]).all() and torch.isnan(self.buf[self.lo + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def device_reference(case, family):
    key = (case.geom, family)
    if _REF.get("key") != key:
        x, gl = (t.to(DEV) for t in wc.make_inputs(case, family))
        _REF.clear()
        _REF.update(key=key, x=x, gl=gl, ref=wc.reference(x, gl, case))
    return _REF["x"], _REF["gl"], _REF["ref"]


def route_name(case):
    p = case.plan
    return f"{wc.kind(case)}/{'direct' if p['direct'] else 'indexed'}"


def record(entry, route, family, value, cid):
    key = f"{entry} / {route} / {family}"
    if key not in WORST or not value <= WORST[key][0]:
        WORST[key] = (value, cid)


def atomics_split(case):
    """(chunks, pixels per chunk) of bcos_conv2d_wgrad (csrc/bcos_train.hip): ~1024 workgroups, chunks of at least 256 pixels, a multiple
    of 32; the tiles are the ordered plan's"""
    p = case.plan
    tiles = p["tiles_co"] * p["tiles_ci"] * p["grid_y"]
    split = max(1, min((1024 + tiles - 1) // tiles, (case.M + 255) // 256, 65535))
    chunk = ((case.M + split - 1) // split + 31) // 32 * 32
    return (case.M + chunk - 1) // chunk, chunk


def run_ordered(lib, blib, x, gl, case, ws):
    gw = Guarded((case.Cout, case.taps, case.C))
    blib.check(lib.bcos_conv2d_wgrad_ordered(ptr(gl), ptr(x), gw.ptr, ws.ptr if ws is not None else None, *case.ints(), stream()),
               "bcos_conv2d_wgrad_ordered")
    torch.cuda.synchronize()
    return gw


PAD_VALUE = 123.0


def run_atomics(lib, blib, x, gl, case, gw_cin):
    gw = Guarded((case.Cout, case.taps, gw_cin))
    gw.t.zero_()                                   # the caller zeroes gw: the entry point accumulates
    gw.t[..., case.C:] = PAD_VALUE
    blib.check(lib.bcos_conv2d_wgrad(ptr(gl), ptr(x), gw.ptr, *case.ints(gw_cin), stream()), "bcos_conv2d_wgrad")
    torch.cuda.synchronize()
    return gw


def judge(gw, ref, case, family, entry, route, steps):
    """`steps`: the accumulations behind an element on the bf16 matrix pipe (0 in mode f32) -- the term of the family `full`"""
    assert gw.guards_untouched(), (case.id, family, entry, "write outside gw")
    k = wc.bound_k(family, steps)
    used = wc.ratio(gw.t[..., :case.C], ref) / k                     # error / bound: <= 1 passes; an error over an empty sum is inf
    print(case.id, family, entry, f"{used:.4f} of the bound (K = {k})")
    record(entry, route, family, used, case.id)
    return used


@pytest.mark.parametrize("case,family", [(c, f) for c in wc.CASES for f in wc.FAMILIES], ids=lambda v: v if isinstance(v, str) else v.id)
def test_case_against_fp64_per_element(blib, case, family):
    lib = blib.load()
    x, gl, ref = device_reference(case, family)
    if case.wgs:
        blib.set_option("wgrad_wgs", case.wgs)     # (put back behind the test by the suite's option fixture)
    plan = blib.wgrad_plan_query(*case.ints())
    assert plan == case.plan
    used = {}

    blib.set_contraction_mode("bf16x3")
    ws = Guarded((plan["ws_floats"],)) if plan["ws_floats"] else None          # NaN throughout: every slab element read was written first
    route = f"{route_name(case)}/combine{plan['combine']}"
    ordered = run_ordered(lib, blib, x, gl, case, ws)
    used["ordered"] = judge(ordered, ref, case, family, "ordered", route, case.steps)
    assert ws is None or ws.guards_untouched(), (case.id, family, "write outside the workspace")
    again = run_ordered(lib, blib, x, gl, case, ws)                            # ... and over a used workspace: the same bits
    assert torch.equal(again.t.view(torch.int32), ordered.t.view(torch.int32)), (case.id, family, "ordered: not the same bits twice")

    for entry, mode in (("atomics_bf16x3", "bf16x3"), ("atomics_f32", "f32")):
        blib.set_contraction_mode(mode)
        a_split, a_chunk = atomics_split(case)
        steps = wc.chain(a_chunk, a_split) if mode == "bf16x3" else 0
        dense = run_atomics(lib, blib, x, gl, case, case.C)
        used[entry] = judge(dense, ref, case, family, entry, route_name(case), steps)
        pitched = run_atomics(lib, blib, x, gl, case, case.C + 2)
        used[entry + "/gw_cin"] = judge(pitched, ref, case, family, entry, route_name(case) + "/gw_cin=C+2", steps)
        assert bool((pitched.t[..., case.C:] == PAD_VALUE).all()), (case.id, family, entry, "pad columns of gw written")
        if mode == "bf16x3" and plan["split"] == 1 and a_split == 1:
            assert torch.equal(dense.t, ordered.t), (case.id, family, "one chunk each: ordered and wgrad_kernel<true> differ")
            assert torch.equal(pitched.t[..., :case.C], ordered.t)
    bad = {k: v for k, v in used.items() if not v <= 1.0}
    assert not bad, (case.id, family, "error / bound", bad)


def test_one_chunk_equality_is_exercised():
    """(no launch: the cases where test_case_against_fp64_per_element compares the two bf16x3 kernels word for word)"""
    same = [c.id for c in wc.CASES if c.plan["split"] == 1 and atomics_split(c)[0] == 1]
    assert {"stem7x7_c6", "pertap_rect_c132", "pertap_c130_scalar", "shortcut_1x1_s2", "tinyQ_multiwrap", "dil2_pad2"} <= set(same)


def test_refusals_write_nothing(blib):
    lib = blib.load()
    case = wc.by_id("fused3x3_c36")
    assert case.plan["split"] > 1
    x, gl, _ = device_reference(case, "normal")
    ws = Guarded((case.plan["ws_floats"],))
    gw = Guarded((case.Cout, case.taps, case.C + 4), offset=0)
    shifted = Guarded((case.Cout, case.taps, case.C), offset=1)
    xs = torch.zeros(x.numel() + 4, device=DEV)[1:1 + x.numel()]               # 4 bytes off a 16-byte boundary
    blib.set_contraction_mode("bf16x3")

    def refused(rc, what, codes):
        torch.cuda.synchronize()
        assert rc in codes, (what, rc)
        assert lib.bcos_last_error_string(), what
        assert gw.untouched() and shifted.untouched() and ws.untouched(), (what, "a refused call wrote")

    inval, nosup = (blib.BCOS_E_INVAL,), (blib.BCOS_E_NOSUP,)
    o = lib.bcos_conv2d_wgrad_ordered
    refused(o(None, ptr(x), gw.ptr, ws.ptr, *case.ints(), stream()), "ordered: NULL glin", inval)
    refused(o(ptr(gl), None, gw.ptr, ws.ptr, *case.ints(), stream()), "ordered: NULL x", inval)
    refused(o(ptr(gl), ptr(x), None, ws.ptr, *case.ints(), stream()), "ordered: NULL gw", inval)
    refused(o(ptr(gl), ptr(x), shifted.ptr, ws.ptr, *case.ints(), stream()), "ordered: misaligned gw", inval)
    refused(o(ptr(gl), ptr(xs), gw.ptr, ws.ptr, *case.ints(), stream()), "ordered: misaligned x", inval)
    refused(o(ptr(gl), ptr(x), gw.ptr, None, *case.ints(), stream()), "ordered: split > 1 without a workspace", inval)
    refused(o(ptr(gl), ptr(x), gw.ptr, ws.ptr, *case.ints(case.C + 4), stream()), "ordered: gw_cin != C", nosup)
    blib.set_contraction_mode("f32")
    refused(o(ptr(gl), ptr(x), gw.ptr, ws.ptr, *case.ints(), stream()), "ordered: mode f32", nosup)
    a = lib.bcos_conv2d_wgrad
    for mode in ("f32", "bf16x3"):
        blib.set_contraction_mode(mode)
        refused(a(None, ptr(x), gw.ptr, *case.ints(), stream()), "atomics: NULL glin", inval)
        refused(a(ptr(gl), ptr(x), None, *case.ints(), stream()), "atomics: NULL gw", inval)
        refused(a(ptr(gl), ptr(xs), gw.ptr, *case.ints(), stream()), "atomics: misaligned x", inval)
        refused(a(ptr(gl), ptr(x), gw.ptr, *case.ints(case.C - 4), stream()), "atomics: gw_cin < C", inval)


# ---- patch-norm backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_patch_norm_bwd_on_rectangular_geometry(blib, case):
    lib = blib.load()
    x, r, addend = pc.make_inputs(case)
    N, H, W = case.shape
    xd, rd = x.to(DEV), r.to(DEV)
    for ad in (addend, None):
        exact, bound, covered = pc.reference(x, r, ad, case)           # (on the CPU: a few hundred pixels)
        add = None
        if ad is not None:
            add = Guarded((N, H, W, case.C), offset=case.addend_offset)
            add.t.copy_(ad)
        elif case.addend_offset:
            continue                                                   # (the misaligned addend IS the case)
        out = Guarded((N, H, W, case.C))
        blib.check(lib.bcos_patch_norm_bwd_add(ptr(xd), ptr(rd), add.ptr if add is not None else None, out.ptr, *case.ints(), stream()),
                   "bcos_patch_norm_bwd_add")
        torch.cuda.synchronize()
        assert out.guards_untouched() and (add is None or add.guards_untouched()), (case.id, "write outside the tensor")
        got = out.t.cpu()
        used = pc.worst(got, (exact, bound))
        print(case.id, "addend" if ad is not None else "no addend", f"{used:.4f} of the bound")
        record("patch_norm_bwd_add", pc.VARIANTS[case.variant][4], "addend" if ad is not None else "no addend", used, case.id)
        assert used <= 1.0, (case.id, used)
        want = ad if ad is not None else torch.zeros_like(got)
        assert torch.equal(got[:, ~covered], want[:, ~covered]), (case.id, "a pixel in no patch must give exactly the addend")
        if add is not None:
            assert torch.equal(add.t.cpu(), ad), (case.id, "the addend was written")
