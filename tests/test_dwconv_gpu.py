"""`-m gpu`: the depthwise 7x7 B-cos convolution (bcos_dwconv7_fwd / bcos_dwconv7_bwd) launched through bcos_hip.ops, every element of
every output judged against the fp64 reference under the per-element bounds of tests/dwconv_cases.py; canaries around every output;
reproducibility across batch positions and calls; adjointness of forward and backward with the scale frozen; B = 1.5 and B = 1."""
import pytest
import torch

import dwconv_cases as DW

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _canvas(shape, extra=256):
    """a NaN buffer with the output in its middle: (buffer, view of the output); the offset keeps the view 16-byte aligned"""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * extra,), float("nan"), device=DEV)
    return buf, buf[extra:extra + n].view(shape), extra


def _guards_intact(buf, extra):
    return bool(buf[:extra].isnan().all()) and bool(buf[-extra:].isnan().all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(name, what, out, ref, bound, worst):
    out = out.cpu()
    assert bool(torch.isfinite(out).all()), (name, what)
    ratio = DW.worst_ratio(out, ref, bound)
    print(f"{what} {name}: worst error / bound = {ratio:.3f}")
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert ratio <= 1.0, (name, what, ratio)


@pytest.mark.parametrize("shape,kind", DW.CASES, ids=[DW.case_id(s, k) for s, k in DW.CASES])
def test_forward_and_backward_per_element(lib, shape, kind):
    from bcos_hip import ops
    inp = DW.make_inputs(shape, kind)
    d = {k: v.to(DEV) for k, v in inp.items()}
    what = DW.case_id(shape, kind)
    worst = {}
    ref = DW.reference_fwd(inp, 2.0)
    bnd = DW.bounds_fwd(ref, 2.0)
    ys = []
    for want_scale, want_norm in ((False, False), (True, False), (False, True), (True, True)):
        buf, y_view, extra = _canvas(shape)
        y, s, n = ops.dwconv7_fwd(d["x"], d["w"], b=2.0, want_scale=want_scale, want_norm=want_norm, out=y_view)
        assert _guards_intact(buf, extra), what
        assert (s is not None) == want_scale and (n is not None) == want_norm
        _check("y", what, y, ref["y"], bnd["y"], worst)
        if s is not None:
            _check("scale", what, s, ref["scale"], bnd["scale"], worst)
        if n is not None:
            _check("norm", what, n, ref["norm"], bnd["norm"], worst)
        if kind == "zero":
            assert bool((y == 0).all()), what
            if n is not None:
                assert torch.equal(n.cpu(), torch.full(shape, 1e-6, dtype=torch.float32).sqrt()), what
        ys.append(y.clone())
    assert all(torch.equal(_bits(ys[0]), _bits(v)) for v in ys[1:]), what          # no output depends on which others were requested
    for use_mul in (False, True):
        for use_add in (False, True):
            refb = DW.reference_bwd(inp, use_mul, use_add)
            buf, g_view, extra = _canvas(shape)
            gx = ops.dwconv7_bwd(d["gy"], d["w"], mul=d["mul"] if use_mul else None, addend=d["addend"] if use_add else None, out=g_view)
            assert _guards_intact(buf, extra), what
            _check("gx", what + f"-mul{int(use_mul)}add{int(use_add)}", gx, refb["gx"], DW.bounds_bwd(refb)["gx"], worst)
    x0 = {k: v.to(DEV) for k, v in inp.items()}
    assert all(torch.equal(_bits(d[k]), _bits(x0[k])) for k in d), what             # inputs are only read


@pytest.mark.parametrize("b", [1.5, 1.0])
def test_other_exponents(lib, b):
    from bcos_hip import ops
    shape = (2, 7, 7, 96)
    inp = DW.make_inputs(shape, "normal")
    ref = DW.reference_fwd(inp, b)
    bnd = DW.bounds_fwd(ref, b)
    worst = {}
    y, s, n = ops.dwconv7_fwd(inp["x"].to(DEV), inp["w"].to(DEV), b=b, want_scale=b != 1.0, want_norm=True)
    _check("y", f"B={b}", y, ref["y"], bnd["y"], worst)
    _check("norm", f"B={b}", n, ref["norm"], bnd["norm"], worst)
    if b != 1.0:
        _check("scale", f"B={b}", s, ref["scale"], bnd["scale"], worst)
    else:
        from bcos_hip.lib import BcosHipError
        with pytest.raises(BcosHipError, match="B = 1"):
            ops.dwconv7_fwd(inp["x"].to(DEV), inp["w"].to(DEV), b=1.0, want_scale=True)


def test_bits_do_not_depend_on_batch_position_or_call(lib):
    from bcos_hip import ops
    shape = (3, 19, 13, 68)
    inp = DW.make_inputs(shape, "normal")
    d = {k: v.to(DEV) for k, v in inp.items()}
    full = ops.dwconv7_fwd(d["x"], d["w"], want_scale=True, want_norm=True)
    again = ops.dwconv7_fwd(d["x"], d["w"], want_scale=True, want_norm=True)
    one = ops.dwconv7_fwd(d["x"][2:3].contiguous(), d["w"], want_scale=True, want_norm=True)
    for a, b, c in zip(full, again, one):
        assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(a[2:3]), _bits(c))
    gfull = ops.dwconv7_bwd(d["gy"], d["w"], mul=d["mul"], addend=d["addend"])
    gagain = ops.dwconv7_bwd(d["gy"], d["w"], mul=d["mul"], addend=d["addend"])
    gone = ops.dwconv7_bwd(d["gy"][2:3].contiguous(), d["w"], mul=d["mul"][2:3].contiguous(), addend=d["addend"][2:3].contiguous())
    assert torch.equal(_bits(gfull), _bits(gagain)) and torch.equal(_bits(gfull[2:3]), _bits(gone))


def test_backward_is_the_adjoint_of_the_linear_forward(lib):
    """<fwd_lin(x), g> = <x, bwd(g)> with the scale frozen (B = 1 forward, no mul), both sums in fp64, within the summed bounds"""
    from bcos_hip import ops
    shape = (2, 19, 13, 64)
    inp = DW.make_inputs(shape, "normal")
    d = {k: v.to(DEV) for k, v in inp.items()}
    lin, _, _ = ops.dwconv7_fwd(d["x"], d["w"], b=1.0)
    gx = ops.dwconv7_bwd(d["gy"], d["w"])
    lhs = float((lin.double() * d["gy"].double()).sum())
    rhs = float((d["x"].double() * gx.double()).sum())
    ref = DW.reference_fwd(inp, 1.0)
    refb = DW.reference_bwd(inp, False, False)
    tol = float((inp["gy"].double().abs() * DW.bounds_fwd(ref, 1.0)["y"]).sum() + (inp["x"].double().abs() * DW.bounds_bwd(refb)["gx"]).sum())
    print(f"adjointness: |lhs - rhs| = {abs(lhs - rhs):.3e}, summed bound {tol:.3e}")
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)
