"""`-m gpu`: the training-mode gradients of the depthwise 7x7 B-cos convolution (bcos_dwconv7_train_bwd / bcos_dwconv7_wgrad) launched
through bcos_hip.ops, every element of every output judged against the fp64 reference under the per-element bounds of
tests/dwconv_train_cases.py; canaries around gx, gw and the workspace; addend on and off; bit-reproducibility of the weight gradient
across calls and of the input gradient across batch positions; B = 1."""
import pytest
import torch

import dwconv_cases as DW
import dwconv_train_cases as DT

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [DT.case_id(s, k) for s, k in DT.CASES]


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


def _check(name, what, out, ref, bound):
    out = out.cpu()
    assert bool(torch.isfinite(out).all()), (name, what)
    ratio = DT.worst_ratio(out, ref, bound)
    print(f"{what} {name}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, what, ratio)


def _device_inputs(inp, given):
    d = {k: v.to(DEV) for k, v in inp.items()}
    d.update({k: v.float().to(DEV) for k, v in given.items()})
    return d


@pytest.mark.parametrize("shape,kind", DT.CASES, ids=IDS)
def test_both_gradients_per_element(lib, shape, kind):
    from bcos_hip import ops
    inp = DT.make_inputs(shape, kind)
    given = DT.forward_given(inp)
    d = _device_inputs(inp, given)
    before = {k: v.clone() for k, v in d.items()}
    what = DT.case_id(shape, kind)
    for use_add in (False, True):
        ref = DT.reference_gx(inp, given, use_add)
        buf, g_view, extra = _canvas(shape)
        gx = ops.dwconv7_train_bwd(d["gy"], d["x"], d["y"], d["scale"], d["norm"], d["w"], b=2.0, addend=d["addend"] if use_add else None,
                                   out=g_view)
        assert gx.data_ptr() == g_view.data_ptr() and _guards_intact(buf, extra), what
        _check("gx", what + f"-add{int(use_add)}", gx, ref["gx"], DT.bounds_gx(ref)["gx"])
        if kind == "zero" and not use_add:
            assert bool((gx == 0).all()), what
    Cc = shape[3]
    need = ops.dwconv7_wgrad_workspace(*shape)
    assert need == DT.workspace_bytes(shape)
    for mul, gain, tag in ((given["scale"], 2.0, "train"), (given["scale"], 1.0, "constant-scale"), (None, 1.0, "plain"), (None, 0.3, "gain")):
        refw = DT.reference_gw(inp, mul, float(torch.tensor(gain, dtype=torch.float32)))
        wbuf, w_view, wextra = _canvas((7, 7, Cc))
        sbuf, s_view, sextra = _canvas((need // 4,))
        gw = ops.dwconv7_wgrad(d["gy"], d["x"], mul=d["scale"] if mul is not None else None, gain=gain, out=w_view, workspace=s_view)
        assert _guards_intact(wbuf, wextra) and _guards_intact(sbuf, sextra), (what, tag)
        assert bool(torch.isfinite(s_view).all()), (what, tag)                       # every word of the workspace is written
        _check("gw", what + "-" + tag, gw, refw["gw"], DT.bounds_gw(refw, shape)["gw"])
        own = ops.dwconv7_wgrad(d["gy"], d["x"], mul=d["scale"] if mul is not None else None, gain=gain)          # the cached workspace
        assert torch.equal(_bits(own), _bits(gw)), (what, tag)
    assert all(torch.equal(_bits(d[k]), _bits(before[k])) for k in d), what             # inputs are only read


def test_exponent_one_and_refused_exponents(lib):
    """B = 1: glin = gy, no norm term -- the explanation-mode gradient without a multiplier, whose reference and bound are dwconv_cases'"""
    from bcos_hip import ops
    from bcos_hip.lib import BCOS_E_INVAL, BcosHipError
    shape = (2, 7, 7, 96)
    inp = DW.make_inputs(shape, "normal")
    d = {k: v.to(DEV) for k, v in inp.items()}
    for use_add in (False, True):
        ref = DW.reference_bwd(inp, False, use_add)
        gx = ops.dwconv7_train_bwd(d["gy"], None, None, None, None, d["w"], b=1.0, addend=d["addend"] if use_add else None)
        _check("gx", f"B=1 add{int(use_add)}", gx, ref["gx"], DW.bounds_bwd(ref)["gx"])
        assert torch.equal(_bits(gx), _bits(ops.dwconv7_bwd(d["gy"], d["w"], addend=d["addend"] if use_add else None)))
    with pytest.raises(BcosHipError, match="bcos_dwconv7_train_bwd") as err:
        ops.dwconv7_train_bwd(d["gy"], d["x"], d["x"], d["x"], d["x"], d["w"], b=1.5)
    assert err.value.code == BCOS_E_INVAL


def test_weight_gradient_bits_do_not_depend_on_the_call(lib):
    """bit-equal across two calls, and again after a call of another shape (and another workspace content) in between"""
    from bcos_hip import ops
    shape = (3, 17, 9, 68)
    inp = DT.make_inputs(shape, "normal")
    d = _device_inputs(inp, DT.forward_given(inp))
    first = ops.dwconv7_wgrad(d["gy"], d["x"], mul=d["scale"], gain=2.0)
    second = ops.dwconv7_wgrad(d["gy"], d["x"], mul=d["scale"], gain=2.0)
    other_inp = DT.make_inputs((9, 33, 41, 4), "hot")
    od = _device_inputs(other_inp, DT.forward_given(other_inp))
    ops.dwconv7_wgrad(od["gy"], od["x"], mul=od["scale"], gain=2.0)
    third = ops.dwconv7_wgrad(d["gy"], d["x"], mul=d["scale"], gain=2.0)
    assert torch.equal(_bits(first), _bits(second)) and torch.equal(_bits(first), _bits(third))


def test_input_gradient_bits_do_not_depend_on_batch_position(lib):
    from bcos_hip import ops
    shape = (3, 19, 13, 68)
    inp = DT.make_inputs(shape, "normal")
    d = _device_inputs(inp, DT.forward_given(inp))
    args = ("gy", "x", "y", "scale", "norm")
    full = ops.dwconv7_train_bwd(*(d[k] for k in args), d["w"], addend=d["addend"])
    again = ops.dwconv7_train_bwd(*(d[k] for k in args), d["w"], addend=d["addend"])
    one = ops.dwconv7_train_bwd(*(d[k][2:3].contiguous() for k in args), d["w"], addend=d["addend"][2:3].contiguous())
    assert torch.equal(_bits(full), _bits(again)) and torch.equal(_bits(full[2:3]), _bits(one))
