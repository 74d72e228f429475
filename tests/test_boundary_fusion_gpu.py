"""`-m gpu`: bcos_boundary_conv3_grad (include/bcos_hip.h) against the two bcos_tapconv_ops launches it replaces -- bit for bit, through
the C ABI -- and the engine with the fusion on and off.

The reference is the library's own two-launch path (boundary launch: mul / addend / out2 with BCOS_EPI_GATE2_FROM_MUL; conv3 input
gradient: mul or the rebuilt multiplier; with and without the mul2 of a shortcut convolution below), so every comparison is torch.equal: out2, g3, the per-pixel maxima of both and the per-image
range of g3's maxima.  Every output sits between NaN / -1 canaries that must survive.  Shapes (rows = N P Q against the 64-row tile):
3 x 9 x 7 = 189 rows (a tile holds rows of two images, the last tile is ragged), 1 x 5 x 5 = 25 (less than a tile), 2 x 19 x 10 = 380
(several tiles)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 256
C1, C4 = 64, 256
SHAPES = [(3, 9, 7), (1, 5, 5), (2, 19, 10)]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


class Canary:
    """an output buffer between NaN (float) / -1 (maxima) canaries, itself filled with the canary value (or zeros)"""

    def __init__(self, numel, dtype=torch.float32, zero=False):
        self.numel = numel
        self.fill = float("nan") if dtype == torch.float32 else -1
        self.buf = torch.full((PAD + numel + PAD,), self.fill, device=DEV, dtype=dtype)
        if zero:
            self.buf[PAD:PAD + numel] = 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * PAD

    def take(self):
        lo, hi = self.buf[:PAD], self.buf[PAD + self.numel:]
        for edge in (lo, hi):
            assert bool(torch.isnan(edge).all() if edge.dtype == torch.float32 else (edge == -1).all()), "canary overwritten"
        return self.buf[PAD:PAD + self.numel].clone()


def make_inputs(N, P, Q, seed):
    """seeded operands: gradients over several decades, multipliers with open and closed gates in their low bit, all-zero rows"""
    gen = torch.Generator().manual_seed(seed)
    M = N * P * Q
    rnd = lambda *s: torch.randn(*s, generator=gen)
    g1 = rnd(M, C1) * torch.exp2(torch.randint(-12, 4, (M, 1), generator=gen).float())
    addend = rnd(M, C4) * torch.exp2(torch.randint(-10, 2, (M, 1), generator=gen).float())
    t3 = rnd(M, C4).abs() + 0.05
    bits = t3.view(torch.int32)
    open_ = torch.rand(M, C4, generator=gen) < 0.6
    t3 = torch.where(open_, bits | 1, torch.zeros_like(bits)).view(torch.float32)          # open: odd low bit; closed: exactly 0
    even = torch.rand(M, C4, generator=gen) < 0.1                                           # a nonzero multiplier with an EVEN low bit: closed for out2
    t3 = torch.where(even & open_, (t3.view(torch.int32) & ~1), t3.view(torch.int32)).view(torch.float32)
    zero_rows = torch.arange(M) % 11 == 3
    g1[zero_rows] = 0
    addend[zero_rows] = 0
    if M > 40:
        t3[40] = 0                                                                          # a row whose G is zero while v is not
    w1t = rnd(C4, 1, 1, C1) * 0.2 * torch.exp2(torch.randint(-3, 3, (C4, 1, 1, 1), generator=gen).float())
    w3t = rnd(C1, 1, 1, C4) * 0.1 * torch.exp2(torch.randint(-3, 3, (C1, 1, 1, 1), generator=gen).float())
    t2 = rnd(M, C1).abs() * (torch.rand(M, C1, generator=gen) < 0.7)                       # stored multiplier, or kept activation (zeros: closed)
    norm = rnd(M).abs() + 0.1
    csc = rnd(C1) * 0.5 + 1.0
    csh = rnd(C1) * 0.1
    td = rnd(M, C4) * 0.5 + 1.0                                                             # multiplier of a shortcut convolution (out2 = v td gate)
    d = lambda t: t.to(DEV).contiguous()
    return dict(g1=d(g1), addend=d(addend), t3=d(t3), w1t=d(w1t), w3t=d(w3t), t2=d(t2), norm=d(norm), csc=d(csc), csh=d(csh), td=d(td))


def geom(N, P, Q, cin, cout):
    from bcos_hip import lib as L
    g = L.TapconvGeom()
    for f, _ in L.TapconvGeom._fields_:
        setattr(g, f, 0)
    for k, v in dict(N=N, H=P, W=Q, C=cin, P=P, Q=Q, in_sh=1, in_sw=1, dstep_h=1, dstep_w=1, TH=1, TW=1, OH=P, OW=Q, out_sh=1, out_sw=1,
                     Cout=cout).items():
        setattr(g, k, v)
    return g


def run_pair(lib, x, N, P, Q, rebuild, optional, mul2):
    """the two launches of the parent: -> dict of outputs"""
    from bcos_hip import lib as L, ops
    M = N * P * Q
    am1 = torch.empty(M, device=DEV, dtype=torch.int32)
    L.check(lib.bcos_rows_absmax(x["g1"].data_ptr(), am1.data_ptr(), M, C1, C1, None), "rows_absmax")
    G = Canary(M * C4)
    amG = Canary(M, torch.int32, zero=True)
    out2, am2 = Canary(M * C4), Canary(M, torch.int32, zero=optional)
    o = L.Operands()
    o.a, o.a_absmax, o.wt, o.contraction = x["g1"].data_ptr(), am1.data_ptr(), x["w1t"].data_ptr(), L.CONTRACT_F16X2
    o.wt_f16x2 = x["img1"].data_ptr()
    e = L.Epilogue()
    e.addend, e.mul, e.out, e.out2, e.out_absmax = x["addend"].data_ptr(), x["t3"].data_ptr(), G.ptr, out2.ptr, amG.ptr
    if optional:
        e.out2_absmax = am2.ptr
    if mul2:
        e.mul2 = x["td"].data_ptr()
    e.b, e.flags = 2.0, L.BCOS_EPI_GATE2_FROM_MUL
    L.check(lib.bcos_tapconv_ops(C.byref(o), C.byref(geom(N, P, Q, C1, C4)), C.byref(e), None), "boundary launch")
    g3, am3 = Canary(M * C1), Canary(M, torch.int32, zero=optional)
    imx, imn = Canary(N, torch.int32, zero=optional), Canary(N, torch.int32, zero=optional)
    o = L.Operands()
    o.a, o.a_absmax, o.wt, o.contraction = G.ptr, amG.ptr, x["w3t"].data_ptr(), L.CONTRACT_F16X2
    o.wt_f16x2 = x["img3"].data_ptr()
    e = L.Epilogue()
    e.mul, e.out = x["t2"].data_ptr(), g3.ptr
    e.b = 2.0
    if rebuild:
        e.mul_norm, e.mul_csc, e.mul_csh, e.flags = x["norm"].data_ptr(), x["csc"].data_ptr(), x["csh"].data_ptr(), L.BCOS_EPI_MUL_FROM_ACT
    if optional:
        e.out_absmax, e.out_imgmax, e.out_imgmin_c = am3.ptr, imx.ptr, imn.ptr
    L.check(lib.bcos_tapconv_ops(C.byref(o), C.byref(geom(N, P, Q, C4, C1)), C.byref(e), None), "conv3 gradient launch")
    torch.cuda.synchronize()
    G.take(), amG.take()
    return dict(out2=out2.take(), am2=am2.take(), g3=g3.take(), am3=am3.take(), imx=imx.take(), imn=imn.take())


def boundary_args(x, N, P, Q, rebuild, optional, mul2, outs):
    from bcos_hip import lib as L
    a = L.BoundaryConv3()
    a.g1, a.g1_absmax, a.w1_f16x2 = x["g1"].data_ptr(), x["am1"].data_ptr(), x["img1"].data_ptr()
    a.addend, a.t3, a.out2 = x["addend"].data_ptr(), x["t3"].data_ptr(), outs["out2"].ptr
    a.w3_f16x2, a.t2, a.g3 = x["img3"].data_ptr(), x["t2"].data_ptr(), outs["g3"].ptr
    if mul2:
        a.mul2 = x["td"].data_ptr()
    if rebuild:
        a.mul_norm, a.mul_csc, a.mul_csh = x["norm"].data_ptr(), x["csc"].data_ptr(), x["csh"].data_ptr()
    if optional:
        a.out2_absmax, a.g3_absmax, a.g3_imgmax, a.g3_imgmin_c = outs["am2"].ptr, outs["am3"].ptr, outs["imx"].ptr, outs["imn"].ptr
    a.N, a.PQ, a.C1, a.C4, a.kh, a.kw, a.stride, a.contraction, a.b = N, P * Q, C1, C4, 1, 1, 1, L.CONTRACT_F16X2, 2.0
    return a


def run_fused(lib, x, N, P, Q, rebuild, optional, mul2):
    from bcos_hip import lib as L
    M = N * P * Q
    x["am1"] = torch.empty(M, device=DEV, dtype=torch.int32)
    L.check(lib.bcos_rows_absmax(x["g1"].data_ptr(), x["am1"].data_ptr(), M, C1, C1, None), "rows_absmax")
    outs = dict(out2=Canary(M * C4), am2=Canary(M, torch.int32, zero=optional), g3=Canary(M * C1), am3=Canary(M, torch.int32, zero=optional),
                imx=Canary(N, torch.int32, zero=optional), imn=Canary(N, torch.int32, zero=optional))
    a = boundary_args(x, N, P, Q, rebuild, optional, mul2, outs)
    L.check(lib.bcos_boundary_conv3_grad(C.byref(a), None), "bcos_boundary_conv3_grad")
    torch.cuda.synchronize()
    return {k: v.take() for k, v in outs.items()}


_INPUTS = {}


def inputs(shape):
    """operands and weight images of a shape, made once and never modified"""
    from bcos_hip import ops
    if shape not in _INPUTS:
        x = make_inputs(*shape, seed=1234 + shape[1])
        x["img1"] = ops.split_weights_f16x2(x["w1t"].view(C4, C1))
        x["img3"] = ops.split_weights_f16x2(x["w3t"].view(C1, C4))
        _INPUTS[shape] = x
    return _INPUTS[shape]


@pytest.mark.parametrize("mul2", [False, True], ids=["identity_below", "shortcut_conv_below"])
@pytest.mark.parametrize("optional", [True, False], ids=["maxima", "plain"])
@pytest.mark.parametrize("rebuild", [False, True], ids=["stored_t2", "rebuilt_t2"])
@pytest.mark.parametrize("shape", SHAPES, ids=["3x9x7", "1x5x5", "2x19x10"])
def test_fused_call_equals_the_two_launches(lib, shape, rebuild, optional, mul2):
    N, P, Q = shape
    x = dict(inputs(shape))
    ref = run_pair(lib, x, N, P, Q, rebuild, optional, mul2)
    got = run_fused(lib, x, N, P, Q, rebuild, optional, mul2)
    assert not torch.isnan(ref["g3"]).any() and not torch.isnan(ref["out2"]).any()
    assert float(ref["g3"].abs().max()) > 0 and float(ref["out2"].abs().max()) > 0
    assert bool((ref["out2"] == 0).any()) and bool((ref["g3"].view(-1, C1).abs().amax(1) == 0).any()), "closed gates and zero rows are in the case"
    for k in ("out2", "g3", "am2", "am3", "imx", "imn"):
        assert torch.equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))
    if optional:
        # the maxima are the maxima of what was stored
        assert torch.equal(got["am3"], got["g3"].view(-1, C1).abs().amax(1).view(torch.int32))
        assert torch.equal(got["am2"], got["out2"].view(-1, C4).abs().amax(1).view(torch.int32))
    else:
        for k in ("am2", "am3", "imx", "imn"):          # arrays the call was not given keep their fill
            assert bool((got[k] == -1).all()), k


def _tiny_resnet50(size=64, batch=4):
    from bcos_hip import synth
    net = synth.build_bcosified_resnet("resnet50").to(DEV)
    x = synth.synthetic_images(batch, size=size).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, x)
    return net, x


def test_engine_fusion_on_off_equal_and_counted():
    """ResNet-50 at 64 x 64 (stage 1 is 16 x 16), batch 4: the explanation with the fused call equals the one with the pair of launches, and
    the fused call ran for the outputs of layer1.0 and layer1.1 -- twice per pass."""
    from bcos_hip import engine
    net, x = _tiny_resnet50()
    eng = engine.attach(net)
    res = {}
    for on in (False, True):
        engine.set_boundary_fusion(on)
        try:
            engine.BOUNDARY_FUSION_CALLS = 0
            out = eng.explain(x)
            torch.cuda.synchronize()
            res[on] = ({k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, engine.BOUNDARY_FUSION_CALLS)
        finally:
            engine.set_boundary_fusion(None)
    passes = max(1, eng.n_streams(x))
    assert res[False][1] == 0 and res[True][1] == 2 * passes, (res[False][1], res[True][1], passes)
    for k in ("logits", "dynamic_linear_weights", "contribution_map"):
        assert k in res[True][0], sorted(res[True][0])
        assert torch.equal(res[True][0][k], res[False][0][k]), k
    # the per-contraction timing records of the roofline (ops.KERNEL_TIMING): the fused launch books its two contractions -- the same
    # number of records, flops and (one [M, 256] write and read-back less) bytes as the pair, time on ONE of the two records
    from bcos_hip import ops
    recs = {}
    for on in (False, True):
        engine.set_boundary_fusion(on)
        ops.KERNEL_TIMING = []
        try:
            eng.explain(x)
            torch.cuda.synchronize()
            recs[on] = ops.KERNEL_TIMING
        finally:
            ops.KERNEL_TIMING = None
            engine.set_boundary_fusion(None)
    assert len(recs[True]) == len(recs[False]) and sum(r[2] for r in recs[True]) == sum(r[2] for r in recs[False])
    M = x.shape[0] * 16 * 16
    assert sum(r[3] for r in recs[False]) - sum(r[3] for r in recs[True]) == 2 * passes * 2 * M * 256 * 4
    markers = [r for r in recs[True] if r[4] is None and r[2] == 0 and r[3] == 0]
    assert len(markers) == 2 * passes and all(r[0].elapsed_time(r[1]) == 0 for r in markers)
