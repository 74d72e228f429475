"""`-m gpu`: linear functionals of the logits on the device -- the two head kernels through the C ABI against float64 evaluations of the
documented formulas (tests/head_functional_emulation.py), the engines' linearity, the oracle, the reference-recorded maps
(tests/golden/make_golden_relative.py), the invariants and the OursRelative explainer.

Bounds (none taken from what the kernels return):
  * bcos_head_rankm_grad: per element |v - v64| <= (J + 4) 2^-24 sum_j |term_j| -- inv_t / R rounded once, four rounded products per
    term, a chain of J - 1 additions whose partial sums are bounded by the sum of magnitudes (first order in 2^-24); out and out2 carry
    one more rounding for their multiplier: (J + 5) 2^-24 sum_j |term_j| |mul|.  Row maxima: exactly the maximum of what was stored.
  * bcos_head_cotangent_grad: |glin - glin64| <= 3 2^-24 |glin64| (the quotient inv_t / R and two products).
  * linearity: 1e-4 relative to sum_k |c_k| ||W_k|| per image, the project's end-to-end map tolerance; completeness: every W_k is
    complete to 1e-4 |y_k - bias| (test_resnet18_config1_against_reference_golden), so the combination is to 1e-4 sum_k |c_k| |y_k - bias|.
  * oracle / module path with free ReLU gates: 2e-3, the free-gate ResNet-18 floor of test_explainer_api_on_hip_path; the reference's
    recorded maps with its recorded gates replayed: 1e-4 in relative L2 and in the worst element per image.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import head_functional_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
PAD = 64


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def maxabs_per_image(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float(((a - b).abs().flatten(1).amax(1) / b.abs().flatten(1).amax(1).clamp_min(1e-300)).max())


def golden_net(golden_dir):
    from bcos_hip import synth
    meta = json.load(open(os.path.join(golden_dir, "resnet18_e2e.json")))
    data = np.load(os.path.join(golden_dir, "resnet18_e2e.npz"))
    net = synth.build_bcosified_resnet(meta["arch"], seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    return net.to(DEV).eval(), meta, data


class Canary:
    """an output buffer between NaN (float) / -1 (maxima) canaries"""

    def __init__(self, numel, dtype=torch.float32):
        self.numel = numel
        fill = float("nan") if dtype == torch.float32 else -1
        self.buf = torch.full((PAD + numel + PAD,), fill, device=DEV, dtype=dtype)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.buf.element_size() * PAD)

    def take(self):
        lo, hi = self.buf[:PAD], self.buf[PAD + self.numel:]
        ok = (torch.isnan(lo).all() and torch.isnan(hi).all()) if self.buf.dtype == torch.float32 else ((lo == -1).all() and (hi == -1).all())
        assert bool(ok), "written outside the addressed tensor"
        return self.buf[PAD:PAD + self.numel]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- 1. sparse form
def rankm_inputs(N, R, K, D, J, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.rand(N, R, K, generator=g) + 0.01
    w = torch.randn(K, D, generator=g)
    cls = torch.randint(0, K, (N, J), generator=g)
    cls[0, J - 1] = K + 3 if seed % 2 else -1                     # one class outside [0, K) per case: contributes zero
    coef = torch.randn(N, J, generator=g)
    rs = torch.rand(N * R, generator=g) + 0.5
    mul = torch.randn(N * R, D, generator=g)
    mul = (mul.view(torch.int32) & ~1 | torch.randint(0, 2, (N * R, D), generator=g, dtype=torch.int32)).view(torch.float32)     # gate bits
    mul2 = torch.randn(N * R, D, generator=g)
    gate2 = torch.randn(N * R, D, generator=g)
    return [t.to(DEV).contiguous() for t in (cls, coef, scale, w, rs, mul, mul2, gate2)]


def run_rankm(lib, cls, coef, scale, w, rs=None, mul=None, mul2=None, gate2=None, gfm=0, want_out2=False, inv_t=0.5):
    N, R, K = scale.shape
    D, J = w.shape[1], cls.shape[1]
    out, out2 = Canary(N * R * D), Canary(N * R * D) if want_out2 else None
    am, am2 = Canary(N * R, torch.int32), Canary(N * R, torch.int32) if want_out2 else None
    code = lib.bcos_head_rankm_grad(ptr(cls), ptr(coef), J, ptr(scale), ptr(w), ptr(rs), ptr(mul), ptr(mul2), ptr(gate2), gfm, out.ptr,
                                    out2.ptr if out2 else None, am.ptr, am2.ptr if am2 else None, N, R, K, D, inv_t, stream())
    assert code == 0, lib.bcos_last_error_string()
    torch.cuda.synchronize()
    res = [out.take().view(N * R, D), am.take()]
    if want_out2:
        res += [out2.take().view(N * R, D), am2.take()]
    for o, m in zip(res[0::2], res[1::2]):
        assert torch.equal(m, o.abs().amax(1).view(torch.int32)), "row maxima are not the maxima of the stored values"
    return res


@pytest.mark.parametrize("J", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", [(3, 5, 37, 20), (2, 49, 1000, 512)], ids=["small", "many_rows"])
def test_rankm_against_float64(lib, shape, J):
    N, R, K, D = shape
    cls, coef, scale, w, rs, mul, mul2, gate2 = rankm_inputs(N, R, K, D, J, seed=10 * J + N)
    for use_rs in (False, True):
        row_scale = rs if use_rs else None
        v64, mag = E.head_rankm_grad64(cls.cpu(), coef.cpu(), scale.cpu(), w.cpu(), 2.0, row_scale=row_scale.cpu() if use_rs else None)
        v64, mag = v64.to(DEV), mag.to(DEV)
        # bare: out = v
        out, _ = run_rankm(lib, cls, coef, scale, w, row_scale)
        err = ((out.double() - v64).abs() - (J + 4) * U * mag).max()
        print(f"rankm {shape} J={J} row_scale={use_rs}: worst |v - v64| / bound = {float(((out.double() - v64).abs() / ((J + 4) * U * mag).clamp_min(1e-300)).max()):.3f}")
        assert float(err) <= 0
        # out = v * mul; out2 = v * mul2 gated by a tensor
        o, _, o2, _ = run_rankm(lib, cls, coef, scale, w, row_scale, mul=mul, mul2=mul2, gate2=gate2, want_out2=True)
        assert float(((o.double() - v64 * mul.double()).abs() - (J + 5) * U * mag * mul.double().abs()).max()) <= 0
        want2 = v64 * mul2.double() * (gate2 > 0)
        assert float(((o2.double() - want2).abs() - (J + 5) * U * mag * mul2.double().abs()).max()) <= 0
        assert bool((o2[gate2 <= 0] == 0).all())
        # out2 = v gated by the low mantissa bit of mul; out2 = v ungated
        o, _, o2, _ = run_rankm(lib, cls, coef, scale, w, row_scale, mul=mul, gfm=1, want_out2=True)
        bit = (mul.view(torch.int32) & 1).bool()
        assert float(((o.double() - v64 * mul.double()).abs() - (J + 5) * U * mag * mul.double().abs()).max()) <= 0
        assert float(((o2.double() - v64 * bit).abs() - (J + 4) * U * mag).max()) <= 0 and bool((o2[~bit] == 0).all())
        o, _, o2, _ = run_rankm(lib, cls, coef, scale, w, row_scale, want_out2=True)
        assert torch.equal(o, out) and torch.equal(o2, out)
    # the image with the out-of-range class: that term is absent
    keep = [j for j in range(J) if 0 <= int(cls[0, j]) < K]
    assert len(keep) == J - 1
    if keep:
        sub, _ = run_rankm(lib, cls[:1, keep].contiguous(), coef[:1, keep].contiguous(), scale[:1].contiguous(), w, rs[:R].contiguous())
        assert torch.equal(sub, out[:R])
    else:
        assert bool((out[:R] == 0).all())


@pytest.mark.parametrize("shape", [(3, 5, 37, 20), (2, 49, 1000, 512)], ids=["small", "many_rows"])
def test_rankm_with_one_unit_term_is_rank1_bit_for_bit(lib, shape):
    from bcos_hip import lib as blib, ops
    N, R, K, D = shape
    cls, _, scale, w, rs, mul, mul2, gate2 = rankm_inputs(N, R, K, D, 1, seed=3)
    one = torch.ones(N, 1, device=DEV)
    prev = blib.get_contraction_mode()
    blib.set_contraction_mode("f16x2")                             # (the wrappers emit row maxima for the f16x2 contraction only)
    try:
        for kw in (dict(), dict(row_scale=rs, want_absmax=True), dict(row_scale=rs, mul=mul, mul2=mul2, gate2=gate2, want_absmax=True, want_absmax2=True),
                   dict(mul=mul, gate2_from_mul=True, want_absmax=True, want_absmax2=True), dict(mul=mul, want_out2=True)):
            a = ops.head_rank1_grad(cls[:, 0].contiguous(), scale, w, 2.0, **kw)
            b = ops.head_rankm_grad(cls, one, scale, w, 2.0, **kw)
            for x, y in zip(a, b):
                assert (x is None) == (y is None)
                if x is not None:
                    assert torch.equal(x, y), kw.keys()
                    assert (ops.absmax_of(x) is None) == (ops.absmax_of(y) is None)
                    if ops.absmax_of(x) is not None:
                        assert torch.equal(ops.absmax_of(x), ops.absmax_of(y))
    finally:
        blib.set_contraction_mode(prev)


# ---------------------------------------------------------------------------------------------------------------- 2. dense form
@pytest.mark.parametrize("N,R,K,offset", [(3, 5, 37, 0), (2, 49, 1000, 0), (2, 49, 1000, 1), (1, 300, 6, 0)],
                         ids=["K37", "K1000", "K1000_unaligned", "K6_many_rows"])
def test_cotangent_against_float64(lib, N, R, K, offset):
    g = torch.Generator().manual_seed(K + R)
    base = torch.rand(N * R * K + 4, generator=g).to(DEV) + 0.01
    scale = base[offset:offset + N * R * K].view(N, R, K)           # offset 1: rows that are not 16-byte aligned take the scalar reads
    cot = torch.randn(N, K, generator=g).to(DEV)
    cot[0, K // 2] = 0.0
    Kp = (K + 3) // 4 * 4
    glin, am = Canary(N * R * Kp), Canary(N * R, torch.int32)
    code = lib.bcos_head_cotangent_grad(ptr(cot), ctypes.c_void_p(scale.data_ptr()), glin.ptr, am.ptr, N, R, K, 0.5, stream())
    assert code == 0, lib.bcos_last_error_string()
    torch.cuda.synchronize()
    out = glin.take().view(N, R, Kp)
    want = E.head_cotangent_grad64(cot.cpu(), scale.cpu(), 2.0).to(DEV)
    assert bool((out[..., K:] == 0).all())                         # pad columns are written, as zeros
    assert float(((out[..., :K].double() - want).abs() - 3 * U * want.abs()).max()) <= 0
    assert torch.equal(am.take(), out.abs().amax(-1).view(-1).view(torch.int32))
    # without maxima: the same values
    glin2 = Canary(N * R * Kp)
    assert lib.bcos_head_cotangent_grad(ptr(cot), ctypes.c_void_p(scale.data_ptr()), glin2.ptr, None, N, R, K, 0.5, stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(glin2.take().view(N, R, Kp), out)
    # a one-hot cotangent is bcos_head_onehot_grad
    from bcos_hip import ops
    cls = torch.randint(0, K, (N,), generator=g).to(DEV)
    s4 = scale.contiguous().view(N, R, 1, K)
    one = ops.head_cotangent_grad(torch.nn.functional.one_hot(cls, K).float(), s4, 2.0)
    assert torch.equal(one[..., :K], ops.head_onehot_grad(cls, s4, 2.0))


# ---------------------------------------------------------------------------------------------------------------- 3. linearity
def device_functionals(N, K, seed):
    """contrast, 3-term sparse, a dense cotangent on 12 random classes, mean-corrected over all K -> [(name, functional, cot [N, K])]"""
    from bcos_hip.functional import LogitFunctional as LF
    g = torch.Generator().manual_seed(seed)
    pos, neg = torch.randint(0, K, (N,), generator=g), torch.randint(0, K, (N,), generator=g)
    cls3, coef3 = torch.randint(0, K, (N, 3), generator=g), torch.randn(N, 3, generator=g)
    dense = torch.zeros(N, K)
    for n in range(N):
        dense[n, torch.randperm(K, generator=g)[:12]] = torch.randn(12, generator=g)
    tgt = torch.randint(0, K, (N,), generator=g)
    fs = [("contrast", LF.contrast(pos, neg)), ("sparse3", LF.sparse(cls3, coef3)), ("dense12", LF.dense(dense)),
          ("mean_corrected", LF.mean_corrected(tgt, K))]
    return [(n, f, f.checked(N, K).as_dense(K).to(DEV)) for n, f in fs]


def linearity_errors(out_w, fs, single_weights, K, chunk=100):
    """max over images of ||W_f - sum_k c_k W_k|| / sum_k |c_k| ||W_k|| per functional; single_weights(ks) -> [N, len(ks), 6, H, W]"""
    N = out_w.shape[0]
    want = [torch.zeros(out_w.shape[:1] + out_w.shape[2:], device=DEV, dtype=torch.float64) for _ in fs]
    scale = [torch.zeros(N, device=DEV, dtype=torch.float64) for _ in fs]
    for lo in range(0, K, chunk):
        ks = torch.arange(lo, min(lo + chunk, K))
        w = single_weights(ks).double()
        norms = w.flatten(2).norm(dim=2)                                            # [N, chunk]
        for i, (_, _, cot) in enumerate(fs):
            c = cot[:, ks.to(DEV)].double()
            want[i] += torch.einsum("nk,nkchw->nchw", c, w)
            scale[i] += (c.abs() * norms).sum(1)
    return {name: float(((out_w[:, i].double() - want[i]).flatten(1).norm(dim=1) / scale[i]).max()) for i, (name, _, _) in enumerate(fs)}


def completeness_error(x, logits, weights, cot, bias):
    """|sum (x - mean) W_f - (f(logits) - bias sum_k c_k)| relative to sum_k |c_k| |y_k - bias| (see the module docstring)"""
    from oracle import bcos_oracle as O
    mean = torch.tensor(O.IMAGENET_MEAN_ADDINVERSE, device=x.device).view(1, 6, 1, 1)
    lhs = ((x - mean) * weights).double().sum((1, 2, 3))
    y = logits.double() - bias
    return float(((lhs - (cot.double() * y).sum(1)).abs() / (cot.double().abs() * y.abs()).sum(1)).max())


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
def test_resnet_functionals_are_linear_on_the_device(lib, golden_dir, mode):
    from bcos_hip import engine, lib as blib, synth
    net, meta, _ = golden_net(golden_dir)
    x = synth.synthetic_images(3, seed=77, size=64).to(DEV)
    prev = blib.get_contraction_mode()
    blib.set_contraction_mode(mode)
    try:
        eng = engine.ResNetEngine(net)
        K = eng.n_logits()
        fs = device_functionals(3, K, seed=5)
        out = eng.explain_functionals(x, [f for _, f, _ in fs], want_weights=True)
        errs = linearity_errors(out["dynamic_linear_weights"], fs,
                                lambda ks: eng.explain_targets(x, ks, want_weights=True)["dynamic_linear_weights"], K)
        print(f"resnet18 linearity [{mode}]:", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= 1e-4, errs
        bias = float(net.logit_layer.logit_bias)
        assert math.isclose(bias, -math.log(999), rel_tol=1e-6)
        for t, (name, f, cot) in enumerate(fs):
            terms = out["logits"].double() * cot.double()                          # (the mean-corrected value cancels: judged against its terms)
            assert bool(((out["functional_values"][:, t].double() - terms.sum(1)).abs() <= 1e-5 * terms.abs().sum(1)).all())
            ce = completeness_error(x, out["logits"], out["dynamic_linear_weights"][:, t], cot, bias)
            print(f"  completeness [{name}]: {ce:.2e}")
            assert ce <= 1e-4, (name, ce)
            assert rel(out["contribution_maps"][:, t], (x * out["dynamic_linear_weights"][:, t]).sum(1)) <= 1e-5
    finally:
        blib.set_contraction_mode(prev)


@pytest.mark.parametrize("gap_reorder", [True, False], ids=["gap_reorder", "head_behind_gap"])
def test_vit_functionals_are_linear_on_the_device(lib, gap_reorder):
    from bcos_hip import synth, vit_engine
    net = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV).eval()
    net.model.gap_reorder = gap_reorder
    eng = vit_engine.ViTEngine(net)
    assert eng.gap_reorder == gap_reorder
    x = synth.synthetic_images(2, seed=78, size=224).to(DEV)
    K = eng.n_logits()
    fs = device_functionals(2, K, seed=6)
    out = eng.explain_functionals(x, [f for _, f, _ in fs], want_weights=True)

    def singles(ks):
        # the ViT engine has no per-target loop: the classes ride in the batch (an image's bits do not depend on its batch)
        rep = x.repeat_interleave(len(ks), dim=0)
        w = eng.explain(rep, targets=ks.repeat(2))["dynamic_linear_weights"]
        return w.view(2, len(ks), *w.shape[1:])
    errs = linearity_errors(out["dynamic_linear_weights"], fs, singles, K, chunk=50)
    print(f"vit-ti linearity [gap_reorder={gap_reorder}]:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-4, errs
    one = eng.explain(x, functional=fs[0][1])
    assert torch.equal(one["dynamic_linear_weights"], out["dynamic_linear_weights"][:, 0])


# ---------------------------------------------------------------------------------------------------------------- 4. oracle
def test_functionals_against_the_oracle(lib, golden_dir):
    from bcos_hip import engine
    from bcos_hip import synth
    from bcos_hip.functional import LogitFunctional as LF
    from oracle import bcos_oracle as O
    net, meta, _ = golden_net(golden_dir)
    eng = engine.ResNetEngine(net)
    x = synth.synthetic_images(2, seed=77, size=64).to(DEV)                          # the two images of test_explainer_api_on_hip_path
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    t, a, b = [3, 17], [3, 17], [500, 250]
    xr = x.cpu().clone().requires_grad_(True)
    y = O.resnet_logits(sd, xr, meta["arch"], detach=True)
    idx = torch.arange(2)
    (g_mean,) = torch.autograd.grad((y[idx, t] - y.mean(1)).sum(), xr, retain_graph=True)
    (g_con,) = torch.autograd.grad((y[idx, a] - y[idx, b]).sum(), xr)
    out = eng.explain_functionals(x, [LF.mean_corrected(t, 1000), LF.contrast(a, b)], want_weights=True)
    for i, (name, gref) in enumerate((("mean_corrected", g_mean), ("contrast", g_con))):
        rw = rel(out["dynamic_linear_weights"][:, i], gref)
        rm = rel(out["contribution_maps"][:, i], (x.cpu() * gref).sum(1))
        print(f"oracle [{name}]: W relL2 {rw:.2e}, map relL2 {rm:.2e}")
        assert rw <= 2e-3 and rm <= 2e-3, (name, rw, rm)
    assert rel(out["logits"], y) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- 5. reference
def test_functionals_against_the_reference_recorded_maps(lib, golden_dir):
    from bcos_hip import engine, synth
    from bcos_hip.functional import LogitFunctional as LF
    net, meta, data = golden_net(golden_dir)
    rmeta = json.load(open(os.path.join(golden_dir, "relative.json")))
    gold = {"mean": np.load(os.path.join(golden_dir, "relative_mean64.npz"))["mean"],
            "contrast": np.load(os.path.join(golden_dir, "relative_contrast64.npz"))["contrast"]}
    for case in rmeta["cases"]:                                                      # the fixture's own floor: fp32 vs fp64 of the reference
        assert case["contrast_fp32_vs_fp64"]["rel_l2"] <= 3e-5 and case["mean_fp32_vs_fp64"]["rel_l2"] <= 3e-5, case
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"]).to(DEV)[:2].contiguous()
    gates = [torch.from_numpy(np.unpackbits(data[f"gate/{i:02d}"])[: int(np.prod(shp))].reshape(shp).astype(np.float32)).to(DEV)
             for i, shp in enumerate(meta["gate_shapes"])]
    eng = engine.ResNetEngine(net)
    tg = [c["target"] for c in rmeta["cases"]]
    con = [c["contrast"] for c in rmeta["cases"]]
    for name, f in (("mean", LF.mean_corrected(tg, 1000)), ("contrast", LF.contrast([c[0] for c in con], [c[1] for c in con]))):
        out = eng.explain(x, gates=gates, functional=f)                              # the reference's recorded gates do not depend on f
        r, m = rel(out["contribution_map"], gold[name]), maxabs_per_image(out["contribution_map"], gold[name])
        print(f"reference [{name}]: map relL2 {r:.2e}, worst element / peak {m:.2e}")
        assert r <= 1e-4 and m <= 1e-4, (name, r, m)
        assert rel(out["logits"], data["logits"][:2]) <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- 6. invariants
def test_functional_passes_are_deterministic_and_batch_independent(lib, golden_dir):
    from bcos_hip import engine, synth
    from bcos_hip.functional import LogitFunctional as LF
    net, _, _ = golden_net(golden_dir)
    eng = engine.ResNetEngine(net)
    N = 2 * engine._SUBBATCH_MIN * max(1, eng.subbatch_streams // 2)
    x = synth.synthetic_images(N, seed=11, size=64).to(DEV)
    assert eng.n_streams(x) >= 2                                                     # the batch takes the sub-batch streams
    g = torch.Generator().manual_seed(2)
    a, b, t = (torch.randint(0, 1000, (N,), generator=g) for _ in range(3))
    for f in (LF.contrast(a, b), LF.mean_corrected(t, 1000)):
        big = eng.explain(x, functional=f)
        again = eng.explain(x, functional=f)
        for k in ("dynamic_linear_weights", "contribution_map", "functional_value", "logits"):
            assert torch.equal(big[k], again[k]), k
        for i in (0, N - 1):                                                         # (first image of the first, last of the last sub-batch)
            alone = eng.explain(x[i:i + 1].contiguous(), functional=f[i:i + 1])
            assert torch.equal(alone["dynamic_linear_weights"][0], big["dynamic_linear_weights"][i])
            assert torch.equal(alone["contribution_map"][0], big["contribution_map"][i])
        assert "explained_class_idx" not in big and big["functional_value"].shape == (N,)


# ---------------------------------------------------------------------------------------------------------------- 7. OursRelative
def test_ours_relative_end_to_end(lib, golden_dir):
    from bcos_hip import engine, localisation, synth
    from interpretability.explanation_methods import get_explainer
    net, _, _ = golden_net(golden_dir)
    small = synth.synthetic_images(2, seed=77, size=64).to(DEV)
    eng = engine.attach(net)
    fused = get_explainer(net, "OursRelative", "default")
    att = fused.attribute(small, [3, 17])
    sel = fused.attribute_selection(small[:1], [3, 500, 999])
    singles = synth.synthetic_images(4, seed=9, size=32).to(DEV)
    multi = localisation.make_multi_image(singles)
    tg = torch.tensor([[3, 500, 77, 999]])
    ours = localisation.grid_pointing_game(eng, multi, tg, single_shape=32, smooth=5)
    game = localisation.grid_pointing_game(eng, multi, tg, single_shape=32, smooth=5, explainer=fused)
    assert set(game) == set(ours) and all(game[k].shape == ours[k].shape for k in ours)
    assert all(bool(torch.isfinite(v).all()) for v in game.values())
    engine.detach(net)
    plain = get_explainer(net, "OursRelative", "default")
    assert plain._engine() is None
    ref, ref_sel = plain.attribute(small, [3, 17]), plain.attribute_selection(small[:1], [3, 500, 999])
    print(f"OursRelative engine vs modules: attribute {rel(att, ref):.2e}, selection {rel(sel, ref_sel):.2e}")
    assert att.shape == ref.shape == (2, 6, 64, 64) and sel.shape == ref_sel.shape == (3, 6, 64, 64)
    assert rel(att, ref) <= 2e-3 and rel(sel, ref_sel) <= 2e-3
