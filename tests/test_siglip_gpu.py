"""`-m gpu`: bcos_siglip_loss on the device -- per element against the fp64 definition within the bounds derived in
tests/siglip_emulation.py, every combination of wanted gradients, bit-identical repeats, the standing parity against the values recorded
from the reference (tests/golden/siglip.*: loss 1e-5 relative, each gradient 1e-4 of its largest magnitude), the autograd op, the module
and bcos_hip.clip_head.distill_loss behind the training plan.

One exception to the parity figures, stated here: with D = 1 a normalised feature is exactly +-1 and its gradient is identically zero --
the recorded fp64 "gradient" is rounding residue of 1e-294, of which no fp32 result is within 1e-4.  For D = 1 the feature gradients are
held to the derived bounds alone (which demand |g| <= a few ulps of the unprojected gradient)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import siglip_emulation as SE

pytestmark = pytest.mark.gpu
DEV = "cuda"
QUANT = ("loss", "gs", "gt", "gscale", "gbias")


@pytest.fixture(scope="module")
def lib():
    from bcos_hip import lib as L
    L.build()
    return L.load()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.load(open(os.path.join(golden_dir, "siglip.json"))), np.load(os.path.join(golden_dir, "siglip.npz"))


def run_kernel(lib, s, t, scale, bias, *, pos_offset=0, p=0, normalize=False, detach_pow=False, want=(True, True, True, True)):
    """one call of the entry point on fp32 CPU tensors -> dict of fp32 CPU tensors (None where not wanted)"""
    from bcos_hip import lib as L
    s3 = (s if s.dim() == 3 else s.unsqueeze(0)).to(DEV).contiguous()
    td = t.to(DEV).contiguous()
    Lc, N, D = s3.shape
    M = td.shape[0]
    need = C.c_int64(0)
    L.check(lib.bcos_siglip_loss_ws_floats(Lc, N, M, D, C.byref(need)), "ws_floats")
    ws = torch.empty(need.value, device=DEV)
    sc, bi = torch.tensor(float(scale), device=DEV), torch.tensor(float(bias), device=DEV)
    out = dict(loss=torch.full((), float("nan"), device=DEV),
               gs=torch.full_like(s3, float("nan")) if want[0] else None, gt=torch.full_like(td, float("nan")) if want[1] else None,
               gscale=torch.full((), float("nan"), device=DEV) if want[2] else None,
               gbias=torch.full((), float("nan"), device=DEV) if want[3] else None)
    ptr = {k: (None if v is None else C.c_void_p(v.data_ptr())) for k, v in out.items()}
    flags = (L.BCOS_SIGLIP_NORMALIZE if normalize else 0) | (L.BCOS_SIGLIP_DETACH_POW if detach_pow else 0)
    L.check(lib.bcos_siglip_loss(C.c_void_p(s3.data_ptr()), C.c_void_p(td.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(bi.data_ptr()),
                                 ptr["loss"], ptr["gs"], ptr["gt"], ptr["gscale"], ptr["gbias"], C.c_void_p(ws.data_ptr()), ws.numel(),
                                 Lc, N, M, D, pos_offset, p, flags, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bcos_siglip_loss")
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().reshape(s.shape) if k == "gs" else v.cpu()) for k, v in out.items()}


def check_bounds(got, s, t, scale, bias, what, **kw):
    """every wanted output per element within the derived bound of the fp64 definition; -> the worst error / bound ratio"""
    ref = SE.reference64(s, t, scale, bias, **kw)
    bnd = SE.bounds(ref, scale, p=kw.get("p", 0), normalize=kw.get("normalize", False), detach_pow=kw.get("detach_pow", False))
    worst = 0.0
    for q in QUANT:
        if got[q] is None:
            continue
        err = np.abs(got[q].double().numpy() - ref[q])
        ratio = float((err / bnd[q]).max())
        print(f"{what} {q}: worst error / bound {ratio:.3f}")
        assert np.isfinite(ratio) and ratio <= 1.0, (what, q, ratio)
        worst = max(worst, ratio)
    return ref, worst


@pytest.mark.parametrize("k", range(len(SE.CASES)), ids=[c["name"] for c in SE.CASES])
def test_recorded_cases_within_bounds_and_at_parity_with_the_reference(lib, recorded, k):
    meta, data = recorded
    case = meta["cases"][k]
    name = case["name"]
    s, t, log_scale, bias = SE.case_inputs(case)
    scale = float(log_scale.exp())
    kw = dict(pos_offset=case["pos_offset"], p=case["p"], normalize=True, detach_pow=case["detach"])
    got = run_kernel(lib, s, t, scale, float(bias), **kw)
    check_bounds(got, s, t, scale, float(bias), name, **kw)
    # the standing parity against the reference's fp64 record
    b = float(data[f"{name}/f64/loss"])
    d = abs(float(got["loss"]) - b) / abs(b)
    print(f"{name} loss: {d:.2e} of the reference's")
    assert d <= 1e-5, (name, "loss", d)
    for q, key in (("gscale", "glogscale"), ("gbias", "gbias")):
        a = float(got[q]) * (scale if q == "gscale" else 1.0)
        b = float(data[f"{name}/f64/{key}"])
        print(f"{name} {key}: {abs(a - b) / abs(b):.2e}")
        assert abs(a - b) <= 1e-4 * abs(b), (name, key, a, b)
    if case["D"] == 1:
        return                                               # (feature gradients identically zero: the module docstring)
    for q in ("gs", "gt"):
        a = got[q].double().numpy().reshape(-1, case["D"])
        den = float(data[f"{name}/f64/{q}_absmax"])
        if f"{name}/f64/{q}" in data:
            d = float(np.abs(a - data[f"{name}/f64/{q}"]).max()) / den
        else:
            norms = data[f"{name}/f64/{q}_norms"]
            d = max(float(np.abs(a[SE.keep_rows(a.shape[0])] - data[f"{name}/f64/{q}_rows"]).max()) / den,
                    float(np.abs(np.linalg.norm(a, axis=1) - norms).max()) / float(norms.max()))
        print(f"{name} {q}: {d:.2e} of the largest magnitude")
        assert d <= 1e-4, (name, q, d)


def unit_inputs(L, N, M, D, seed):
    """seeded features: the student near its teacher; fp32 unit rows for the runs without NORMALIZE are made from these"""
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(M, D, generator=gen)
    base = t[:N] if M >= N else t.repeat(-(-N // M), 1)[:N]
    s = base.unsqueeze(0) + 0.8 * torch.randn(max(L, 1), N, D, generator=gen)
    return (s if L else s[0]), t


@pytest.mark.parametrize("D", [1, 63, 64, 65, 1024])
def test_shapes_offsets_and_flags_within_bounds(lib, D):
    """N != M with every position of the positives (none, first block, a middle block, the last block), NORMALIZE and DETACH_POW on and
    off, pooled and per-location features, at a row length below / at / above one wave's 64 lanes and at the recipe's 1024"""
    N, M = 3, 7
    worst = 0.0
    for pos_offset, normalize, (L, p, detach) in itertools.product((-1, 0, N, M - N), (False, True), ((0, 0, False), (3, 2, False), (3, 2, True))):
        s, t = unit_inputs(L, N, M, D, seed=100 + D)
        if not normalize:
            s, t = F.normalize(s.double(), dim=-1).float(), F.normalize(t.double(), dim=-1).float()
        kw = dict(pos_offset=pos_offset, p=p, normalize=normalize, detach_pow=detach)
        got = run_kernel(lib, s, t, 10.0, -10.0, **kw)
        worst = max(worst, check_bounds(got, s, t, 10.0, -10.0, f"D={D} {kw} L={L}", **kw)[1])
    print(f"D={D}: worst error / bound over the sweep {worst:.3f}")


def test_more_than_one_lane_chain_step_over_the_columns_and_rows(lib):
    """M = 130 and N = 70: a row's sums over j and the scalars' sums over i take more than one chain step per lane (64 lanes), and the
    batch rows span several workgroups of every pass"""
    s, t = unit_inputs(2, 70, 130, 33, seed=5)
    for pos_offset in (0, 60):
        kw = dict(pos_offset=pos_offset, p=3, normalize=True, detach_pow=False)
        got = run_kernel(lib, s, t, 10.0, -10.0, **kw)
        check_bounds(got, s, t, 10.0, -10.0, f"N=70 M=130 pos_offset={pos_offset}", **kw)


def test_a_zero_teacher_row_and_large_logits(lib):
    """a teacher row of zeros (its gradient is g / 1e-12, no projection) and scale 100 / bias -10 on both tails of the sigmoid"""
    s, t = unit_inputs(0, 4, 6, 40, seed=9)
    t[2] = 0.0
    s[3] = -t[3]                                              # a positive pair at cosine -1: z = -110
    kw = dict(pos_offset=0, p=0, normalize=True, detach_pow=False)
    got = run_kernel(lib, s, t, 100.0, -10.0, **kw)
    assert all(bool(torch.isfinite(got[q]).all()) for q in QUANT)
    check_bounds(got, s, t, 100.0, -10.0, "zero teacher row", **kw)


def test_every_combination_of_wanted_gradients(lib):
    """which gradients are written follows from the pointers alone; what is written does not depend on the others"""
    s, t = unit_inputs(3, 5, 9, 70, seed=11)
    kw = dict(pos_offset=2, p=2, normalize=True, detach_pow=False)
    full = run_kernel(lib, s, t, 10.0, -10.0, **kw)
    for want in itertools.product((False, True), repeat=4):
        got = run_kernel(lib, s, t, 10.0, -10.0, want=want, **kw)
        assert torch.equal(got["loss"], full["loss"]), want
        for q, w in zip(("gs", "gt", "gscale", "gbias"), want):
            assert (got[q] is None) if not w else torch.equal(got[q], full[q]), (want, q)


@pytest.mark.parametrize("name", ["pooled_n64_d1024_s10", "unpool_l49_n8_d63_p3_grad"])
def test_two_calls_are_bit_identical(lib, name):
    case = SE.case_by_name(name)
    s, t, log_scale, bias = SE.case_inputs(case)
    kw = dict(pos_offset=0, p=case["p"], normalize=True, detach_pow=case["detach"])
    a = run_kernel(lib, s, t, float(log_scale.exp()), float(bias), **kw)
    b = run_kernel(lib, s, t, float(log_scale.exp()), float(bias), **kw)
    for q in QUANT:
        assert torch.equal(a[q], b[q]), q


def test_autograd_op_scales_by_grad_output_and_feeds_scale_and_bias(lib):
    """ops.siglip_loss: the gradients of the one call, times grad_output (exactly, for a power of two), to s, t and to scale / bias
    tensors that require them; numbers for scale / bias take no gradient"""
    from bcos_hip import ops
    s, t = unit_inputs(3, 5, 5, 70, seed=13)
    raw = run_kernel(lib, s, t, 10.0, -10.0, p=2, normalize=True)
    outs = {}
    for mult in (1.0, 4.0):
        sd, td = s.to(DEV).requires_grad_(True), t.to(DEV).requires_grad_(True)
        scale = torch.tensor(10.0, device=DEV, requires_grad=True)
        bias = torch.tensor([-10.0], device=DEV, requires_grad=True)
        loss = ops.siglip_loss(sd, td, scale, bias, p=2, normalize=True)
        assert loss.shape == () and bias.grad is None
        (loss * mult).backward()
        assert bias.grad.shape == (1,)
        outs[mult] = [v.detach().cpu() for v in (loss, sd.grad, td.grad, scale.grad, bias.grad[0])]
    for a, q in zip(outs[1.0], QUANT):
        assert torch.equal(a, raw[q]), q
    for a, b in zip(outs[1.0][1:], outs[4.0][1:]):
        assert torch.equal(a * 4.0, b)
    sd = s.to(DEV).requires_grad_(True)
    ops.siglip_loss(sd, t.to(DEV), 10.0, -10.0, p=2, normalize=True).backward()        # numbers: constants; the teacher frozen
    assert torch.equal(sd.grad.cpu(), raw["gs"])
    with pytest.raises(ops.BcosHipError):
        ops.siglip_loss(s.to(DEV), t.to(DEV), 10.0, -10.0, p=1.5)


def test_module_on_device_tensors_takes_the_fused_op(lib, recorded):
    """SigLipLoss on float32 device tensors: the bits of ops.siglip_loss (no NORMALIZE: the features arrive normalised), explanation mode
    as DETACH_POW, a learnable scale through .exp(); fp64 device tensors take the torch form"""
    from bcos.modules.losses import SigLipLoss, siglip_loss_torch
    case = SE.case_by_name("unpool_l4_n5_d65_p2_grad")
    s, t, log_scale, bias = SE.case_inputs(case)
    us, ut = F.normalize(s, dim=-1), F.normalize(t, dim=-1)
    crit = SigLipLoss()
    scale = float(log_scale.to(DEV).exp())                   # the device's fp32 exp
    for detach in (False, True):
        crit.set_explanation_mode(detach)
        raw = run_kernel(lib, us, ut, scale, float(bias), p=2, detach_pow=detach)
        ud = us.to(DEV).requires_grad_(True)
        ls = log_scale.to(DEV).requires_grad_(True)
        loss = crit(ud, ut.to(DEV), ls.exp(), bias.to(DEV), cos_scaling=2)
        loss.backward()
        assert torch.equal(loss.detach().cpu(), raw["loss"]) and torch.equal(ud.grad.cpu(), raw["gs"])
        assert abs(float(ls.grad) - float(raw["gscale"]) * scale) <= 1e-6 * abs(float(ls.grad))
        assert torch.equal(crit(us.to(DEV), ut.to(DEV), torch.tensor(scale), bias, cos_scaling=2).cpu(), raw["loss"])     # host scalars: constants
    l64 = crit(us.double().to(DEV), ut.double().to(DEV), 10.0, -10.0, cos_scaling=2)
    assert l64.dtype == torch.float64
    assert abs(float(l64) - float(siglip_loss_torch(us.double(), ut.double(), 10.0, -10.0, cos_scaling=2, detach=True))) <= 1e-12 * abs(float(l64))


def _distill_torch(out, teacher, cos_power):
    """the step's objective as torch operators on the same device (trainer.py:673-707)"""
    from bcos.modules.losses import siglip_loss_torch
    return siglip_loss_torch(F.normalize(out, dim=-1), F.normalize(teacher, dim=-1), 10.0, -10.0, cos_scaling=cos_power if out.dim() == 3 else 0)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("head", ["attnpool_plan", "attn_unpool_layers"])
def test_distill_loss_behind_the_training_step_of_the_small_clip_tower(lib, golden_dir, head):
    """clip_head.distill_loss behind one train()-mode step of the clip_tiny fixture network -- the pooled head through the training plan,
    the attn_unpool head (cos_power 2) on the module path -- against the same step with the torch-operator form of the loss on the same
    device: loss and every parameter gradient within the step tolerance of the CLIP step tests (1e-4), and the fused step's weight
    gradients identical from one step to the next"""
    from bcos_hip import clip_head, engine, synth
    from bcosify import BcosifyNetwork
    meta = json.load(open(os.path.join(golden_dir, "clip_tiny_train_step.json")))
    data = np.load(os.path.join(golden_dir, "clip_tiny_train_step.npz"))
    if head == "attnpool_plan":
        net = synth.build_bcosified_clip_resnet(meta["layers"], meta["output_dim"], meta["heads"], meta["width"], seed=meta["weight_seed"])
    else:
        std = synth.standard_clip_resnet(meta["layers"], meta["output_dim"], meta["heads"], meta["width"], meta["weight_seed"])
        net = synth.finish_clip_conversion(BcosifyNetwork(std, dict(synth.clip_model_config(), attn_unpool=True), add_channels=True,
                                                          logit_layer=False)).eval()
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    net = net.to(DEV)
    x = synth.synthetic_images(4, seed=meta["image_seed"], size=meta["size"]).to(DEV)
    teacher = torch.randn(4, meta["output_dim"], generator=torch.Generator().manual_seed(77)).to(DEV)
    if head == "attnpool_plan":
        engine.attach(net)
    net.train()
    params = [p for p in net.parameters() if p.requires_grad]

    def step(loss_of):
        out = net(x)
        assert out.dim() == (2 if head == "attnpool_plan" else 3), out.shape
        loss = loss_of(out)
        return loss.detach(), torch.autograd.grad(loss, params)

    fused = step(lambda o: clip_head.distill_loss(o, teacher, cos_power=2))
    again = step(lambda o: clip_head.distill_loss(o, teacher, cos_power=2))
    plain = step(lambda o: _distill_torch(o, teacher, 2))
    if head == "attnpool_plan":
        engine.detach(net)
    net.eval()
    assert _rel(fused[0], plain[0]) <= 1e-4, (float(fused[0]), float(plain[0]))
    worst = max(_rel(a, b) for a, b in zip(fused[1], plain[1]))
    print(f"{head}: loss {float(fused[0]):.6f} vs {float(plain[0]):.6f}, worst parameter-gradient distance {worst:.2e}")
    assert worst <= 1e-4, worst
    assert torch.equal(fused[0], again[0]) and all(torch.equal(a, b) for a, b in zip(fused[1], again[1]))


@pytest.mark.parametrize("unpool", [False, True])
def test_distill_loss_with_learnable_scale_and_bias(lib, unpool):
    """the recipe's non-fixed variant: model.logit_scale (the logarithm; .exp() under autograd) and model.logit_bias as parameters --
    loss and all three gradients against the torch-operator form on the same device"""
    from bcos.modules.losses import siglip_loss_torch
    from bcos_hip import clip_head
    s, t = unit_inputs(5 if unpool else 0, 6, 6, 96, seed=21)
    outs = []
    for fused in (True, False):
        sd = s.to(DEV).requires_grad_(True)
        log_scale = torch.tensor(float(np.log(10.0)), device=DEV, requires_grad=True)
        bias = torch.tensor(-10.0, device=DEV, requires_grad=True)
        if fused:
            loss = clip_head.distill_loss(sd, t.to(DEV), cos_power=3, logit_scale=log_scale, logit_bias=bias)
        else:
            loss = siglip_loss_torch(F.normalize(sd, dim=-1), F.normalize(t.to(DEV), dim=-1), log_scale.exp(), bias, cos_scaling=3 if unpool else 0)
        loss.backward()
        outs.append((loss.detach(), sd.grad, log_scale.grad, bias.grad))
    for a, b, what in zip(outs[0], outs[1], ("loss", "gs", "glogscale", "gbias")):
        assert _rel(a, b) <= 1e-5, (what, _rel(a, b))
