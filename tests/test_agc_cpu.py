"""Adaptive gradient clipping without a device: the unit rules, the descriptors handed to bcos_agc_clip, a torch emulation of the kernel,
the argument checks of the C ABI and the recipe losses, against what the reference recorded (tests/golden/make_golden_agc.py)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cases():
    meta = json.load(open(os.path.join(GOLDEN, "agc_cases.json")))
    return meta, np.load(os.path.join(GOLDEN, "agc_cases.npz"))


def unit_view(t):
    return t.reshape(1, -1) if t.squeeze().ndim <= 1 else t.reshape(t.shape[0], -1)


def case_inputs(case, data):
    """the seeded inputs of a fixture case: randn * per-unit scale (make_golden_agc.py: case_inputs)"""
    shape, name = case["shape"], case["name"]
    gen = torch.Generator().manual_seed(case["seed"])
    p = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    p = (unit_view(p) * torch.from_numpy(data[f"{name}/p_scale"])[:, None]).reshape(shape)
    g = (unit_view(g) * torch.from_numpy(data[f"{name}/g_scale"])[:, None]).reshape(shape)
    assert [float(p.double().sum()), float(g.double().abs().sum())] == case["checksum"], name
    return p, g


def reference_output(case, data, g):
    """the reference's clipped gradient: recorded in full, or rebuilt bit for bit from its per-unit factor (checked at generation)"""
    name = case["name"]
    if f"{name}/clipped" in data.files:
        return torch.from_numpy(data[f"{name}/clipped"])
    clip = torch.from_numpy(data[f"{name}/clip"])
    gu = unit_view(g.cpu())
    return torch.where(clip[:, None], gu * torch.from_numpy(data[f"{name}/factor"])[:, None], gu).reshape(g.shape)


def emulate_agc_clip(p, g, units, unit_len, clip_factor=0.01, eps=1e-3):
    """torch restatement of bcos_agc_clip on one tensor (fp32): -> clipped gradient, clip decision per unit"""
    pu, gu = p.reshape(units, unit_len), g.reshape(units, unit_len)
    pn, gn = pu.norm(dim=1), gu.norm(dim=1)
    max_norm = pn.clamp(min=eps) * clip_factor
    clip = ~(gn < max_norm)
    scale = max_norm / gn.clamp(min=1e-6)
    return torch.where(clip[:, None], gu * scale[:, None], gu).reshape(g.shape), clip


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------- unit rules
def test_unitwise_norm_matches_the_reference_for_every_case():
    from bcos.training.agc import unitwise_norm
    meta, data = cases()
    for case in meta["cases"]:
        p, g = case_inputs(case, data)
        for t, key in ((p, "p_norm"), (g, "g_norm")):
            ref = torch.from_numpy(data[f"{case['name']}/{key}"]).double()
            got = unitwise_norm(t).reshape(-1).double()
            assert got.shape == ref.shape, case["name"]
            assert float(((got - ref).abs() / ref).max()) <= 1e-6, (case["name"], key)
    for name in ("norm3d", "norm5d_squeezable"):
        got = unitwise_norm(torch.from_numpy(data[f"{name}/x"]))
        ref = torch.from_numpy(data[f"{name}/norm"])
        assert got.shape == ref.shape and float(((got - ref).abs() / ref).max()) <= 1e-6, name
    with pytest.raises(ValueError):
        unitwise_norm(torch.ones(2, 3, 1, 4, 5))


def test_descriptors_follow_the_unit_rules():
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    meta, _ = cases()
    for case in meta["cases"]:
        assert ops.agc_units(case["shape"]) == (case["units"], case["unit_len"]), case["name"]
    expected = {(64, 6, 7, 7): (64, 294), (64, 1, 1, 1): (1, 64), (1, 64, 3, 3): (1, 576), (100, 2048, 1, 1): (100, 2048), (576, 192): (576, 192),
                (1, 192): (1, 192), (192, 1): (1, 192), (2048,): (1, 2048), (): (1, 1), (1,): (1, 1), (1, 1, 1, 1, 7): (1, 7)}
    for shape, want in expected.items():
        assert ops.agc_units(shape) == want, shape
    with pytest.raises(BcosHipError, match="pos_embedding"):
        ops.agc_units((4, 5, 6), "pos_embedding")
    for shape in ((2, 3, 4, 5, 6), (1, 5, 6, 1, 1)):       # (the second squeezes to 2-D but has five dimensions)
        with pytest.raises(ValueError):
            ops.agc_units(shape)


def test_descriptors_reach_the_library_in_one_call(monkeypatch):
    """ResNet-50's 107 parameter tensors: ONE call of bcos_agc_clip (the library splits them into 2 launches), with the units of every
    tensor; gradients that are None are left out; the gradients' version counters move"""
    from bcos_hip import ops, synth
    net = synth.build_bcosified_resnet("resnet50")
    params = [p for p in net.parameters() if p.requires_grad]
    assert len(params) == 107
    for i, p in enumerate(params):
        p.grad = None if i in (5, 50) else torch.zeros_like(p)
    calls = []

    class FakeLib:
        def bcos_agc_clip(self, arr, n, clip_factor, eps, stream):
            calls.append(([(d.p, d.g, d.units, d.unit_len) for d in arr[:n]], clip_factor, eps))
            return 0

    monkeypatch.setattr(ops._l, "load", lambda: FakeLib())
    monkeypatch.setattr(ops, "_agc_refuse", lambda *a: None)          # (CPU tensors stand in for device tensors: host logic only)
    monkeypatch.setattr(ops, "_RAW_STREAM", lambda index: 0)
    versions = [p.grad._version for p in params if p.grad is not None]
    ops.agc_clip(params, clip_factor=0.02, eps=1e-2)
    assert len(calls) == 1
    descs, cf, ep = calls[0]
    assert math.isclose(cf, 0.02) and math.isclose(ep, 1e-2)
    with_grad = [p for p in params if p.grad is not None]
    assert len(descs) == 105
    for d, p in zip(descs, with_grad):
        assert (d[0], d[1]) == (p.data_ptr(), p.grad.data_ptr())
        assert (d[2], d[3]) == ops.agc_units(p.shape)
        assert d[2] * d[3] == p.numel()
    assert all(p.grad._version > v for p, v in zip(with_grad, versions))
    for p in params:
        p.grad = None
    calls.clear()
    ops.agc_clip(params)
    assert calls == []


def test_emulation_reproduces_the_reference():
    meta, data = cases()
    for case in meta["cases"]:
        p, g = case_inputs(case, data)
        out, clip = emulate_agc_clip(p, g, case["units"], case["unit_len"], meta["clip_factor"], meta["eps"])
        ref = reference_output(case, data, g)
        assert rel(out, ref) <= 1e-6, case["name"]
        assert torch.equal(clip, torch.from_numpy(data[f"{case['name']}/clip"])), case["name"]
    assert 0.3 <= meta["clipped_units"] / meta["units"] <= 0.7
    assert float(np.abs(np.concatenate([data[f"{c['name']}/margin"] for c in meta["cases"]])).min()) >= 1e-3
    p, g = torch.from_numpy(data["nan/p"]), torch.from_numpy(data["nan/g"])
    out, clip = emulate_agc_clip(p, g, 8, 40)
    ref = torch.from_numpy(data["nan/clipped"])
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.isnan(ref[3]).all() and torch.isnan(ref[5]).all()
    ok = ~torch.isnan(ref)
    assert float((out[ok] - ref[ok]).abs().max()) <= 1e-6 * float(ref[ok].abs().max())


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_agc_clip_refuses_what_the_kernel_cannot_take():
    from bcos.training.agc import adaptive_clip_grad_
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError

    def param(t, g=None):
        p = torch.nn.Parameter(t)
        p.grad = torch.zeros_like(t) if g is None else g
        return p
    with pytest.raises(BcosHipError, match="HIP device"):
        ops.agc_clip([param(torch.ones(4, 4))])
    with pytest.raises(BcosHipError, match="float32|HIP device"):
        ops.agc_clip([param(torch.ones(4, 4, dtype=torch.float64))])
    with pytest.raises(BcosHipError):
        ops.agc_clip([param(torch.ones(4, 4).t())])
    with pytest.raises(BcosHipError, match="net.w"):
        ops.agc_clip([("net.w", param(torch.ones(4, 4)))])
    with pytest.raises(NotImplementedError):
        adaptive_clip_grad_([param(torch.ones(3))], norm_type=1.0)
    p = torch.nn.Parameter(torch.ones(3))                 # no gradient: nothing to do, nothing loaded
    adaptive_clip_grad_(p)
    adaptive_clip_grad_([p, torch.nn.Parameter(torch.ones(2, 3, 4))])


def test_abi_refuses_malformed_arguments(hip_lib):
    from bcos_hip import lib
    fake = C.c_void_p(1 << 20)

    def call(descs, n=None, clip_factor=0.01, eps=1e-3):
        arr = (lib.AgcTensor * max(len(descs), 1))(*descs) if descs is not None else None
        return hip_lib.bcos_agc_clip(arr, len(descs or []) if n is None else n, clip_factor, eps, None)

    good = (fake, fake, 4, 8)
    assert call(None, n=1) == -22
    assert call([good], n=0) == -22
    assert call([good], n=-1) == -22
    for bad in ((None, fake, 4, 8), (fake, None, 4, 8), (fake, fake, 0, 8), (fake, fake, -1, 8), (fake, fake, 4, 0), (fake, fake, 4, -3),
                (fake, fake, 1 << 62, 4)):
        assert call([good, bad]) == -22, bad
    for cf, ep in ((0.0, 1e-3), (-0.01, 1e-3), (math.inf, 1e-3), (math.nan, 1e-3), (0.01, 0.0), (0.01, -1e-3), (0.01, math.inf), (0.01, math.nan)):
        assert call([good], clip_factor=cf, eps=ep) == -22, (cf, ep)
    # the units of 64 tensors together past int64
    assert call([(fake, fake, (1 << 62), 1)] * 3) == -22
    assert "bcos_agc_clip" in hip_lib.bcos_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------------- losses
def test_recipe_losses_match_the_reference():
    import bcos.modules
    from bcos.modules.losses import BinaryCrossEntropyLoss, UniformOffLabelsBCEWithLogitsLoss
    # re-exported by the package, as the reference's bcos/modules/__init__.py does
    assert bcos.modules.BinaryCrossEntropyLoss is BinaryCrossEntropyLoss
    assert bcos.modules.UniformOffLabelsBCEWithLogitsLoss is UniformOffLabelsBCEWithLogitsLoss
    meta, data = cases()
    logits, labels, dense = (torch.from_numpy(data[k]) for k in ("loss/logits", "loss/labels", "loss/dense"))
    assert len(meta["losses"]) == 14
    for c in meta["losses"]:
        cls = UniformOffLabelsBCEWithLogitsLoss if c["kind"] == "uniform" else BinaryCrossEntropyLoss
        got = float(cls(**c["kwargs"])(logits, labels if c["target"] == "sparse" else dense))
        assert abs(got - c["value"]) <= 1e-6 * abs(c["value"]), c
