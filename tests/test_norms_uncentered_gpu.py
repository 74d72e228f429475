"""`-m gpu`: the uncentered position / group / all norm MODULES against tests/golden/unorms.npz -- the reference's own classes run on the
CPU in fp64 by tests/golden/make_golden_unorms.py -- at the project's per-layer tolerance: 1e-5 of the tensor's maximum (the fixture's
JSON records the reference's own fp32-vs-fp64 distance, at most a tenth of that).  Output, explanation-mode input gradient (through
`explanation_mode()`), training-mode gradients of input, weight and bias, and running_var / num_batches_tracked after the step(s).
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def fx(golden_dir, hip_lib):
    with open(os.path.join(golden_dir, "unorms.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "unorms.npz"))


def _make(name):
    import bcos.modules.norms as norms
    return {
        "pnu_c20": lambda: norms.PositionNormUncentered2d(20),
        "pnu_c6_nobias": lambda: norms.NoBias(norms.PositionNormUncentered2d)(6, eps=1e-6),
        "gnu_g4_c12": lambda: norms.GroupNormUncentered2d(4, 12),
        "gnu_instance_c12": lambda: norms.GNInstanceNormUncentered2d(12),
        "gnu_layer_c12_unaffine": lambda: norms.Unaffine(norms.GNLayerNormUncentered2d)(12),
        "allnorm_train": lambda: norms.AllNormUncentered2d(8),
        "allnorm_train_cma": lambda: norms.AllNormUncentered2d(8, momentum=None),
        "allnorm_eval": lambda: norms.AllNormUncentered2d(8),
    }[name]()


NAMES = ["pnu_c20", "pnu_c6_nobias", "gnu_g4_c12", "gnu_instance_c12", "gnu_layer_c12_unaffine", "allnorm_train", "allnorm_train_cma",
         "allnorm_eval"]


def _close(got, want, tol, what):
    want = torch.as_tensor(want, dtype=torch.float64)
    got = got.detach().double().cpu().reshape(want.shape)
    err = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    print(f"  {what}: max |got - fp64| / max |fp64| = {err:.3g}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("name", NAMES)
def test_module_against_the_reference_record(fx, name):
    from bcos.modules.common import BcosSequential
    meta, arr = fx
    info, tol = meta["modules"][name], meta["tolerance"]
    assert tol == 1e-5 and max(info["fp32_vs_fp64"].values()) <= tol / 10
    m = _make(name)
    assert type(m).__name__ == info["cls"] and m.eps == info["eps"]
    with torch.no_grad():
        for k in ("weight", "bias", "running_var"):
            if f"{name}/{k}" in arr.files:
                getattr(m, k).copy_(torch.from_numpy(arr[f"{name}/{k}"]))
            else:
                assert getattr(m, k, None) is None, k
    m = m.to(DEV).train(info["mode"] == "train")
    x = torch.from_numpy(arr[name + "/x"]).to(DEV)
    cot = torch.from_numpy(arr[name + "/cot"]).to(DEV)
    for s in range(info["steps"] - 1, 0, -1):                     # the earlier steps only move the statistics
        with torch.no_grad():
            m(x * (1 + 0.5 * s) + 0.3 * s)
    stats = {k: v.clone() for k, v in m.state_dict().items()}
    ref = lambda k: arr[f"{name}/f64/{k}"]                         # noqa: E731

    net = BcosSequential(m)
    xe = x.clone().requires_grad_(True)
    with net.explanation_mode():
        assert m.detach
        gx_expl = torch.autograd.grad((net(xe) * cot).sum(), xe)[0]
    assert not m.detach
    _close(gx_expl, ref("gx_expl"), tol, name + " gx_expl")
    m.load_state_dict(stats)

    params = [p for p in (m.weight, m.bias) if p is not None]
    xt = x.clone().requires_grad_(True)
    y = m(xt)
    grads = list(torch.autograd.grad((y * cot).sum(), [xt] + params))
    _close(y, ref("y"), tol, name + " y")
    _close(grads.pop(0), ref("gx"), tol, name + " gx")
    if m.weight is not None:
        _close(grads.pop(0), ref("gw"), tol, name + " gw")
    if m.bias is not None:
        _close(grads.pop(0), ref("gb"), tol, name + " gb")
    assert sorted(info["outputs"]) == sorted(k.split("/")[-1] for k in arr.files if k.startswith(name + "/f64/"))
    if "running_var" in info["outputs"]:
        _close(m.running_var, ref("running_var"), tol, name + " running_var")
        assert float(m.num_batches_tracked) == float(ref("num_batches_tracked"))


def test_functionals_agree_with_the_modules(fx):
    """group_norm_uncentered and all_norm_uncentered_2d are what the modules call: the same bits"""
    import bcos.modules.norms as norms
    from bcos.modules.norms.uncentered_norms.allnorm_uncentered import all_norm_uncentered_2d
    _, arr = fx
    x = torch.from_numpy(arr["gnu_g4_c12/x"]).to(DEV)
    m = norms.GroupNormUncentered2d(4, 12).to(DEV)
    assert torch.equal(m(x), norms.group_norm_uncentered(x, 4, m.weight, m.bias, m.eps))
    x = torch.from_numpy(arr["allnorm_eval/x"]).to(DEV)
    a = norms.AllNormUncentered2d(8).to(DEV).eval()
    assert torch.equal(a(x), all_norm_uncentered_2d(x, a.running_var, a.weight, a.bias, training=False, eps=a.eps))
