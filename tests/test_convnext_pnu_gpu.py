"""`-m gpu`: the native B-cos ConvNeXt built with NoBias(PositionNormUncentered2d) against the fixtures recorded from the reference
(tests/golden/make_golden_convnext_pnu.py): module path and fused plan (bcos_hip/convnext_engine.py) against the fp64 record, the plan's
launch list, one recorded train()-mode step, and attach() still refusing the `_bnu` model.

Bounds (the project's model tolerances, those of test_convnext_gpu.py and test_convnext_train_gpu.py): logits within 1e-4 of the fp64
record (absolute: the logits are O(1)), class indices exact, W(x) and the contribution maps within 1e-4 of their per-image maximum; the
training step in relative L2, 1e-5 for the logits and the loss, 1e-4 for the input gradient and every parameter gradient.  The
reference's own fp32-vs-fp64 distance, in the fixtures' JSON, is at most a tenth of each."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("f32", "bf16x3", "f16x2")
STEM = "convnext_two_pnu"
TOL = 1e-4
OUT_TOL, GRAD_TOL = 1e-5, 1e-4


def _build(meta, **kw):
    from bcos.models import convnext
    from bcos.modules import norms
    from bcos_hip import synth
    stages = [convnext.CNBlockConfig(*s) for s in meta["block_setting"]]
    torch.manual_seed(0)
    net = convnext.BcosConvNeXt(stages, num_classes=meta["num_classes"], norm_layer=norms.NoBias(norms.PositionNormUncentered2d), **kw)
    pn = [m for m in net.modules() if isinstance(m, torch.nn.LayerNorm)]
    assert pn and all(type(m) is norms.PositionNormUncentered2d and m.bias is None for m in pn)
    return synth.seed_convnext(net, meta["weight_seed"])


@pytest.fixture(scope="module")
def recorded(golden_dir, hip_lib):
    from bcos_hip import synth
    assert torch.cuda.is_available()
    with open(os.path.join(golden_dir, STEM + ".json")) as f:
        meta = json.load(f)
    assert meta["tolerance"] == TOL and max(meta["d_ref"].values()) <= TOL / 10
    ref = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, STEM + "_fp64.npz")).items()}
    net = _build(meta).eval().to(DEV)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == meta["state_keys"]
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"]).to(DEV)
    return meta, ref, net, x


def _per_image(a, b):
    """worst image of max |a - b| / max |b|"""
    a, b = a.double().cpu().flatten(1), b.double().cpu().flatten(1)
    return float(((a - b).abs().amax(1) / b.abs().amax(1)).max())


def _check(out, ref, what, logits=None):
    dl = float((out["logits"].double().cpu() - ref["logits"]).abs().max())
    dw = _per_image(out["dynamic_linear_weights"], ref["weights"])
    dm = _per_image(out["contribution_map"], ref["contribution_map"])
    print(f"{what}: logits {dl:.2e}, W(x) {dw:.2e}, maps {dm:.2e} (bound {TOL:g})")
    assert out["prediction"].cpu().tolist() == ref["prediction"].tolist(), what
    assert dl <= TOL and dw <= TOL and dm <= TOL, (what, dl, dw, dm)
    if logits is not None:
        assert float((logits.double().cpu() - ref["logits"]).abs().max()) <= TOL, what


class _mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from bcos_hip import lib as blib
        self.prev = blib.get_contraction_mode()
        blib.set_contraction_mode(self.mode)

    def __exit__(self, *exc):
        from bcos_hip import lib as blib
        blib.set_contraction_mode(self.prev)
        return False


@pytest.mark.parametrize("mode", MODES)
def test_module_path(recorded, mode):
    meta, ref, net, x = recorded
    with _mode(mode):
        with torch.no_grad():
            logits = net(x)
        out = net.explain_batch(x)
    _check(out, ref, f"PNU, module path, {mode}", logits)


@pytest.mark.parametrize("mode", MODES)
def test_engine(recorded, mode):
    from bcos_hip import convnext_engine
    meta, ref, net, x = recorded
    with _mode(mode):
        eng = convnext_engine.attach(net)
        try:
            with torch.no_grad():
                logits = net(x)
            out = net.explain_batch(x)
            assert net._bcos_engine is eng
        finally:
            convnext_engine.detach(net)
    assert torch.equal(logits, out["logits"]), mode
    _check(out, ref, f"PNU, engine, {mode}", logits)


def test_engine_launch_list(recorded):
    """four launches per block forward, none of them elementwise; the norms of the plan are the uncentered ones"""
    from bcos_hip import convnext_engine
    meta, ref, net, x = recorded
    eng = convnext_engine.attach(net)
    try:
        assert eng.stem_pn.unc and eng.head_pn.unc
        convnext_engine.PLAN_LOG = []
        eng.forward(x[:1])
        log, convnext_engine.PLAN_LOG = convnext_engine.PLAN_LOG, None
        blocks = sum(s[2] for s in meta["block_setting"])
        downs = sum(1 for s in meta["block_setting"] if s[1] is not None)
        kinds = [k for k, _ in log]
        assert kinds.count("dw") == blocks and kinds.count("pn") == blocks + downs + 2 and kinds.count("conv") == 2 * blocks + downs + 2
        starts = [i for i, k in enumerate(kinds) if k == "dw"]
        assert all(kinds[i:i + 4] == ["dw", "pn", "conv", "conv"] for i in starts)
        assert len(kinds) == 4 * blocks + 2 * downs + 4          # stem (conv, pn), downsampling (pn, conv), head (pn, conv): nothing else
        convnext_engine.PLAN_LOG = []
        eng.explain(x[:1])
        log, convnext_engine.PLAN_LOG = convnext_engine.PLAN_LOG, None
        assert [k for k, _ in log].count("pn_bwd") == blocks + downs + 2
    finally:
        convnext_engine.PLAN_LOG = None
        convnext_engine.detach(net)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


def test_recorded_training_step(golden_dir, hip_lib):
    from bcos_hip import synth
    with open(os.path.join(golden_dir, STEM + "_train_step.json")) as f:
        meta = json.load(f)
    data = dict(np.load(os.path.join(golden_dir, STEM + "_train_step.npz")))
    floor = meta["reference_self_floor"]
    assert (meta["out_tolerance"], meta["grad_tolerance"]) == (OUT_TOL, GRAD_TOL)
    assert max(floor["output"], floor["loss"]) <= OUT_TOL / 10 and max(floor["gx"], floor["worst_param"]) <= GRAD_TOL / 10
    net = _build(meta, stochastic_depth_prob=meta["stochastic_depth_prob"], layer_scale=meta["layer_scale"]).to(DEV).train()
    x = synth.synthetic_images(meta["n_images"], seed=meta["image_seed"], size=meta["size"]).to(DEV)
    target = F.one_hot(torch.tensor(meta["labels"]), meta["num_classes"]).float().to(DEV)
    xr = x.clone().requires_grad_(True)
    out = net(xr)
    loss = F.binary_cross_entropy_with_logits(out, target)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == meta["param_names"]
    gs = torch.autograd.grad(loss, [xr] + [p for _, p in named])
    fig = dict(output=_rel(out.detach(), data["output"]), loss=abs(float(loss.detach()) - float(data["loss"])) / abs(float(data["loss"])),
               gx=_rel(gs[0], data["gx"]))
    per = {n: _rel(g, data["grad/" + n]) for (n, _), g in zip(named, gs[1:])}
    worst = max(per, key=per.get)
    print("recorded PNU step:", fig, "worst parameter", worst, per[worst], "reference's own fp32-vs-fp64", floor)
    assert fig["output"] <= OUT_TOL and fig["loss"] <= OUT_TOL, fig
    assert fig["gx"] <= GRAD_TOL, fig
    assert all(v <= GRAD_TOL for v in per.values()), {n: v for n, v in per.items() if v > GRAD_TOL}


def test_attach_still_refuses_the_bnu_model(hip_lib):
    from bcos.models import convnext
    from bcos.modules import norms
    from bcos_hip import convnext_engine
    from bcos_hip.lib import BcosHipError
    stages = [convnext.CNBlockConfig(8, None, 2)]
    bnu = convnext.BcosConvNeXt(stages, num_classes=4, norm_layer=norms.NoBias(norms.BatchNormUncentered2d)).to(DEV).eval()
    with pytest.raises(BcosHipError, match="position-norm"):
        convnext_engine.attach(bnu)
    assert not hasattr(bnu, "_bcos_engine")
    for other in (norms.NoBias(norms.GNLayerNormUncentered2d), norms.NoBias(norms.AllNormUncentered2d)):
        net = convnext.BcosConvNeXt(stages, num_classes=4, norm_layer=other).to(DEV).eval()
        with pytest.raises(BcosHipError, match="position-norm"):
            convnext_engine.attach(net)
        with torch.no_grad():
            assert net(torch.rand(1, 6, 8, 8, device=DEV)).shape == (1, 4)          # the module path runs them
