"""`-m "not gpu"`: the B-cosified DenseNet surface -- model classes, factory, experiment table, synthetic builder -- against what was
recorded from the reference (tests/golden/make_golden_densenet.py), the module path on emulated kernels against the densenet_tiny
fixture, and the host side of the two dense-block entry points (bindings, wrappers' argument checks, header)."""
import json
import os
import re

import pytest
import torch

import cpu_emulation as E
import densenet_cases as DC
import densenet_emulation as DE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tiny():
    return DC.golden_net("densenet_tiny")


def test_state_dict_is_the_recorded_one(tiny):
    """keys, order, shapes and (after the recorded calibration) the checksums of the reference's B-cosified DenseNet; strict loading"""
    net, meta, data, x = tiny
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == meta["state_keys"]
    mine = DC.state_checksum(sd)
    assert mine.keys() == meta["state_checksum"].keys()
    for k, (s, a) in meta["state_checksum"].items():
        assert abs(mine[k][0] - s) <= 1e-6 * max(a, 1e-30) and abs(mine[k][1] - a) <= 1e-6 * max(a, 1e-30), k
    from bcos_hip import synth
    other = synth.build_bcosified_densenet(meta["growth"], tuple(meta["block_config"]), meta["init_features"], meta["bn_size"],
                                           meta["num_classes"], seed=1)
    other.load_state_dict(sd, strict=True)


def test_densenet121_factory_matches_the_recorded_state_dict():
    from bcos.experiments.ImageNet.bcosification.experiment_parameters import CONFIGS
    from bcos.experiments.ImageNet.bcosification.model import get_model
    from bcos.models.standard_models import DenseNetBcos
    from bcos.modules.pooling import AvgPool2d
    meta = json.load(open(os.path.join(DC.GOLDEN, "densenet121_small.json")))
    cfg = CONFIGS["densenet_121"]["model"]
    assert cfg["name"] == "densenet121" and cfg["last_layer_name"] == "classifier" and list(cfg["standard_changes"]) == ["features[3]"]
    assert cfg["bcosify_args"] == CONFIGS["resnet_50"]["model"]["bcosify_args"] and cfg["bcos_args"] == dict(b=2, max_out=1)
    with pytest.warns(UserWarning, match="no network access"):
        net = get_model(cfg)
    assert isinstance(net.model, DenseNetBcos)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == meta["state_keys"]
    pool = net.model.features[3]
    assert type(pool) is AvgPool2d and (pool.kernel_size, pool.stride, pool.padding) == (3, 2, 1)
    assert all(getattr(m, "bias", None) is None for m in net.modules())
    for seed in (5, 420, 1337):
        assert CONFIGS[f"densenet_121-seed={seed}"]["seed"] == seed


def test_tv_densenet_keys_are_torchvisions():
    """the restated topology carries torchvision's names (spot checks of every kind of key) and DenseNet-121's parameter count"""
    from bcos.models._tv_densenet import DenseNet
    net = DenseNet(32, (6, 12, 24, 16), 64, memory_efficient=True, drop_rate=0.0)
    keys = list(net.state_dict())
    for k in ("features.conv0.weight", "features.norm0.running_var", "features.denseblock1.denselayer1.norm1.weight",
              "features.denseblock3.denselayer24.conv2.weight", "features.transition2.conv.weight", "features.norm5.bias",
              "classifier.weight", "classifier.bias"):
        assert k in keys, k
    assert keys[0] == "features.conv0.weight" and keys[-1] == "classifier.bias"
    assert sum(p.numel() for p in net.parameters()) == 7978856          # torchvision's densenet121
    assert net.features.denseblock2.denselayer3.conv1.in_channels == 128 + 2 * 32
    with torch.no_grad():
        assert net.eval()(torch.zeros(1, 3, 64, 64)).shape == (1, 1000)


def test_assign_path():
    from bcos_hip.synth import assign_path
    root = torch.nn.Module()
    root.features = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Sequential(torch.nn.ReLU(), torch.nn.ReLU()))
    new = torch.nn.Identity()
    assign_path(root, "features[1][0]", new)
    assert root.features[1][0] is new
    assign_path(root, "features[1].extra", new)
    assert root.features[1].extra is new
    assign_path(root, "maxpool", new)
    assert root.maxpool is new
    for bad in ("features[x]", "__import__('os')", "a b", ""):
        with pytest.raises(ValueError):
            assign_path(root, bad, new)


def test_module_execution_order_is_the_references(monkeypatch):
    """DenseNet-121 through this package's modules calls the same modules on the same shapes in the same order as the imported
    reference did (densenet_exec_trace.json): every B-cos conv once, with its norm in front of or behind it"""
    from bcos_hip import synth
    E.install(monkeypatch)
    recorded = json.load(open(os.path.join(DC.GOLDEN, "densenet_exec_trace.json")))["densenet121"]
    net = synth.build_bcosified_densenet()
    names = {m: n for n, m in net.named_modules()}
    trace, hooks = [], []
    kinds = {"BcosifyConv2d": "BcosifyConv2d", "BatchNormUncentered2d": "BatchNormUncentered2d", "AvgPool2d": "AvgPool2d", "ReLU": "ReLU",
             "LogitLayer": "LogitLayer", "Normalize6": "Normalize"}
    for m in net.modules():
        if type(m).__name__ in kinds:
            hooks.append(m.register_forward_hook(lambda m, inp, res: trace.append(
                [names[m], kinds[type(m).__name__], list(inp[0].shape), list(res.shape)])))
    # shapes only: every contraction returns zeros of its output shape (the values are the parity tests' business)
    from bcos.modules.bcosifyconv2d import BcosifyConv2d
    monkeypatch.setattr(BcosifyConv2d, "forward", lambda self, x: x.new_zeros(
        x.shape[0], self.linear.out_channels, _out(x.shape[2], self.linear, 0), _out(x.shape[3], self.linear, 1)))
    with torch.no_grad():
        net(synth.synthetic_images(1, seed=5))
    convs = [t for t in trace if t[1] == "BcosifyConv2d"]
    assert len(convs) == len({t[0] for t in convs}) == 1 + 2 * 58 + 3 + 1
    assert trace == recorded


def _out(size, lin, axis):
    k, s, p = lin.kernel_size[axis], lin.stride[axis], lin.padding[axis]
    return (size + 2 * p - k) // s + 1


def test_module_path_against_densenet_tiny(tiny, monkeypatch):
    """net(x) and net.explain_batch(x) through the per-layer modules and torch.cat on emulated kernels: logits <= 1e-4, classes exact,
    W(x) and maps <= 1e-4 in relative L2 and in the worst element per image over the map's peak (d_ref of the fixture <= 3e-5)"""
    net, meta, data, x = tiny
    E.install(monkeypatch)
    assert max(meta["d_ref"].values()) <= 3e-5
    with torch.no_grad():
        assert DC.rel(net(x), data["logits"]) <= 1e-4
    out = net.explain_batch(x)
    DC.check_against_fixture(out, data, 1e-4, 1e-4, "module path, emulated kernels")
    assert float(DC.completeness_residual(x, out, meta["logit_bias"]).max()) <= 1e-4
    one = net.explain(x[1:2].clone().requires_grad_(True))
    assert one["prediction"] == int(data["prediction"][1])
    assert DC.rel(one["dynamic_linear_weights"], data["weights"][1:2]) <= 1e-4


def test_header_and_bindings():
    from bcos_hip import lib
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header) and lib.ABI_VERSION == 12
    for sym in ("bcos_slice_affine_rows", "bcos_slice_affine_bwd_acc"):
        assert sym in lib.SIGNATURES and re.search(r"\bint " + sym + r"\(", header), sym
    assert "bcos_dense.hip" in lib.SOURCES and os.path.exists(os.path.join(REPO, "b-cosification_amd", "csrc", "bcos_dense.hip"))
    for cite in ("standard_models.py:56-63", "batchnorm_uncentered.py:46-60"):
        assert cite in header[header.index("bcos_slice_affine_rows") - 1500:header.index("bcos_slice_affine_bwd_acc(")], cite
    # one argument type per parameter of the C declarations
    for sym in ("bcos_slice_affine_rows", "bcos_slice_affine_bwd_acc"):
        decl = re.search(r"\bint " + sym + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[sym][1]), sym


def test_library_exports_and_refuses_malformed_calls(hip_lib):
    """the built library carries both symbols; what the header lists as BCOS_E_INVAL is refused before anything is launched (host
    pointers stand in for device ones: validation never dereferences them)"""
    import ctypes as C
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, off = C.c_void_p(base), C.c_void_p(base + 4)
    rows_ok = [p, 64, p, p, p, p, 64, p, 4, 32, 1, None]
    assert hip_lib.bcos_slice_affine_rows(None, 64, p, p, p, p, 64, p, 4, 32, 1, None) == -22
    for idx, bad in ((0, off), (2, off), (3, off), (4, off), (5, off), (1, 28), (1, 34), (6, 30), (8, 0), (9, 30), (9, 0), (10, 2),
                     (7, C.c_void_p(base + 2))):
        args = list(rows_ok)
        args[idx] = bad
        assert hip_lib.bcos_slice_affine_rows(*args) == -22, (idx, bad)
        assert b"bcos_slice_affine_rows" in hip_lib.bcos_last_error_string()
    bwd_ok = [p, p, 64, p, p, p, 64, 4, 32, 1, 1, None]
    for idx, bad in ((0, None), (5, None), (1, None), (0, off), (1, off), (5, off), (3, off), (4, off), (2, 28), (6, 34), (7, -1), (8, 6),
                     (9, 3), (10, 2)):
        args = list(bwd_ok)
        args[idx] = bad
        assert hip_lib.bcos_slice_affine_bwd_acc(*args) == -22, (idx, bad)
        assert b"bcos_slice_affine_bwd_acc" in hip_lib.bcos_last_error_string()


def test_asan_program_is_listed():
    """tests/asan/dense_abi_validation.c runs with its siblings in scripts/asan_host_check.sh (which the occlusion suite runs)"""
    script = open(os.path.join(REPO, "scripts", "asan_host_check.sh")).read()
    assert "dense_abi_validation" in script
    assert os.path.exists(os.path.join(REPO, "tests", "asan", "dense_abi_validation.c"))


def test_wrappers_refuse_what_is_not_a_channel_slice(monkeypatch):
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    X = torch.zeros(2, 5, 5, 96)
    assert ops._row_slice(X[..., :64], "x") == (50, 64, 96)
    assert ops._row_slice(X, "x") == (50, 96, 96)
    assert ops._row_slice(X[..., 32:64].reshape(-1, 32)[:1], "x")[:2] == (1, 32)
    for bad in (X[:, ::2, :, :64], X.permute(0, 3, 1, 2), X[..., ::2]):
        with pytest.raises(BcosHipError):
            ops._row_slice(bad, "x")


def test_emulation_states_the_header():
    """the restatement itself: stages off is a copy, the gate is the fp32 forward's decision, accumulate = 0 ignores g"""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(7, 40, generator=g)
    sc, sh, mul = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g), torch.randn(7, 24, generator=g)
    x = X[:, :24]
    y, am = DE.slice_affine_rows32(x)
    assert torch.equal(y, x) and torch.equal(am.view(torch.float32), x.abs().amax(1))
    y, _ = DE.slice_affine_rows32(x, sc, sh, None, True)
    y64, bound, y64_pre = DE.slice_affine_rows64(x, sc, sh, mul, True)
    assert torch.equal(y > 0, DE.pre_activation32(x, sc, sh) > 0)
    assert bool(((DE.slice_affine_rows32(x, sc, sh, mul, True)[0].double() - y64).abs() <= bound).all())
    d = torch.randn(7, 24, generator=g)
    G = torch.full((7, 40), float("nan"))
    DE.slice_affine_bwd_acc(d, G[:, :24], x, sc, sh, True, accumulate=False)
    g64, gb, gate = DE.slice_affine_bwd_acc64(d, G[:, :24], x, sc, sh, True, accumulate=False)
    assert torch.equal(gate, y > 0) and bool(((G[:, :24].double() - g64).abs() <= gb).all()) and bool(G[:, 24:].isnan().all())
    out = torch.zeros(7, 40)
    DE.slice_affine_rows(d, out=out[:, 8:32])
    assert torch.equal(out[:, 8:32], d) and float(out[:, :8].abs().sum() + out[:, 32:].abs().sum()) == 0.0


# ---- the fused plan (bcos_hip/densenet_engine.py) on emulated kernels ---------------------------------------------------------------
def _install(monkeypatch):
    E.install(monkeypatch)
    DE.install(monkeypatch)


def test_plan_against_densenet_tiny(tiny, monkeypatch):
    """attach + explain_batch / forward / explain_targets through the plan on emulated kernels, held to the fixture like the module path;
    the forward-only pass (conv2 written into its slice through out_pitch) and the explanation pass (dense conv2 + placement) agree"""
    from bcos_hip import densenet_engine
    net, meta, data, x = tiny
    _install(monkeypatch)
    eng = densenet_engine.attach(net)
    try:
        assert net._bcos_engine is eng
        with torch.no_grad():
            fwd = net(x)
        out = net.explain_batch(x)
        assert torch.equal(fwd, out["logits"])
        DC.check_against_fixture(out, data, 1e-4, 1e-4, "plan, emulated kernels")
        assert float(DC.completeness_residual(x, out, meta["logit_bias"]).max()) <= 1e-4
        tg = torch.tensor([[7, 0], [3, 7], [7, 11]])
        rep = eng.explain_targets(x, tg, want_weights=True)
        assert DC.rel(rep["dynamic_linear_weights"][:, 0][[0, 2]], data["weights"][[0, 2]]) <= 1e-4
        single = eng.explain(x, targets=tg[:, 1])
        assert DC.rel(rep["contribution_maps"][:, 1], single["contribution_map"]) <= 1e-6
        assert torch.equal(single["explained_class_idx"], tg[:, 1])
    finally:
        densenet_engine.detach(net)
    assert not hasattr(net, "_bcos_engine")
    module = net.explain_batch(x)
    assert DC.rel(out["dynamic_linear_weights"], module["dynamic_linear_weights"]) <= 1e-5


def test_plan_launch_list_is_the_recorded_execution_order(monkeypatch):
    """DenseNet-121: every B-cos conv of densenet_exec_trace.json once, on the recorded shapes, in the recorded order, with the norm the
    reference runs in front of it (dense layers' norm1, transitions, norm5) or behind it (norm0, norm2) -- shapes only: the contraction
    stand-in fills zeros"""
    from bcos_hip import densenet_engine, ops, synth
    _install(monkeypatch)

    def zeros(a, wt, geom, *, out=None, out2=None, scale_out=None, norm_out=None, **kw):
        for t in (out, out2, scale_out, norm_out):
            if t is not None:
                t.zero_()
    monkeypatch.setattr(ops, "tapconv", zeros)
    recorded = json.load(open(os.path.join(DC.GOLDEN, "densenet_exec_trace.json")))["densenet121"]
    expect = []
    for i, (name, kind, shp_in, shp_out) in enumerate(recorded):
        if kind != "BcosifyConv2d":
            continue
        j = i - 2 if recorded[i - 1][1] == "ReLU" else i - 1
        before, after = recorded[j], (recorded[i + 1] if i + 1 < len(recorded) else None)
        # a norm that reads a convolution's own output is that convolution's (norm0, norm2); any other norm belongs to the one it feeds
        own = recorded[j - 1][1] == "BcosifyConv2d" and recorded[j - 1][3] == before[2]
        pre = before[0] if before[1] == "BatchNormUncentered2d" and before[3] == shp_in and not own else None
        post = after[0] if after is not None and after[1] == "BatchNormUncentered2d" and after[2] == shp_out else None
        nhwc = lambda s: (s[0], s[2], s[3], s[1])          # noqa: E731
        cin = nhwc(shp_in)
        expect.append((name, pre, post, cin[:3] + (8 if cin[3] == 6 else cin[3],), nhwc(shp_out)))
    assert len(expect) == 121 - 1 + 1          # 120 convolutions + the classifier
    net = synth.build_bcosified_densenet()
    eng = densenet_engine.attach(net)
    for keep in (False, True):
        monkeypatch.setattr(densenet_engine, "PLAN_LOG", [])
        from bcos_hip.passes import _drive
        from bcos_hip.plan import Images
        _drive(eng._run_forward_gen(Images(synth.synthetic_images(1, seed=5)), keep=keep))
        assert densenet_engine.PLAN_LOG == expect, keep


def _tiny_net(**over):
    from bcos_hip import synth
    from bcosify import BcosifyNetwork
    cfg = synth.densenet_model_config(12)
    for k, v in over.items():
        cfg[k] = dict(cfg[k], **v)
    net = BcosifyNetwork(synth.standard_densenet(32, (2, 2), 64, 2, 12, 0), cfg, add_channels=True, logit_layer=True)
    return synth.finish_conversion(net, cfg).eval()


def test_attach_refuses_what_the_plan_does_not_cover(monkeypatch):
    from bcos_hip import densenet_engine, engine, synth
    from bcos_hip.lib import BcosHipError
    _install(monkeypatch)
    densenet_engine.attach(_tiny_net())                                   # the scope itself attaches
    with pytest.raises(BcosHipError, match="B = "):
        densenet_engine.attach(_tiny_net(bcos_args=dict(b=1.5)))
    net = _tiny_net()
    net.model.features[4].denselayer2.conv2.max_out = 2
    with pytest.raises(BcosHipError, match="MaxOut"):
        densenet_engine.attach(net)
    net = _tiny_net()
    net.model.features[4].denselayer1.conv1.linear.groups = 2
    with pytest.raises(BcosHipError, match="groups"):
        densenet_engine.attach(net)
    net = _tiny_net()
    net.train()
    with pytest.raises(BcosHipError, match="eval"):
        densenet_engine.attach(net)
    with pytest.raises(BcosHipError, match="DenseNet"):
        densenet_engine.attach(synth.build_bcosified_resnet("resnet18"))
    with pytest.raises(BcosHipError):
        engine.attach(_tiny_net())                                         # (and the ResNet plan does not take a DenseNet)
    assert not hasattr(net, "_bcos_engine")


def test_unsupported_arguments_raise(tiny, monkeypatch):
    from bcos_hip import densenet_engine
    from bcos_hip.lib import BcosHipError
    net, meta, data, x = tiny
    _install(monkeypatch)
    eng = densenet_engine.DenseNetEngine(net)
    for name in ("occlude", "perturb"):
        with pytest.raises(BcosHipError, match=name):
            eng.forward(x, **{name: object()})
    for name in ("occlude", "perturb", "functional", "gates", "cotangent"):
        with pytest.raises(BcosHipError, match=name):
            eng.explain(x, **{name: object()})
    with pytest.raises(IndexError):
        eng.explain(x, targets=torch.tensor([0, 1, 12]))


def test_plan_notices_changed_parameters(tiny, monkeypatch):
    """an in-place parameter update (calibration, an optimiser step) reaches the plan without an explicit refresh()"""
    import copy
    from bcos_hip import densenet_engine
    net, meta, data, x = tiny
    net = copy.deepcopy(net)
    _install(monkeypatch)
    eng = densenet_engine.attach(net)
    with torch.no_grad():
        before = net(x)
        net.model.features[4].denselayer1.norm1.running_var.mul_(4.0)
        net.model.features[11].weight.mul_(0.5)
        after = net(x)
        densenet_engine.detach(net)
        want = net(x)
    assert DC.rel(after, want) <= 1e-5 and DC.rel(before, want) > 1e-3
