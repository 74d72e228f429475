"""`-m "not gpu"`: the fused DenseNet training plan (bcos_hip/densenet_train_plan.py) on emulated kernels against the step recorded from
the reference (tests/golden/densenet_tiny_train_step.*), the per-layer path against the same fixture, the plan's refusals and frozen
norms, the sharing of batch statistics, and the host side of the four training-mode dense-block entry points."""
import copy
import json
import os
import re

import pytest
import torch

import cpu_emulation as E
import densenet_emulation as DE
import densenet_train_cases as TC
import densenet_train_emulation as TE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bcos_slice_col_ws_floats", "bcos_slice_batch_stats", "bcos_bn_reader_finish", "bcos_slice_relu_bwd_colsums", "bcos_slice_bn_bwd_acc")


def _install(monkeypatch):
    E.install(monkeypatch)
    DE.install(monkeypatch)
    TE.install(monkeypatch)


def test_fixture_carries_the_references_floors_and_the_null_set():
    meta, data = TC.fixture()
    fl = meta["reference_self_floor"]
    for which in ("one_thread_vs_eight", "fp32_vs_fp64"):
        assert set(fl[which]) >= {"output", "gx", "worst_param"}
    f = fl["fp32_vs_fp64"]
    assert max(f["output"], f["gx"], f["worst_param"]) <= 2e-5          # the condition for holding the fixture to 1e-4
    assert meta["null_gradient_params"] == ["model.features.1.weight"]
    norms = meta["grad_norms_fp64"]
    assert len(norms) == 46 and norms["model.features.1.weight"] < 1e-2 * meta["median_grad_norm_fp64"]
    assert sorted(n for n, v in norms.items() if v < 1e-2 * meta["median_grad_norm_fp64"]) == meta["null_gradient_params"]
    recorded = {k.split("/", 1)[1] for k in data if k.startswith(("grad/", "gradrows/"))}
    assert recorded == set(meta["param_names"]) and data["grad_norms"].dtype.name == "float64"
    for stem in (TC.STEM + ".json", TC.STEM + ".npz"):
        assert os.path.getsize(os.path.join(TC.GOLDEN, stem)) < (1 << 20)


def test_train_step_is_one_autograd_node(monkeypatch):
    """net.train(); net(x) with the engine attached is train_plan._TrainStepFn (it ran per layer before this plan existed)"""
    from bcos_hip import densenet_engine, densenet_train_plan
    _install(monkeypatch)
    net, x, target = TC.tiny_net()
    eng = densenet_engine.attach(net)
    assert densenet_train_plan.DenseNetTrainPlan.supported(eng) == (True, "")
    net.train()
    logits = net(x[:2].clone().requires_grad_(True))
    assert type(logits.grad_fn).__name__ == "_TrainStepFnBackward"
    assert isinstance(eng._train_plan, densenet_train_plan.DenseNetTrainPlan)


def test_plan_step_against_the_reference_fixture(monkeypatch):
    from bcos_hip import densenet_engine
    _install(monkeypatch)
    net, x, target = TC.tiny_net()
    nbt = {k: int(b) for k, b in net.named_buffers() if k.endswith("num_batches_tracked")}
    densenet_engine.attach(net)
    res = TC.step(net, x, target)
    assert res["node"] == "_TrainStepFnBackward"
    TC.check_against_fixture(res, net, "plan, emulated kernels")
    assert len(nbt) == 23 and all(int(b) == nbt[k] + 1 for k, b in net.named_buffers() if k.endswith("num_batches_tracked"))
    # ... and behind the step the inference plan reads the updated statistics
    net.eval()
    with torch.no_grad():
        fused = net(x)
        densenet_engine.detach(net)
        assert TC.rel(fused, net(x)) <= 1e-5


def test_per_layer_step_against_the_reference_fixture(monkeypatch):
    """no engine attached: one autograd node per module, torch.cat in front of every dense layer -- not disturbed by the plan"""
    _install(monkeypatch)
    net, x, target = TC.tiny_net()
    res = TC.step(net, x, target)
    assert res["node"] != "_TrainStepFnBackward"
    TC.check_against_fixture(res, net, "layers, emulated kernels")


def test_refused_networks_keep_the_per_layer_path(monkeypatch):
    from bcos_hip import densenet_engine, densenet_train_plan
    _install(monkeypatch)
    net, x, target = TC.tiny_net()
    net.model.features[4].denselayer2.drop_rate = 0.25
    eng = densenet_engine.attach(net)
    ok, why = densenet_train_plan.DenseNetTrainPlan.supported(eng)
    assert not ok and "dropout" in why
    net.train()
    out = net(x[:2].clone().requires_grad_(True))
    assert type(out.grad_fn).__name__ != "_TrainStepFnBackward" and eng._train_plan is False
    out.sum().backward()
    net, x, target = TC.tiny_net()
    conv = net.model.features[5][2]                                        # the first transition's convolution
    conv.b = torch.nn.Parameter(torch.tensor(2.0))
    eng = densenet_engine.attach(net)
    ok, why = densenet_train_plan.DenseNetTrainPlan.supported(eng)
    assert not ok and "exponent" in why
    with pytest.raises(densenet_engine.BcosHipError, match="train plan"):
        densenet_train_plan.DenseNetTrainPlan(eng)
    net.train()
    out = net(x[:2].clone().requires_grad_(True))
    assert type(out.grad_fn).__name__ != "_TrainStepFnBackward" and eng._train_plan is False
    out.sum().backward()
    # a native unit-norm layer (NormedConv2d: the projection is part of the graph in a training step)
    from bcos.modules.bcosconv2d import NormedConv2d
    net, x, target = TC.tiny_net()
    conv = net.model.features[4].denselayer1.conv1
    old = conv.linear
    normed = NormedConv2d(old.in_channels, old.out_channels, old.kernel_size, old.stride, old.padding, bias=False)
    with torch.no_grad():
        normed.weight.copy_(old.weight)
    conv.linear = normed
    eng = densenet_engine.attach(net)
    ok, why = densenet_train_plan.DenseNetTrainPlan.supported(eng)
    assert not ok and "unit-norm" in why
    net.train()
    out = net(x[:2].clone().requires_grad_(True))
    assert type(out.grad_fn).__name__ != "_TrainStepFnBackward" and eng._train_plan is False
    out.sum().backward()
    assert normed.weight.grad is not None


def test_frozen_norms_inside_train_mode(monkeypatch):
    """norms put in eval() under net.train() (a reader of a dense block, a transition's norm, a norm behind a convolution): normalised
    with their running variance, no variance term, buffers untouched; the other norms keep their batch statistics; `detach` likewise
    has no variance term -- all against the per-layer path"""
    from bcos_hip import densenet_engine
    _install(monkeypatch)
    base, x, target = TC.tiny_net()
    start = TC.scale_running_var(base)                   # (statistics that are NOT the batch's: frozen and batch paths differ)
    pick = lambda n: (n.model.features[4].denselayer2.norm1, n.model.features[5][0], n.model.features[6].denselayer1.norm2,   # noqa: E731
                      n.model.features[10].denselayer2.norm1)

    def run(net, attach):
        if attach:
            densenet_engine.attach(net)
        net.train()
        frozen = pick(net)
        for m in frozen[:3]:
            m.eval()
        frozen[3].detach = True
        before = [m.running_var.clone() for m in frozen[:3]]
        counts = [int(m.num_batches_tracked) for m in frozen[:3]]
        res = TC.step_in_current_mode(net, x, target)
        for m, rv, cnt in zip(frozen[:3], before, counts):
            assert torch.equal(m.running_var, rv) and int(m.num_batches_tracked) == cnt
        return res
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    plan, layers = run(nets[0], True), run(nets[1], False)
    assert plan["node"] == "_TrainStepFnBackward" and layers["node"] != "_TrainStepFnBackward"
    TC.check_same_step(plan, layers, 1e-5, 1e-5, "frozen norms")
    # every other norm's running_var followed the batch with ITS momentum, in the plan as on the per-layer path
    assert TC.check_buffers(nets[0], nets[1], start, frozen=pick(nets[0])[:3], what="frozen norms") == 23 - 3


def test_running_var_follows_the_batch(monkeypatch):
    """the plan's running_var update -- which reader's buffer takes which range of the block's shared variance, with which momentum --
    against the per-layer path, from buffers that are NOT the batch variance; one norm with a momentum of its own, one that does not
    track running statistics"""
    from bcos_hip import densenet_engine
    _install(monkeypatch)
    base, x, target = TC.tiny_net()
    base.model.features[6].denselayer3.norm1.momentum = 0.5
    base.model.features[7][0].momentum = 1.0
    start = TC.scale_running_var(base)
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    densenet_engine.attach(nets[0])
    res = [TC.step(n, x, target) for n in nets]
    assert res[0]["node"] == "_TrainStepFnBackward" and res[1]["node"] != "_TrainStepFnBackward"
    assert TC.check_buffers(nets[0], nets[1], start, what="running_var") == 23
    TC.check_same_step(res[0], res[1], 1e-5, 1e-4, "running_var")
    # track_running_stats = False on a reader: batch statistics, no buffer to move, nothing raised
    for n in nets:
        bn = n.model.features[8].denselayer2.norm1
        bn.track_running_stats = False
        bn.running_var = bn.running_mean = bn.num_batches_tracked = None
    res = [TC.step(n, x, target) for n in nets]
    assert res[0]["node"] == "_TrainStepFnBackward"
    TC.check_same_step(res[0], res[1], 1e-5, 1e-4, "no running statistics")


def test_cumulative_average_momentum(monkeypatch):
    """momentum = None: running_var is the cumulative average, the count advances before it is used (reference :84-88)"""
    from bcos_hip import densenet_engine
    _install(monkeypatch)
    base, x, target = TC.tiny_net()
    for m in base.modules():
        if hasattr(m, "running_var"):
            m.momentum = None
            m.num_batches_tracked.fill_(3)
    start = TC.scale_running_var(base)
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    densenet_engine.attach(nets[0])
    res = [TC.step(n, x, target) for n in nets]
    assert res[0]["node"] == "_TrainStepFnBackward"
    assert TC.check_buffers(nets[0], nets[1], start, what="momentum = None") == 23
    for k, a in nets[0].named_buffers():
        if k.endswith("running_var"):                    # the factor 1 / 4: rv' - rv = (var - rv) / 4 with rv = 1.7 var
            assert abs(TC.rel(a, start[k]) - (0.7 / 1.7) / 4) <= 1e-2, k
        elif k.endswith("num_batches_tracked"):
            assert int(a) == 4, k


def test_readers_share_the_statistics_of_their_channels(monkeypatch):
    """what a reader takes from the block's vector -- written slice by slice, as each slice was completed -- equals the statistics of
    the reader's own channel range computed in one call"""
    g = torch.Generator().manual_seed(11)
    X = torch.randn(3, 5, 7, 96, generator=g) * torch.rand(96, generator=g) * 3 + torch.randn(96, generator=g)
    mean, var = torch.full((96,), float("nan")), torch.full((96,), float("nan"))
    for lo, hi in ((0, 32), (32, 64), (64, 96)):
        TE.slice_batch_stats(X[..., lo:hi], mean[lo:hi], var[lo:hi])
    for c in (32, 64, 96):
        m1, v1 = TE.slice_batch_stats(X[..., :c], torch.empty(c), torch.empty(c))
        assert torch.equal(m1, mean[:c]) and torch.equal(v1, var[:c]), c
    ref = X.reshape(-1, 96).double()
    assert TC.rel(mean, ref.mean(0)) <= 1e-6 and TC.rel(var, ref.var(0, unbiased=False)) <= 1e-6
    # the plan itself: the vector a block's readers read holds the statistics of the whole buffer
    from bcos_hip import densenet_engine, ops
    _install(monkeypatch)
    seen = []
    real = ops.bn_reader_finish
    monkeypatch.setattr(ops, "bn_reader_finish", lambda var, *a, **k: (seen.append(var.clone()), real(var, *a, **k))[1])
    net, x, target = TC.tiny_net()
    eng = densenet_engine.attach(net)
    net.train()
    out = net(x.clone().requires_grad_(True))
    st = out.grad_fn.st
    assert len(seen) == 9 + 3 + 1                                          # one finish per reader: 9 norm1, 3 transitions, norm5
    widths = [v.numel() for v in seen]
    assert widths == [64, 96, 128, 64, 96, 128, 160, 80, 112, 144, 72, 104, 136]
    X0 = st["blocks"][0]["X"]
    own = TE.slice_batch_stats(X0, torch.empty(128), torch.empty(128))[1]
    assert torch.equal(seen[2], own) and torch.equal(seen[1], own[:96]) and torch.equal(seen[0], own[:64])


def test_emulation_states_the_header():
    g = torch.Generator().manual_seed(5)
    X = torch.randn(300, 40, generator=g) + 0.5
    x = X[:, 8:32]
    gv, sh = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g) * 0.3
    d = torch.randn(300, 24, generator=g)
    mean, var = TE.slice_batch_stats(x, torch.empty(24), torch.empty(24))
    m64, v64, bm, bv = TE.slice_batch_stats64(x)
    assert bool(((mean.double() - m64).abs() <= bm).all()) and bool(((var.double() - v64).abs() <= bv).all())
    rstd, gg = TE.bn_reader_finish(var, gv, 1e-5)
    sgx, sg, gw, coef = TE.slice_relu_bwd_colsums(d, x, gg, sh, rstd=rstd, want_sg=True, want_gw=True, want_coef=True)
    y, _ = DE.slice_affine_rows32(x, gg, sh, None, True)
    s64, g64, bs, bg, gate = TE.slice_relu_bwd_colsums64(d, x, gg, sh)
    assert torch.equal(gate, y > 0)
    assert bool(((sgx.double() - s64).abs() <= bs).all()) and bool(((sg.double() - g64).abs() <= bg).all())
    G = torch.full((300, 40), float("nan"))
    TE.slice_bn_bwd_acc(d, G[:, 8:32], x, gg, sh, mean, coef, accumulate=False)
    want, bound, gate2 = TE.slice_bn_bwd_acc64(d, G[:, 8:32], x, gg, sh, mean, coef, accumulate=False)
    assert torch.equal(gate2, gate) and bool(((G[:, 8:32].double() - want).abs() <= bound).all())
    assert bool(G[:, :8].isnan().all()) and bool(G[:, 32:].isnan().all())
    # it IS the norm's gradient: autograd through y = relu(x w / sqrt(var(x) + eps) + b)
    xa, wa, ba = x.double().clone().requires_grad_(True), gv.double().clone().requires_grad_(True), sh.double().clone().requires_grad_(True)
    ya = torch.relu(xa * wa / torch.sqrt(xa.var(0, unbiased=False) + 1e-5) + ba)
    gx, gwa, gba = torch.autograd.grad((ya * d.double()).sum(), [xa, wa, ba])
    assert TC.rel(G[:, 8:32], gx) <= 1e-5 and TC.rel(gw, gwa) <= 1e-5 and TC.rel(sg, gba) <= 1e-5
    # no variance term: the bits of the explanation-mode map
    A, B = torch.randn(300, 24, generator=g), None
    B = A.clone()
    TE.slice_bn_bwd_acc(d, A, x, gg, sh, None, None, accumulate=True)
    DE.slice_affine_bwd_acc(d, B, x, gg, sh, True, accumulate=True)
    assert torch.equal(A, B)
    assert TE.col_plan(1) == (1, 1) and TE.col_plan(4099) == (33, 125) and TE.col_plan(200704) == (1024, 196)


def test_header_and_bindings():
    from bcos_hip import lib, ops
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header)            # additive entry points: the ABI version stays
    for sym in SYMBOLS:
        assert sym in lib.SIGNATURES and re.search(r"\bint " + sym + r"\(", header), sym
        decl = re.search(r"\bint " + sym + r"\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[sym][1]), sym
    assert "batchnorm_uncentered.py:36-44" in header[header.index("bcos_slice_col_ws_floats") - 3000:header.index("bcos_slice_bn_bwd_acc(")]
    for name in ("slice_batch_stats", "bn_reader_finish", "slice_relu_bwd_colsums", "slice_bn_bwd_acc"):
        assert callable(getattr(ops, name))


def test_library_exports_and_refuses_malformed_calls(hip_lib):
    """the built library carries the entry points; what the header lists as BCOS_E_INVAL is refused before anything is launched (host
    pointers stand in for device ones: validation never dereferences them)"""
    import ctypes as C
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, off, odd = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 2)
    n = C.c_int64(0)
    assert hip_lib.bcos_slice_col_ws_floats(4099, 32, C.byref(n)) == 0 and n.value == TE.ws_floats(4099, 32) == 3 * 33 * 32
    assert hip_lib.bcos_slice_col_ws_floats(200704, 96, C.byref(n)) == 0 and n.value == TE.ws_floats(200704, 96)
    for bad in ((0, 32), (4, 30), (4, 0)):
        assert hip_lib.bcos_slice_col_ws_floats(bad[0], bad[1], C.byref(n)) == -22
    assert hip_lib.bcos_slice_col_ws_floats(4, 32, None) == -22

    def refuse(fn, ok, cases, name):
        for idx, bad in cases:
            args = list(ok)
            args[idx] = bad
            assert fn(*args) == -22, (name, idx, bad)
            assert name.encode() in hip_lib.bcos_last_error_string()
    # x, x_pitch, mean, var, workspace, workspace_floats, rows, C, stream
    refuse(hip_lib.bcos_slice_batch_stats, [p, 64, p, p, p, 96, 4, 32, None],
           ((0, None), (2, None), (3, None), (4, None), (0, off), (4, off), (2, odd), (3, odd), (1, 28), (1, 34), (5, 95), (6, 0), (7, 30), (7, 0)),
           "bcos_slice_batch_stats")
    # var, weight, running_var, rstd, g, C, eps, momentum, stream
    refuse(hip_lib.bcos_bn_reader_finish, [p, p, p, p, p, 32, 1e-5, 0.1, None],
           ((0, None), (3, None), (4, None), (0, odd), (1, odd), (2, odd), (3, odd), (4, odd), (5, 0), (6, -1.0), (7, 1.5), (7, -0.1)),
           "bcos_bn_reader_finish")
    # d, x, x_pitch, gvec, shift, rstd, sgx, sg, gw, coef, workspace, workspace_floats, rows, C, stream
    refuse(hip_lib.bcos_slice_relu_bwd_colsums, [p, p, 64, p, p, p, p, p, p, p, p, 64, 4, 32, None],
           ((0, None), (1, None), (3, None), (6, None), (10, None), (5, None), (0, off), (1, off), (3, off), (4, off), (10, off), (5, odd),
            (6, odd), (7, odd), (8, odd), (9, odd), (2, 28), (2, 34), (11, 63), (12, 0), (13, 30)), "bcos_slice_relu_bwd_colsums")
    # d, x, x_pitch, scale, shift, mean, coef, g, g_pitch, rows, C, accumulate, stream
    refuse(hip_lib.bcos_slice_bn_bwd_acc, [p, p, 64, p, p, p, p, p, 64, 4, 32, 1, None],
           ((0, None), (1, None), (7, None), (6, None), (0, off), (1, off), (3, off), (4, off), (5, off), (6, off), (7, off), (2, 28), (8, 34),
            (9, -1), (10, 6), (11, 2)), "bcos_slice_bn_bwd_acc")
    ok = [p, p, 64, p, p, None, None, p, 64, 4, 33000, 1, None]                      # the looping form's limit, as for the other slice kernels
    ok[2] = ok[8] = 33000
    assert hip_lib.bcos_slice_bn_bwd_acc(*ok) == -95


def test_documents_name_the_plan():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "densenet_train_plan.py" in design and "bcos_slice_batch_stats" in design
    assert "densenet_train_plan.py" in open(os.path.join(REPO, "README.md")).read()
    assert json.load(open(os.path.join(TC.GOLDEN, TC.STEM + ".json")))["loss"] == "bce_with_logits"


def test_plan_contractions_run_under_the_f32_override(monkeypatch):
    """every contraction launch of the plan's forward and backward sees ops.contraction_override("f32"); the context nests, restores
    and refuses unknown modes; the per-layer path sees none"""
    from bcos_hip import densenet_engine, densenet_train_plan, ops
    from bcos_hip.lib import BcosHipError
    assert ops._CONTRACTION_OVERRIDE is None
    with ops.contraction_override("bf16x3"):
        with ops.contraction_override("f32"):
            assert ops._CONTRACTION_OVERRIDE == "f32"
        assert ops._CONTRACTION_OVERRIDE == "bf16x3"
    assert ops._CONTRACTION_OVERRIDE is None
    with pytest.raises(BcosHipError):
        ops.contraction_override("fp8")
    assert densenet_train_plan.DenseNetTrainPlan.CONTRACTION == "f32"
    _install(monkeypatch)
    seen = []
    real = ops.tapconv
    monkeypatch.setattr(ops, "tapconv", lambda *a, **k: (seen.append(ops._CONTRACTION_OVERRIDE), real(*a, **k))[1])
    net, x, target = TC.tiny_net()
    TC.step(net, x[:2], target[:2])
    assert seen and set(seen) == {None}
    del seen[:]
    net.eval()
    densenet_engine.attach(net)
    res = TC.step(net, x[:2], target[:2])
    assert res["node"] == "_TrainStepFnBackward" and len(seen) >= 2 * 20 and set(seen) == {"f32"}
    assert ops._CONTRACTION_OVERRIDE is None
    # a refused width never reaches supported(): attach itself raises
    from bcos_hip import synth
    from bcosify import BcosifyNetwork
    cfg = synth.densenet_model_config(12)
    odd = synth.finish_conversion(BcosifyNetwork(synth.standard_densenet(6, (2, 2), 64, 2, 12, 0), cfg, add_channels=True, logit_layer=True), cfg).eval()
    with pytest.raises(BcosHipError, match="multiples of 4"):
        densenet_engine.attach(odd)
