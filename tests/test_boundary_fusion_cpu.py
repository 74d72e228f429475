"""`-m "not gpu"`: the fused boundary launch (ops.boundary_conv3_grad / bcos_boundary_conv3_grad) on the host side -- when the engine
issues it, what it replaces, when it falls back, and how the C entry point rejects arguments.

Kernels are the interpreters of tests/cpu_emulation.py and tests/boundary_fusion_emulation.py.  The network is a Bottleneck ResNet with
TWO blocks in stage 1 and one in every other stage: a one-block-per-stage network has no identity-shortcut boundary at widths 64 / 256
(its only stage-1 block is read by layer2.0, which has a shortcut convolution), so it could only show the fall-back."""
import ctypes as C

import pytest
import torch

import boundary_fusion_emulation
import cpu_emulation

LOGGED = ("tapconv", "tapconv_group", "boundary_conv3_grad", "avgpool2d_bwd", "head_rank1_grad", "finalize_explanation", "prep_input")


def small_bottleneck_net(layers=(2, 1, 1, 1), seed=0):
    from bcos.models.standard_models import Bottleneck, ResNetBcos
    from bcos_hip import synth
    from bcosify import BcosifyNetwork
    torch.manual_seed(seed)
    std = ResNetBcos(Bottleneck, list(layers))
    synth.randomize_batchnorm(std, torch.Generator().manual_seed(seed + 1))
    cfg = synth.resnet_model_config("resnet50")
    net = BcosifyNetwork(std, cfg, add_channels=True, logit_layer=True)
    return rescaled(synth.finish_conversion(net, cfg).eval())


def rescaled(net):
    """un-calibrated nets collapse numerically; a cheap analytic rescale keeps activations O(1) (test_host_cpu.py does the same)"""
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "linear") and isinstance(m.linear, torch.nn.Conv2d):
                m.linear.weight.mul_(3.0)
    return net


def install(monkeypatch):
    """emulated kernels + a log of the ops the engine issues: (name, A width, output width, sorted epilogue tensors)"""
    from bcos_hip import ops
    cpu_emulation.install(monkeypatch)
    boundary_fusion_emulation.install(monkeypatch)
    log = []

    def wrap(name, fn):
        def logged(*a, **kw):
            if name == "tapconv":
                log.append((name, a[2]["C"], a[2]["Cout"], tuple(sorted(k for k, v in kw.items() if torch.is_tensor(v)))))
            else:
                log.append((name,))
            return fn(*a, **kw)
        return logged
    for name in LOGGED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return log


def explain_logged(eng, x, log, on):
    from bcos_hip import engine
    engine.set_boundary_fusion(on)
    try:
        del log[:]
        engine.BOUNDARY_FUSION_CALLS = 0
        out = eng.explain(x)
        return out, list(log), engine.BOUNDARY_FUSION_CALLS
    finally:
        engine.set_boundary_fusion(None)


BOUNDARY = ("tapconv", 64, 256, ("addend", "mul", "out", "out2"))
BOUNDARY_SC = ("tapconv", 64, 256, ("addend", "mul", "mul2", "out", "out2"))       # ... below a block with a shortcut convolution


def is_conv3_grad(op):
    return op[0] == "tapconv" and op[1:3] == (256, 64) and "mul" in op[3] and "out" in op[3] and "addend" not in op[3]


@pytest.fixture(scope="module")
def net():
    from bcos_hip import synth
    return small_bottleneck_net(), synth.synthetic_images(2, size=32, seed=3)


def test_fused_call_replaces_exactly_the_pair_and_gives_equal_explanations(net, monkeypatch):
    from bcos_hip import engine
    log = install(monkeypatch)
    model, x = net
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    off, ops_off, n_off = explain_logged(eng, x, log, False)
    on, ops_on, n_on = explain_logged(eng, x, log, True)
    assert n_off == 0 and n_on == 1                  # one site: the output of layer1.0, read by layer1.1 beside its identity shortcut
    assert "mul2" in ops_off[ops_on.index(("boundary_conv3_grad",))][3]          # (layer1.0 has a shortcut convolution: its multiplier rides along)
    assert ("boundary_conv3_grad",) not in ops_off
    at = ops_on.index(("boundary_conv3_grad",))
    assert ops_off[at] in (BOUNDARY, BOUNDARY_SC) and is_conv3_grad(ops_off[at + 1]), ops_off[at:at + 2]
    assert ops_on[:at] == ops_off[:at] and ops_on[at + 1:] == ops_off[at + 2:]
    assert set(on) == set(off)
    for k, v in on.items():
        assert torch.equal(v, off[k]), k
    assert float(on["contribution_map"].abs().max()) > 0


def test_sub_batch_streams_and_functionals_keep_working(net, monkeypatch):
    from bcos_hip import engine, passes
    from bcos_hip.functional import LogitFunctional as LF
    import head_functional_emulation
    log = install(monkeypatch)
    head_functional_emulation.install(monkeypatch)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 1)
    model, x = net
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    f = LF.contrast(torch.tensor([1, 2]), torch.tensor([3, 4]))
    engine.set_boundary_fusion(True)
    try:
        engine.BOUNDARY_FUSION_CALLS = 0
        got = eng.explain_functionals(x, [f, f])
        assert engine.BOUNDARY_FUSION_CALLS == 2      # one fused launch per input-gradient pass over the kept forward
        engine.set_boundary_fusion(False)
        ref = eng.explain_functionals(x, [f, f])
    finally:
        engine.set_boundary_fusion(None)
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k


def capture_site(eng, x, monkeypatch):
    """(consumer, block, record, H, W) of the call of engine._boundary_fusable that answered True"""
    from bcos_hip import engine
    inner, hits = engine._boundary_fusable, []

    def spy(*a):
        r = inner(*a)
        if r:
            hits.append(a)
        return r
    monkeypatch.setattr(engine, "_boundary_fusable", spy)
    engine.set_boundary_fusion(True)
    try:
        eng.explain(x)
    finally:
        engine.set_boundary_fusion(None)
        monkeypatch.setattr(engine, "_boundary_fusable", inner)
    assert len(hits) == 1
    return hits[0]


def test_every_fallback_condition_refuses_the_site(net, monkeypatch):
    """the conditions of the engine, one at a time on the site that is fused otherwise"""
    from bcos_hip import engine, lib, ops
    install(monkeypatch)
    model, x = net
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    consumer, blk, rec0, H, W = capture_site(eng, x, monkeypatch)
    # (the pass consumed its record: rebuild what the predicate reads)
    t3 = torch.ones(tuple(consumer.g_sc.shape))
    rec = dict(rec0, ts=[None, torch.ones(1), t3], td=None, gate_t=None, gated=True)
    fus = engine._boundary_fusable
    engine.set_boundary_fusion(True)
    try:
        assert fus(consumer, blk, rec, H, W)
        c1, c3 = consumer.conv, blk.convs[-1]

        def refused(obj, attr, value):
            old = getattr(obj, attr)
            setattr(obj, attr, value)
            try:
                return not fus(consumer, blk, rec, H, W)
            finally:
                setattr(obj, attr, old)
        assert refused(c1, "cin", 512) and refused(c1, "cout_all", 128)              # another stage's widths
        assert refused(c3, "cin", 128) and refused(c3, "cout_all", 512)
        assert refused(consumer, "shortcut_conv", c1)                               # a shortcut convolution: the addend is not the identity gradient
        assert refused(blk, "pool", 2)                                              # CLIP's pool between conv2 and conv3
        assert refused(c1, "max_out", 2) and refused(c3, "max_out", 2)              # MaxOut
        assert refused(c3, "b", 1.5) and refused(c1, "b", 2.5)
        assert refused(blk, "convs", blk.convs[-1:])                                # no conv below conv3
        assert fus(consumer, blk, dict(rec, td=t3), H, W)                           # (a shortcut multiplier below is part of the call)
        for key, val in (("gated", False), ("gate_t", t3), ("td", t3[..., :8])):    # no ReLU / a gate tensor / a multiplier of another shape
            assert not fus(consumer, blk, dict(rec, **{key: val}), H, W), key
        assert not fus(consumer, blk, rec, H + 1, W)
        assert not fus(engine._RawConsumer(consumer.g_main), blk, rec, H, W)         # the reader is not a plain _Consumer
        assert not fus(engine._Consumer(engine._HeadConv(c1.dgrad, 256), consumer.g_main, None, consumer.g_sc, 0), blk, rec, H, W)
        real_absmax_of = ops.absmax_of
        monkeypatch.setattr(ops, "absmax_of", lambda t: None)                       # no per-pixel maxima of the gradient
        assert not fus(consumer, blk, rec, H, W)
        monkeypatch.setattr(ops, "absmax_of", real_absmax_of)
        assert fus(consumer, blk, rec, H, W)
        # what the entry point and its binding refuse (BCOS_E_NOSUP): a weight bank without its pre-split image, the development switch
        # that splits inside the kernels, tensors of 2 GiB and more, views that are not contiguous
        assert refused(c1.dgrad.classes[0][8], "_bcos_static", False) and refused(c3.dgrad.classes[0][8], "_bcos_static", False)
        assert refused(ops, "_NO_PRESPLIT", True)
        assert refused(consumer, "g_main", consumer.g_main.transpose(1, 2))
        assert not fus(consumer, blk, dict(rec, ts=[None, torch.ones(4, 2).t(), t3]), H, W)

        def site_of(n):          # the same site with n images, on the meta device: shapes and maxima without the memory
            g = torch.empty((n, H, W, 64), device="meta")
            ops._attach_absmax(g, torch.empty(n * H * W, device="meta", dtype=torch.int32))
            wide = torch.empty((n, H, W, 256), device="meta")
            return engine._Consumer(c1, g, None, wide, 0), dict(rec, ts=[None, torch.ones(1), wide])
        limit = 2 ** 31 // (H * W * 1024)          # the first image count whose [M, 256] fp32 tensors reach 2 GiB
        big, big_rec = site_of(limit)
        assert not fus(big, blk, big_rec, H, W)
        ok, ok_rec = site_of(limit - 1)
        assert fus(ok, blk, ok_rec, H, W)
        old = lib.get_contraction_mode()
        try:
            for mode in ("bf16x3", "f32"):
                lib.set_contraction_mode(mode)
                assert not fus(consumer, blk, rec, H, W), mode
        finally:
            lib.set_contraction_mode(old)
        engine.set_boundary_fusion(False)
        assert not fus(consumer, blk, rec, H, W)
    finally:
        engine.set_boundary_fusion(None)


@pytest.mark.parametrize("case", ["switch_off", "bf16x3", "basic_blocks", "one_block_per_stage", "no_presplit", "call_refuses"])
def test_fallbacks_leave_the_op_sequence_of_the_parent(case, net, monkeypatch):
    """whole passes: with the fusion allowed but a condition unmet, the ops are those of a pass with the fusion switched off"""
    from bcos_hip import engine, lib, ops, synth
    log = install(monkeypatch)
    model, x = net
    if case == "no_presplit":
        monkeypatch.setattr(ops, "_NO_PRESPLIT", True)
    elif case == "call_refuses":
        # a refusal the engine's predicate did not foresee: the call answers BCOS_E_NOSUP before it launches anything
        def refuse(*a, **kw):
            err = lib.BcosHipError("bcos_boundary_conv3_grad failed with code -95")
            err.code = lib.BCOS_E_NOSUP
            raise err
        monkeypatch.setattr(ops, "boundary_conv3_grad", refuse)
    if case == "basic_blocks":
        model = rescaled(synth.build_bcosified_resnet("resnet18"))
    elif case == "one_block_per_stage":
        model = rescaled(synth.build_bcosified_resnet("resnet14b"))
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    old = lib.get_contraction_mode()
    try:
        if case == "bf16x3":
            lib.set_contraction_mode("bf16x3")
        ref, ops_ref, _ = explain_logged(eng, x, log, False)
        got, ops_got, n = explain_logged(eng, x, log, case != "switch_off")
    finally:
        lib.set_contraction_mode(old)
    assert n == 0 and ops_got == ops_ref and ("boundary_conv3_grad",) not in ops_got
    assert BOUNDARY_SC in ops_ref or case in ("basic_blocks", "one_block_per_stage")
    for k, v in got.items():
        assert torch.equal(v, ref[k]), k


def test_environment_switch():
    """BCOS_BOUNDARY_FUSION as a fresh process reads it: unset and 1 = on, 0 = off; set_boundary_fusion overrides and hands back"""
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "b-cosification_amd")
    code = ("import sys; sys.path.insert(0, %r)\nfrom bcos_hip import engine as e\n"
            "a = e._BOUNDARY_FUSION; p = e.set_boundary_fusion(not a); b = e._BOUNDARY_FUSION; e.set_boundary_fusion(None)\n"
            "print(int(a), int(p), int(b), int(e._BOUNDARY_FUSION))" % pkg)
    for value, on in ((None, 1), ("1", 1), ("0", 0)):
        env = {k: v for k, v in os.environ.items() if k != "BCOS_BOUNDARY_FUSION"}
        if value is not None:
            env["BCOS_BOUNDARY_FUSION"] = value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert out.stdout.split() == [str(on), str(on), str(1 - on), str(on)], (value, out.stdout, out.stderr[-500:])


def test_argument_rejection_codes(hip_lib):
    """the C entry point refuses before any HIP call: BCOS_E_INVAL for malformed calls, BCOS_E_NOSUP outside its one configuration"""
    from bcos_hip import lib
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16

    def call(**over):
        a = lib.BoundaryConv3()
        for k in ("g1", "g1_absmax", "w1_f16x2", "addend", "t3", "out2", "out2_absmax", "w3_f16x2", "t2", "g3", "g3_absmax"):
            setattr(a, k, base)
        a.N, a.PQ, a.C1, a.C4, a.kh, a.kw, a.stride, a.contraction, a.b = 2, 25, 64, 256, 1, 1, 1, lib.CONTRACT_F16X2, 2.0
        for k, v in over.items():
            setattr(a, k, v)
        rc = hip_lib.bcos_boundary_conv3_grad(C.byref(a), None)
        assert rc != 0 and b"bcos_boundary_conv3_grad" in hip_lib.bcos_last_error_string()
        return rc
    INVAL, NOSUP = -22, lib.BCOS_E_NOSUP
    assert hip_lib.bcos_boundary_conv3_grad(None, None) == INVAL
    for k in ("g1", "addend", "t3", "out2", "t2", "g3"):
        assert call(**{k: None}) == INVAL, k
    assert call(N=0) == INVAL and call(PQ=-1) == INVAL
    assert call(g3_imgmax=base) == INVAL and call(g3_imgmin_c=base) == INVAL
    assert call(g3_imgmax=base, g3_imgmin_c=base, g3_absmax=None) == INVAL
    assert call(mul_csc=base) == INVAL and call(mul_csh=base) == INVAL
    assert call(C1=128) == NOSUP and call(C4=512) == NOSUP
    assert call(kh=3, kw=3) == NOSUP and call(stride=2) == NOSUP
    assert call(b=1.5) == NOSUP
    assert call(contraction=lib.CONTRACT_BF16X3) == NOSUP and call(contraction=lib.CONTRACT_F32) == NOSUP
    assert call(w1_f16x2=None) == NOSUP and call(w3_f16x2=None) == NOSUP and call(g1_absmax=None) == NOSUP
    assert call(N=1 << 10, PQ=1 << 11) == NOSUP                      # 2 GiB
    for k in ("g1", "addend", "t3", "mul2", "out2", "t2", "g3", "w1_f16x2", "w3_f16x2"):
        assert call(**{k: base + 4}) == NOSUP, k
    assert call(g3_absmax=base + 2) == NOSUP
    old = hip_lib.bcos_get_contraction_mode()
    try:
        hip_lib.bcos_set_contraction_mode(1)
        assert call(contraction=lib.CONTRACT_DEFAULT) == NOSUP
    finally:
        hip_lib.bcos_set_contraction_mode(old)


def test_entry_point_is_declared_bound_and_built():
    import os
    import re
    from bcos_hip import lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bcos_hip.h")).read()
    assert re.search(r"\bint bcos_boundary_conv3_grad\(", header) and "bcos_boundary_conv3_grad" in lib.SIGNATURES
    assert "bcos_boundary.hip" in lib.SOURCES and f"#define BCOS_ABI_VERSION {lib.ABI_VERSION}" in header
    fields = re.search(r"typedef struct bcos_boundary_conv3 \{(.*?)\} bcos_boundary_conv3;", header, flags=re.S).group(1)
    declared = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [n for n, _ in lib.BoundaryConv3._fields_], declared
