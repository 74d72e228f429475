"""`-m "not gpu"`: the fused shortcut launch (ops.shortcut_conv3_fwd / bcos_shortcut_conv3_fwd) on the host side -- when the engine
issues it, what it replaces, when it falls back, and how the C entry point rejects arguments.

Kernels are the interpreters of tests/cpu_emulation.py and tests/shortcut_fusion_emulation.py.  The network is a Bottleneck ResNet with
one block per stage on 32 x 32 images: layer1.0 (64, 64 -> 256, stride 1) and layer2.0 (128, 256 -> 512, stride 2) are the two
configurations the call takes; layer3.0 and layer4.0 keep the pair of launches.  The engine hands only layer1.0 to the call by default
(the stride-2 site measured no gain on the device); BOTH widens engine._SHORTCUT_CONFIGS to what the call supports."""
import ctypes as C

import pytest
import torch

import cpu_emulation
import shortcut_fusion_emulation
from test_boundary_fusion_cpu import rescaled, small_bottleneck_net

LOGGED = ("tapconv", "shortcut_conv3_fwd", "avgpool2d_fwd", "global_avgpool_logits", "prep_input")
FUSED = ("shortcut_conv3_fwd",)
BOTH = ((64, 64, 1, 256), (128, 256, 2, 512))


def install(monkeypatch):
    """emulated kernels + a log of the ops the engine issues: (name, A width, output width, stride, sorted epilogue tensors)"""
    from bcos_hip import ops
    cpu_emulation.install(monkeypatch)
    shortcut_fusion_emulation.install(monkeypatch)
    log = []

    def wrap(name, fn):
        def logged(*a, **kw):
            if name == "tapconv":
                log.append((name, a[2]["C"], a[2]["Cout"], a[2]["in_sh"], tuple(sorted(k for k, v in kw.items() if torch.is_tensor(v)))))
            else:
                log.append((name,))
            return fn(*a, **kw)
        return logged
    for name in LOGGED:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return log


def run_logged(eng, x, log, on, what="explain", **kw):
    from bcos_hip import engine
    engine.set_shortcut_fusion(on)
    try:
        del log[:]
        engine.SHORTCUT_FUSION_CALLS = 0
        out = getattr(eng, what)(x, **kw)
        return out, list(log), engine.SHORTCUT_FUSION_CALLS
    finally:
        engine.set_shortcut_fusion(None)


def same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return set(a) == set(b) and all(torch.equal(v, b[k]) for k, v in a.items())


@pytest.fixture(scope="module")
def net():
    from bcos_hip import synth
    return small_bottleneck_net(layers=(1, 1, 1, 1)), synth.synthetic_images(2, size=32, seed=3)


@pytest.mark.parametrize("what,configs", [("explain", None), ("forward", None), ("explain", BOTH)], ids=["explain", "forward", "explain-both"])
def test_fused_call_replaces_exactly_the_pair_and_gives_equal_results(net, monkeypatch, what, configs):
    from bcos_hip import engine
    log = install(monkeypatch)
    if configs is not None:
        monkeypatch.setattr(engine, "_SHORTCUT_CONFIGS", configs)
    model, x = net
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    off, ops_off, n_off = run_logged(eng, x, log, False, what)
    on, ops_on, n_on = run_logged(eng, x, log, True, what)
    pairs = [(64, 64, 1), (128, 256, 2)][:1 if configs is None else 2]      # (K3, Kd, stride) of layer1.0 [and layer2.0], in execution order
    assert n_off == 0 and n_on == len(pairs) and FUSED not in ops_off and ops_on.count(FUSED) == len(pairs)
    kept = what == "explain"                        # the multipliers are written in the explanation pass only
    i = j = 0
    while i < len(ops_on):
        if ops_on[i] == FUSED:
            k3, kd, s = pairs.pop(0)
            sc, c3 = ops_off[j], ops_off[j + 1]
            assert sc[:4] == ("tapconv", kd, 4 * k3, s) and "addend" not in sc[4] and ("scale_out" in sc[4]) == kept, sc
            assert c3[:4] == ("tapconv", k3, 4 * k3, 1) and "addend" in c3[4] and ("scale_out" in c3[4]) == kept, c3
            j += 2
        else:
            assert ops_on[i] == ops_off[j], (i, ops_on[i], ops_off[j])
            j += 1
        i += 1
    assert j == len(ops_off) and not pairs
    # layer3.0 / layer4.0 (and by default layer2.0) keep the pair
    left = [o[:4] for o in ops_on if o[0] == "tapconv" and o[3] == 2 and o[2] == 2 * o[1]]
    assert left == [("tapconv", 256, 512, 2)][:1 if configs is None else 0] + [("tapconv", 512, 1024, 2), ("tapconv", 1024, 2048, 2)]
    assert same(on, off)
    if what == "explain":
        assert float(on["contribution_map"].abs().max()) > 0 and float(on["dynamic_linear_weights"].abs().max()) > 0


def test_sub_batch_streams_and_explain_targets_keep_working(net, monkeypatch):
    from bcos_hip import engine, passes
    import test_passes_cpu
    install(monkeypatch)
    monkeypatch.setattr(engine, "_SHORTCUT_CONFIGS", BOTH)
    test_passes_cpu.Streams(monkeypatch)             # (side streams on the host: the scheduler's stand-ins of that file)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 1)
    model, x = net
    eng = engine.ResNetEngine(model)
    targets = torch.tensor([[1, 2], [3, 4]])
    for streams in (1, 2):
        eng.subbatch_streams = streams
        engine.set_shortcut_fusion(True)
        try:
            engine.SHORTCUT_FUSION_CALLS = 0
            got = eng.explain(x)
            assert engine.SHORTCUT_FUSION_CALLS == 2 * streams          # two sites per forward, one forward per sub-batch
            engine.SHORTCUT_FUSION_CALLS = 0
            got_t = eng.explain_targets(x, targets) if streams == 1 else None
            assert streams > 1 or engine.SHORTCUT_FUSION_CALLS == 2    # ONE kept forward serves every target's pass
            engine.set_shortcut_fusion(False)
            ref = eng.explain(x)
            ref_t = eng.explain_targets(x, targets) if streams == 1 else None
        finally:
            engine.set_shortcut_fusion(None)
        assert same(got, ref) and (streams > 1 or same(got_t, ref_t))


def capture_sites(eng, x, monkeypatch):
    """the arguments (block, shortcut input, conv3 input, gates) of the calls of engine._shortcut_fusable that answered True"""
    from bcos_hip import engine
    inner, hits = engine._shortcut_fusable, []

    def spy(*a):
        r = inner(*a)
        if r:
            hits.append(a)
        return r
    monkeypatch.setattr(engine, "_shortcut_fusable", spy)
    monkeypatch.setattr(engine, "_SHORTCUT_CONFIGS", BOTH)
    engine.set_shortcut_fusion(True)
    try:
        eng.explain(x)
    finally:
        engine.set_shortcut_fusion(None)
        monkeypatch.setattr(engine, "_shortcut_fusable", inner)
    assert len(hits) == 2
    return hits


def test_every_fallback_condition_refuses_the_site(net, monkeypatch):
    """the conditions of the engine, one at a time on the sites that are fused otherwise"""
    from bcos_hip import engine, lib, ops
    install(monkeypatch)
    model, x = net
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    fus = engine._shortcut_fusable
    engine.set_shortcut_fusion(True)
    try:
        for blk, sc_in, h, gates in capture_sites(eng, x, monkeypatch):
            assert gates is None and fus(blk, sc_in, h, None)
            cd, c3 = blk.shortcut, blk.convs[-1]

            def refused(obj, attr, value):
                old = getattr(obj, attr)
                setattr(obj, attr, value)
                try:
                    return not fus(blk, sc_in, h, None)
                finally:
                    setattr(obj, attr, old)
            assert not fus(blk, sc_in, h, [torch.ones(1)])                               # replayed gates
            assert refused(engine, "_GATE_TENSOR", True)                               # the gate as a tensor of its own
            assert refused(ops, "_NO_PRESPLIT", True)                                  # weights split inside the kernels
            assert refused(cd.w_fwd, "_bcos_static", False) and refused(c3.w_fwd, "_bcos_static", False)
            assert refused(cd, "max_out", 2) and refused(c3, "max_out", 2)             # MaxOut
            assert refused(cd, "b", 1.5) and refused(c3, "b", 2.5)                     # B != 2
            assert refused(cd, "force_pow", True) and refused(c3, "force_pow", True)
            assert refused(cd, "bias", torch.zeros(cd.cout)) and refused(c3, "bias", torch.zeros(c3.cout))
            assert refused(blk, "shortcut_pool", 2) and refused(blk, "pool", 2)        # CLIP's anti-aliasing pools
            assert refused(blk, "relu", False)
            assert refused(cd, "groups", 2) and refused(c3, "groups", 2)
            assert refused(cd, "k", (3, 3)) and refused(c3, "k", (3, 3))
            assert refused(cd, "cin", 512) and refused(c3, "cin", 256) and refused(c3, "cout", 1024)      # another stage's widths
            assert refused(cd, "stride", (3 - cd.stride[0],) * 2)                      # the other configuration's stride
            assert refused(blk, "shortcut", None) and refused(blk, "convs", blk.convs[-2:])
            real_absmax_of = ops.absmax_of
            for missing in (sc_in, h):                                                 # no per-pixel maxima of one operand
                monkeypatch.setattr(ops, "absmax_of", lambda t: None if t is missing else real_absmax_of(t))
                assert not fus(blk, sc_in, h, None)
            monkeypatch.setattr(ops, "absmax_of", real_absmax_of)
            assert not fus(blk, sc_in.transpose(1, 2), h, None) and not fus(blk, sc_in, h.transpose(1, 2), None)
            assert refused(engine, "_SHORTCUT_CONFIGS", tuple(c for c in BOTH if c[0] != c3.cin))      # a site left to the pair of launches
            assert refused(ops, "F16X2_MIN_K", 512)                                    # the pair would run the bf16x3 loop
            # CPU operands reach the call only where an emulator stands in its place
            native = lambda *a, **kw: None      # noqa: E731
            native.native = True
            assert refused(ops, "shortcut_conv3_fwd", native)
            old = lib.get_contraction_mode()
            try:
                for mode in ("bf16x3", "f32"):
                    lib.set_contraction_mode(mode)
                    assert not fus(blk, sc_in, h, None), mode
            finally:
                lib.set_contraction_mode(old)
            assert fus(blk, sc_in, h, None)
        # tensors of 2 GiB and more (the meta device: shapes and maxima without the memory)
        blk, sc_in, h, _ = capture_sites(eng, x, monkeypatch)[0]

        def site_of(n):
            H, W = sc_in.shape[1:3]
            a, b = torch.empty((n, H, W, 64), device="meta"), torch.empty((n, H, W, 64), device="meta")
            for t in (a, b):
                ops._attach_absmax(t, torch.empty(n * H * W, device="meta", dtype=torch.int32))
            return a, b
        limit = 2 ** 31 // (sc_in.shape[1] * sc_in.shape[2] * 1024)
        assert fus(blk, *site_of(limit - 1), None) and not fus(blk, *site_of(limit), None)
        engine.set_shortcut_fusion(False)
        assert not fus(blk, sc_in, h, None)
    finally:
        engine.set_shortcut_fusion(None)


@pytest.mark.parametrize("case", ["switch_off", "bf16x3", "basic_blocks", "no_presplit", "call_refuses", "replayed_gates", "native_on_cpu"])
def test_fallbacks_leave_the_op_sequence_of_the_parent(case, net, monkeypatch):
    """whole passes: with the fusion allowed but a condition unmet, the ops are those of a pass with the fusion switched off"""
    from bcos_hip import engine, lib, ops, synth
    import test_passes_cpu
    log = install(monkeypatch)
    model, x = net
    if case == "no_presplit":
        monkeypatch.setattr(ops, "_NO_PRESPLIT", True)
    elif case == "call_refuses":
        # a refusal the engine's predicate did not foresee: the call answers BCOS_E_NOSUP before it launches anything
        def refuse(*a, **kw):
            err = lib.BcosHipError("bcos_shortcut_conv3_fwd failed with code -95")
            err.code = lib.BCOS_E_NOSUP
            raise err
        monkeypatch.setattr(ops, "shortcut_conv3_fwd", refuse)
    elif case == "native_on_cpu":
        def native(*a, **kw):
            raise AssertionError("the native call was reached with CPU tensors")
        native.native = True
        monkeypatch.setattr(ops, "shortcut_conv3_fwd", native)
    if case == "basic_blocks":
        model = rescaled(synth.build_bcosified_resnet("resnet18"))
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    kw = {}
    if case == "replayed_gates":
        engine.set_shortcut_fusion(False)
        try:
            kw = dict(gates=test_passes_cpu.relu_gates(eng, x, monkeypatch))
        finally:
            engine.set_shortcut_fusion(None)
    old = lib.get_contraction_mode()
    try:
        if case == "bf16x3":
            lib.set_contraction_mode("bf16x3")
        ref, ops_ref, _ = run_logged(eng, x, log, False, **kw)
        got, ops_got, n = run_logged(eng, x, log, case != "switch_off", **kw)
    finally:
        lib.set_contraction_mode(old)
    assert n == 0 and ops_got == ops_ref and FUSED not in ops_got
    assert same(got, ref)


def test_environment_switch():
    """BCOS_SHORTCUT_FUSION as a fresh process reads it: unset and 1 = on, 0 = off; set_shortcut_fusion overrides and hands back"""
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "b-cosification_amd")
    code = ("import sys; sys.path.insert(0, %r)\nfrom bcos_hip import engine as e\n"
            "a = e._SHORTCUT_FUSION; p = e.set_shortcut_fusion(not a); b = e._SHORTCUT_FUSION; e.set_shortcut_fusion(None)\n"
            "print(int(a), int(p), int(b), int(e._SHORTCUT_FUSION))" % pkg)
    for value, on in ((None, 1), ("1", 1), ("0", 0)):
        env = {k: v for k, v in os.environ.items() if k != "BCOS_SHORTCUT_FUSION"}
        if value is not None:
            env["BCOS_SHORTCUT_FUSION"] = value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert out.stdout.split() == [str(on), str(on), str(1 - on), str(on)], (value, out.stdout, out.stderr[-500:])


def test_argument_rejection_codes(hip_lib):
    """the C entry point refuses before any HIP call: BCOS_E_INVAL for malformed calls, BCOS_E_NOSUP outside its two configurations"""
    from bcos_hip import lib
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16
    cfg1 = dict(K3=64, Kd=64, stride=1, C4=256)
    cfg2 = dict(K3=128, Kd=256, stride=2, C4=512)

    def call(**over):
        a = lib.ShortcutConv3()
        for k in ("x", "x_absmax", "wd_f16x2", "csc_d", "csh_d", "td", "h", "h_absmax", "w3_f16x2", "csc_3", "csh_3", "out", "t3", "out_absmax"):
            setattr(a, k, base)
        a.N, a.H, a.W, a.kh, a.kw, a.max_out, a.groups, a.contraction, a.flags, a.b = 2, 5, 5, 1, 1, 1, 1, lib.CONTRACT_F16X2, 0, 2.0
        for k, v in dict(cfg1, **over).items():
            setattr(a, k, v)
        rc = hip_lib.bcos_shortcut_conv3_fwd(C.byref(a), None)
        assert rc != 0 and b"bcos_shortcut_conv3_fwd" in hip_lib.bcos_last_error_string()
        return rc
    INVAL, NOSUP = -22, lib.BCOS_E_NOSUP
    assert hip_lib.bcos_shortcut_conv3_fwd(None, None) == INVAL
    for k in ("x", "h", "out"):
        assert call(**{k: None}) == INVAL, k
    assert call(N=0) == INVAL and call(H=-1) == INVAL and call(W=0) == INVAL
    assert call(td=None) == INVAL and call(t3=None) == INVAL                     # the multipliers go together
    assert call(flags=lib.BCOS_EPI_SCALE_GATE_LSB | lib.BCOS_EPI_FORCE_POW) == INVAL
    for bad in (dict(K3=128), dict(Kd=256), dict(stride=2), dict(C4=512), dict(cfg2, stride=1), dict(cfg2, K3=64), dict(cfg2, C4=1024),
                dict(K3=256, Kd=512, stride=2, C4=1024)):
        assert call(**bad) == NOSUP, bad
    assert call(kh=3, kw=3) == NOSUP and call(kw=3) == NOSUP
    assert call(b=1.5) == NOSUP and call(max_out=2) == NOSUP and call(groups=2) == NOSUP
    assert call(bias_d=base) == NOSUP and call(bias_3=base) == NOSUP and call(relu_gate=base) == NOSUP
    assert call(contraction=lib.CONTRACT_BF16X3) == NOSUP and call(contraction=lib.CONTRACT_F32) == NOSUP
    for k in ("wd_f16x2", "w3_f16x2", "x_absmax", "h_absmax"):
        assert call(**{k: None}) == NOSUP, k
    assert call(N=1 << 10, H=1 << 6, W=1 << 5) == NOSUP                          # out: 2 GiB
    assert call(**dict(cfg2, N=1 << 10, H=1 << 6, W=1 << 5)) == NOSUP            # x: 2 GiB
    for k in ("x", "h", "out", "t3", "td", "wd_f16x2", "w3_f16x2", "csc_d", "csh_d", "csc_3", "csh_3"):
        assert call(**{k: base + 4}) == NOSUP, k
    for k in ("x_absmax", "h_absmax", "out_absmax"):
        assert call(**{k: base + 2}) == NOSUP, k
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
    assert re.search(r"\bint bcos_shortcut_conv3_fwd\(", header) and "bcos_shortcut_conv3_fwd" in lib.SIGNATURES
    assert "bcos_shortcut.hip" in lib.SOURCES and f"#define BCOS_ABI_VERSION {lib.ABI_VERSION}" in header and lib.ABI_VERSION == 12
    fields = re.search(r"typedef struct bcos_shortcut_conv3 \{(.*?)\} bcos_shortcut_conv3;", header, flags=re.S).group(1)
    declared = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert declared == [n for n, _ in lib.ShortcutConv3._fields_], declared
