"""`-m "not gpu"`: the fused stem launch (ops.stem_conv_fwd / bcos_stem_conv_fwd) on the host side -- when the engine issues it, what it
replaces, when it falls back, and how the C entry point rejects arguments.

Kernels are the interpreters of tests/cpu_emulation.py and tests/stem_kernel_emulation.py.  The network is a Bottleneck ResNet with one
block per stage on 32 x 32 images (and ResNet-18 for the basic-block plan)."""
import ctypes as C

import pytest
import torch

import cpu_emulation
import stem_kernel_emulation
from test_boundary_fusion_cpu import rescaled, small_bottleneck_net

LOGGED = ("tapconv", "stem_conv_fwd", "prep_input", "avgpool2d_fwd", "global_avgpool_logits", "finalize_explanation")
FUSED = ("stem_conv_fwd",)
PREP = ("prep_input",)


def install(monkeypatch):
    """emulated kernels + a log of the ops the engine issues: (name, A width, output width, stride, sorted epilogue tensors)"""
    from bcos_hip import ops
    cpu_emulation.install(monkeypatch)
    stem_kernel_emulation.install(monkeypatch)
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
    engine.set_stem_kernel(on)
    try:
        del log[:]
        engine.STEM_KERNEL_CALLS = 0
        out = getattr(eng, what)(x, **kw)
        return out, list(log), engine.STEM_KERNEL_CALLS
    finally:
        engine.set_stem_kernel(None)


def same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return set(a) == set(b) and all(torch.equal(v, b[k]) for k, v in a.items())


@pytest.fixture(scope="module")
def net():
    from bcos_hip import synth
    return small_bottleneck_net(layers=(1, 1, 1, 1)), synth.synthetic_images(2, size=32, seed=3)


@pytest.mark.parametrize("what", ["explain", "forward"])
@pytest.mark.parametrize("channels", [6, 3])
def test_fused_call_replaces_exactly_the_pair_and_gives_equal_results(net, monkeypatch, what, channels):
    from bcos_hip import engine
    log = install(monkeypatch)
    model, x = net
    x = x[:, :channels]                             # (3 channels: the engine applies AddInverse)
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    off, ops_off, n_off = run_logged(eng, x, log, False, what)
    on, ops_on, n_on = run_logged(eng, x, log, True, what)
    assert n_off == 0 and n_on == 1 and FUSED not in ops_off and ops_on.count(FUSED) == 1 and PREP not in ops_on
    # the pass with the switch off starts with prep_input and the stem's tapconv; the fused call stands exactly in their place
    kept = what == "explain"
    assert ops_off[0] == PREP and ops_off[1][:4] == ("tapconv", 8, 64, 2) and ("scale_out" in ops_off[1][4]) == kept
    assert ops_on[0] == FUSED and ops_on[1:] == ops_off[2:]
    assert same(on, off)
    if what == "explain":
        assert float(on["contribution_map"].abs().max()) > 0 and float(on["dynamic_linear_weights"].abs().max()) > 0


def test_sub_batch_streams_keep_working(net, monkeypatch):
    from bcos_hip import engine, passes
    import test_passes_cpu
    install(monkeypatch)
    test_passes_cpu.Streams(monkeypatch)             # (side streams on the host: the scheduler's stand-ins of that file)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 1)
    model, x = net
    eng = engine.ResNetEngine(model)
    for streams in (1, 2):
        eng.subbatch_streams = streams
        engine.set_stem_kernel(True)
        try:
            engine.STEM_KERNEL_CALLS = 0
            got = eng.explain(x)
            assert engine.STEM_KERNEL_CALLS == streams          # one forward per sub-batch
            engine.set_stem_kernel(False)
            ref = eng.explain(x)
        finally:
            engine.set_stem_kernel(None)
        assert same(got, ref)


def test_every_fallback_condition_refuses_the_site(net, monkeypatch):
    """the conditions of the engine, one at a time on a stem that is fused otherwise"""
    from bcos_hip import engine, lib, ops, plan
    install(monkeypatch)
    model, x = net
    eng = engine.ResNetEngine(model)
    fus = engine._stem_fusable
    src = plan.Images(x)
    c = eng.stem[0][0]
    engine.set_stem_kernel(True)
    try:
        assert fus(eng, src, None)

        def refused(obj, attr, value):
            old = getattr(obj, attr)
            setattr(obj, attr, value)
            try:
                return not fus(eng, src, None)
            finally:
                setattr(obj, attr, old)
        assert not fus(eng, src, [torch.ones(1)])                                      # replayed gates
        assert refused(engine, "_GATE_TENSOR", True)                                   # the gate as a tensor of its own
        assert refused(ops, "_NO_PRESPLIT", True)                                      # weights split inside the kernels
        assert refused(c.w_fwd, "_bcos_static", False)
        assert refused(c, "max_out", 2) and refused(c, "groups", 2)                    # MaxOut, groups
        assert refused(c, "b", 1.5) and refused(c, "force_pow", True)                  # B != 2
        assert refused(c, "bias", torch.zeros(c.cout))
        assert refused(c, "k", (3, 3)) and refused(c, "stride", (1, 1)) and refused(c, "padding", (2, 2)) and refused(c, "dilation", (2, 2))
        assert refused(c, "cout", 32) and refused(c, "cin", 8)                         # other widths
        assert refused(eng, "stem", eng.stem * 3)                                      # CLIP's 3-conv stem
        # occluded, perturbed and RISE-prepared inputs keep their own prep launches
        for cls in (plan.OccludedCopies, plan.PerturbedCopies, plan.RiseCopies):
            other = object.__new__(cls)
            other.x = x
            assert not fus(eng, other, None), cls.__name__
        view = plan.Images(x)
        view.x = x.transpose(2, 3)                                                     # not contiguous
        assert not fus(eng, view, None)
        # CPU operands reach the call only where an emulator stands in its place
        native = lambda *a, **kw: None      # noqa: E731
        native.native = True
        assert refused(ops, "stem_conv_fwd", native)
        old = lib.get_contraction_mode()
        try:
            for mode in ("bf16x3", "f32"):
                lib.set_contraction_mode(mode)
                assert not fus(eng, src, None), mode
        finally:
            lib.set_contraction_mode(old)
        # tensors of 2 GiB and more (the meta device: shapes without the memory)
        big = plan.Images(x)
        limit = 2 ** 31 // (128 * 128 * 64 * 4)          # images [n, 6, 256, 256]: the output [n, 128, 128, 64] is the larger tensor
        big.x = torch.empty((limit - 1, 6, 256, 256), device="meta")
        assert fus(eng, big, None)
        big.x = torch.empty((limit, 6, 256, 256), device="meta")
        assert not fus(eng, big, None)
        big.x = torch.empty((65536, 6, 8, 8), device="meta")          # more images than the launch's grid takes
        assert not fus(eng, big, None)
        assert fus(eng, src, None)
        engine.set_stem_kernel(False)
        assert not fus(eng, src, None)
    finally:
        engine.set_stem_kernel(None)


@pytest.mark.parametrize("case", ["switch_off", "bf16x3", "no_presplit", "call_refuses", "replayed_gates", "native_on_cpu", "occluded"])
def test_fallbacks_leave_the_op_sequence_of_the_parent(case, net, monkeypatch):
    """whole passes: with the fused launch allowed but a condition unmet, the ops are those of a pass with it switched off"""
    from bcos_hip import engine, lib, ops
    import test_passes_cpu
    log = install(monkeypatch)
    model, x = net
    if case == "no_presplit":
        monkeypatch.setattr(ops, "_NO_PRESPLIT", True)
    elif case == "call_refuses":
        # a refusal the engine's predicate did not foresee: the call answers BCOS_E_NOSUP before it launches anything
        def refuse(*a, **kw):
            log.append(("refused",))
            err = lib.BcosHipError("bcos_stem_conv_fwd failed with code -95")
            err.code = lib.BCOS_E_NOSUP
            raise err
        monkeypatch.setattr(ops, "stem_conv_fwd", refuse)
    elif case == "native_on_cpu":
        def native(*a, **kw):
            raise AssertionError("the native call was reached with CPU tensors")
        native.native = True
        monkeypatch.setattr(ops, "stem_conv_fwd", native)
    eng = engine.ResNetEngine(model)
    eng.subbatch_streams = 1
    kw, what = {}, "explain"
    if case == "replayed_gates":
        engine.set_stem_kernel(False)
        try:
            kw = dict(gates=test_passes_cpu.relu_gates(eng, x, monkeypatch))
        finally:
            engine.set_stem_kernel(None)
    if case == "occluded":
        what, x = "forward", x[:1]
        kw = dict(occlude=torch.tensor([[0, 8, 0, 8], [4, 20, 4, 20]], dtype=torch.int32))
        monkeypatch.setattr(ops, "prep_input_occluded", lambda xx, rects, mean, std, first=0, n=None, cpad=8, want_absmax=False:
                            cpu_emulation.prep_input(torch.stack([xx[0] * occlusion_mask(xx, r) for r in rects[first:first + (n or len(rects))]]),
                                                     mean, std, cpad=cpad))
    old = lib.get_contraction_mode()
    try:
        if case == "bf16x3":
            lib.set_contraction_mode("bf16x3")
        ref, ops_ref, _ = run_logged(eng, x, log, False, what, **kw)
        got, ops_got, n = run_logged(eng, x, log, case != "switch_off", what, **kw)
    finally:
        lib.set_contraction_mode(old)
    assert n == 0 and FUSED not in ops_got
    assert [o for o in ops_got if o != ("refused",)] == ops_ref and (("refused",) in ops_got) == (case == "call_refuses")
    assert same(got, ref)


def occlusion_mask(x, rect):
    r0, r1, c0, c1 = (int(v) for v in rect)
    m = torch.ones_like(x[0])
    m[:, r0:r1, c0:c1] = 0
    return m


def test_basic_block_network_takes_the_call_too(monkeypatch):
    from bcos_hip import engine, synth
    log = install(monkeypatch)
    eng = engine.ResNetEngine(rescaled(synth.build_bcosified_resnet("resnet18")))
    eng.subbatch_streams = 1
    x = synth.synthetic_images(2, size=32, seed=3)
    off, ops_off, n_off = run_logged(eng, x, log, False)
    on, ops_on, n_on = run_logged(eng, x, log, True)
    assert (n_off, n_on) == (0, 1) and ops_on[0] == FUSED and ops_on[1:] == ops_off[2:] and same(on, off)


def test_environment_switch():
    """BCOS_STEM_KERNEL as a fresh process reads it: unset and 1 = on, 0 = off; set_stem_kernel overrides and hands back"""
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "b-cosification_amd")
    code = ("import sys; sys.path.insert(0, %r)\nfrom bcos_hip import engine as e\n"
            "a = e._STEM_KERNEL; p = e.set_stem_kernel(not a); b = e._STEM_KERNEL; e.set_stem_kernel(None)\n"
            "print(int(a), int(p), int(b), int(e._STEM_KERNEL))" % pkg)
    for value, on in ((None, 1), ("1", 1), ("0", 0)):
        env = {k: v for k, v in os.environ.items() if k != "BCOS_STEM_KERNEL"}
        if value is not None:
            env["BCOS_STEM_KERNEL"] = value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert out.stdout.split() == [str(on), str(on), str(1 - on), str(on)], (value, out.stdout, out.stderr[-500:])


def test_argument_rejection_codes(hip_lib):
    """the C entry point refuses before any HIP call: BCOS_E_INVAL for malformed calls, BCOS_E_NOSUP outside its one configuration"""
    from bcos_hip import lib
    buf = (C.c_float * 1024)()
    base = C.addressof(buf)
    base += (-base) % 16

    def call(**over):
        a = lib.StemConv()
        for k in ("x", "mean6", "std6", "w_f16x2", "csc", "csh", "y", "t", "norm_out", "y_absmax", "x_imgmax", "x_imgmin"):
            setattr(a, k, base)
        a.N, a.Cx, a.H, a.W, a.add_inverse = 2, 6, 9, 9, 0
        a.Cout, a.kh, a.kw, a.stride, a.padding, a.relu = 64, 7, 7, 2, 3, 1
        a.max_out, a.groups, a.contraction, a.flags, a.b = 1, 1, lib.CONTRACT_F16X2, 0, 2.0
        for k, v in over.items():
            setattr(a, k, v)
        rc = hip_lib.bcos_stem_conv_fwd(C.byref(a), None)
        assert rc != 0 and b"bcos_stem_conv_fwd" in hip_lib.bcos_last_error_string()
        return rc
    INVAL, NOSUP = lib.BCOS_E_INVAL, lib.BCOS_E_NOSUP
    assert hip_lib.bcos_stem_conv_fwd(None, None) == INVAL
    for k in ("x", "mean6", "std6", "y"):
        assert call(**{k: None}) == INVAL, k
    assert call(N=0) == INVAL and call(H=-1) == INVAL and call(W=0) == INVAL
    assert call(Cx=3) == INVAL and call(Cx=6, add_inverse=1) == INVAL and call(Cx=8) == INVAL
    assert call(x_imgmax=None) == INVAL and call(x_imgmin=None) == INVAL             # the range comes as a pair
    assert call(flags=lib.BCOS_EPI_SCALE_GATE_LSB | lib.BCOS_EPI_FORCE_POW) == INVAL
    for bad in (dict(kh=3), dict(kw=3), dict(kh=3, kw=3), dict(stride=1), dict(padding=2), dict(Cout=32), dict(Cout=128)):
        assert call(**bad) == NOSUP, bad
    assert call(b=1.5) == NOSUP and call(max_out=2) == NOSUP and call(groups=2) == NOSUP and call(relu=2) == NOSUP
    assert call(bias=base) == NOSUP and call(relu_gate=base) == NOSUP
    assert call(contraction=lib.CONTRACT_BF16X3) == NOSUP and call(contraction=lib.CONTRACT_F32) == NOSUP
    assert call(w_f16x2=None) == NOSUP
    assert call(N=1 << 10, H=1 << 8, W=1 << 8) == NOSUP                              # 2 GiB
    assert call(N=1 << 16, H=1, W=1) == NOSUP                                        # more images than the grid takes
    for k in ("y", "t", "w_f16x2"):
        assert call(**{k: base + 4}) == NOSUP, k
    for k in ("x", "mean6", "std6", "csc", "csh", "norm_out", "y_absmax", "x_imgmax", "x_imgmin"):
        assert call(**{k: base + 2}) == NOSUP, k
    old = hip_lib.bcos_get_contraction_mode()
    try:
        hip_lib.bcos_set_contraction_mode(1)
        assert call(contraction=lib.CONTRACT_DEFAULT) == NOSUP
    finally:
        hip_lib.bcos_set_contraction_mode(old)
    # the range helper
    assert hip_lib.bcos_stem_image_range(None, base, base, base, base, 1, 6, 4, 4, 0, None) == INVAL
    assert hip_lib.bcos_stem_image_range(base, base, base, base, base, 0, 6, 4, 4, 0, None) == INVAL
    assert hip_lib.bcos_stem_image_range(base, base, base, base, base, 1, 3, 4, 4, 0, None) == INVAL


def test_entry_point_is_declared_bound_and_built():
    import os
    import re
    from bcos_hip import lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bcos_hip.h")).read()
    assert re.search(r"\bint bcos_stem_conv_fwd\(", header) and "bcos_stem_conv_fwd" in lib.SIGNATURES
    assert re.search(r"\bint bcos_stem_image_range\(", header) and "bcos_stem_image_range" in lib.SIGNATURES
    assert "bcos_stem.hip" in lib.SOURCES and f"#define BCOS_ABI_VERSION {lib.ABI_VERSION}" in header and lib.ABI_VERSION == 12
    fields = re.search(r"typedef struct bcos_stem_conv \{(.*?)\} bcos_stem_conv;", header, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == [n for n, _ in lib.StemConv._fields_], declared
    assert getattr(ops.stem_conv_fwd, "native", False)
