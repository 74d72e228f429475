"""The pass scheduler of the fused engines (bcos_hip/passes.py) without a device: torch's stream API replaced by stand-ins that log, the
kernels by the emulators of tests/cpu_emulation.py.  What the GPU suite can only see as equal bits -- the stream decision, the cuts, the
round-robin issue order with its per-resume arena switch, the error path, the second-thread refusal -- is asserted here as such."""
import contextlib
import threading

import pytest
import torch
import torch.nn as nn

import cpu_emulation
import head_functional_emulation
import occlusion_emulation

CPU = torch.device("cpu")


class Stream:
    """stands in for torch.cuda.Stream: logs who waits for whom"""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_stream(self, other):
        self.log.append(("wait", self.name, other.name))

    def __repr__(self):
        return self.name


class Streams:
    """the stand-ins of one test: `log` of (event, ...) tuples, `caller` (the stream the test 'runs on'), `current()`"""

    def __init__(self, monkeypatch, on_device=True):
        from bcos_hip import passes
        self.log, self.made, self.capturing = [], [], False
        self.caller = Stream(self.log, "caller")
        self._stack = [self.caller]
        monkeypatch.setattr(torch.cuda, "Stream", self._new)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: self._stack[-1])
        monkeypatch.setattr(torch.cuda, "stream", self._scope)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: self.capturing)
        monkeypatch.setattr(passes, "_record_stream", lambda t, st: self.log.append(("record", tuple(t.shape), st.name)))
        if on_device:
            monkeypatch.setattr(passes, "_on_device", lambda device: True)

    def _new(self, device=None):
        self.made.append(Stream(self.log, f"side{len(self.made)}"))
        return self.made[-1]

    @contextlib.contextmanager
    def _scope(self, st):
        self.log.append(("enter", st.name))
        self._stack.append(st)
        try:
            yield
        finally:
            self._stack.pop()
            self.log.append(("exit", st.name))

    def current(self):
        return self._stack[-1]


@pytest.fixture
def streams(monkeypatch):
    return Streams(monkeypatch)


def counting_gen(side, st, log, i, yields, fail_at=None):
    """a pass generator that logs (i, is the arena mine?, current stream) at every resume and returns a tensor"""
    from bcos_hip import ops
    try:
        for k in range(yields + 1):
            log.append((i, ops._ARENA is side.get(CPU, 2)[1][i], st.current().name))
            if k + 1 == fail_at:
                raise RuntimeError(f"pass {i} failed")
            if k < yields:
                yield
    except GeneratorExit:
        log.append((i, "closed"))
        raise
    return torch.full((2,), float(i))


# ------------------------------------------------------------------------------------------------------------ decision and cuts
def test_stream_decision_and_cuts(monkeypatch):
    from bcos_hip import engine, passes
    assert passes._SUBBATCH_MIN == 32 == engine._SUBBATCH_MIN
    assert passes.n_streams(96, 3, CPU) == 1                      # not on a device (the real _on_device)
    st = Streams(monkeypatch)
    for n, limit, want in ((63, 2, 1), (64, 2, 2), (95, 3, 2), (96, 3, 3), (4096, 1, 1)):
        assert passes.n_streams(n, limit, CPU) == want, (n, limit)
    st.capturing = True
    assert passes.n_streams(96, 3, CPU) == 1                      # capture in progress
    assert passes.cuts(65, 2) == [0, 32, 65] and passes.cuts(96, 3) == [0, 32, 64, 96]


def test_occluded_resnet_forward_on_emulated_kernels_stays_on_one_stream(monkeypatch):
    """a bank of 2 x _SUBBATCH_MIN rectangles on a host tensor: the occluded forward used to leave the `is_cuda` clause out of its
    stream decision"""
    from bcos_hip import engine, ops, synth
    cpu_emulation.install(monkeypatch)
    monkeypatch.setattr(ops, "prep_input_occluded", occlusion_emulation.prep_input_occluded)

    def no_stream(*a, **k):
        raise AssertionError("a side stream for a batch that is not on a device")
    monkeypatch.setattr(torch.cuda, "Stream", no_stream)
    eng = engine.ResNetEngine(synth.build_bcosified_resnet("resnet18").eval())
    img = synth.synthetic_images(1, size=32, seed=2)        # (6 channels: AddInverse-encoded)
    bank = torch.tensor([[i % 24, i % 24 + 8, i // 3, i // 3 + 8] for i in range(64)], dtype=torch.int32)
    out = eng.forward(img, occlude=bank)
    assert tuple(out.shape) == (64, eng.n_logits())
    assert torch.equal(out[:3], eng.forward(img, occlude=bank[:3]))


# ------------------------------------------------------------------------------------------------------------------ the protocol
def test_passes_are_issued_round_robin_each_under_its_stream_and_arena(streams, monkeypatch):
    from bcos_hip import ops, passes
    side, own, outer, resumes = passes.SideStreams(), ops.AbsmaxArena(), ops.AbsmaxArena(), []
    resets, inner_reset = [], ops.AbsmaxArena.reset

    def reset(self, device):
        resets.append((self, streams.current().name))
        streams.log.append(("reset", streams.current().name))
        inner_reset(self, device)
    monkeypatch.setattr(ops.AbsmaxArena, "reset", reset)
    bounds = []

    def make_gen(lo, hi):
        bounds.append((lo, hi))
        return counting_gen(side, streams, resumes, len(bounds) - 1, (3, 5)[len(bounds) - 1])
    ops.set_absmax_arena(outer)
    try:
        outs = side.run(CPU, 65, 2, make_gen, own, lambda: streams.log.append(("prepare", streams.current().name)))
        assert ops._ARENA is outer                              # restored
    finally:
        ops.set_absmax_arena(None)
    arenas = side.get(CPU, 2)[1]
    assert bounds == [(0, 32), (32, 65)] and [o.tolist() for o in outs] == [[0.0, 0.0], [1.0, 1.0]]
    # strict round-robin until the shorter pass ends (3 yields = 4 resumes), then the longer one alone
    assert resumes == [(i, True, f"side{i}") for i in (0, 1, 0, 1, 0, 1, 0, 1, 1, 1)]
    assert resets == [(arenas[0], "side0"), (arenas[1], "side1")] and own.gen == 0
    log = streams.log
    # prepare on the caller's stream, then the side streams behind the caller, the zero fills, the passes, the caller behind the side
    # streams, the results recorded on the caller's stream
    assert log[:3] == [("prepare", "caller"), ("wait", "side0", "caller"), ("wait", "side1", "caller")]
    assert log[3:9] == [("enter", "side0"), ("reset", "side0"), ("exit", "side0"), ("enter", "side1"), ("reset", "side1"), ("exit", "side1")]
    assert log[9:-4] == [ev for i in (0, 1, 0, 1, 0, 1, 0, 1, 1, 1) for ev in (("enter", f"side{i}"), ("exit", f"side{i}"))]
    assert log[-4:] == [("wait", "caller", "side0"), ("wait", "caller", "side1"), ("record", (2,), "caller"), ("record", (2,), "caller")]


def test_one_stream_runs_on_the_callers_stream_under_the_engines_own_arena(streams):
    from bcos_hip import ops, passes
    side, own, seen = passes.SideStreams(), ops.AbsmaxArena(), []

    def make_gen(lo, hi):
        seen.append((lo, hi, ops._ARENA is own, streams.current().name))
        yield
        return lo, hi
    assert side.run(CPU, 63, 2, make_gen, own, lambda: seen.append("prepare")) == [(0, 63)]
    assert seen == [(0, 63, True, "caller")] and streams.log == [] and streams.made == [] and own.gen == 1 and ops._ARENA is None


def test_a_failing_pass_closes_the_others_and_orders_the_caller_behind_every_side_stream(streams):
    from bcos_hip import ops, passes
    side, own, resumes = passes.SideStreams(), ops.AbsmaxArena(), []

    def failing(lo, hi):
        return counting_gen(side, streams, resumes, 0 if lo == 0 else 1, 4, fail_at=2 if lo else None)
    with pytest.raises(RuntimeError, match="pass 1 failed"):
        side.run(CPU, 64, 2, failing, own, lambda: None)
    assert resumes == [(0, True, "side0"), (1, True, "side1"), (0, True, "side0"), (1, True, "side1"), (0, "closed")]
    assert streams.log[-2:] == [("wait", "caller", "side0"), ("wait", "caller", "side1")]       # before the exception left
    assert not any(ev[0] == "record" for ev in streams.log) and ops._ARENA is None
    del resumes[:]
    outs = side.run(CPU, 64, 2, lambda lo, hi: counting_gen(side, streams, resumes, 0 if lo == 0 else 1, 1), own, lambda: None)
    assert len(outs) == 2 and len(resumes) == 4                 # the lock was released


def test_a_second_thread_is_refused_while_a_pass_sequence_is_being_issued(streams):
    from bcos_hip import ops, passes
    from bcos_hip.lib import BcosHipError
    side, other, caught = passes.SideStreams(), passes.SideStreams(), []

    def intruder():
        try:
            other.run(CPU, 64, 2, lambda lo, hi: iter(()), ops.AbsmaxArena(), lambda: None)
        except Exception as e:      # noqa: BLE001
            caught.append(e)

    def make_gen(lo, hi):
        if lo == 0:
            th = threading.Thread(target=intruder)
            th.start()
            th.join()
        yield
        return lo
    assert side.run(CPU, 64, 2, make_gen, ops.AbsmaxArena(), lambda: None) == [0, 32]
    assert len(caught) == 1 and isinstance(caught[0], BcosHipError) and "second thread" in str(caught[0])


# --------------------------------------------------------------------------------------------------------- both engines end to end
def small_vit():
    import bcos.models.vit as vit
    from bcos_hip import synth
    from bcosify_vit import BcosifyNetwork
    torch.manual_seed(3)
    cfg = synth.vit_model_config("simple_vit_ti_patch16_224")
    std = vit.SimpleViT(image_size=64, patch_size=16, num_classes=12, dim=64, depth=2, heads=1, mlp_dim=96, channels=3,
                        linear_layer=nn.Linear, norm_layer=nn.LayerNorm, act_layer=nn.GELU)
    net = BcosifyNetwork(std, cfg, add_channels=True, logit_layer=cfg["logit_layer"])
    synth.finish_vit_conversion(net, cfg)
    return net.eval()


def relu_gates(eng, x, monkeypatch):
    """random 0/1 gates of the shapes of the engine's ReLUs for the batch x, in execution order"""
    from bcos_hip import engine
    shapes, inner = [], engine.Conv.fwd

    def fwd(self, a, **kw):
        y, t = inner(self, a, **kw)
        if kw.get("relu"):
            shapes.append(tuple(y.shape))
        return y, t
    monkeypatch.setattr(engine.Conv, "fwd", fwd)
    eng.forward(x)
    monkeypatch.setattr(engine.Conv, "fwd", inner)
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(s, generator=g) > 0.3).float() for s in shapes]


@pytest.mark.parametrize("kind", ["resnet18", "vit"])
def test_engines_on_side_streams_equal_the_same_calls_per_cut(kind, streams, monkeypatch):
    """batch of 5 (and a 5-rectangle bank) with the minimum at 2: two streams for the ResNet, its default of three capped at two for the
    ViT -- per CUT and not against the whole batch: torch's CPU kernels do not promise batch-independent bits, equal shapes into equal
    emulators do"""
    from bcos_hip import engine, ops, passes, synth, vit_engine
    from bcos_hip.functional import LogitFunctional as LF
    cpu_emulation.install(monkeypatch)
    head_functional_emulation.install(monkeypatch)
    monkeypatch.setattr(ops, "prep_input_occluded", occlusion_emulation.prep_input_occluded)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 2)
    if kind == "resnet18":
        eng, limit, size = engine.ResNetEngine(synth.build_bcosified_resnet("resnet18").eval()), 2, 32
    else:
        eng, limit, size = vit_engine.ViTEngine(small_vit()), 3, 64
    x = synth.synthetic_images(5, size=size, seed=4)
    img = x[:1]
    bank = torch.tensor([[i, i + 8, 2 * i, 2 * i + 9] for i in range(5)], dtype=torch.int32)
    K = eng.n_logits()
    f = LF.contrast(torch.arange(5) % K, (torch.arange(5) + 3) % K)
    calls = dict(forward=lambda lo, hi: eng.forward(x[lo:hi]),
                 occluded=lambda lo, hi: eng.forward(img, occlude=bank[lo:hi]),
                 explain=lambda lo, hi: eng.explain(x[lo:hi]),
                 functional=lambda lo, hi: eng.explain(x[lo:hi], functional=f[lo:hi]))
    if kind == "resnet18":
        eng.subbatch_streams = 1
        gates = relu_gates(eng, x, monkeypatch)
        calls["gates"] = lambda lo, hi: eng.explain(x[lo:hi], gates=[g[lo:hi].clone() for g in gates])
    S = 2                                        # min(limit, 5 // 2)
    b = passes.cuts(5, S)
    for name, call in calls.items():
        eng.subbatch_streams = 1
        refs = [call(b[i], b[i + 1]) for i in range(S)]
        assert streams.made == [] or name != "forward"          # one stream: no side stream is ever made
        eng.subbatch_streams = limit
        del streams.log[:]
        got = call(0, 5)
        entered = {ev[1] for ev in streams.log if ev[0] == "enter"}
        assert entered == {f"side{i}" for i in range(S)}, (name, entered)
        assert [ev for ev in streams.log if ev[0] == "wait"][-S:] == [("wait", "caller", f"side{i}") for i in range(S)]
        if torch.is_tensor(got):
            assert got.shape[0] == 5 and torch.equal(got, torch.cat(refs)), name
            continue
        assert set(got) == set(refs[0]), name
        for k, v in got.items():
            assert v.shape[0] == 5 and v.is_contiguous() and torch.equal(v, torch.cat([r[k] for r in refs])), (name, k)
    if kind == "resnet18":
        assert eng.n_streams(x) == 2 and eng.n_streams(x[:3]) == 1 and eng.n_streams(x, cotangent=lambda e: e) == 1
