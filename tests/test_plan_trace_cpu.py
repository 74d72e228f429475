"""Every entry point of the three fused plans issues the launches it issued before the plans were moved onto plan.FusedPlan: same
functions, same order, same stream, same tensor shapes, same scalar arguments -- on one stream and on two.

tests/golden/plan_launch_trace.json was recorded from the commit BEFORE that change (this module copied into a checkout of it,
`python tests/test_plan_trace_cpu.py record` there, the written file copied back); recording again on the current code must leave it
unchanged.  The module therefore touches the plans through their public entry points only.

A trace is taken on the emulated kernels: every bcos_hip.ops callable an emulation module replaces, plus ops.DgradPlan.run /
run_compact, is wrapped to log (name, stand-in stream, shapes of the tensor arguments, scalar keyword arguments).  `weights_out` /
`contrib_out` are left out: a one-stream ViT pass used to be handed the shared output pair and now allocates its own, like the other plans.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # (the recorder, run as a script: the paths tests/conftest.py sets up)
    sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import pytest       # noqa: E402
import torch        # noqa: E402

import boundary_fusion_emulation        # noqa: E402
import cpu_emulation                    # noqa: E402
import densenet_cases                   # noqa: E402
import densenet_emulation               # noqa: E402
import head_functional_emulation        # noqa: E402
import occlusion_emulation              # noqa: E402
import perturbation_emulation           # noqa: E402
from test_passes_cpu import Streams, small_vit      # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "plan_launch_trace.json")
LEFT_OUT = ("weights_out", "contrib_out")


def _scalar(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return True
    return isinstance(v, (tuple, list)) and all(_scalar(e) for e in v)


class Tracer:
    """the emulators over bcos_hip.ops, each wrapped to log its calls; `streams` are the stand-ins of tests/test_passes_cpu.py"""

    def __init__(self, monkeypatch):
        from bcos_hip import ops
        self.streams, self.log = Streams(monkeypatch), []
        before = dict(vars(ops))
        cpu_emulation.install(monkeypatch)
        head_functional_emulation.install(monkeypatch)
        densenet_emulation.install(monkeypatch)
        boundary_fusion_emulation.install(monkeypatch)
        monkeypatch.setattr(ops, "prep_input_occluded", occlusion_emulation.prep_input_occluded)
        monkeypatch.setattr(ops, "prep_input_perturbed", perturbation_emulation.prep_input_perturbed)
        self.replaced = sorted(k for k, v in vars(ops).items() if callable(v) and before.get(k) is not v)
        for name in self.replaced:
            monkeypatch.setattr(ops, name, self.wrap(name, getattr(ops, name)))
        for name in ("run", "run_compact"):
            monkeypatch.setattr(ops.DgradPlan, name, self.wrap("DgradPlan." + name, getattr(ops.DgradPlan, name)))

    def wrap(self, name, inner):
        def logged(*args, **kw):
            shapes = [list(a.shape) for a in args if torch.is_tensor(a)]
            shapes += [[k, list(v.shape)] for k, v in sorted(kw.items()) if torch.is_tensor(v) and k not in LEFT_OUT]
            scalars = {k: v for k, v in sorted(kw.items()) if _scalar(v) and k not in LEFT_OUT}
            self.log.append(json.dumps([name, self.streams.current().name, shapes, scalars]))
            return inner(*args, **kw)
        return logged

    def take(self, call):
        del self.log[:]
        call()
        return list(self.log)


def relu_gates(tracer, eng, x):
    """random 0/1 gates of the shapes of the ResNet plan's ReLUs for the batch x, in execution order"""
    from bcos_hip import ops
    shapes, inner = [], ops.conv2d_fwd

    def fwd(*a, **kw):
        out = inner(*a, **kw)
        if kw.get("relu"):
            shapes.append(tuple(out[0].shape))
        return out
    ops.conv2d_fwd = fwd
    try:
        eng.forward(x)
    finally:
        ops.conv2d_fwd = inner
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(s, generator=g) > 0.3).float() for s in shapes]


def cases(tracer):
    """{case name: (engine, call)} over the smallest networks the CPU suite builds: five images, so that a minimum of two per
    sub-batch gives two streams"""
    from bcos_hip import densenet_engine, engine, perturbation, synth, vit_engine
    from bcos_hip.functional import LogitFunctional as LF
    out = {}
    bank = torch.tensor([[i, i + 8, 2 * i, 2 * i + 9] for i in range(5)], dtype=torch.int32)
    g = torch.Generator().manual_seed(7)

    def plan_for(x):
        scores = torch.rand(2, x.shape[2] * x.shape[3], generator=g)
        return perturbation.PerturbPlan(scores, perturbation_emulation.perturb_select(scores, [0, 5, 40]))       # (2 images x 3 counts = 6 copies)

    def shared(eng, x, prefix, names):
        K = eng.n_logits()
        tg = (torch.arange(5) * 3) % K
        sparse, dense = LF.contrast(torch.arange(5) % K, (torch.arange(5) + 3) % K), LF.mean_corrected(tg, K)
        pl = plan_for(x)
        calls = dict(forward=lambda: eng.forward(x), occluded=lambda: eng.forward(x[:1], occlude=bank),
                     perturbed=lambda: eng.forward(x[:2], perturb=pl), explain=lambda: eng.explain(x),
                     explain_targets_arg=lambda: eng.explain(x, targets=tg), explain_sparse_functional=lambda: eng.explain(x, functional=sparse),
                     explain_dense_functional=lambda: eng.explain(x, functional=dense),
                     explain_targets=lambda: eng.explain_targets(x, torch.stack([tg, (tg + 1) % K], 1), want_weights=True),
                     explain_functionals=lambda: eng.explain_functionals(x, [sparse, dense]))
        for name in names:
            out[f"{prefix}/{name}"] = (eng, calls[name])

    rn = engine.ResNetEngine(synth.build_bcosified_resnet("resnet18").eval())
    x32 = synth.synthetic_images(5, size=32, seed=4)
    shared(rn, x32, "resnet18", ("forward", "occluded", "perturbed", "explain", "explain_targets_arg", "explain_sparse_functional",
                                 "explain_dense_functional", "explain_targets", "explain_functionals"))
    rn.subbatch_streams = 1
    gates = relu_gates(tracer, rn, x32)
    out["resnet18/explain_gates"] = (rn, lambda: rn.explain(x32, gates=[gt.clone() for gt in gates]))

    clip = engine.ResNetEngine(synth.build_bcosified_clip_resnet(layers=(1, 1, 1, 1), output_dim=64, heads=8, width=16, seed=5).eval())
    x64 = synth.synthetic_images(5, size=64, seed=4)
    out["clip_attnpool/explain_cotangent"] = (clip, lambda: clip.explain(x64, cotangent=lambda emb: torch.ones_like(emb)))

    vit = vit_engine.ViTEngine(small_vit())
    shared(vit, x64, "vit", ("forward", "occluded", "perturbed", "explain_targets_arg", "explain_sparse_functional", "explain_functionals"))

    net, _, _, xd = densenet_cases.golden_net("densenet_tiny")
    dn = densenet_engine.DenseNetEngine(net)
    shared(dn, torch.cat([xd, xd[:2]]), "densenet_tiny", ("forward", "explain", "explain_targets"))
    return out


def record(monkeypatch):
    """-> {case: {"1": trace on one stream, "2": trace with two sub-batch streams allowed}}, each trace a list of JSON strings"""
    from bcos_hip import passes
    tracer = Tracer(monkeypatch)
    monkeypatch.setattr(passes, "_SUBBATCH_MIN", 2)
    traces = {}
    for name, (eng, call) in cases(tracer).items():
        traces[name] = {}
        for limit in (1, 2):
            eng.subbatch_streams = limit
            traces[name][str(limit)] = tracer.take(call)
    return traces, tracer


def packed(traces):
    """the fixture's form: every distinct launch once, the traces as indices into that table"""
    table = sorted({e for per in traces.values() for t in per.values() for e in t})
    index = {e: i for i, e in enumerate(table)}
    return dict(launches=[json.loads(e) for e in table], traces={c: {k: [index[e] for e in t] for k, t in per.items()} for c, per in traces.items()})


@pytest.fixture(scope="module")
def recorded():
    with pytest.MonkeyPatch.context() as mp:
        traces, tracer = record(mp)
        return traces, tracer.replaced


def test_every_entry_point_issues_the_recorded_launches(recorded):
    traces, replaced = recorded
    want = json.load(open(FIXTURE))
    assert {"tapconv", "prep_input", "prep_input_occluded", "prep_input_perturbed", "head_rankm_grad", "head_cotangent_grad", "slice_affine_rows",
            "boundary_conv3_grad", "finalize_explanation", "finalize_explanation_patches"} <= set(replaced)
    got = packed(traces)
    assert sorted(got["traces"]) == sorted(want["traces"])
    for case, per in want["traces"].items():
        for limit, idx in per.items():
            mine = [got["launches"][i] for i in got["traces"][case][limit]]
            theirs = [want["launches"][i] for i in idx]
            first = next((i for i, (a, b) in enumerate(zip(mine, theirs)) if a != b), min(len(mine), len(theirs)))
            assert mine == theirs, (case, limit, first, mine[first:first + 1], theirs[first:first + 1])


def test_the_traces_cover_one_and_two_streams(recorded):
    """what makes the comparison above mean something: with two streams allowed every case but the cotangent one runs on both side
    streams, a `cotangent` pass and every one-stream run on the caller's stream alone; the two-stream trace of a case is its one-stream
    trace per cut"""
    traces, _ = recorded
    for case, per in traces.items():
        per = {limit: [e for e in t if json.loads(e)[0] != "require_device"] for limit, t in per.items()}       # (a host-side check, no launch)
        streams = {limit: {json.loads(e)[1] for e in t} for limit, t in per.items()}
        assert streams["1"] == {"caller"} and len(per["1"]) > 0, case
        repeated = case.split("/")[1] in ("explain_targets", "explain_functionals")      # (ONE kept forward: on the caller's stream)
        if repeated or case.endswith("cotangent"):
            assert streams["2"] == {"caller"}, (case, streams["2"])
            continue
        a, b = sorted(streams["2"])                                  # (the two side streams of this case's engine)
        assert a.startswith("side") and b.startswith("side"), (case, streams["2"])
        names = lambda t, s=None: [json.loads(e)[0] for e in t if s is None or json.loads(e)[1] == s]      # noqa: E731
        assert names(per["2"], a) == names(per["2"], b) == names(per["1"]), case


def test_capabilities_and_refusals_are_what_they_were(monkeypatch):
    from bcos_hip import densenet_engine, engine, vit_engine
    cpu_emulation.install(monkeypatch)
    densenet_emulation.install(monkeypatch)
    from bcos_hip.lib import BcosHipError
    has = {cls.__name__: [hasattr(cls, n) for n in ("explain_targets", "explain_functionals")]
           for cls in (engine.ResNetEngine, vit_engine.ViTEngine, densenet_engine.DenseNetEngine)}
    assert has == dict(ResNetEngine=[True, True], ViTEngine=[False, True], DenseNetEngine=[True, False])
    assert hasattr(engine.ResNetEngine(_resnet18()), "supports_explain") and not hasattr(vit_engine.ViTEngine(small_vit()), "supports_explain")
    net, _, _, x = densenet_cases.golden_net("densenet_tiny")
    eng = densenet_engine.DenseNetEngine(net)
    assert eng.supports_explain is True
    for name in ("occlude", "perturb"):
        with pytest.raises(BcosHipError, match=name):
            eng.forward(x, **{name: object()})
    for name in ("occlude", "perturb", "functional", "gates", "cotangent"):
        with pytest.raises(BcosHipError, match=name):
            eng.explain(x, **{name: object()})


def _resnet18():
    from bcos_hip import synth
    return synth.build_bcosified_resnet("resnet18").eval()


if __name__ == "__main__":
    if sys.argv[1:] != ["record"]:
        sys.exit("usage: python tests/test_plan_trace_cpu.py record")
    with pytest.MonkeyPatch.context() as mp:
        data = packed(record(mp)[0])
    with open(FIXTURE, "w") as f:
        f.write("{\n\"launches\": [\n" + ",\n".join(json.dumps(e) for e in data["launches"]) + "\n],\n\"traces\": {\n")
        f.write(",\n".join(json.dumps(c) + ": " + json.dumps(per) for c, per in data["traces"].items()) + "\n}\n}\n")
    print(f"wrote {FIXTURE}: {len(data['launches'])} distinct launches, {sum(len(t) for per in data['traces'].values() for t in per.values())} in all")
