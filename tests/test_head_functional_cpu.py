"""Linear functionals of the logits on the fused engines, without a device: the engines' routing and linearity on emulated kernels
(tests/head_functional_emulation.py on top of cpu_emulation.install), the OursRelative explainer's engine path, the host-side error
handling and the argument checks of the two entry points (bcos_head_rankm_grad, bcos_head_cotangent_grad)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import cpu_emulation
import head_functional_emulation as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def install(monkeypatch):
    cpu_emulation.install(monkeypatch)
    E.install(monkeypatch)


def small_vit(gap_reorder, classes=12):
    import bcos.models.vit as vit
    from bcos_hip import synth
    from bcosify_vit import BcosifyNetwork
    torch.manual_seed(3)
    cfg = synth.vit_model_config("simple_vit_ti_patch16_224")
    cfg = dict(cfg, args=dict(cfg["args"], gap_reorder=gap_reorder))
    std = vit.SimpleViT(image_size=64, patch_size=16, num_classes=classes, dim=64, depth=2, heads=1, mlp_dim=96, channels=3,
                        linear_layer=nn.Linear, norm_layer=nn.LayerNorm, act_layer=nn.GELU)
    net = BcosifyNetwork(std, cfg, add_channels=True, logit_layer=cfg["logit_layer"])
    synth.finish_vit_conversion(net, cfg)
    with torch.no_grad():
        for p_ in net.parameters():
            if p_.dim() == 1:
                p_.add_(0.1 * torch.randn_like(p_))          # LayerNorm affine parameters and biases away from 1 / 0
    return net.eval()


def spy(monkeypatch, name):
    from bcos_hip import ops
    calls, inner = [], getattr(ops, name)

    def wrapper(*a, **k):
        calls.append(name)
        return inner(*a, **k)
    monkeypatch.setattr(ops, name, wrapper)
    return calls


def functionals(N, K, gen):
    """a contrast, a 3-term sparse functional (one repeated class, negative index) and the mean-corrected one -> [(name, f, cot [N, K])]"""
    from bcos_hip.functional import LogitFunctional as LF
    pos, neg = torch.randint(0, K, (N,), generator=gen), torch.randint(0, K, (N,), generator=gen)
    cls3 = torch.randint(0, K, (N, 3), generator=gen)
    cls3[0, 2] = cls3[0, 0]                                   # a class named twice: its coefficients add up
    cls3[-1, 1] -= K                                          # a negative index counts from the end
    coef3 = torch.randn(N, 3, generator=gen)
    tgt = torch.randint(0, K, (N,), generator=gen)
    out = [("contrast", LF.contrast(pos, neg)), ("sparse3", LF.sparse(cls3, coef3)), ("mean_corrected", LF.mean_corrected(tgt, K))]
    return [(n, f, f.checked(N, K).as_dense(K)) for n, f in out]


def check_linearity(got, singles, cots, tol):
    """got [N, T, 6, H, W] against sum_k c_k W_k with W_k = singles[k] [N, 6, H, W], per image, relative to sum_k |c_k| ||W_k||"""
    worst = 0.0
    for t, cot in enumerate(cots):
        for n in range(got.shape[0]):
            ks = torch.nonzero(cot[n]).view(-1).tolist()
            want = sum(float(cot[n, k]) * singles[k][n].double() for k in ks)
            scale = sum(abs(float(cot[n, k])) * float(singles[k][n].double().norm()) for k in ks)
            err = float((got[n, t].double() - want).norm()) / scale
            worst = max(worst, err)
            assert err <= tol, (t, n, err)
    return worst


# ---------------------------------------------------------------------------------------------------------------------- emulation
def test_emulators_reduce_to_the_single_class_forms():
    g = torch.Generator().manual_seed(0)
    N, R, K, D = 3, 5, 37, 20
    scale, w = torch.rand(N, R, K, generator=g), torch.randn(K, D, generator=g)
    rs, mul = torch.rand(N * R, generator=g) + 0.5, torch.randn(N * R, D, generator=g)
    cls = torch.tensor([4, 36, 0])
    a = cpu_emulation.head_rank1_grad(cls, scale, w, 2.0, row_scale=rs, mul=mul, want_out2=True)
    b = E.head_rankm_grad(cls.view(N, 1), torch.ones(N, 1), scale, w, 2.0, row_scale=rs, mul=mul, want_out2=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # an out-of-range class contributes zero
    c = E.head_rankm_grad(torch.tensor([[4, K], [36, -1], [0, 99]]), torch.ones(N, 2), scale, w, 2.0, row_scale=rs, mul=mul, want_out2=True)
    assert torch.equal(c[0], a[0])
    s4 = scale.view(N, R, 1, K)
    one = E.head_cotangent_grad(torch.nn.functional.one_hot(cls, K).float(), s4, 2.0)
    assert one.shape == (N, R, 1, 40) and torch.equal(one[..., K:], torch.zeros(N, R, 1, 3))
    assert torch.equal(one[..., :K], cpu_emulation.head_onehot_grad(cls, s4, 2.0))
    v64, mag = E.head_rankm_grad64(cls.view(N, 1), torch.ones(N, 1), scale, w, 2.0, row_scale=rs)
    assert float((b[1].double() - v64).abs().max()) <= 5 * 2.0 ** -24 * float(mag.max())


# ---------------------------------------------------------------------------------------------------------------------- linearity
def test_resnet_functionals_are_linear_combinations_of_single_targets(monkeypatch):
    """explain_functionals against sum_k c_k W_k of explain_targets on the same kept-forward pattern; the sparse functionals take the
    rank-m head launch, the mean-corrected one the dense launch followed by the head's contraction"""
    install(monkeypatch)
    from bcos_hip import engine, synth
    net = synth.build_bcosified_resnet("resnet18").eval()
    eng = engine.ResNetEngine(net)
    x = synth.synthetic_images(2, size=64, seed=4)
    K = eng.n_logits()
    fs = functionals(2, K, torch.Generator().manual_seed(1))
    sparse_calls, dense_calls = spy(monkeypatch, "head_rankm_grad"), spy(monkeypatch, "head_cotangent_grad")
    prep = spy(monkeypatch, "prep_input")
    out = eng.explain_functionals(x, [f for _, f, _ in fs], want_weights=True)
    assert len(prep) == 1 and len(dense_calls) == 1 and len(sparse_calls) >= 2          # one forward; (a rank-m launch per consumer run)
    assert out["dynamic_linear_weights"].shape == (2, 3, 6, 64, 64) and out["contribution_maps"].shape == (2, 3, 64, 64)
    singles = {}
    for lo in range(0, K, 50):                                # every class: the mean-corrected functional touches all of them
        ks = list(range(lo, min(lo + 50, K)))
        w = eng.explain_targets(x, torch.tensor(ks), want_weights=True)["dynamic_linear_weights"]
        for i, k in enumerate(ks):
            singles[k] = w[:, i].clone()
    check_linearity(out["dynamic_linear_weights"], singles, [c for _, _, c in fs], 1e-5)
    # functional_value is sum_k c_k logit_k and the maps are complete up to the constant logit bias
    for t, (_, f, cot) in enumerate(fs):
        val = (out["logits"].double() * cot.double()).sum(1)
        mag = (out["logits"].double() * cot.double()).abs().sum(1)          # (the mean-corrected value cancels: judged against its terms)
        assert bool(((out["functional_values"][:, t].double() - val).abs() <= 1e-5 * mag).all())
        bias = float(net.logit_layer.logit_bias) * cot.double().sum(1)
        assert bool(((out["contribution_maps"][:, t].double().sum((1, 2)) - (val - bias)).abs() <= 1e-4 * mag).all())
    # explain(functional=) is one pass of the same thing, through the public mixin too
    one = net_with(eng, net).explain_batch(x, functional=fs[0][1])
    assert "explained_class_idx" not in one and torch.equal(one["dynamic_linear_weights"], out["dynamic_linear_weights"][:, 0])
    assert torch.equal(one["functional_value"], out["functional_values"][:, 0])
    # ... and without `functional` explain() never touches the two new launches
    before = (len(sparse_calls), len(dense_calls))
    eng.explain(x, targets=torch.tensor([3, 5]))
    assert (len(sparse_calls), len(dense_calls)) == before


def net_with(eng, net):
    object.__setattr__(net, "_bcos_engine", eng)
    return net


@pytest.mark.parametrize("gap_reorder", [True, False], ids=["gap_reorder", "head_behind_gap"])
def test_vit_functionals_are_linear_combinations_of_single_targets(monkeypatch, gap_reorder):
    install(monkeypatch)
    from bcos_hip import synth, vit_engine
    net = small_vit(gap_reorder)
    eng = vit_engine.ViTEngine(net)
    x = synth.synthetic_images(2, size=64, seed=5)
    K = eng.n_logits()
    fs = functionals(2, K, torch.Generator().manual_seed(2))
    sparse_calls, dense_calls = spy(monkeypatch, "head_rankm_grad"), spy(monkeypatch, "head_cotangent_grad")
    prep = spy(monkeypatch, "prep_input")
    out = eng.explain_functionals(x, [f for _, f, _ in fs], want_weights=True)
    assert len(prep) == 1
    assert (len(sparse_calls), len(dense_calls)) == ((2, 1) if gap_reorder else (0, 3))        # (no rank-one form behind the token mean)
    singles = {k: eng.explain(x, targets=torch.full((2,), k))["dynamic_linear_weights"] for k in range(K)}
    check_linearity(out["dynamic_linear_weights"], singles, [c for _, _, c in fs], 1e-5)
    one = eng.explain(x, functional=fs[2][1])
    assert torch.equal(one["dynamic_linear_weights"], out["dynamic_linear_weights"][:, 2])
    assert torch.equal(one["functional_value"], out["functional_values"][:, 2]) and "explained_class_idx" not in one


# ---------------------------------------------------------------------------------------------------------------------- OursRelative
def test_ours_relative_takes_the_engine_path(monkeypatch):
    """with an engine: the dense head launch once per attribute() and ONE forward for the T targets of attribute_selection(); without
    one, autograd over the modules and neither launch.  Both agree."""
    install(monkeypatch)
    from bcos_hip import engine, synth
    from interpretability.explanation_methods.explainers import get_explainer
    from interpretability.explanation_methods.explainers.ours import OursRelative
    net = synth.build_bcosified_resnet("resnet18").eval()
    x = synth.synthetic_images(1, size=64, seed=6)
    plain = get_explainer(net, "OursRelative", "default")
    assert isinstance(plain, OursRelative)
    sparse_calls, dense_calls = spy(monkeypatch, "head_rankm_grad"), spy(monkeypatch, "head_cotangent_grad")
    prep = spy(monkeypatch, "prep_input")
    ref = plain.attribute(x, 7)
    ref_sel = plain.attribute_selection(x, [7, 500, 3])
    assert not sparse_calls and not dense_calls and not prep              # no engine: per-layer autograd, none of the fused launches
    assert not any(getattr(m, "detach", False) for m in net.modules())    # (explanation mode was left again)
    engine.attach(net)
    fused = get_explainer(net, "OursRelative", "default")
    att = fused.attribute(x, 7)
    assert len(dense_calls) == 1 and len(prep) == 1 and not sparse_calls
    assert att.shape == (1, 6, 64, 64)
    sel = fused.attribute_selection(x, [7, 500, 3])
    assert len(prep) == 2 and len(dense_calls) == 4                        # ONE more forward for the three targets
    assert sel.shape == (3, 6, 64, 64) and torch.equal(sel[0], att[0])
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    assert rel(att, ref) <= 1e-4 and rel(sel, ref_sel) <= 1e-4, (rel(att, ref), rel(sel, ref_sel))
    # a batch: one target per sample, target-major selection like the reference's concatenation
    xb = synth.synthetic_images(2, size=64, seed=8)
    selb = fused.attribute_selection(xb, [[1, 2], [3, 4]])
    assert selb.shape == (4, 6, 64, 64) and torch.equal(selb[2:], fused.attribute(xb, [3, 4]))
    net.train()                                                             # train(): the module path again
    n = len(dense_calls)
    assert fused._engine() is None
    net.eval()
    engine.detach(net)
    assert fused._engine() is None and len(dense_calls) == n


def test_grid_pointing_game_takes_ours_relative(monkeypatch):
    install(monkeypatch)
    from bcos_hip import engine, localisation, synth
    from interpretability.explanation_methods.explainers import get_explainer
    net = synth.build_bcosified_resnet("resnet18").eval()
    eng = engine.attach(net)
    multi = localisation.make_multi_image(synth.synthetic_images(4, size=32, seed=9))
    tg = torch.tensor([[3, 500, 77, 999]])
    prep = spy(monkeypatch, "prep_input")
    ours = localisation.grid_pointing_game(eng, multi, tg, single_shape=32, smooth=5)
    rel = localisation.grid_pointing_game(eng, multi, tg, single_shape=32, smooth=5, explainer=get_explainer(net, "OursRelative", "default"))
    assert len(prep) == 2                                                   # one forward each
    assert set(rel) == set(ours) and all(rel[k].shape == ours[k].shape for k in ours)
    assert all(bool(torch.isfinite(v).all()) for v in rel.values())


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_functional_constructors_and_host_checks(monkeypatch):
    from bcos_hip import ops
    from bcos_hip.functional import LogitFunctional as LF
    f = LF.contrast([1, 2], [3, 4])
    assert f.is_sparse and f.classes.tolist() == [[1, 3], [2, 4]] and f.coeffs.tolist() == [[1.0, -1.0], [1.0, -1.0]] and len(f) == 2
    m = LF.mean_corrected([1, -1], 4)
    assert not m.is_sparse and torch.allclose(m.cot, torch.tensor([[-.25, .75, -.25, -.25], [-.25, -.25, -.25, .75]]))
    assert torch.equal(LF.sparse([[0, 0, 2]], [[1.0, 2.0, -1.0]]).as_dense(3), torch.tensor([[3.0, 0.0, -1.0]]))
    assert torch.equal(f.value(torch.arange(10.0).view(2, 5)), torch.tensor([-2.0, -2.0]))
    assert f[1:].classes.tolist() == [[2, 4]]
    with pytest.raises(ValueError, match="1 .. 8"):
        LF.sparse(torch.zeros(2, 9, dtype=torch.int64), torch.zeros(2, 9))
    with pytest.raises(ValueError):
        LF.sparse(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 0))
    with pytest.raises(ValueError):
        LF.sparse([[1, 2]], [[1.0]])
    with pytest.raises(ValueError):
        LF.dense(torch.zeros(5))
    with pytest.raises(ValueError):
        LF.contrast([1, 2], [3])
    with pytest.raises(TypeError):
        LF.sparse([[0.5]], [[1.0]])
    with pytest.raises(IndexError):
        LF.mean_corrected([4], 4)
    with pytest.raises(IndexError):
        f.checked(2, 4)                                                     # class 4 of 4 logits
    with pytest.raises(IndexError):
        LF.contrast([0], [-6]).checked(1, 5)
    assert LF.contrast([0], [-5]).checked(1, 5).classes.tolist() == [[0, 0]]
    with pytest.raises(ValueError, match="batch of 3"):
        f.checked(3, 10)
    with pytest.raises(ValueError, match="5 logits"):
        LF.dense(torch.zeros(2, 5)).checked(2, 10)
    # the host check does not touch a device: lists and host tensors
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (_ for _ in ()).throw(AssertionError("synchronised")))
    assert ops.check_functional_classes([[1, -1]], 10).tolist() == [[1, 9]]
    with pytest.raises(IndexError):
        ops.check_functional_classes(torch.tensor([[1, 10]]), 10)
    with pytest.raises(ValueError):
        ops.check_functional_classes([1, 2], 10)


def test_engines_refuse_malformed_functionals(monkeypatch, hip_lib):
    install(monkeypatch)
    from bcos_hip import engine, synth
    from bcos_hip.functional import LogitFunctional as LF
    from bcos_hip.lib import BcosHipError
    net = synth.build_bcosified_resnet("resnet18").eval()
    eng = engine.ResNetEngine(net)
    x = synth.synthetic_images(2, size=32, seed=4)
    prep = spy(monkeypatch, "prep_input")
    with pytest.raises(IndexError):
        eng.explain(x, functional=LF.contrast([1, 2], [3, 1000]))
    with pytest.raises(ValueError):
        eng.explain(x, functional=LF.contrast([1], [3]))                   # one row for two images
    with pytest.raises(ValueError):
        eng.explain(x, functional=LF.dense(torch.zeros(2, 999)))
    with pytest.raises(ValueError):
        eng.explain(x, targets=torch.tensor([1, 2]), functional=LF.contrast([1, 2], [3, 4]))
    with pytest.raises(TypeError):
        eng.explain(x, functional=torch.zeros(2, 1000))
    with pytest.raises(ValueError):
        eng.explain_functionals(x, [])
    assert not prep                                                        # all refused before the first launch
    # ops wrappers: J > 8 and mismatched shapes
    from bcos_hip import ops
    monkeypatch.undo()
    scale, w = torch.zeros(2, 3, 10), torch.zeros(10, 8)
    for bad_cls, bad_coef in ((torch.zeros(2, 9, dtype=torch.int64), torch.zeros(2, 9)), (torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 3)),
                              (torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 2)), (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 0))):
        with pytest.raises(ValueError):
            ops.head_rankm_grad(bad_cls, bad_coef, scale, w)
    with pytest.raises(BcosHipError, match="HIP tensor"):                  # (no CPU path)
        ops.head_rankm_grad(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 2), scale, w)
    with pytest.raises(ValueError):
        ops.head_cotangent_grad(torch.zeros(2, 9), scale)


def test_attn_unpool_still_refuses_and_attnpool_takes_embedding_functionals(monkeypatch):
    install(monkeypatch)
    from bcos_hip import engine, synth
    from bcos_hip.functional import LogitFunctional as LF
    from bcos_hip.lib import BcosHipError
    from bcosify import BcosifyNetwork
    tiny = dict(layers=(1, 1, 1, 1), output_dim=64, heads=8, width=16)     # (the instance of tests/golden/clip_tiny_train_step)
    net = synth.build_bcosified_clip_resnet(**tiny, seed=5)
    eng = engine.ResNetEngine(net.eval())
    x = synth.synthetic_images(2, size=64, seed=4)
    out = eng.explain_functionals(x, [LF.contrast([1, 2], [3, 4])], want_weights=True)
    a = eng.explain(x, targets=torch.tensor([1, 2]))["dynamic_linear_weights"]
    b = eng.explain(x, targets=torch.tensor([3, 4]))["dynamic_linear_weights"]
    err = float((out["dynamic_linear_weights"][:, 0].double() - (a.double() - b.double())).norm() / (a.double().norm() + b.double().norm()))
    assert eng.n_logits() == 64 and err <= 1e-5, err
    cfg = dict(synth.clip_model_config(), attn_unpool=True)
    unp = synth.finish_clip_conversion(BcosifyNetwork(synth.standard_clip_resnet(**tiny, seed=5), cfg, add_channels=True, logit_layer=False))
    eng_u = engine.ResNetEngine(unp.eval())
    assert eng_u.head_kind == "attn_unpool"
    with pytest.raises(BcosHipError, match="attn_unpool"):
        eng_u.explain(x, functional=LF.contrast([1, 2], [3, 4]))
    with pytest.raises(BcosHipError, match="attn_unpool"):
        eng_u.explain_functionals(x, [LF.contrast([1, 2], [3, 4])])


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_header_binding_and_library_carry_the_two_entry_points(hip_lib):
    from bcos_hip import lib
    header = open(os.path.join(REPO, "include", "bcos_hip.h")).read()
    assert re.search(r"#define BCOS_ABI_VERSION 12\b", header) and hip_lib.bcos_version() == 12          # additive: the version stays
    for name in ("bcos_head_rankm_grad", "bcos_head_cotangent_grad"):
        assert re.search(r"\bint " + name + r"\(", header) and name in lib.SIGNATURES
        assert getattr(hip_lib, name) is not None
    assert "bcos/common.py:163-181" in header and "explainers/ours.py:28-33" in header
    assert "bcos_head.hip" in lib.SOURCES


def test_abi_refuses_malformed_arguments(hip_lib):
    fake = C.c_void_p(1 << 20)
    off4, off8 = C.c_void_p((1 << 20) + 4), C.c_void_p((1 << 20) + 8)
    rankm = lambda **k: hip_lib.bcos_head_rankm_grad(*[k.get(a, d) for a, d in (  # noqa: E731
        ("cls", fake), ("coef", fake), ("J", 2), ("scale", fake), ("w", fake), ("row_scale", None), ("mul", None), ("mul2", None),
        ("gate2", None), ("gfm", 0), ("out", fake), ("out2", None), ("am", None), ("am2", None), ("N", 2), ("R", 4), ("K", 10), ("D", 8),
        ("inv_t", 1.0), ("stream", None))])
    for bad in (dict(cls=None), dict(coef=None), dict(scale=None), dict(w=None), dict(out=None), dict(J=0), dict(J=-1), dict(D=6), dict(D=0),
                dict(N=0), dict(N=-2), dict(R=0), dict(K=-1), dict(w=off4), dict(out=off8), dict(mul=off4), dict(mul2=fake), dict(gate2=fake),
                dict(am2=fake), dict(gfm=1), dict(gfm=1, out2=fake), dict(gfm=1, out2=fake, mul=fake, gate2=fake), dict(out2=off4),
                dict(cls=off4), dict(coef=C.c_void_p((1 << 20) + 2))):
        assert rankm(**bad) == -22, bad
        assert b"bcos_head_rankm_grad" in hip_lib.bcos_last_error_string()
    assert rankm(J=9) == -95 and b"8 terms" in hip_lib.bcos_last_error_string()
    cot = lambda **k: hip_lib.bcos_head_cotangent_grad(*[k.get(a, d) for a, d in (  # noqa: E731
        ("cot", fake), ("scale", fake), ("glin", fake), ("am", None), ("N", 2), ("R", 4), ("K", 10), ("inv_t", 1.0), ("stream", None))])
    for bad in (dict(cot=None), dict(scale=None), dict(glin=None), dict(N=0), dict(R=-1), dict(K=0), dict(glin=off4), dict(glin=off8),
                dict(cot=C.c_void_p((1 << 20) + 2)), dict(scale=C.c_void_p((1 << 20) + 1)), dict(am=C.c_void_p((1 << 20) + 2)),
                dict(K=2 ** 31 - 2)):
        assert cot(**bad) == -22, bad
        assert b"bcos_head_cotangent_grad" in hip_lib.bcos_last_error_string()


def test_head_functional_abi_validation_under_address_sanitizer():
    """tests/asan/head_functional_abi_validation.c against the ASan host build (scripts/asan_host_check.sh), as the occlusion file"""
    import subprocess
    proc = subprocess.run(["bash", os.path.join(REPO, "scripts", "asan_host_check.sh")], capture_output=True, text=True, timeout=1500)
    assert proc.returncode == 0 and "bcos_head_rankm_grad, bcos_head_cotangent_grad: all refusals ok" in proc.stdout, \
        proc.stdout[-2000:] + proc.stderr[-2000:]
