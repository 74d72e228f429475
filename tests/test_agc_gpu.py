"""`-m gpu`: bcos_agc_clip (csrc/bcos_agc.hip) through bcos.training.agc against the reference's recorded clipping, against a torch
restatement on the parameter sets of the supported networks, and inside the reference recipe (UniformOffLabelsBCEWithLogitsLoss, clip,
torch.optim.AdamW) on the resnet14b fixture network through both training paths."""
import json
import os

import numpy as np
import pytest
import torch

from test_agc_cpu import case_inputs, cases, reference_output, rel, unit_view

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _param(p, g):
    t = torch.nn.Parameter(p.to(DEV))
    t.grad = g.to(DEV)
    return t


def test_fixture_cases_against_the_reference(lib):
    """every unit rule in ONE call: clipped gradients to 1e-6 per tensor, the same decisions, unclipped units and all parameters
    untouched bit for bit, the NaN units as the reference leaves them"""
    from bcos.training.agc import adaptive_clip_grad_
    meta, data = cases()
    inputs = [case_inputs(c, data) for c in meta["cases"]]
    params = [_param(p, g) for p, g in inputs]
    nan_p, nan_g = torch.from_numpy(data["nan/p"]), torch.from_numpy(data["nan/g"])
    params.append(_param(nan_p, nan_g))
    adaptive_clip_grad_(params, clip_factor=meta["clip_factor"], eps=meta["eps"])
    torch.cuda.synchronize()
    for c, (p, g), t in zip(meta["cases"], inputs, params):
        out = t.grad.cpu()
        ref = reference_output(c, data, g)
        assert rel(out, ref) <= 1e-6, (c["name"], rel(out, ref))
        changed = ~torch.all(unit_view(out) == unit_view(g), dim=1)
        assert torch.equal(changed, torch.from_numpy(data[f"{c['name']}/clip"])), c["name"]
        assert torch.equal(t.detach().cpu(), p), c["name"]
    out, ref = params[-1].grad.cpu(), torch.from_numpy(data["nan/clipped"])
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and torch.isnan(out[3]).all() and torch.isnan(out[5]).all()
    ok = ~torch.isnan(ref)
    assert rel(out[ok], ref[ok]) <= 1e-6
    assert torch.equal(torch.nan_to_num(params[-1].detach().cpu(), 7.0), torch.nan_to_num(nan_p, 7.0))


def test_fixture_cases_with_gradients_off_the_parameters_alignment(lib):
    """gradients as views one float into a larger buffer (as in a flat gradient bucket): p and g then sit at different offsets modulo
    16 bytes and every unit takes the kernel's scalar path -- the same results to 1e-6, the same decisions, and the same bits again on
    a second call over the same data"""
    from bcos.training.agc import adaptive_clip_grad_
    meta, data = cases()
    inputs = [case_inputs(c, data) for c in meta["cases"]]
    runs = []
    for _ in range(2):
        total = sum(g.numel() for _, g in inputs) + 1
        bucket = torch.zeros(total + 3, device=DEV)
        params, off = [], 1
        for p, g in inputs:
            t = torch.nn.Parameter(p.to(DEV))
            view = bucket[off:off + g.numel()].view(g.shape)
            view.copy_(g.to(DEV))
            assert (view.data_ptr() - t.data_ptr()) % 16 != 0 or g.numel() == 1
            t.grad = view
            params.append(t)
            off += g.numel()
        adaptive_clip_grad_(params, clip_factor=meta["clip_factor"], eps=meta["eps"])
        torch.cuda.synchronize()
        runs.append([t.grad.cpu() for t in params])
        for c, (p, g), out, t in zip(meta["cases"], inputs, runs[-1], params):
            ref = reference_output(c, data, g)
            assert rel(out, ref) <= 1e-6, (c["name"], rel(out, ref))
            changed = ~torch.all(unit_view(out) == unit_view(g), dim=1)
            assert torch.equal(changed, torch.from_numpy(data[f"{c['name']}/clip"])), c["name"]
            assert torch.equal(t.detach().cpu(), p), c["name"]
        assert float(bucket[0]) == 0.0 and torch.equal(bucket[off:].cpu(), torch.zeros(bucket.numel() - off))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _network_params(arch):
    from bcos_hip import synth
    torch.manual_seed(0)
    if arch == "vit_ti":
        net = synth.build_bcosified_vit(seed=0)
    elif arch == "clip_rn50":
        net = synth.build_bcosified_clip_rn50(seed=0)
    else:
        net = synth.build_bcosified_resnet(arch, seed=0)
    return [(n, p) for n, p in net.to(DEV).named_parameters() if p.requires_grad]


def _seeded_grads(named, seed):
    """gradients whose unit norms lie around each unit's threshold: randn times a per-unit factor 10^U(-0.5, 0.5) of max_norm"""
    from bcos_hip import ops
    gen = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _, p in named:
        units, unit_len = ops.agc_units(p.shape)
        g = torch.randn(units, unit_len, device=DEV, generator=gen)
        target = p.detach().reshape(units, unit_len).double().norm(dim=1).clamp(min=1e-3) * 0.01
        target *= 10.0 ** (torch.rand(units, device=DEV, generator=gen, dtype=torch.float64) - 0.5)
        out.append((g * (target / g.double().norm(dim=1).clamp(min=1e-30)).float()[:, None]).reshape(p.shape))
    return out


@pytest.mark.parametrize("arch", ["resnet50", "vit_ti", "clip_rn50"])
def test_network_parameter_sets_against_a_torch_restatement(lib, arch):
    """the parameter lists of the supported networks: within 1e-6 of a torch restatement on the same device whose decisions use fp64 norms,
    the same decisions outside a 1e-5 band around the threshold, and two calls on the same data give the same bits"""
    from bcos.training.agc import adaptive_clip_grad_
    from bcos_hip import ops
    named = _network_params(arch)
    grads = _seeded_grads(named, 7)
    runs = []
    for _ in range(2):
        for (_, p), g in zip(named, grads):
            p.grad = g.clone()
        adaptive_clip_grad_([p for _, p in named])
        runs.append([p.grad.clone() for _, p in named])
    torch.cuda.synchronize()
    clipped = total = 0
    for (name, p), g, a, b in zip(named, grads, runs[0], runs[1]):
        assert torch.equal(a, b), name
        units, unit_len = ops.agc_units(p.shape)
        pu, gu = p.detach().reshape(units, unit_len), g.reshape(units, unit_len)
        max_norm = pu.double().norm(dim=1).clamp(min=1e-3) * 0.01
        gn = gu.double().norm(dim=1)
        decide = gn >= max_norm
        ref = torch.where(decide[:, None], gu * (max_norm / gn.clamp(min=1e-6)).float()[:, None], gu)
        assert rel(a, ref.reshape(p.shape)) <= 1e-6, (name, rel(a, ref))
        changed = ~torch.all(a.reshape(units, unit_len) == gu, dim=1)
        outside = (gn / max_norm - 1.0).abs() > 1e-5
        assert torch.equal(changed[outside], decide[outside]), name
        clipped += int(decide.sum())
        total += units
    assert 0.2 <= clipped / total <= 0.8, (arch, clipped, total)


def test_device_refusals(lib):
    from bcos_hip import ops
    from bcos_hip.lib import BcosHipError
    p = torch.nn.Parameter(torch.ones(8, 8, device=DEV))
    p.grad = torch.ones(8, 16, device=DEV)[:, ::2]
    with pytest.raises(BcosHipError, match="contiguous"):
        ops.agc_clip([p])
    d = torch.nn.Parameter(torch.ones(8, 8, device=DEV, dtype=torch.float64))
    d.grad = torch.ones_like(d)
    with pytest.raises(BcosHipError, match="float32"):
        ops.agc_clip([d])
    q = torch.nn.Parameter(torch.ones(2, 3, 4, device=DEV))
    q.grad = torch.ones_like(q)
    p.grad = torch.ones_like(p)
    with pytest.raises(BcosHipError, match="blocks.0.w"):
        ops.agc_clip([("w", p), ("blocks.0.w", q)])
    torch.cuda.synchronize()
    assert torch.equal(p.grad, torch.ones_like(p))            # refused before any launch


def _recipe_net(meta, data):
    from bcos_hip import synth
    net = synth.build_bcosified_resnet("resnet14b", seed=meta["weight_seed"])
    synth.apply_calibration(net, {k: torch.from_numpy(data["calib/" + k]) for k in meta["calib_order"]})
    return net.to(DEV)


@pytest.mark.parametrize("path", ["plan", "layers"])
def test_resnet14b_recipe_against_reference_golden(lib, golden_dir, path):
    """three steps of the reference recipe -- UniformOffLabelsBCEWithLogitsLoss, adaptive_clip_grad_, AdamW(weight_decay 0, lr 1e-4) -- on the
    resnet14b fixture network through the training plan and per layer.  Each quantity within max(its bound, 3 x the reference's own
    fp32-vs-fp64 distance at that step): Adam moves every coordinate by ~lr however small its gradient, so from the second step on the
    reference is ~1e-2 from itself and its clip decisions move by as much."""
    from bcos.modules.losses import UniformOffLabelsBCEWithLogitsLoss
    from bcos.training.agc import adaptive_clip_grad_
    from bcos_hip import engine, synth
    meta = json.load(open(os.path.join(golden_dir, "resnet14b_recipe.json")))
    data = np.load(os.path.join(golden_dir, "resnet14b_recipe.npz"))
    net = _recipe_net(meta, data)
    if path == "plan":
        engine.attach(net)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == meta["param_names"]
    p0 = [p.detach().clone() for _, p in named]
    crit = UniformOffLabelsBCEWithLogitsLoss()
    opt = torch.optim.AdamW([{"params": net.parameters(), "weight_decay": 0}], lr=1e-4)
    xs = [synth.synthetic_images(4, seed=s, size=meta["size"]).to(DEV) for s in meta["image_seeds"]]

    def norms(ts):
        return torch.stack([t.detach().cpu().double().norm() for t in ts])

    def worst(a, b):
        return float(((a - b).abs() / b.clamp_min(1e-300)).max())

    for k in range(meta["steps"]):
        fl = meta["reference_self_floor"]["fp32_vs_fp64"][k]
        tol = {q: max(bound, 3.0 * fl[q]) for q, bound in (("loss", 1e-5), ("grads", 1e-4), ("exp_avg", 1e-4), ("exp_avg_sq", 2e-4), ("delta", 1e-4))}
        net.train()
        opt.zero_grad(set_to_none=True)
        out = net(xs[k])
        if path == "plan":
            assert type(out.grad_fn).__name__ == "_TrainStepFnBackward"
        loss = crit(out, torch.tensor(meta["labels"][k], device=DEV)) * meta["loss_scale"]
        ref_loss = float(data[f"step{k}/loss"])
        assert abs(float(loss.detach()) - ref_loss) <= tol["loss"] * abs(ref_loss), (k, float(loss.detach()), ref_loss)
        loss.backward()
        margin = []
        for _, p in named:
            pu, gu = unit_view(p.detach()), unit_view(p.grad.detach())
            margin.append(gu.double().norm(dim=1) / (pu.double().norm(dim=1).clamp(min=1e-3) * 0.01) - 1.0)
        margin = torch.cat(margin).cpu()
        before = [p.grad.detach().clone() for _, p in named]
        adaptive_clip_grad_(net.parameters())
        grads = [p.grad.detach().clone() for _, p in named]
        # the units the kernel rewrote
        clipped = torch.cat([~torch.all(unit_view(a) == unit_view(b), dim=1) for a, b in zip(grads, before)]).cpu()
        opt.step()
        st = [opt.state[p] for _, p in named]
        got = dict(grads=norms(grads), exp_avg=norms([s["exp_avg"] for s in st]), exp_avg_sq=norms([s["exp_avg_sq"] for s in st]),
                   delta=norms([p.detach() - q for (_, p), q in zip(named, p0)]))
        for q, v in got.items():
            assert worst(v, torch.from_numpy(data[f"step{k}/{q}_norms"])) <= tol[q], (k, q, worst(v, torch.from_numpy(data[f"step{k}/{q}_norms"])))
        for n in meta["keep"]:
            assert rel(grads[meta["param_names"].index(n)], torch.from_numpy(data[f"step{k}/grad/{n}"])) <= tol["grads"], (k, n)
        # the same units clip, apart from those within 1e-3 of the threshold (from the second step on: within the reference's own spread)
        ref_clip = torch.from_numpy(data[f"step{k}/clip"])
        ref_margin = torch.from_numpy(data[f"step{k}/margin"]).double()
        band = max(1e-3, 3.0 * fl["grads"])
        far = (ref_margin.abs() > band) & (margin.abs() > band)
        assert torch.equal(clipped[far], ref_clip[far]), (k, int((clipped != ref_clip)[far].sum()))
    st = {n: opt.state[p] for n, p in named}
    fl = meta["reference_self_floor"]["fp32_vs_fp64"][-1]
    for n in meta["keep"]:
        i = meta["param_names"].index(n)
        for q, v, bound in (("exp_avg", st[n]["exp_avg"], 1e-4), ("exp_avg_sq", st[n]["exp_avg_sq"], 2e-4), ("delta", named[i][1].detach() - p0[i], 1e-4)):
            assert rel(v, torch.from_numpy(data[f"final/{q}/{n}"])) <= max(bound, 3.0 * fl[q]), (q, n)
    if path == "plan":
        # eval mode after the updates: the inference plan re-reads the parameters the optimizer wrote
        net.eval()
        x = xs[0]
        with torch.no_grad():
            le = net(x)
        engine.detach(net)
        with torch.no_grad():
            lm = net(x)
        assert rel(le, lm) <= 1e-5
