"""Generate the adaptive-gradient-clipping fixtures under tests/golden/ by RUNNING THE REFERENCE (its bcos/training/agc.py and
bcos/modules/losses.py) on CPU.  Build container only:   python tests/golden/make_golden_agc.py

  agc_cases.{json,npz}         every unit rule of unitwise_norm (bcos/training/agc.py:12-25) and adaptive_clip_grad_ (agc.py:28-42) on
                               seeded inputs: p = randn * p_scale[unit], g = randn * g_scale[unit], the scales chosen so that every unit lies
                               at least 1e-3 (relative) from its threshold and about half of them clip.  Recorded: the reference's norms,
                               clip decisions and clipped gradients (full tensors for the small cases; for the large ones the fp32 factor of
                               every unit, which reproduces the reference's output bit for bit -- checked here); a NaN unit; unitwise_norm of
                               a 3-D tensor; the recipe losses on dense and sparse targets.
  resnet14b_recipe.{json,npz}  three steps of the reference recipe on the resnet14b fixture network (the weights and calibration of
                               make_golden.py: resnet14b_training_step): UniformOffLabelsBCEWithLogitsLoss, adaptive_clip_grad_,
                               optim.AdamW([{'params': ..., 'weight_decay': 0}], lr=1e-4) as bcos/training/trainer.py:564-627 builds it,
                               with the reference's own fp32-vs-fp64 distance of the same steps.

The reference's agc.py is loaded by file path: its package __init__ (bcos/training/__init__.py) imports pytorch_lightning, which is absent.
"""
import copy
import importlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (sets up the reference import: oracle/refimport.py)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import refimport  # noqa: E402

from bcos_hip import synth  # noqa: E402


def reference_agc():
    spec = importlib.util.spec_from_file_location("_reference_agc", os.path.join(refimport.REFERENCE_ROOT, "bcos", "training", "agc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RA = reference_agc()
RL = importlib.import_module("bcos.modules.losses")
CLIP_FACTOR, EPS = 0.01, 1e-3

# (name, shape): every unit rule -- stem filters of 294 floats (unit starts not 16-byte aligned), pointwise / 3x3 filters, a wide 1x1 head,
# tensors that squeeze to one dimension ([64,1,1,1] is ONE unit, not 64), rows of matrices, 1-D / 0-d / [1], a long 1-D unit
AGC_CASES = [("stem", [64, 6, 7, 7]), ("pointwise", [256, 64, 1, 1]), ("conv3x3", [64, 64, 3, 3]), ("head1x1", [100, 2048, 1, 1]),
             ("scale4d", [64, 1, 1, 1]), ("single_filter", [1, 64, 3, 3]), ("matrix", [576, 192]), ("row", [1, 192]), ("column", [192, 1]),
             ("bn", [2048]), ("scalar", []), ("one", [1]), ("long", [100003])]
FULL_MAX = 40000          # cases up to this size record the reference's clipped gradient in full, larger ones the factor of every unit
SEED = 2024


def unit_view(t):
    """[units, unit_len] view of a tensor along the units of unitwise_norm (contiguous units: every case above)"""
    if t.squeeze().ndim <= 1:
        return t.reshape(1, -1)
    return t.reshape(t.shape[0], -1)


def case_inputs(shape, seed, p_scale, g_scale):
    """the seeded inputs of a case (tests/test_agc_*.py regenerate them the same way)"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    p = (unit_view(p) * p_scale[:, None]).reshape(shape)
    g = (unit_view(g) * g_scale[:, None]).reshape(shape)
    return p, g


def agc_cases():
    out, meta = {}, dict(seed=SEED, clip_factor=CLIP_FACTOR, eps=EPS, full_max=FULL_MAX, cases=[], torch_version=torch.__version__)
    rng = np.random.default_rng(SEED)
    total = clipped = 0
    for k, (name, shape) in enumerate(AGC_CASES):
        seed = SEED + k
        units = unit_view(torch.empty(shape)).shape[0]
        # p scales spread over 1e-4 .. 10 (some units below eps: the clamp), g scales aimed at a ratio gn / max_norm in [0.3, 0.9] or [1.1, 3]
        p_scale = torch.from_numpy(10.0 ** rng.uniform(-4, 1, units)).float()
        if name in ("stem", "conv3x3"):
            p_scale[:3] = 1e-5                                     # whole filters under eps
        p, g1 = case_inputs(shape, seed, p_scale, torch.ones(units))
        pn = unit_view(p).double().norm(dim=1)
        gn1 = unit_view(g1).double().norm(dim=1)
        ratio = torch.from_numpy(np.where(rng.random(units) < 0.5, rng.uniform(0.3, 0.9, units), rng.uniform(1.1, 3.0, units)))
        g_scale = (ratio * pn.clamp(min=EPS) * CLIP_FACTOR / gn1).float()
        p, g = case_inputs(shape, seed, p_scale, g_scale)
        max_norm = unit_view(p).double().norm(dim=1).clamp(min=EPS) * CLIP_FACTOR
        margin = unit_view(g).double().norm(dim=1) / max_norm - 1.0
        assert float(margin.abs().min()) >= 1e-3, (name, float(margin.abs().min()))
        pr, gr = p.clone().requires_grad_(True), g.clone()
        pr.grad = gr
        RA.adaptive_clip_grad_([pr], clip_factor=CLIP_FACTOR, eps=EPS)
        ref = pr.grad.detach()
        clip = ~torch.all(unit_view(ref) == unit_view(g), dim=1)
        assert torch.equal(clip, margin >= 0), name
        # the reference's factor of every unit, in its own arithmetic: it reproduces the output bit for bit
        pn32 = RA.unitwise_norm(p).reshape(-1)
        gn32 = RA.unitwise_norm(g).reshape(-1)
        factor = (pn32.clamp(min=EPS) * CLIP_FACTOR) / gn32.clamp(min=1e-6)
        rebuilt = torch.where(clip[:, None], unit_view(g) * factor[:, None], unit_view(g)).reshape(shape)
        assert torch.equal(rebuilt, ref), name
        out[f"{name}/p_scale"], out[f"{name}/g_scale"] = p_scale, g_scale
        out[f"{name}/p_norm"], out[f"{name}/g_norm"] = pn32, gn32
        out[f"{name}/clip"], out[f"{name}/margin"] = clip, margin.float()
        out[f"{name}/factor"] = factor
        if p.numel() <= FULL_MAX:
            out[f"{name}/clipped"] = ref
        meta["cases"].append(dict(name=name, shape=list(shape), seed=seed, units=int(units), unit_len=int(p.numel() // units),
                                  checksum=[float(p.double().sum()), float(g.double().abs().sum())]))
        total += units
        clipped += int(clip.sum())
    meta["clipped_units"], meta["units"] = clipped, total

    # a NaN gradient unit (row 3) and a NaN parameter unit (row 5): torch.where takes the clipped -- NaN -- gradient for both
    gen = torch.Generator().manual_seed(SEED + 100)
    p = torch.randn(8, 40, generator=gen)
    g = torch.randn(8, 40, generator=gen) * 0.02
    g[3, 7] = float("nan")
    p[5, 0] = float("nan")
    pr = p.clone().requires_grad_(True)
    pr.grad = g.clone()
    RA.adaptive_clip_grad_([pr], clip_factor=CLIP_FACTOR, eps=EPS)
    out.update({"nan/p": p, "nan/g": g, "nan/clipped": pr.grad.detach()})
    meta["nan_case"] = dict(shape=[8, 40], nan_grad_row=3, nan_param_row=5)

    # unitwise_norm of a 3-D tensor (dim 1, strided units) and of a 5-D one that squeezes to one dimension
    x3 = torch.randn(4, 5, 6, generator=gen)
    out.update({"norm3d/x": x3, "norm3d/norm": RA.unitwise_norm(x3)})
    x5 = torch.randn(1, 1, 7, 1, 1, generator=gen)
    out.update({"norm5d_squeezable/x": x5, "norm5d_squeezable/norm": RA.unitwise_norm(x5)})

    # the recipe losses: sparse and dense targets, off_label set and unset, smoothing and threshold
    logits = torch.randn(6, 1000, generator=gen) * 3
    labels = torch.randint(0, 1000, (6,), generator=gen)
    dense = torch.rand(6, 1000, generator=gen)
    out.update({"loss/logits": logits, "loss/labels": labels, "loss/dense": dense})
    losses = []
    for kind, kw in (("uniform", {}), ("uniform", dict(off_label=2e-3)), ("uniform", dict(reduction="sum")),
                     ("bce", {}), ("bce", dict(smoothing=0.1)), ("bce", dict(smoothing=0.1, target_threshold=0.2)), ("bce", dict(reduction="sum"))):
        cls = RL.UniformOffLabelsBCEWithLogitsLoss if kind == "uniform" else RL.BinaryCrossEntropyLoss
        for target in ("sparse", "dense"):
            t = labels if target == "sparse" else dense
            losses.append(dict(kind=kind, kwargs=kw, target=target, value=float(cls(**kw)(logits, t))))
    meta["losses"] = losses

    np.savez_compressed(os.path.join(HERE, "agc_cases.npz"), **MG.t2n(out))
    with open(os.path.join(HERE, "agc_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"agc_cases: {clipped} of {total} units clip")


# ----------------------------------------------------------------------------------------------------------------------------------
RECIPE_KEEP = ("model.conv1.linear.weight", "model.layer4.0.bn3.weight")
RECIPE_STEPS = 3


def units_of(t):
    return unit_view(t) if t.ndim != 3 else None


def recipe_steps(net, xs, labels, loss_scale, dtype=torch.float32):
    """RECIPE_STEPS steps of the reference recipe on `net` (train mode): per step the loss, every clipped gradient, the optimizer state and
    the parameters' movement, and per unit the margin gn / max_norm - 1 of the clip decision"""
    net = net.to(dtype)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    p0 = [p.detach().clone() for _, p in named]
    crit = RL.UniformOffLabelsBCEWithLogitsLoss()
    opt = torch.optim.AdamW([{"params": net.parameters(), "weight_decay": 0}], lr=1e-4)
    steps = []
    for k in range(RECIPE_STEPS):
        net.train()
        opt.zero_grad(set_to_none=True)
        loss = crit(net(xs[k].to(dtype)), labels[k]) * loss_scale
        loss.backward()
        margin = []
        for _, p in named:
            pu, gu = units_of(p.detach()), units_of(p.grad.detach())
            margin.append((gu.double().norm(dim=1) / (pu.double().norm(dim=1).clamp(min=EPS) * CLIP_FACTOR) - 1.0))
        RA.adaptive_clip_grad_(net.parameters())
        grads = [p.grad.detach().clone() for _, p in named]
        opt.step()
        st = [opt.state[p] for _, p in named]
        steps.append(dict(loss=loss.detach().clone(), grads=grads, exp_avg=[s["exp_avg"].clone() for s in st],
                          exp_avg_sq=[s["exp_avg_sq"].clone() for s in st], delta=[p.detach() - q for (_, p), q in zip(named, p0)],
                          margin=torch.cat(margin)))
    return [n for n, _ in named], steps


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def resnet14b_recipe():
    base = json.load(open(os.path.join(HERE, "resnet14b_train_step.json")))
    net = MG.reference_resnet("resnet14b", seed=base["weight_seed"])
    record = synth.calibrate(net, synth.synthetic_images(4, seed=base["calib_seed"], size=64))
    xs = [synth.synthetic_images(4, seed=61 + k, size=64) for k in range(RECIPE_STEPS)]
    labels = [torch.tensor(v) for v in ([5, 321, 999, 40], [77, 0, 512, 640], [3, 900, 128, 250])]
    sd = copy.deepcopy(net.state_dict())
    loss_scale = 1.0
    while True:                          # (a loss scale, recorded, until 5 .. 95 % of the units clip in the first step)
        net.load_state_dict(sd)
        names, steps = recipe_steps(copy.deepcopy(net), xs, labels, loss_scale)
        frac = float((steps[0]["margin"] >= 0).double().mean())
        if frac >= 0.05 or loss_scale >= 1e6:
            break
        loss_scale *= 4.0
    assert 0.05 <= frac <= 0.95, frac
    _, steps64 = recipe_steps(copy.deepcopy(net).double(), [x.double() for x in xs], labels, loss_scale, dtype=torch.float64)

    def norms(ts):
        return torch.stack([t.double().norm() for t in ts])

    out = {f"calib/{k}": v for k, v in record.items()}
    # per step: Adam moves every coordinate by ~lr whatever the size of its gradient, so the coordinates whose gradients are at rounding level
    # move differently in fp32 and fp64 -- the first step's update already differs by ~1e-2, and the later gradients follow it
    floors = []
    for k, (s, s64) in enumerate(zip(steps, steps64)):
        out[f"step{k}/loss"] = s["loss"]
        floor = dict(loss=abs(float(s["loss"]) - float(s64["loss"])) / abs(float(s64["loss"])),
                     flips=int(((s["margin"] >= 0) != (s64["margin"] >= 0)).sum()))
        for q in ("grads", "exp_avg", "exp_avg_sq", "delta"):
            out[f"step{k}/{q}_norms"] = norms(s[q])
            floor[q] = max(_rel(a, b) for a, b in zip(s[q], s64[q]) if b.norm() > 0)
        floors.append(floor)
        out[f"step{k}/margin"] = s["margin"].float()
        out[f"step{k}/clip"] = s["margin"] >= 0
        for n in RECIPE_KEEP:
            out[f"step{k}/grad/{n}"] = s["grads"][names.index(n)]
    last = steps[-1]
    for n in RECIPE_KEEP:
        i = names.index(n)
        out[f"final/exp_avg/{n}"], out[f"final/exp_avg_sq/{n}"], out[f"final/delta/{n}"] = last["exp_avg"][i], last["exp_avg_sq"][i], last["delta"][i]
    np.savez_compressed(os.path.join(HERE, "resnet14b_recipe.npz"), **MG.t2n(out))
    meta = dict(arch="resnet14b", weight_seed=base["weight_seed"], calib_seed=base["calib_seed"], image_seeds=[61 + k for k in range(RECIPE_STEPS)],
                size=64, labels=[v.tolist() for v in labels], loss="UniformOffLabelsBCEWithLogitsLoss() * loss_scale", loss_scale=loss_scale,
                clip_factor=CLIP_FACTOR, eps=EPS, optimizer="AdamW([{'params': ..., 'weight_decay': 0}], lr=1e-4)", steps=RECIPE_STEPS,
                param_names=names, calib_order=list(record.keys()), keep=list(RECIPE_KEEP),
                clipped_fraction=[float((s["margin"] >= 0).double().mean()) for s in steps],
                reference_self_floor=dict(fp32_vs_fp64=floors), torch_version=torch.__version__)
    with open(os.path.join(HERE, "resnet14b_recipe.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("resnet14b_recipe: loss scale", loss_scale, "clipped", meta["clipped_fraction"], "floors", floors)


if __name__ == "__main__":
    which = sys.argv[1:] or ["cases", "recipe"]
    if "cases" in which:
        agc_cases()
    if "recipe" in which:
        resnet14b_recipe()
