"""Cost of explaining a linear functional of the logits on the fused engines, one JSON line (needs a HIP device):

  step       ResNet-50, batch 256, 224 x 224, three explanation steps alternated in one process and timed with device events after a warm-up:
             (a) explain(x, targets)                          the single-target step (rank-one head launch);
             (b) explain(x, functional=contrast(a, b))        the sparse form (bcos_head_rankm_grad, J = 2);
             (c) explain(x, functional=mean_corrected(t, K))  the dense form (bcos_head_cotangent_grad + the head's K = 1000 contraction).
             A sparse step over 1.03 x the single-target step (the node-to-node spread of DESIGN §7) wants an explanation before merging.
  selection  OursRelative.attribute_selection for a 2 x 2 and a 3 x 3 grid image (T = 4 and 9 targets) on ResNet-50 and ViT-Ti: the engine
             path (one forward, T backward passes) against the same call after engine.detach -- per-layer autograd, one image and one target
             at a time, what the explainer did before the engines took functionals.  Wall time around a device synchronise.

python scripts/head_functional_bench.py [--rounds 5] [--batch 256] [--out profiles/head_functional_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import engine, lib, localisation, synth, vit_engine  # noqa: E402
from bcos_hip.functional import LogitFunctional  # noqa: E402
from interpretability.explanation_methods.explainers import get_explainer  # noqa: E402

DEV = "cuda"


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(variants, rounds, timer, warmup=2):
    for _ in range(warmup):
        for fn in variants.values():
            timer(fn)
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timer(fn))
    return times


def step_times(args):
    net = synth.build_bcosified_resnet("resnet50", seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    eng = engine.attach(net.eval())
    x = synth.synthetic_images(args.batch, seed=1000).to(DEV)
    g = torch.Generator().manual_seed(0)
    t, a, b = (torch.randint(0, 1000, (args.batch,), generator=g) for _ in range(3))
    contrast, mean = LogitFunctional.contrast(a, b), LogitFunctional.mean_corrected(t, 1000)
    variants = dict(single_target=lambda: eng.explain(x, targets=t), contrast=lambda: eng.explain(x, functional=contrast),
                    mean_corrected=lambda: eng.explain(x, functional=mean))
    times = alternate(variants, args.rounds, event_ms, warmup=3)
    res = {k: dict(ms=round(median(v), 4), spread_ms=[round(min(v), 4), round(max(v), 4)]) for k, v in times.items()}
    base = median(times["single_target"])
    res["contrast_over_single"] = round(median(times["contrast"]) / base, 4)
    res["mean_corrected_over_single"] = round(median(times["mean_corrected"]) / base, 4)
    res["sparse_within_node_spread"] = bool(median(times["contrast"]) / base <= 1.03)
    res.update(batch=args.batch, streams=eng.n_streams(x))
    return res


def selection_times(args, name, net, attach, detach, size):
    out = {}
    for grid in (2, 3):
        n = grid * grid
        cell = {2: size // 2, 3: 80}[grid]                       # 224 x 224 and 240 x 240 grid images (multiples of the ViT patch)
        singles = synth.synthetic_images(n, seed=40 + grid, size=cell).to(DEV)
        multi = localisation.make_multi_image(singles).contiguous()
        tg = torch.randint(0, 1000, (n,), generator=torch.Generator().manual_seed(grid)).tolist()
        attach(net)
        fused = get_explainer(net, "OursRelative", "default")
        assert fused._engine() is not None
        tf = alternate(dict(engine=lambda: fused.attribute_selection(multi, tg)), args.rounds, wall, warmup=2)["engine"]
        detach(net)
        plain = get_explainer(net, "OursRelative", "default")
        assert plain._engine() is None
        tp = alternate(dict(modules=lambda: plain.attribute_selection(multi, tg)), max(2, args.rounds // 2), wall, warmup=1)["modules"]
        out[f"grid{grid}x{grid}"] = dict(targets=n, image=list(multi.shape[-2:]), engine_s=round(median(tf), 5), modules_s=round(median(tp), 5),
                                         modules_over_engine=round(median(tp) / median(tf), 2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "head_functional_bench.py needs a HIP device"
    step = step_times(args)
    r50 = synth.build_bcosified_resnet("resnet50", seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(r50, synth.synthetic_images(8, seed=123).to(DEV))
    sel = dict(resnet50=selection_times(args, "resnet50", r50.eval(), engine.attach, engine.detach, 224))
    vit = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV).eval()
    sel["vit_ti"] = selection_times(args, "vit_ti", vit, vit_engine.attach, engine.detach, 224)
    out = dict(metric="linear functionals of the logits on the fused engines: a single-target, a contrast and a mean-corrected explanation step "
                      "(device events, alternated), and OursRelative.attribute_selection on the engine against the per-layer module path",
               step=step, selection=sel, rounds=args.rounds, contraction=lib.get_contraction_mode(), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
