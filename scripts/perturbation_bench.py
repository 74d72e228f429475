"""Cost of the pixel-perturbation analysis on the fused engine, one JSON line (needs a HIP device):

  forward   ResNet-50, 224 x 224, B = 32 images x K = 11 removal levels = 352 copies, three variants alternated in one process and timed
            with device events after a warm-up:
            (a) engine.forward on the PRE-BUILT batch of the 352 copies -- what a caller has who already paid for masking;
            (b) engine.forward(x, perturb=plan) -- the perturbed forward, nothing pre-built;
            (c) the copies masked with torch ops from the same thresholds, then engine.forward: the route without the new keyword.
            Target: time of (b) <= 1.03 x time of (a) (the node and round-to-round spread of DESIGN §7).
  launches  bcos_perturb_select (32 images, 11 counts) and bcos_prep_input_perturbed (352 copies) alone, each beside bcos_stream_copy of
            the same number of bytes (the scores the select reads; the prepared input the prep writes).  Ratios only.
  harness   the whole pixel_perturbation call for the 32 images (explain for the scores, select, the perturbed forwards, the class
            scores), wall time.  No target.

python scripts/perturbation_bench.py [--rounds 5] [--iters 20] [--out FILE]     (writes profiles/perturbation_bench.json unless told otherwise)
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import engine, lib, ops, perturbation, synth  # noqa: E402

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


def stats(ts):
    return dict(device_ms=round(median(ts), 4), spread_ms=[round(min(ts), 4), round(max(ts), 4)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "perturbation_bench.json"))
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "perturbation_bench.py needs a HIP device"
    net = synth.build_bcosified_resnet(args.arch, seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    net.eval()
    eng = engine.attach(net)
    B = args.images
    x = synth.synthetic_images(B, seed=1000).to(DEV)
    H, W = x.shape[-2:]
    HW = H * W
    counts = perturbation.removal_counts(perturbation.DEFAULT_FRACTIONS, HW)
    K = len(counts)
    scores = eng.explain(x, want_weights=False)["contribution_map"].reshape(B, HW).contiguous()
    thr = ops.perturb_select(scores, counts)
    plan = perturbation.PerturbPlan(scores, thr, False)
    prebuilt = perturbation.materialise(x, scores, thr).contiguous()

    variants = dict(a_forward_prebuilt=lambda: eng.forward(prebuilt), b_forward_perturbed=lambda: eng.forward(x, perturb=plan),
                    c_mask_then_forward=lambda: eng.forward(perturbation.materialise(x, scores, thr)))
    assert torch.equal(variants["a_forward_prebuilt"](), variants["b_forward_perturbed"]())
    for fn in variants.values():                                          # warm-up: plans, workspaces, the allocator's pools
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    fwd = {k: stats(v) for k, v in times.items()}
    ta, tb, tc = (median(times[k]) for k in variants)
    fwd["copies"] = B * K
    fwd["b_over_a_time"] = round(tb / ta, 4)
    fwd["c_over_a_time"] = round(tc / ta, 4)
    fwd["b_over_c_time"] = round(tb / tc, 4)
    fwd["target"] = dict(b_over_a_max=1.03, met=bool(tb / ta <= 1.03))

    # the two launches alone, beside the library's streaming copy of as many bytes
    mean, std = eng._consts(x.device)
    launches = {}

    def timed(fn):
        for _ in range(3):
            fn()
        return [event_ms(fn) for _ in range(args.iters)]
    for label, fn, floats in (("perturb_select", lambda: ops.perturb_select(scores, counts), scores.numel()),
                              ("prep_input_perturbed", lambda: ops.prep_input_perturbed(x, scores, thr, mean, std), B * K * HW * 8)):
        src = torch.empty(floats, device=DEV)
        dst = torch.empty_like(src)
        ts, cs = timed(fn), timed(lambda: ops.stream_copy(src, dst))
        launches[label] = dict(stats(ts), bytes=4 * floats, stream_copy_same_bytes=stats(cs), time_over_stream_copy=round(median(ts) / median(cs), 3))
        del src, dst

    def harness():
        perturbation.pixel_perturbation(net, x)
    harness()
    hs = [wall(harness) for _ in range(args.rounds)]
    out = dict(metric="pixel perturbation on the fused engine: the perturbed forward against engine.forward on a pre-built batch and against "
                      "masking with torch ops, the select and prep launches against bcos_stream_copy, and the whole harness call",
               arch=args.arch, images=B, levels=K, counts=counts, image=[int(H), int(W)], rounds=args.rounds, forward=fwd, launches=launches,
               harness=dict(seconds=round(median(hs), 5), spread_s=[round(min(hs), 5), round(max(hs), 5)], images=B, copies=B * K),
               contraction=lib.get_contraction_mode(), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
