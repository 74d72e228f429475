"""Cost of the RISE explainer on the fused engine, one JSON line (needs a HIP device).  ResNet-50, one 224 x 224 image, two
configurations: `default` (n = 500, s = 8, batch_size 8) and the class default (n = 6000, s = 6, batch_size 2).  Per configuration, the
variants alternated in one process:

  forward     chunks of 256 copies:
              (a) engine.forward on a PRE-BUILT masked batch -- what a caller gets who has already paid for `img * masks`;
              (b) engine.forward(img, rise=bank[lo:hi]) -- nothing pre-built, neither masks nor copies stored;
              (c) `img * masks[lo:hi]` with torch ops on dense masks already in device memory, then engine.forward.
              Reported as copies per second.
  accumulate  bcos_rise_accumulate alone (device events, arguments prebuilt) for 4 targets and for all 1000 classes, with the bytes it
              writes per second as a fraction of what bcos_stream_copy writes per second for the same bytes in the same run.
  attribute   the whole RISE.attribute_selection call with T = 4 on the engine (wall time, median) against the module path (no engine:
              `model(img * ops.rise_masks(chunk))` per batch_size; wall time of ONE call).

python scripts/rise_bench.py [--rounds 3] [--iters 20] [--out profiles/rise_bench.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import engine, lib, ops, synth  # noqa: E402
from interpretability.explanation_methods.explainers.rise import RISE  # noqa: E402

DEV = "cuda"
CHUNK = 256
TARGETS = [1, 250, 500, 999]


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return median(ts), min(ts)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def one_config(name, net, eng, img, kwargs, args):
    H, W = img.shape[-2:]
    rise = RISE(net, **kwargs)
    rise.engine_batch_size = CHUNK
    first_call = wall(lambda: rise.attribute_selection(img, TARGETS))        # builds and uploads the bank, warms every plan
    bank = rise._bank(img)
    n = len(bank)
    cuts = [(lo, min(n, lo + CHUNK)) for lo in range(0, n, CHUNK)]
    dense = ops.rise_masks(bank, H, W, first=0, n=min(CHUNK, n))             # one chunk of dense masks, reused by (a) and (c)
    prebuilt = (img * dense[:, None]).contiguous()
    per_chunk = prebuilt.shape[0]
    variants = {
        "prebuilt_batch": (lambda: [eng.forward(prebuilt) for _ in cuts], per_chunk * len(cuts)),
        "rise_forward": (lambda: [eng.forward(img, rise=bank[lo:hi]) for lo, hi in cuts], n),
        "torch_masking": (lambda: [eng.forward(img * dense[:, None]) for _ in cuts], per_chunk * len(cuts)),
    }
    times = {k: [] for k in variants}
    for fn, _ in variants.values():
        fn()
    for _ in range(args.rounds):
        for k, (fn, _) in variants.items():
            times[k].append(wall(fn))
    fwd = {k: dict(seconds=median(times[k]), copies=variants[k][1], copies_per_s=variants[k][1] / median(times[k])) for k in variants}
    fwd["rise_over_prebuilt"] = fwd["rise_forward"]["copies_per_s"] / fwd["prebuilt_batch"]["copies_per_s"]
    fwd["rise_over_torch_masking"] = fwd["rise_forward"]["copies_per_s"] / fwd["torch_masking"]["copies_per_s"]

    acc = {}
    for T in (4, 1000):
        scores = torch.rand(n, T, device=DEV)
        out = ops.rise_accumulate(scores, bank, H, W, rise.p1)
        src = torch.empty_like(out)
        ops.stream_copy(src, out)
        a_ms, a_min = event_ms(lambda: ops.rise_accumulate(scores, bank, H, W, rise.p1), args.iters)
        c_ms, c_min = event_ms(lambda: ops.stream_copy(src, out), args.iters)
        acc[f"T{T}"] = dict(accumulate_ms=a_ms, accumulate_ms_min=a_min, stream_copy_ms=c_ms, stream_copy_ms_min=c_min,
                            bytes_written=out.numel() * 4, write_rate_over_stream_copy=c_ms / a_ms)

    t_eng = median([wall(lambda: rise.attribute_selection(img, TARGETS)) for _ in range(args.rounds)])
    engine.detach(net)
    try:
        mod = RISE(net, **kwargs)
        t_mod = wall(lambda: mod.attribute_selection(img, TARGETS))
    finally:
        engine.attach(net)
    return dict(config=name, kwargs=kwargs, n=n, first_call_s=first_call, forward=fwd, accumulate=acc,
                attribute_selection_T4=dict(engine_s=t_eng, module_path_s=t_mod, module_over_engine=t_mod / t_eng))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "rise_bench.py needs a HIP device"
    net = synth.build_bcosified_resnet(args.arch, seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    net.eval()
    eng = engine.attach(net)
    img = synth.synthetic_images(1, seed=1000).to(DEV)
    from interpretability.explanation_methods.explanation_configs import explainer_configs
    res = dict(bench="rise", arch=args.arch, image=list(img.shape), chunk=CHUNK, rounds=args.rounds, iters=args.iters,
               device=torch.cuda.get_device_name(0), configs=[])
    for name, kwargs in (("default", dict(explainer_configs["RISE"]["default"])), ("class_default", dict(batch_size=2, n=6000, s=6, p1=0.1))):
        res["configs"].append(one_config(name, net, eng, img, kwargs, args))
        eng = net._bcos_engine
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
