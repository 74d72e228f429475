"""Cost of the Occlusion explainer on the fused engine, one JSON line (needs a HIP device):

  forward     `Occ9` (stride 2, ks 9: 12,544 masks) on one 224 x 224 image, ResNet-50, chunks of 256, three variants alternated in one process:
              (a) engine.forward on a PRE-BUILT masked batch of 256 images, once per chunk -- the baseline: what the parent commit offers a
                  caller who has already paid for building `img * masks`;
              (b) engine.forward(img, occlude=bank[lo:hi]) per chunk -- the occluded forward, nothing pre-built;
              (c) the whole Occlusion.attribute call (the image's forward, the chunks, the bank, one accumulate launch), wall time.
              Targets: images/s of (b) >= 0.97 x (a); time of (c) <= 1.10 x the time (a) needs for the same number of images.
  accumulate  bcos_occlusion_accumulate alone (device events, arguments prebuilt) for all 1000 classes (about 200 MB written) and for 4
              targets, with its written bytes per second as a fraction of the bytes bcos_stream_copy writes per second in the same run.

python scripts/occlusion_bench.py [--rounds 3] [--iters 20] [--out profiles/occlusion_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import engine, lib, ops, synth  # noqa: E402
from interpretability.explanation_methods.explainers import get_explainer  # noqa: E402

DEV = "cuda"
CHUNK = 256


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--config", default="Occ9")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "occlusion_bench.py needs a HIP device"
    net = synth.build_bcosified_resnet(args.arch, seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    net.eval()
    eng = engine.attach(net)
    img = synth.synthetic_images(1, seed=1000).to(DEV)
    occ = get_explainer(net, "Occlusion", args.config)
    occ.engine_batch_size = CHUNK
    first_call = wall(lambda: occ.attribute(img, 1))                 # builds and uploads the bank, warms every plan
    bank = occ._bank(img)
    n = bank.shape[0]
    H, W = img.shape[-2:]
    cuts = list(range(0, n, CHUNK))
    rows = torch.arange(H, device=DEV)[None, :]
    r = bank[:CHUNK].long()
    keep = ~(((rows >= r[:, 0:1]) & (rows < r[:, 1:2]))[:, :, None] & ((rows >= r[:, 2:3]) & (rows < r[:, 3:4]))[:, None, :])
    masked = (img * keep[:, None].float()).contiguous()              # the pre-built batch of the baseline
    full = [lo for lo in cuts if lo + CHUNK <= n]                     # (12,544 = 49 x 256: every chunk is full)

    def baseline():
        for _ in full:
            eng.forward(masked)

    def occluded():
        for lo in full:
            eng.forward(img, occlude=bank[lo:lo + CHUNK])

    def attribute():
        occ.attribute(img, 1)
    variants = dict(a_forward_prebuilt=baseline, b_forward_occluded=occluded, c_attribute=attribute)
    times = {k: [] for k in variants}
    for fn in variants.values():
        wall(fn)
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(wall(fn))
    imgs = len(full) * CHUNK
    res = {k: dict(seconds=round(median(v), 5), spread_s=[round(min(v), 5), round(max(v), 5)]) for k, v in times.items()}
    ta, tb, tc = (median(times[k]) for k in variants)
    res["a_forward_prebuilt"]["images_per_s"] = round(imgs / ta, 1)
    res["b_forward_occluded"]["images_per_s"] = round(imgs / tb, 1)
    res["b_over_a_images_per_s"] = round(ta / tb, 4)
    res["c_images"] = n + 1
    res["c_over_a_time_same_images"] = round(tc / (ta * (n + 1) / imgs), 4)
    res["targets"] = dict(b_over_a_min=0.97, c_over_a_max=1.10, b_met=bool(ta / tb >= 0.97), c_met=bool(tc / (ta * (n + 1) / imgs) <= 1.10))
    res["attribute_first_call_s"] = round(first_call, 4)

    # where the time of attribute() goes, each part alone
    org = eng.forward(img)
    pert = torch.empty((n, org.shape[1]), device=DEV)
    for lo in cuts:
        pert[lo:lo + CHUNK] = eng.forward(img, occlude=bank[lo:lo + CHUNK])
    parts = dict(image_forward_s=wall(lambda: eng.forward(img)), bank_upload_s=wall(lambda: occ.masks.to(DEV)),
                 accumulate_call_s=wall(lambda: ops.occlusion_accumulate(org.reshape(-1), pert, bank, H, W, targets=[1], rects_host=occ.masks)))
    res["attribute_parts"] = {k: round(v, 6) for k, v in parts.items()}

    # the accumulate launch alone
    handle = lib.load()
    host = occ.masks
    CL = org.shape[1]
    orgv = org.reshape(-1).contiguous()
    acc = {}
    src = torch.empty(CL * H * W, device=DEV)
    dst = torch.empty_like(src)
    for _ in range(3):
        ops.stream_copy(src, dst)
    copy_ms, copy_min = event_ms(lambda: ops.stream_copy(src, dst), args.iters)
    copy_write_bps = 4 * src.numel() / (copy_ms * 1e-3)
    for label, tg in (("all_classes", None), ("four_targets", torch.tensor([1, 10, 100, 999], dtype=torch.int32, device=DEV))):
        T = CL if tg is None else tg.numel()
        out = dst[:T * H * W].view(T, H, W)

        def launch():
            lib.check(handle.bcos_occlusion_accumulate(C.c_void_p(orgv.data_ptr()), C.c_void_p(pert.data_ptr()), C.c_void_p(bank.data_ptr()),
                                                       None, C.c_void_p(tg.data_ptr()) if tg is not None else None, C.c_void_p(out.data_ptr()),
                                                       n, CL, T, H, W, 0, ops._stream()), "bcos_occlusion_accumulate")
        for _ in range(3):
            launch()
        ms, ms_min = event_ms(launch, args.iters)
        written = 4 * T * H * W
        acc[label] = dict(T=T, written_mb=round(written / 1e6, 2), device_ms=round(ms, 4), device_min_ms=round(ms_min, 4),
                          written_gbps=round(written / (ms * 1e-3) / 1e9, 1), frac_of_stream_copy_write_rate=round(written / (ms * 1e-3) / copy_write_bps, 4))
    acc["stream_copy"] = dict(floats=src.numel(), device_ms=round(copy_ms, 4), device_min_ms=round(copy_min, 4),
                              written_gbps=round(copy_write_bps / 1e9, 1), note="bytes WRITTEN per second (the copy reads as many)")
    out = dict(metric="Occlusion on the fused engine: occluded forward against engine.forward on a pre-built masked batch, the whole attribute "
                      "call, and the accumulate launch", arch=args.arch, config=args.config, masks=n, chunk=CHUNK, image=[int(H), int(W)],
               rounds=args.rounds, forward=res, accumulate=acc, contraction=lib.get_contraction_mode(), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
