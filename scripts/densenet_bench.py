"""B-cosified DenseNet-121 on the fused plan against the module path, one JSON line (needs a HIP device):

  network   DenseNet-121, 224 x 224, batch 256 (the module path in chunks of --module-chunk images: its autograd graph keeps every
            concatenation): forward and forward + explanation in images/s, the plan (bcos_hip.densenet_engine) and the module path
            alternated in one process and timed with device events after a warm-up.  No target; no number is asserted anywhere.
  launches  bcos_slice_affine_rows (norm + ReLU of a [M, 512] slice of a [M, 1024] buffer, with row maxima) and
            bcos_slice_affine_bwd_acc (accumulating into the same slice, gate rebuilt) alone, each beside bcos_stream_copy of the bytes
            the launch moves.  Ratios only.

python scripts/densenet_bench.py [--batch 256] [--rounds 5] [--iters 20] [--out FILE]     (writes profiles/densenet_bench.json unless told otherwise)
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import densenet_engine, lib, ops, synth  # noqa: E402

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


def stats(ts, images=None):
    out = dict(device_ms=round(median(ts), 4), spread_ms=[round(min(ts), 4), round(max(ts), 4)])
    if images:
        out["images_per_s"] = round(images / (median(ts) * 1e-3), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--module-chunk", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "densenet_bench.json"))
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "densenet_bench.py needs a HIP device"
    net = synth.build_bcosified_densenet(seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123, size=args.size).to(DEV))
    net.eval()
    B, chunk = args.batch, args.module_chunk
    x = synth.synthetic_images(B, seed=1000, size=args.size).to(DEV)
    eng = densenet_engine.DenseNetEngine(net)

    def module_forward():
        with torch.no_grad():
            return torch.cat([net(x[i:i + chunk]) for i in range(0, B, chunk)])

    def module_explain():
        return [net.explain_batch(x[i:i + chunk])["contribution_map"] for i in range(0, B, chunk)]

    variants = dict(plan_forward=lambda: eng.forward(x), module_forward=module_forward,
                    plan_explain=lambda: eng.explain(x), module_explain=module_explain)
    # same results before anything is timed: logits of the two paths, and the maps of the first chunk
    lp, lm = variants["plan_forward"](), variants["module_forward"]()
    agree = dict(logits_rel_l2=float((lp.double() - lm.double()).norm() / lm.double().norm()),
                 classes_equal=bool(torch.equal(lp.argmax(1), lm.argmax(1))))
    mp, mm = eng.explain(x[:chunk])["contribution_map"], net.explain_batch(x[:chunk])["contribution_map"]
    agree["maps_rel_l2"] = float((mp.double() - mm.double()).norm() / mm.double().norm())
    for fn in variants.values():                                          # warm-up: plans, weight images, the allocator's pools
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    network = {k: stats(v, B) for k, v in times.items()}
    network["plan_over_module_forward_time"] = round(median(times["plan_forward"]) / median(times["module_forward"]), 4)
    network["plan_over_module_explain_time"] = round(median(times["plan_explain"]) / median(times["module_explain"]), 4)

    # the two launches alone, beside the library's streaming copy of as many bytes
    M, C, pitch = B * 14 * 14, 512, 1024
    X = torch.randn(M, pitch, device=DEV)
    G = torch.randn(M, pitch, device=DEV)
    d = torch.randn(M, C, device=DEV)
    sc, sh = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1
    y = torch.empty(M, C, device=DEV)

    def timed(fn):
        for _ in range(3):
            fn()
        return [event_ms(fn) for _ in range(args.iters)]
    launches = {}
    for label, fn, floats in (("slice_affine_rows", lambda: ops.slice_affine_rows(X[:, :C], sc, sh, relu=True, out=y), 2 * M * C),
                              ("slice_affine_bwd_acc", lambda: ops.slice_affine_bwd_acc(d, G[:, :C], X[:, :C], sc, sh, relu=True), 4 * M * C)):
        src = torch.empty(floats // 2, device=DEV)             # a copy moves its bytes twice: read + write
        dst = torch.empty_like(src)
        ts, cs = timed(fn), timed(lambda: ops.stream_copy(src, dst))
        launches[label] = dict(stats(ts), bytes_moved=4 * floats, stream_copy_same_bytes=stats(cs),
                               time_over_stream_copy=round(median(ts) / median(cs), 3))
        del src, dst
    out = dict(metric="B-cosified DenseNet-121: the fused plan against the module path (forward, forward + explanation), and the two dense-block "
                      "launches against bcos_stream_copy of the bytes they move",
               batch=B, module_chunk=chunk, image=[args.size, args.size], rounds=args.rounds, agreement=agree, network=network,
               launches=launches, contraction=lib.get_contraction_mode(), device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
