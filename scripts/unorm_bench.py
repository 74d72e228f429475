"""The uncentered position / group norm kernels (csrc/bcos_norms.hip, centered=False) and the B-cos ConvNeXt-T built on them, one JSON line (DESIGN:
"Uncentered norms"; needs a HIP device):

  kernels   bcos_layernorm_unc_fwd (rstd kept), _bwd_detached and _bwd over the rows of the NHWC image at the four ConvNeXt-T stages, batch
            64: rows x D = 64 H^2 x C for C x H^2 = 96 x 56^2, 192 x 28^2, 384 x 14^2, 768 x 7^2 (the first two on the float4 kernels, the
            last two on the strided ones), and bcos_groupnorm_unc_fwd / _bwd_detached / _bwd at a GroupNorm stem shape, 64 x 56^2 x 96 in 8
            groups.  Each beside its CENTRED twin (bcos_layernorm_* / bcos_groupnorm_*) on the same tensors and beside bcos_stream_copy
            moving the same algorithmic bytes (the tensors the launch must read and write, once each), alternated in one run: median of
            --iters runs each, device events, with the spread.  Ratios; no target.
  network   ConvNeXt-T at 224^2, batch 64, on the fused plan (bcos_hip.convnext_engine): forward and forward + explanation in images/s with
            NoBias(PositionNormUncentered2d) and with the default centred position norm, alternated in one process (u c c u ...), and
            again with ONE plan per process (pnu, centred, pnu, centred: four processes) -- the two do not agree, DESIGN says why.

Each step runs in a child process of its own under a time limit; a step that fails ends the script.

python scripts/unorm_bench.py [--batch 64] [--iters 20] [--out FILE]     (writes profiles/unorm_bench.json unless told otherwise)
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

DEV = "cuda"
STAGES = ((96, 56), (192, 28), (384, 14), (768, 7))
GROUP_STEM = (56, 96, 8)          # H = W, C, G
STEP_LIMIT_S = {"kernels": 240, "network": 420, "network_alone": 180}


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def event_ms(fn):
    import torch
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


def _time_group(launches, iters):
    """launches: (label, uncentered fn, centred fn, floats moved).  -> {label: record}; every fn and the copy of its bytes alternated"""
    import torch
    from bcos_hip import ops
    fns = {}
    for label, unc, cen, floats in launches:
        src, dst = torch.empty(floats // 2, device=DEV), torch.empty(floats // 2, device=DEV)
        fns[label + "/unc"], fns[label + "/centred"] = unc, cen
        fns[label + "/copy"] = (lambda s=src, d=dst: ops.stream_copy(s, d))
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            times[k].append(event_ms(fn))
    rec = {}
    for label, _, _, floats in launches:
        u, c, cp = (times[f"{label}/{k}"] for k in ("unc", "centred", "copy"))
        rec[label] = dict(stats(u), algorithmic_bytes=4 * floats, gb_per_s=round(4 * floats / (median(u) * 1e-3) / 1e9, 1),
                          centred_twin=stats(c), stream_copy_same_bytes=stats(cp),
                          time_over_centred_twin=round(median(u) / median(c), 3), time_over_stream_copy=round(median(u) / median(cp), 3),
                          slower_than_twin_beyond_spread=bool(min(u) > max(c)))
    return rec


def step_kernels(args):
    import torch
    from bcos_hip import lib, ops
    lib.load()
    N = args.batch
    shapes = {}
    for Cc, HW in STAGES:
        g = torch.Generator().manual_seed(Cc)
        rows = N * HW * HW
        mk = lambda: torch.randn(rows, Cc, generator=g).to(DEV)      # noqa: E731
        x, gy, out = mk() + 0.5, mk(), mk()
        w = (torch.rand(Cc, generator=g) + 0.5).to(DEV)
        _, rstd_u = ops.layernorm_fwd(x, w, None, 1e-6, want_rstd=True, centered=False)
        _, rstd_c = ops.layernorm_fwd(x, w, None, 1e-6, want_rstd=True)
        n = x.numel()
        launches = (
            ("forward_keep_rstd", lambda: ops.layernorm_fwd(x, w, None, 1e-6, want_rstd=True, out=out, centered=False),
             lambda: ops.layernorm_fwd(x, w, None, 1e-6, want_rstd=True, out=out), 2 * n),
            ("backward_detached", lambda: ops.layernorm_bwd_detached(gy, w, rstd_u, out=out, centered=False),
             lambda: ops.layernorm_bwd_detached(gy, w, rstd_c, out=out), 2 * n),
            ("backward_full", lambda: ops.layernorm_bwd(gy, x, w, rstd_u, centered=False), lambda: ops.layernorm_bwd(gy, x, w, rstd_c), 3 * n))
        shapes[f"rows {N}x{HW}x{HW}, D {Cc}"] = dict(_time_group(launches, args.iters), kernel_form="float4" if Cc <= 256 else "strided")
        del x, gy, out
        torch.cuda.empty_cache()
    HW, Cc, G = GROUP_STEM
    g = torch.Generator().manual_seed(7)
    mk = lambda: torch.randn(N, HW, HW, Cc, generator=g).to(DEV)      # noqa: E731
    x, gy = mk() + 0.5, mk()
    w, b = (torch.rand(Cc, generator=g) + 0.5).to(DEV), torch.randn(Cc, generator=g).to(DEV)
    _, rstd_u = ops.groupnorm_fwd(x, G, w, b, 1e-5, want_rstd=True, centered=False)
    _, rstd_c = ops.groupnorm_fwd(x, G, w, b, 1e-5, want_rstd=True)
    n = x.numel()
    launches = (
        ("forward_keep_rstd", lambda: ops.groupnorm_fwd(x, G, w, b, 1e-5, want_rstd=True, centered=False), lambda: ops.groupnorm_fwd(x, G, w, b, 1e-5, want_rstd=True), 2 * n),
        ("backward_detached", lambda: ops.groupnorm_bwd_detached(gy, G, w, rstd_u, centered=False), lambda: ops.groupnorm_bwd_detached(gy, G, w, rstd_c), 2 * n),
        ("backward_full", lambda: ops.groupnorm_bwd(gy, x, G, w, rstd_u, centered=False), lambda: ops.groupnorm_bwd(gy, x, G, w, rstd_c), 3 * n))
    shapes[f"group {N}x{HW}x{HW}x{Cc}, G {G}"] = dict(_time_group(launches, args.iters), kernel_form="one workgroup per (image, group)")
    return dict(batch=N, shapes=shapes, iters=args.iters, device=torch.cuda.get_device_name(0))


def step_network(args):
    import torch
    from bcos.models import convnext
    from bcos.modules import norms
    from bcos_hip import convnext_engine, lib, synth
    lib.load()
    B = args.batch
    setting = [(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)]
    centred = synth.build_bcos_convnext(setting, 1000, seed=0).to(DEV)
    torch.manual_seed(0)
    pnu = convnext.BcosConvNeXt([convnext.CNBlockConfig(*s) for s in setting], num_classes=1000,
                                norm_layer=norms.NoBias(norms.PositionNormUncentered2d))
    pnu = synth.seed_convnext(pnu, 0).eval().to(DEV)
    x = synth.synthetic_images(B, seed=1000, size=224).to(DEV)
    eng_c, eng_u = convnext_engine.ConvNeXtEngine(centred), convnext_engine.ConvNeXtEngine(pnu)
    variants = dict(pnu_forward=lambda: eng_u.forward(x), centred_forward=lambda: eng_c.forward(x),
                    pnu_explain=lambda: eng_u.explain(x), centred_explain=lambda: eng_c.explain(x))
    for fn in variants.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    # one kind at a time, the two plans in the order u c c u u c c u ...: each follows itself as often as the other (a pass's time depends
    # on what ran before it -- the allocator's state, the streams of the sub-batch scheduler -- by more than the two plans differ)
    for kind in ("forward", "explain"):
        for i in range(args.iters):
            for which in (("pnu", "centred") if i % 2 == 0 else ("centred", "pnu")):
                times[f"{which}_{kind}"].append(event_ms(variants[f"{which}_{kind}"]))
    network = {k: stats(v, B) for k, v in times.items()}
    for kind in ("forward", "explain"):
        u, c = times[f"pnu_{kind}"], times[f"centred_{kind}"]
        network[f"pnu_over_centred_{kind}_time"] = round(median(u) / median(c), 4)
        network[f"pnu_slower_{kind}_beyond_spread"] = bool(min(u) > max(c))
    return dict(batch=B, image=[224, 224], iters=args.iters, network=network, contraction=lib.get_contraction_mode(),
                device=torch.cuda.get_device_name(0))


def step_network_alone(args):
    """ONE plan in the process (args.norm), forward and forward + explanation: two plans in one process do not time as each does alone"""
    import torch
    from bcos.models import convnext
    from bcos.modules import norms
    from bcos_hip import convnext_engine, lib, synth
    lib.load()
    B = args.batch
    setting = [(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)]
    torch.manual_seed(0)
    kw = dict(norm_layer=norms.NoBias(norms.PositionNormUncentered2d)) if args.norm == "pnu" else {}
    net = convnext.BcosConvNeXt([convnext.CNBlockConfig(*s) for s in setting], num_classes=1000, **kw)
    net = synth.seed_convnext(net, 0).eval().to(DEV)
    x = synth.synthetic_images(B, seed=1000, size=224).to(DEV)
    eng = convnext_engine.ConvNeXtEngine(net)
    variants = dict(forward=lambda: eng.forward(x), explain=lambda: eng.explain(x))
    for fn in variants.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.iters):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    return dict(norm=args.norm, **{k: stats(v, B) for k, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "unorm_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--norm", choices=("pnu", "centred"), default="pnu", help="(internal) the plan of --step network_alone")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "unorm_bench.py needs a HIP device"
        print("RESULT " + json.dumps({"kernels": step_kernels, "network": step_network, "network_alone": step_network_alone}[args.step](args)))
        return
    out = dict(metric="uncentered position / group norm kernels against their centred twins and bcos_stream_copy; B-cos ConvNeXt-T on the fused "
                      "plan with uncentered and with centred position norms")
    alone = []
    for step, norm in (("kernels", None), ("network", None), ("network_alone", "pnu"), ("network_alone", "centred"), ("network_alone", "pnu"),
                       ("network_alone", "centred")):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--batch", str(args.batch), "--iters", str(args.iters)] + (["--norm", norm] if norm else [])
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"step `{step}` failed with exit status {res.returncode}: nothing further is started")
        rec = json.loads(lines[-1][len("RESULT "):])
        if norm:
            alone.append(rec)
        else:
            out[step] = rec
    out["network_one_plan_per_process"] = alone
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
