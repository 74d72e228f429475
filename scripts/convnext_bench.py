"""The depthwise 7x7 B-cos kernels and the native B-cos ConvNeXt-T, one JSON line (DESIGN: "ConvNeXt"; needs a HIP device):

  kernels   bcos_dwconv7_fwd, the same keeping its scale, and bcos_dwconv7_bwd (with `mul` and `addend`, as the plan calls it) at the four
            ConvNeXt-T stages, batch 64: C x H^2 = 96 x 56^2, 192 x 28^2, 384 x 14^2, 768 x 7^2.  Each beside bcos_stream_copy moving the same
            algorithmic bytes (the tensors the launch must read and write, once each) in the same run, and beside the fp32 vector bound:
            49 (backward) or 98 (forward: lin and the patch norm) FMAs per output element at 128 FMA / clock / CU, 256 CUs, at the clock the
            device reports while the script runs.  Ratios and which bound is nearer; no target.
  network   ConvNeXt-T at 224^2, batch 64: forward and forward + explanation in images/s for (a) the fused plan
            (bcos_hip.convnext_engine), (b) the module path, (c) the same algorithm in eager PyTorch operators, restated below; the three
            alternated in one process, medians after a warm-up, device events.  Outputs of (a) and (c) are compared on the timed inputs.

Each of the two steps runs in a child process of its own under a time limit; a step that fails ends the script.

python scripts/convnext_bench.py [--batch 64] [--iters 20] [--out FILE]     (writes profiles/convnext_bench.json unless told otherwise)
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
CUS, FMA_PER_CLK_CU = 256, 128
STEP_LIMIT_S = {"kernels": 240, "network": 420}


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


def clock_mhz():
    """(MHz, source): the engine clock the device reports now, or the device properties' maximum where it reports none"""
    import torch
    try:
        return float(torch.cuda.clock_rate()), "torch.cuda.clock_rate() while the kernels ran"
    except Exception:      # noqa: BLE001  (no management library in this image)
        return torch.cuda.get_device_properties(0).clock_rate / 1e3, "device properties (maximum engine clock): not measured under load"


def step_kernels(args):
    import torch
    from bcos_hip import lib, ops
    lib.load()
    N = args.batch
    shapes = {}
    clocks = []
    for Cc, HW in STAGES:
        g = torch.Generator().manual_seed(Cc)
        mk = lambda: torch.randn(N, HW, HW, Cc, generator=g).to(DEV)      # noqa: E731
        x, gy, mul, addend, y, gx = mk(), mk(), mk().abs(), mk(), mk(), mk()
        w = torch.randn(7, 7, Cc, generator=g)
        w = (w / w.flatten(0, 1).norm(dim=0)).to(DEV)
        n = x.numel()
        scale = torch.empty_like(x)

        def fwd_keep():         # (through the C ABI: the scale goes into a buffer made once, as the copies' buffers are)
            lib.check(lib.load().bcos_dwconv7_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), None, N, HW, HW, Cc, 2.0,
                                                  ops._stream()), "bcos_dwconv7_fwd")
        launches = (("forward", lambda: ops.dwconv7_fwd(x, w, out=y), 2 * n, 98),
                    ("forward_keep_scale", fwd_keep, 3 * n, 98),
                    ("backward", lambda: ops.dwconv7_bwd(gy, w, mul=mul, addend=addend, out=gx), 4 * n, 49))
        copies = {f: (torch.empty(f // 2, device=DEV), torch.empty(f // 2, device=DEV)) for f in {l[2] for l in launches}}
        fns = {}
        for label, fn, floats, _ in launches:
            fns[label] = fn
            src, dst = copies[floats]
            fns[label + "/copy"] = (lambda s=src, d=dst: ops.stream_copy(s, d))
        for fn in fns.values():
            for _ in range(3):
                fn()
        times = {k: [] for k in fns}
        for _ in range(args.iters):                 # alternated: a launch, then the copy of its bytes
            for k, fn in fns.items():
                times[k].append(event_ms(fn))
        mhz, src_clock = clock_mhz()
        clocks.append(mhz)
        rec = {}
        for label, _, floats, fma in launches:
            t, c = median(times[label]), median(times[label + "/copy"])
            valu_ms = n * fma / (CUS * FMA_PER_CLK_CU * mhz * 1e6) * 1e3
            rec[label] = dict(stats(times[label]), algorithmic_bytes=4 * floats, gb_per_s=round(4 * floats / (t * 1e-3) / 1e9, 1),
                              stream_copy_same_bytes=stats(times[label + "/copy"]), time_over_stream_copy=round(t / c, 3),
                              fp32_vector_bound_ms=round(valu_ms, 4), time_over_vector_bound=round(t / valu_ms, 3),
                              nearer_bound="hbm (stream copy)" if c >= valu_ms else "fp32 vector")
        shapes[f"{Cc}x{HW}x{HW}"] = rec
        del x, gy, mul, addend, y, gx, scale, copies
    return dict(batch=N, shapes=shapes, clock_mhz=clocks, clock_source=src_clock, iters=args.iters,
                vector_peak="128 FMA / clock / CU x 256 CUs")


# ---- (c): the same algorithm in eager PyTorch operators ---------------------------------------------------------------------------
def eager_plan(net):
    import torch
    import torch.nn.functional as F

    def unit(w):
        return (w / w.flatten(1).norm(dim=1).view(-1, 1, 1, 1)).detach()

    def conv(x, w, stride=1, padding=0, groups=1):
        lin = F.conv2d(x, w, stride=stride, padding=padding, groups=groups)
        sq = x * x if groups > 1 else (x * x).sum(1, keepdim=True)
        k = w.shape[2]
        norm = (F.avg_pool2d(sq, k, stride=stride, padding=padding, divisor_override=1) + 1e-6).sqrt()
        return lin * (lin.abs() / norm).detach()

    def pn(x, weight):
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True).detach()
        return weight.view(1, -1, 1, 1) * (x - mean) / (var + 1e-6).sqrt()

    sd = {k: v.detach() for k, v in net.state_dict().items()}
    W = {k: unit(v) for k, v in sd.items() if k.endswith("linear.weight")}
    feats = net.features
    bias = net.logit_layer.logit_bias

    def forward(x):
        x = pn(conv(x, W["features.0.linear.weight"], stride=4), sd["features.1.weight"])
        for k in range(2, len(feats)):
            if hasattr(feats[k][0], "block"):
                for j in range(len(feats[k])):
                    p = f"features.{k}.{j}."
                    C_ = x.shape[1]
                    h = conv(x, W[p + "block.0.linear.weight"], padding=3, groups=C_)
                    h = pn(h, sd[p + "block.1.weight"])
                    h = conv(conv(h, W[p + "block.2.linear.weight"]), W[p + "block.3.linear.weight"])
                    x = x + sd[p + "layer_scale"] * h
            else:
                x = conv(pn(x, sd[f"features.{k}.0.weight"]), W[f"features.{k}.1.linear.weight"], stride=2)
        x = conv(pn(x, sd["classifier.0.weight"]), W["classifier.1.linear.weight"])
        return x.mean((2, 3)) + bias

    def explain(x):
        x = x.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            logits = forward(x)
            (g,) = torch.autograd.grad(logits.max(1).values.sum(), x)
        return dict(logits=logits.detach(), dynamic_linear_weights=g, contribution_map=(x.detach() * g).sum(1))

    def forward_ng(x):
        with torch.no_grad():
            return forward(x)
    return forward_ng, explain


def step_network(args):
    import torch
    from bcos_hip import convnext_engine, lib, synth
    lib.load()
    B = args.batch
    net = synth.build_bcos_convnext([(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)], 1000, seed=0).to(DEV)
    x = synth.synthetic_images(B, seed=1000, size=224).to(DEV)
    eng = convnext_engine.ConvNeXtEngine(net)
    eager_fwd, eager_explain = eager_plan(net)

    def module_forward():
        with torch.no_grad():
            return net(x)
    variants = dict(plan_forward=lambda: eng.forward(x), module_forward=module_forward, eager_forward=lambda: eager_fwd(x),
                    plan_explain=lambda: eng.explain(x), module_explain=lambda: net.explain_batch(x), eager_explain=lambda: eager_explain(x))
    # (a) against (c) on the timed inputs, at the parity tolerances of tests/test_convnext_gpu.py
    a, c = variants["plan_explain"](), variants["eager_explain"]()

    def per_image(u, v):
        u, v = u.double().flatten(1), v.double().flatten(1)
        return float(((u - v).abs().amax(1) / v.abs().amax(1)).max())
    agree = dict(logits_max_abs=float((a["logits"] - c["logits"]).abs().max()),
                 classes_equal=bool(torch.equal(a["logits"].argmax(1), c["logits"].argmax(1))),
                 weights_per_image=per_image(a["dynamic_linear_weights"], c["dynamic_linear_weights"]),
                 maps_per_image=per_image(a["contribution_map"], c["contribution_map"]), tolerance=1e-4)
    agree["within_tolerance"] = bool(max(agree["logits_max_abs"], agree["weights_per_image"], agree["maps_per_image"]) <= 1e-4
                                     and agree["classes_equal"])
    del a, c
    for fn in variants.values():
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.iters):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    network = {k: stats(v, B) for k, v in times.items()}
    for kind in ("forward", "explain"):
        p, m, e = (times[f"{v}_{kind}"] for v in ("plan", "module", "eager"))
        network[f"plan_over_module_{kind}_time"] = round(median(p) / median(m), 4)
        network[f"plan_over_eager_{kind}_time"] = round(median(p) / median(e), 4)
        # required: (a) >= (b) and (a) > (c) by more than the spread of the alternated medians -- the plan's slowest against the others' fastest
        network[f"plan_not_slower_than_module_{kind}"] = bool(median(p) <= median(m))
        network[f"plan_faster_than_eager_{kind}_beyond_spread"] = bool(max(p) < min(e))
    return dict(batch=B, image=[224, 224], iters=args.iters, agreement_plan_vs_eager=agree, network=network,
                contraction=lib.get_contraction_mode(), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convnext_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "convnext_bench.py needs a HIP device"
        print("RESULT " + json.dumps({"kernels": step_kernels, "network": step_network}[args.step](args)))
        return
    out = dict(metric="depthwise 7x7 B-cos kernels against bcos_stream_copy and the fp32 vector bound; B-cos ConvNeXt-T on the fused plan, the "
                      "module path and eager PyTorch operators")
    for step in ("kernels", "network"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--batch", str(args.batch), "--iters", str(args.iters)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"step `{step}` failed with exit status {res.returncode}: nothing further is started")
        out[step] = json.loads(lines[-1][len("RESULT "):])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
