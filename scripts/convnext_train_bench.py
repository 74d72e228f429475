"""The training-mode gradients of the depthwise 7x7 B-cos convolution and one training step of the native B-cos ConvNeXt-T, one JSON line
(DESIGN: "ConvNeXt"; needs a HIP device; not run by the tests):

  kernels   bcos_dwconv7_train_bwd (with an addend), bcos_dwconv7_wgrad (mul = scale, gain = 2: both launches) and the forward launch a
            training step makes (scale and norm kept) at the four ConvNeXt-T stages, batch 64: C x H^2 = 96 x 56^2, 192 x 28^2, 384 x 14^2,
            768 x 7^2.  Each beside bcos_stream_copy moving the same algorithmic bytes (the tensors the launch must read and write, once
            each) in the same run, alternated, and beside the fp32 vector bound (49 FMAs + 49 additions per element for the input
            gradient, 49 FMAs for the weight gradient, 98 FMAs for the forward, at 128 lanes / clock / CU, 256 CUs, at the clock the device
            reports while the script runs).  Beside them PyTorch-ROCm eager autograd of the same expressions, written below: the backward
            of y = lin |lin| / sqrt(box7(x^2) + 1e-6), lin = F.conv2d(x, w, padding=3, groups=C), for x and w together (channels_last).
  step      ConvNeXt-T at 224^2, batch 64: forward + backward of a BCE loss through the module path (net.train(); one autograd node per
            layer), device events, median.  The share of the depthwise launches is the sum over the 18 blocks of the three standalone
            medians above over the step's median: arithmetic on separately timed launches, not a trace (no trace is taken here).

Each of the two steps runs in a child process of its own under a time limit; a step that fails ends the script.

python scripts/convnext_train_bench.py [--batch 64] [--iters 20] [--out FILE]     (writes profiles/convnext_train_bench.json unless told otherwise)
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
BLOCKS = (3, 3, 9, 3)
CUS, LANES_PER_CLK_CU = 256, 128
STEP_LIMIT_S = {"kernels": 300, "step": 420}


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


def stats(ts):
    return dict(device_ms=round(median(ts), 4), spread_ms=[round(min(ts), 4), round(max(ts), 4)])


def clock_mhz():
    """(MHz, source): the engine clock the device reports now, or the device properties' maximum where it reports none"""
    import torch
    try:
        return float(torch.cuda.clock_rate()), "torch.cuda.clock_rate() while the kernels ran"
    except Exception:      # noqa: BLE001  (no management library in this image)
        return torch.cuda.get_device_properties(0).clock_rate / 1e3, "device properties (maximum engine clock): not measured under load"


def step_kernels(args):
    import torch
    import torch.nn.functional as F
    from bcos_hip import lib, ops
    lib.load()
    N = args.batch
    shapes = {}
    clocks = []
    for Cc, HW in STAGES:
        g = torch.Generator().manual_seed(Cc)
        mk = lambda: torch.randn(N, HW, HW, Cc, generator=g).to(DEV)      # noqa: E731
        x, gy, addend, gx = mk(), mk(), mk(), mk()
        w = torch.randn(7, 7, Cc, generator=g)
        w = (w / w.flatten(0, 1).norm(dim=0)).to(DEV)
        n = x.numel()
        y, scale, norm = ops.dwconv7_fwd(x, w, want_scale=True, want_norm=True)
        gw = torch.empty(7, 7, Cc, device=DEV)

        def fwd_keep():         # (through the C ABI: the outputs go into buffers made once, as the copies' buffers are)
            lib.check(lib.load().bcos_dwconv7_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), norm.data_ptr(), N, HW, HW, Cc,
                                                  2.0, ops._stream()), "bcos_dwconv7_fwd")
        # eager autograd of the same expressions: the graph is built outside the timed region, the backward is what is timed
        xe = x.permute(0, 3, 1, 2).detach().requires_grad_(True)             # logical NCHW, channels_last strides
        we = w.permute(2, 0, 1).unsqueeze(1).contiguous().requires_grad_(True)
        ge = gy.permute(0, 3, 1, 2)
        graph = {}

        def eager_build():
            lin = F.conv2d(xe, we, padding=3, groups=Cc)
            nrm = (F.avg_pool2d(xe * xe, 7, stride=1, padding=3, divisor_override=1) + 1e-6).sqrt()
            graph["y"] = lin * lin.abs() / nrm

        def eager_backward():
            torch.autograd.grad(graph["y"], (xe, we), ge)
        launches = (("forward_keep_scale_norm", fwd_keep, 4 * n, 98),
                    ("train_bwd", lambda: ops.dwconv7_train_bwd(gy, x, y, scale, norm, w, addend=addend, out=gx), 7 * n, 98),
                    ("wgrad", lambda: ops.dwconv7_wgrad(gy, x, mul=scale, gain=2.0, out=gw), 3 * n, 49))
        copies = {f: (torch.empty(f // 2, device=DEV), torch.empty(f // 2, device=DEV)) for f in {l[2] for l in launches}}
        fns = {}
        for label, fn, floats, _ in launches:
            fns[label] = fn
            src, dst = copies[floats]
            fns[label + "/copy"] = (lambda s=src, d=dst: ops.stream_copy(s, d))
        for fn in fns.values():
            for _ in range(3):
                fn()
        for _ in range(2):
            eager_build()
            eager_backward()
        times = {k: [] for k in fns}
        times["eager_backward"] = []
        for _ in range(args.iters):                 # alternated: a launch, then the copy of its bytes; then eager's backward
            for k, fn in fns.items():
                times[k].append(event_ms(fn))
            eager_build()
            torch.cuda.synchronize()
            times["eager_backward"].append(event_ms(eager_backward))
        mhz, src_clock = clock_mhz()
        clocks.append(mhz)
        rec = {}
        for label, _, floats, vops in launches:
            t, c = median(times[label]), median(times[label + "/copy"])
            valu_ms = n * vops / (CUS * LANES_PER_CLK_CU * mhz * 1e6) * 1e3
            rec[label] = dict(stats(times[label]), algorithmic_bytes=4 * floats, gb_per_s=round(4 * floats / (t * 1e-3) / 1e9, 1),
                              stream_copy_same_bytes=stats(times[label + "/copy"]), time_over_stream_copy=round(t / c, 3),
                              fp32_vector_bound_ms=round(valu_ms, 4), time_over_vector_bound=round(t / valu_ms, 3),
                              nearer_bound="hbm (stream copy)" if c >= valu_ms else "fp32 vector")
        ours = median(times["train_bwd"]) + median(times["wgrad"])
        rec["eager_backward_gx_and_gw"] = dict(stats(times["eager_backward"]),
                                               native_train_bwd_plus_wgrad_ms=round(ours, 4),
                                               native_over_eager_time=round(ours / median(times["eager_backward"]), 4))
        shapes[f"{Cc}x{HW}x{HW}"] = rec
        del x, gy, addend, gx, y, scale, norm, copies, xe, graph
    return dict(batch=N, shapes=shapes, clock_mhz=clocks, clock_source=src_clock, iters=args.iters,
                vector_peak="128 lanes / clock / CU x 256 CUs", trace="not measured")


def step_train(args):
    import torch
    import torch.nn.functional as F
    from bcos_hip import lib, synth
    lib.load()
    B = args.batch
    net = synth.build_bcos_convnext([(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)], 1000, seed=0).to(DEV).train()
    x = synth.synthetic_images(B, seed=1000, size=224).to(DEV)
    target = F.one_hot(torch.arange(B) % 1000, 1000).float().to(DEV)
    params = [p for p in net.parameters() if p.requires_grad]

    def step():
        loss = F.binary_cross_entropy_with_logits(net(x), target)
        return torch.autograd.grad(loss, params)
    grads = step()
    finite = all(bool(torch.isfinite(g).all()) for g in grads)
    nodes = type(net.features[2][0].block[0](torch.zeros(1, 96, 8, 8, device=DEV, requires_grad=True)).grad_fn).__name__
    del grads
    step()
    ts = [event_ms(step) for _ in range(max(3, args.iters // 2))]
    return dict(batch=B, image=[224, 224], iters=len(ts), forward_backward=dict(stats(ts), images_per_s=round(B / (median(ts) * 1e-3), 1)),
                gradients_finite=finite, depthwise_autograd_node=nodes, contraction=lib.get_contraction_mode(),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "convnext_train_bench.json"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "convnext_train_bench.py needs a HIP device"
        print("RESULT " + json.dumps({"kernels": step_kernels, "step": step_train}[args.step](args)))
        return
    out = dict(metric="depthwise 7x7 B-cos training-mode gradients against bcos_stream_copy, the fp32 vector bound and eager autograd; one "
                      "B-cos ConvNeXt-T training step (forward + backward) on the module path")
    for step in ("kernels", "step"):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--batch", str(args.batch), "--iters", str(args.iters)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
        if res.returncode != 0 or not lines:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"step `{step}` failed with exit status {res.returncode}: nothing further is started")
        out[step] = json.loads(lines[-1][len("RESULT "):])
    # the depthwise launches' share of the step: standalone medians x blocks per stage (not a trace)
    per_stage = []
    for (Cc, HW), blocks in zip(STAGES, BLOCKS):
        rec = out["kernels"]["shapes"][f"{Cc}x{HW}x{HW}"]
        per_stage.append(blocks * sum(rec[k]["device_ms"] for k in ("forward_keep_scale_norm", "train_bwd", "wgrad")))
    step_ms = out["step"]["forward_backward"]["device_ms"]
    out["depthwise_share_of_step"] = dict(depthwise_ms=round(sum(per_stage), 3), per_stage_ms=[round(v, 3) for v in per_stage],
                                          step_ms=step_ms, share=round(sum(per_stage) / step_ms, 4),
                                          method="sum over the 18 blocks of the standalone medians (forward keeping scale and norm, input "
                                                 "gradient, weight gradient) over the step's median; trace: not measured")
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
