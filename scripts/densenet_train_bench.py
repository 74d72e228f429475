"""One training step of the B-cosified DenseNet-121 through the fused plan against the per-layer path, one JSON line (DESIGN §3.5.1;
needs a HIP device):

  step      DenseNet-121, 224 x 224, batch 64: forward in train() mode, BCE with logits, backward to every parameter.  `plan`: the
            network with a DenseNetEngine attached (bcos_hip.densenet_train_plan: one autograd node); `layers`: the same weights with
            no engine attached -- one autograd node per module, torch.cat in front of every dense layer, which is how a DenseNet
            trained before the plan existed.  The two are alternated in one process and timed with device events after a warm-up,
            --steps steps per timed window; medians.  The gradients of the two paths are compared before anything is timed and the
            parameters they differ most on are named with their gradient norms.  No number is asserted anywhere.
  yardstick --yardstick FILE [FILE ...] (one per batch size; written by tests/golden/make_densenet121_train_yardstick.py from the reference's float64 step at the
            same depth, small batch): both fp32 paths start from the file's weights and run its step; the distance of EACH path's
            parameter gradients from the float64 ones, and of the per-layer path under f32 products (`layers_f32`, the arithmetic of the
            plan's contractions) -- two fp32 evaluations of 120 layers of ReLU gates differ from each other by
            more than either differs from the truth only if one of them is wrong.
  launches  the four training-mode dense-block kernels alone on a [M, 512] slice of a [M, 1024] buffer, each beside bcos_stream_copy of
            the bytes the launch moves.  Ratios only.

python scripts/densenet_train_bench.py [--batch 64] [--rounds 7] [--steps 5] [--iters 20] [--yardstick FILE ...] [--out FILE]   (writes profiles/densenet_train_bench.json unless told otherwise)
"""
import argparse
import contextlib
import copy
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402

from bcos_hip import densenet_engine, densenet_train_plan, lib, ops, synth  # noqa: E402

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


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def worst_named(names, dists, norms, k=3):
    order = sorted(range(len(names)), key=lambda i: -dists[i])[:k]
    return [dict(name=names[i], rel_l2=dists[i], grad_norm=norms[i]) for i in order]


def against_yardstick(path, base):
    """both paths' step from the yardstick's weights on its batch against its float64 gradients"""
    import numpy as np
    data = np.load(path)
    B = int(data["batch"])
    state = {k[6:]: torch.from_numpy(data[k]) for k in data.files if k.startswith("state/")}
    x = synth.synthetic_images(B, seed=1000, size=224).to(DEV)
    target = torch.nn.functional.one_hot(torch.arange(B, device=DEV) * 37 % 1000, 1000).float()
    out = dict(batch=B, output_rel_l2={}, grads={})
    grads = {}
    for which in ("plan", "layers", "layers_f32"):
        net = copy.deepcopy(base)
        net.load_state_dict(state)
        net.eval()
        if which == "plan":
            densenet_engine.attach(net)
        net.train()
        named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
        # (`layers_f32`: the per-layer path with the arithmetic the plan's contractions use -- the same path under another rounding,
        #  which shows how far two correct fp32 evaluations of this step are from each other and from float64)
        with (ops.contraction_override("f32") if which == "layers_f32" else contextlib.nullcontext()):
            res = net(x)
            assert (type(res.grad_fn).__name__ == "_TrainStepFnBackward") == (which == "plan")
            gs = torch.autograd.grad(torch.nn.functional.binary_cross_entropy_with_logits(res, target), [p for _, p in named])
        names = [n for n, _ in named]
        ref = [torch.from_numpy(data["grad/" + n]).to(DEV) for n in names]
        dists = [rel(g, r) for g, r in zip(gs, ref)]
        num = sum(float((g.double() - r.double()).pow(2).sum()) for g, r in zip(gs, ref))
        den = sum(float(r.double().pow(2).sum()) for r in ref)
        out["output_rel_l2"][which] = rel(res.detach(), torch.from_numpy(data["output"]).to(DEV))
        out["grads"][which] = dict(all_parameters_rel_l2=(num / den) ** 0.5, median_rel_l2=median(dists),
                                   worst=worst_named(names, dists, [float(v) for v in data["grad_norms"]]))
        grads[which] = (names, gs, dists)
    (names, gp, dp), (_, gl, dl) = grads["plan"], grads["layers"]
    out["plan_vs_layers_f32"] = dict(median_rel_l2=median([rel(a, b) for a, b in zip(gp, grads["layers_f32"][1])]),
                                     parameters_where_plan_is_further_from_fp64=sum(a > b for a, b in zip(dp, grads["layers_f32"][2])))
    out["plan_vs_layers"] = dict(median_rel_l2=median([rel(a, b) for a, b in zip(gp, gl)]),
                                 parameters_where_plan_is_further_from_fp64=sum(a > b for a, b in zip(dp, dl)), parameters=len(names))
    out["median_grad_norm_fp64"] = median([float(v) for v in data["grad_norms"]])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed window")
    ap.add_argument("--yardstick", nargs="*", default=[], help="one file per batch size")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "densenet_train_bench.json"))
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "densenet_train_bench.py needs a HIP device"
    base = synth.build_bcosified_densenet(seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(base, synth.synthetic_images(8, seed=123, size=args.size).to(DEV))
    base.eval()
    yard = [against_yardstick(f, base) for f in args.yardstick] or None
    nets = dict(plan=base, layers=copy.deepcopy(base))
    densenet_engine.attach(nets["plan"])
    B = args.batch
    x = synth.synthetic_images(B, seed=1000, size=args.size).to(DEV)
    target = torch.nn.functional.one_hot(torch.arange(B, device=DEV) * 37 % 1000, 1000).float()
    for n in nets.values():
        n.train()
    params = {k: [p for p in n.parameters() if p.requires_grad] for k, n in nets.items()}

    def step(which):
        out = nets[which](x)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(out, target)
        return out, torch.autograd.grad(loss, params[which])

    # same step before anything is timed (each path moves its own copy of the running statistics)
    (op, gp), (ol, gl) = step("plan"), step("layers")
    assert type(op.grad_fn).__name__ == "_TrainStepFnBackward" and type(ol.grad_fn).__name__ != "_TrainStepFnBackward"
    names = [n for n, p in nets["plan"].named_parameters() if p.requires_grad]
    dists = [rel(a, b) for a, b in zip(gp, gl)]
    agree = dict(logits_rel_l2=rel(op.detach(), ol.detach()), grad_rel_l2_median=median(dists),
                 worst=worst_named(names, dists, [float(b.double().norm()) for b in gl], k=5),
                 median_grad_norm=median([float(b.double().norm()) for b in gl]))
    del op, gp, ol, gl

    def window(which):
        for _ in range(args.steps):
            step(which)
    variants = dict(plan=lambda: window("plan"), layers=lambda: window("layers"))
    for fn in variants.values():                                          # warm-up: weight images, workspaces, the allocator's pools
        fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(event_ms(fn))
    network = {k: stats(v, B * args.steps) for k, v in times.items()}
    for k in times:
        network[k]["step_ms"] = round(median(times[k]) / args.steps, 4)
    network["steps_per_window"] = args.steps
    network["plan_over_layers_step_time"] = round(median(times["plan"]) / median(times["layers"]), 4)
    del variants, nets, params
    torch.cuda.empty_cache()

    # the four launches alone, beside the library's streaming copy of as many bytes
    M, C, pitch = B * 14 * 14, 512, 1024
    X = torch.randn(M, pitch, device=DEV)
    G = torch.randn(M, pitch, device=DEV)
    d = torch.randn(M, C, device=DEV)
    g, sh = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV) * 0.1
    mean, var, rv = torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.ones(C, device=DEV)
    ops.slice_batch_stats(X[:, :C], mean, var)
    rstd, _ = ops.bn_reader_finish(var, g, 1e-5)
    coef = ops.slice_relu_bwd_colsums(d, X[:, :C], g, sh, rstd=rstd, want_coef=True)[3]

    def timed(fn):
        for _ in range(3):
            fn()
        return [event_ms(fn) for _ in range(args.iters)]
    launches = {}
    for label, fn, floats in (("slice_batch_stats", lambda: ops.slice_batch_stats(X[:, :C], mean, var), M * C),
                              ("bn_reader_finish", lambda: ops.bn_reader_finish(var, g, 1e-5, running_var=rv, momentum=0.1), 6 * C),
                              ("slice_relu_bwd_colsums", lambda: ops.slice_relu_bwd_colsums(d, X[:, :C], g, sh, rstd=rstd, want_sg=True, want_gw=True,
                                                                                            want_coef=True), 2 * M * C),
                              ("slice_bn_bwd_acc", lambda: ops.slice_bn_bwd_acc(d, G[:, :C], X[:, :C], g, sh, mean, coef), 4 * M * C)):
        src = torch.empty(max(floats // 2, 4), device=DEV)             # a copy moves its bytes twice: read + write
        dst = torch.empty_like(src)
        ts, cs = timed(fn), timed(lambda: ops.stream_copy(src, dst))
        launches[label] = dict(stats(ts), bytes_moved=4 * floats, stream_copy_same_bytes=stats(cs),
                               time_over_stream_copy=round(median(ts) / median(cs), 3))
        del src, dst
    out = dict(metric="B-cosified DenseNet-121, one training step (forward, BCE, backward): the fused plan against the per-layer path with no "
                      "engine attached, and the four training-mode dense-block launches against bcos_stream_copy of the bytes they move",
               batch=B, image=[args.size, args.size], rounds=args.rounds, agreement=agree, yardstick_fp64=yard, network=network, launches=launches,
               contraction=lib.get_contraction_mode(), plan_contraction=densenet_train_plan.DenseNetTrainPlan.CONTRACTION, device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
