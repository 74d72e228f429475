"""Cost of adaptive gradient clipping on the device, one JSON line (needs a HIP device):

  clip      the clip alone on the parameter sets of ResNet-50, ViT-Ti and CLIP RN50 with seeded gradients (about half the units clip), timed
            with device events: the reference-form loop (bcos/training/agc.py:28-42 of the reference: two norms and eight elementwise launches
            per tensor, restated in torch below) against bcos_agc_clip -- as the whole adaptive_clip_grad_ call (hip_call_ms, host descriptor
            building included) and as the library call alone on a prebuilt descriptor array (hip_device_ms: the device time); achieved
            bytes/s = (p and g read once + the clipped units written) over hip_device_ms, against bcos_stream_copy of the same bytes measured in
            the same run; hip_host_issue_us = host time of one adaptive_clip_grad_ call
  recipe    the recipe step at batch 64 through the training plans (ResNet-50, ViT-Ti), three variants alternated in one process:
            (a) SGD-momentum, bench.py --train's update; (b) the reference-form clip + torch.optim.AdamW; (c) bcos_agc_clip + AdamW

python scripts/agc_bench.py [--steps 10] [--rounds 3] [--batch 64] [--skip-recipe]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "b-cosification_amd"), REPO]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bcos.modules.losses import UniformOffLabelsBCEWithLogitsLoss  # noqa: E402
from bcos.training.agc import adaptive_clip_grad_, unitwise_norm  # noqa: E402
from bcos_hip import lib, ops, synth  # noqa: E402

DEV = "cuda"


def reference_form_clip(parameters, clip_factor=0.01, eps=1e-3):
    """the reference's per-tensor eager loop (same launches: norms of p and g, clamp / mul of the bound, the clamped division, the product,
    the comparison, where, copy_)"""
    for p in parameters:
        if p.grad is None:
            continue
        g = p.grad.detach()
        bound = unitwise_norm(p.detach()).clamp_(min=eps).mul_(clip_factor)
        gn = unitwise_norm(g)
        p.grad.detach().copy_(torch.where(gn < bound, g, g * (bound / gn.clamp(min=1e-6))))


def build(arch):
    if arch == "vit_ti":
        return synth.build_bcosified_vit(seed=0).to(DEV)
    if arch == "clip_rn50":
        return synth.build_bcosified_clip_rn50(seed=0).to(DEV)
    return synth.build_bcosified_resnet(arch, seed=0).to(DEV)


def seeded_grads(params, seed=7):
    """gradients whose unit norms lie within a factor 10^(+-1/2) of each unit's threshold: about half the units clip"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for p in params:
        units, unit_len = ops.agc_units(p.shape)
        g = torch.randn(units, unit_len, device=DEV, generator=gen)
        target = p.detach().reshape(units, unit_len).norm(dim=1).clamp(min=1e-3) * 0.01
        target = target * 10.0 ** (torch.rand(units, device=DEV, generator=gen) - 0.5)
        out.append((g * (target / g.norm(dim=1))[:, None]).reshape(p.shape))
    return out


def timed(fn, restore, iters):
    """device time of fn() per call in ms (median over iters); restore() runs before each call, outside the events"""
    ts = []
    for _ in range(iters):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def clip_alone(arch, iters):
    net = build(arch)
    params = [p for p in net.parameters() if p.requires_grad]
    grads = seeded_grads(params)
    # the gradients as 16-byte aligned slices of ONE buffer, restored before every timed call by one streaming copy from a snapshot
    offs, total = [], 0
    for g in grads:
        offs.append(total)
        total += (g.numel() + 3) // 4 * 4
    flat, snap = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV)
    cur = [flat[o:o + g.numel()].view(g.shape) for o, g in zip(offs, grads)]
    for p, c, g in zip(params, cur, grads):
        c.copy_(g)
        p.grad = c
    snap.copy_(flat)

    def restore():
        ops.stream_copy(snap, flat)
    restore()
    adaptive_clip_grad_(params)
    torch.cuda.synchronize()
    clipped_elems = sum(int((~torch.all(c.reshape(ops.agc_units(c.shape)) == g.reshape(ops.agc_units(g.shape)), dim=1)).sum())
                        * ops.agc_units(c.shape)[1] for c, g in zip(cur, grads))
    n = sum(p.numel() for p in params)
    units = sum(ops.agc_units(p.shape)[0] for p in params)
    traffic = 4 * (2 * n + clipped_elems)
    for fn in (lambda: adaptive_clip_grad_(params), lambda: reference_form_clip(params)):     # warm-up
        for _ in range(3):
            restore()
            fn()
    # hip_call_ms: the whole adaptive_clip_grad_ call.  Its ~0.1-0.2 ms of Python descriptor building outlasts the restore copy queued ahead of
    # it (ResNet-50: ~40 us), so the device idles inside the events for part of it: a CALL time, not a device time
    hip_ms, hip_min = timed(lambda: adaptive_clip_grad_(params), restore, iters)
    ref_ms, ref_min = timed(lambda: reference_form_clip(params), restore, iters)
    # hip_device_ms, the figure held to the issue's 0.15 ms target: the same library call with its descriptor array built once -- one ctypes
    # call issued while the restore copy still runs, so the events bracket the two launches (the kernel trace of the clip agrees: DESIGN §8)
    arr = (lib.AgcTensor * len(params))(*[(p.data_ptr(), p.grad.data_ptr()) + ops.agc_units(p.shape) for p in params])
    handle = lib.load()
    dev_ms, dev_min = timed(lambda: lib.check(handle.bcos_agc_clip(arr, len(params), 0.01, 1e-3, ops._stream()), "bcos_agc_clip"), restore, iters)
    src = torch.empty((2 * n + 3) // 4 * 4, device=DEV)            # (bcos_stream_copy: a multiple of 4 floats)
    dst = torch.empty_like(src)
    for _ in range(3):
        ops.stream_copy(src, dst)
    copy_ms, _ = timed(lambda: ops.stream_copy(src, dst), lambda: None, iters)
    copy_bps = 2 * 4 * src.numel() / (copy_ms * 1e-3)                     # read + write of the p and g bytes
    host = time.perf_counter()
    for _ in range(20):
        adaptive_clip_grad_(params)
    host_us = (time.perf_counter() - host) / 20 * 1e6
    torch.cuda.synchronize()
    del net, src, dst, flat, snap
    return dict(tensors=len(params), parameters=n, units=units, clipped_units_elems=clipped_elems, launches=(len(params) + 63) // 64,
                algorithmic_mb=round(traffic / 1e6, 1), hip_call_ms=round(hip_ms, 4), hip_call_min_ms=round(hip_min, 4),
                hip_device_ms=round(dev_ms, 4), hip_device_min_ms=round(dev_min, 4), reference_form_ms=round(ref_ms, 4),
                reference_form_min_ms=round(ref_min, 4), speedup_call=round(ref_ms / hip_ms, 1), hip_device_tbps=round(traffic / (dev_ms * 1e-3) / 1e12, 3),
                stream_copy_tbps=round(copy_bps / 1e12, 3), frac_of_stream_copy=round(traffic / (dev_ms * 1e-3) / copy_bps, 3),
                hip_host_issue_us=round(host_us, 1))


def recipe(arch, batch, steps, rounds):
    from bcos_hip import engine, vit_engine
    net = build(arch)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    (vit_engine if arch == "vit_ti" else engine).attach(net)
    net.train()
    x = synth.synthetic_images(batch, seed=1000).to(DEV)
    labels = torch.randint(0, 1000, (batch,), generator=torch.Generator().manual_seed(0)).to(DEV)
    target = F.one_hot(labels, 1000).float()
    params = [p for p in net.parameters() if p.requires_grad]
    sgd = torch.optim.SGD(params, lr=1e-4, momentum=0.9)
    adam_b = torch.optim.AdamW([{"params": params, "weight_decay": 0}], lr=1e-4)
    adam_c = torch.optim.AdamW([{"params": params, "weight_decay": 0}], lr=1e-4)
    crit = UniformOffLabelsBCEWithLogitsLoss()

    def step_a():
        sgd.zero_grad(set_to_none=True)
        F.binary_cross_entropy_with_logits(net(x), target).backward()
        sgd.step()

    def step_b():
        adam_b.zero_grad(set_to_none=True)
        crit(net(x), labels).backward()
        reference_form_clip(params)
        adam_b.step()

    def step_c():
        adam_c.zero_grad(set_to_none=True)
        crit(net(x), labels).backward()
        adaptive_clip_grad_(params)
        adam_c.step()

    variants = dict(a_sgd_momentum=step_a, b_reference_agc_adamw=step_b, c_hip_agc_adamw=step_c)
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps)
    res = {}
    for name, ts in times.items():
        ts.sort()
        res[name] = dict(ms_per_step=round(1e3 * ts[len(ts) // 2], 3), images_per_s=round(batch / ts[len(ts) // 2], 1),
                         spread_ms=[round(1e3 * ts[0], 3), round(1e3 * ts[-1], 3)])
    a = res["a_sgd_momentum"]["images_per_s"]
    res["b_over_a"] = round(res["b_reference_agc_adamw"]["images_per_s"] / a, 4)
    res["c_over_a"] = round(res["c_hip_agc_adamw"]["images_per_s"] / a, 4)
    res["plan"] = getattr(getattr(net, "_bcos_engine", None), "_train_plan", None) not in (None, False)
    del net
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-recipe", action="store_true")
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "agc_bench.py needs a HIP device"
    out = dict(metric="adaptive gradient clipping: the clip alone (device events) and the recipe step (images/s)", clip={}, recipe={})
    for arch in ("resnet50", "vit_ti", "clip_rn50"):
        out["clip"][arch] = clip_alone(arch, args.iters)
        torch.cuda.empty_cache()
    if not args.skip_recipe:
        for arch in ("resnet50", "vit_ti"):
            out["recipe"][arch] = dict(batch=args.batch, steps=args.steps, rounds=args.rounds, **recipe(arch, args.batch, args.steps, args.rounds))
            torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
