"""Cost of the SigLIP distillation loss on the device, one JSON line, also written to profiles/siglip_bench.json (needs a
HIP device):

  loss      loss + backward alone at the recipe's shapes (N = 64, D = 1024, L = 1 and L = 49 with cos_power 2): the fused op
            (bcos_hip.clip_head.distill_loss: one bcos_siglip_loss call, the student's gradient wanted, the teacher frozen) against the
            torch-operator form on the same device (two F.normalize, matmul, pow / abs / mean, scale, bias, labels, logsigmoid, sum and
            their autograd), alternated in one process: device time from HIP events around forward + backward (median over the
            iterations), host-issue time as the host clock around the same calls without a synchronise
  step      the CLIP RN50 training step at batch 64 through the training plan with a seeded random teacher output and SGD-momentum
            (bench.py --train's update): (a) the BCE stand-in of bench.py over the embedding coordinates, (b) the torch-form SigLIP,
            (c) the fused SigLIP, alternated; medians and spreads over the rounds

python scripts/siglip_bench.py [--iters 50] [--steps 10] [--rounds 3] [--batch 64] [--skip-step] [--out profiles/siglip_bench.json]
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

from bcos.modules.losses import siglip_loss_torch  # noqa: E402
from bcos_hip import clip_head, lib, synth  # noqa: E402

DEV = "cuda"


def torch_form(out, teacher, cos_power):
    return siglip_loss_torch(F.normalize(out, dim=-1), F.normalize(teacher, dim=-1), 10.0, -10.0, cos_scaling=cos_power if out.dim() == 3 else 0)


def loss_alone(L, N, D, cos_power, iters):
    gen = torch.Generator(device=DEV).manual_seed(L)
    teacher = torch.randn(N, D, device=DEV, generator=gen)
    shape = (L, N, D) if L > 1 else (N, D)
    student = (teacher + 0.8 * torch.randn(shape, device=DEV, generator=gen)).requires_grad_(True)
    variants = dict(fused=lambda: clip_head.distill_loss(student, teacher, cos_power=cos_power),
                    torch_form=lambda: torch_form(student, teacher, cos_power))

    def run(fn):
        student.grad = None
        fn().backward()
    for fn in variants.values():
        for _ in range(5):
            run(fn)
    torch.cuda.synchronize()
    dev = {k: [] for k in variants}
    host = {k: [] for k in variants}
    for _ in range(iters):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            run(fn)
            b.record()
            host[name].append(time.perf_counter() - t0)
            b.synchronize()
            dev[name].append(a.elapsed_time(b))
    res = dict(L=L, N=N, D=D, cos_power=cos_power if L > 1 else 0, iters=iters)
    for name in variants:
        d, h = sorted(dev[name]), sorted(host[name])
        res[name] = dict(device_ms=round(d[len(d) // 2], 4), device_min_ms=round(d[0], 4), host_issue_us=round(1e6 * h[len(h) // 2], 1))
    run(variants["fused"])
    g_fused = student.grad.clone()
    run(variants["torch_form"])
    res["gradient_distance"] = float((g_fused - student.grad).double().norm() / student.grad.double().norm())
    res["fused_over_torch_device"] = round(res["fused"]["device_ms"] / res["torch_form"]["device_ms"], 3)
    return res


def step(batch, steps, rounds):
    from bcos_hip import engine
    net = synth.build_bcosified_clip_rn50(seed=0).to(DEV)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(DEV))
    engine.attach(net)
    net.train()
    x = synth.synthetic_images(batch, seed=1000).to(DEV)
    teacher = torch.randn(batch, 1024, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    target = (teacher > 0).float()
    params = [p for p in net.parameters() if p.requires_grad]
    sgd = torch.optim.SGD(params, lr=1e-4, momentum=0.9)
    losses = dict(a_bce_stand_in=lambda o: F.binary_cross_entropy_with_logits(o, target),
                  b_torch_siglip=lambda o: torch_form(o, teacher, 0),
                  c_fused_siglip=lambda o: clip_head.distill_loss(o, teacher))

    def one(loss_of):
        sgd.zero_grad(set_to_none=True)
        loss_of(net(x)).backward()
        sgd.step()
    times = {k: [] for k in losses}
    for fn in losses.values():
        for _ in range(3):
            one(fn)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in losses.items():
            one(fn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one(fn)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps)
    res = dict(arch="clip_rn50", batch=batch, steps=steps, rounds=rounds,
               plan=getattr(getattr(net, "_bcos_engine", None), "_train_plan", None) not in (None, False))
    for name, ts in times.items():
        ts.sort()
        res[name] = dict(ms_per_step=round(1e3 * ts[len(ts) // 2], 3), images_per_s=round(batch / ts[len(ts) // 2], 1),
                         spread_ms=[round(1e3 * ts[0], 3), round(1e3 * ts[-1], 3)])
    res["c_over_b_ms"] = round(res["c_fused_siglip"]["ms_per_step"] / res["b_torch_siglip"]["ms_per_step"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "siglip_bench.json"))
    args = ap.parse_args()
    lib.load()
    assert torch.cuda.is_available(), "siglip_bench.py needs a HIP device"
    out = dict(metric="SigLIP distillation loss: loss + backward alone (HIP events, host clock) and the CLIP RN50 training step",
               loss=[loss_alone(1, 64, 1024, 0, args.iters), loss_alone(49, 64, 1024, 2, args.iters)])
    if not args.skip_step:
        out["step"] = step(args.batch, args.steps, args.rounds)
    out["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
