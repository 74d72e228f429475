#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric: images/s, forward + explanation, B-cosified ResNet-50 @224, batch 256 per GPU.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`)

One "step" = one pass of the hot path over one batch of 256 synthetic 224x224 images per GPU: input
preparation, 54 fused B-cos conv launches, head, arg-max, 54 layers of input-gradient launches, W(x) and
contribution maps -- followed (N > 1) by the single all-gather of per-rank logits and maps.  Inputs and
weights are resident in HBM before the timed region.  Weak scaling: every rank processes its own 256 images.

A plain run sets up, warms up, times the K steps and prints the contract fields (metric, value, unit, higher_is_better,
dtype, ms_per_step, step_times, config); `roofline` and `cpu_baseline` are null.  `--full` adds everything else the
benchmark measures:
  roofline      fp32-MFMA roofline of the dominant kernel family (tapconv_kernel): algorithmic FLOP of the B-cos
                contractions of one step (17.22 GFLOP/image) / the time spent in those launches,
                measured live with HIP events on the launch stream inside the timed region (around every contraction
                launch of every 20th timed step, which runs on ONE stream so that an event pair times its own launch only),
                the shader clock / socket power sampled during the timed region, and the vendor GEMM / device copy beside it;
  cpu_baseline  the CPU oracle (the PyTorch-CPU restatement of the reference's path) timed on this host's cores on
                a bounded sample (rank 0, N = 1 only);
  gather_ms_per_step  (N > 1) the all-gather of one step by itself, outside the timed region.

`--dump-outputs DIR` writes what the last timed step returned to its caller as DIR/<name>.npy (float32 / float64; integer
outputs as float64, large outputs as a fixed seeded sample of their elements, 64 MB at most in all).  The inputs and weights
are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(REPO, "b-cosification_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

# The CPU baseline (rank 0 of an N = 1 run) wants its OpenMP threads pinned to cores, and the OpenMP runtime reads its environment
# when torch is imported: decide from the command line alone, before that import.  Multi-rank runs and runs without the baseline
# keep the default (eight ranks must not all bind their master threads to core 0).
def _argv_value(flag, default):
    for i, a in enumerate(sys.argv):
        if a == flag and i + 1 < len(sys.argv):
            return sys.argv[i + 1]
        if a.startswith(flag + "="):
            return a.split("=", 1)[1]
    return default


try:
    _AVAIL_CPUS = len(os.sched_getaffinity(0))      # (before the OpenMP runtime binds this thread to its first place)
except AttributeError:
    _AVAIL_CPUS = os.cpu_count() or 1
if (_argv_value("--gpus", "1") == "1" and "WORLD_SIZE" not in os.environ and "--no-cpu-baseline" not in sys.argv
        and "--train" not in sys.argv and "--forward-only" not in sys.argv):
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# forward GFLOP per image = 2*MAC of the B-cos convs / linears only; the
# explanation adds one input-gradient contraction per layer = the same again.  The default (resnet50, batch 256) is the
# configuration BASELINE.json's metric is quoted on; the other architectures are the remaining BASELINE configs and
# are diagnostics (same JSON shape, `config.workload` names them).
ARCHS = {
    "resnet50": dict(gflop_fwd=8.611, family="resnet", explain=True),
    "resnet18": dict(gflop_fwd=3.913, family="resnet", explain=True),
    "vit_ti": dict(gflop_fwd=1.752, family="vit", explain=True),
    "clip_rn50": dict(gflop_fwd=10.756, family="clip", explain=True),    # explains the arg-max embedding coordinate
}
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_16BIT_MFMA_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 / f16 MFMA (the pipe the split contractions execute on)
SPEC_SCLK_MHZ = 2400.0             # MI355X_MICROARCH.md: the shader clock the dense MFMA peaks are quoted at
PEAK_HBM_GBPS = 8000.0             # MI355X_MICROARCH.md: HBM3E spec (6 290 GB/s measured with a float4 copy)
PRODUCTS = {"f32": 1, "bf16x3": 6, "f16x2": 3}     # matrix instructions per algorithmic fp32 product, by contraction mode
DTYPES = {
    "f32": "f32",
    "bf16x3": "f32 (contraction: exact 3-way bf16 split of the fp32 operands, 6 bf16 MFMA products, fp32 accumulate)",
    "f16x2": "f32 (contraction: row-scaled 2-way fp16 split of the fp32 operands, 3 f16 MFMA products, fp32 accumulate; "
             "launches without operand maxima or with K < {min_k} use the exact 3-way bf16 split)",
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per step")
    ap.add_argument("--arch", default="resnet50", choices=sorted(ARCHS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=256, help="images in the CPU-baseline sample (BASELINE.md section 4 asks "
                    "for 256; cut down to ~30 s of CPU work and flagged when the host is slower)")
    ap.add_argument("--forward-only", action="store_true", help="diagnostic: time the forward pass only")
    ap.add_argument("--train", action="store_true",
                    help="diagnostic (NOT the BASELINE.json metric): one TRAINING step per step -- train-mode forward (batch statistics in "
                         "every BatchNormUncentered2d, dynamic scales differentiated), BCE-with-logits loss, backward to every parameter, "
                         "(N > 1) bucketed gradient all-reduce, SGD-momentum update -- the reference trainer's step "
                         "(bcos/training/trainer.py:666-784) at its ImageNet batch of 64 per GPU unless --batch is given")
    ap.add_argument("--no-vendor-ref", action="store_true", help="skip the vendor fp16 GEMM reference of the matrix-bound launches (a few seconds, outside the timed region)")
    ap.add_argument("--no-train-plan", action="store_true", help="diagnostic (--train): no engine attached, every layer its own autograd node")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step from a captured hipGraph (engine.CapturedPass) instead of launching eagerly; "
                         "measured 1 %% SLOWER than eager launches on ROCm 7.2 (6 667 vs 6 745 images/s), hence off")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="diagnostic: do not bracket the contraction launches with HIP events (roofline fields become null)")
    ap.add_argument("--no-telemetry", action="store_true", help="diagnostic: do not sample shader clock / socket power during the timed region")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: roofline (per-launch HIP events in every 20th timed step, "
                         "clock / power telemetry, vendor GEMM and device-copy references), CPU baseline, (N > 1) the all-gather by itself")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step returned as DIR/<name>.npy (float32 / float64, a fixed "
                         "seeded sample of large outputs, 64 MB at most in all)")
    ap.add_argument("--contraction", choices=("f16x2", "bf16x3", "f32"), default=None,
                    help="arithmetic of the contraction kernel (include/bcos_hip.h: bcos_set_contraction_mode); default: "
                         "the library default (f16x2 = row-scaled 2-way fp16 split, 3 products, fp32 accumulation)")
    return ap.parse_args()


def _host_description():
    """CPU model / sockets / cores of the node from lscpu (stated with the baseline)."""
    try:
        import subprocess
        info = {}
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = line.partition(":")
            info[k.strip()] = v.strip()
        return (f"{info.get('Model name', '?')}, {info.get('Socket(s)', '?')} socket(s) x {info.get('Core(s) per socket', '?')} cores, "
                f"{info.get('CPU(s)', '?')} hardware threads")
    except Exception:
        return "lscpu unavailable"


def _physical_cores():
    try:
        import subprocess
        info = {}
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = line.partition(":")
            info[k.strip()] = v.strip()
        return int(info["Socket(s)"]) * int(info["Core(s) per socket"])
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline(net, arch, n_images, budget_s=60.0):
    """The oracle (kind 'port': PyTorch-CPU restatement of the reference path, pinned by tests/golden) on the host cores,
    following BASELINE.md section 4: fp32, warm-up before timing, forward + explanation AND forward-only, the thread count
    stated.  Thread count: BASELINE.md says "all host threads", but torch's intra-op pool collapses on the 2 x 64-core
    hosts of this pool well below that, so a sweep over {16, 32, 48, 64, 96, 128} threads (OpenMP threads pinned: OMP_PROC_BIND=close,
    OMP_PLACES=cores, set before torch is imported) picks the fastest setting on THIS host; the sweep runs the same 32-image chunks
    as the timed passes (four per entry), and a timed pass more than 20 % off its own sweep entry is flagged in `note`.  Sample: up to `n_images` (256 = the metric's batch)
    images per pass, processed in chunks of 32 to bound host memory (throughput is per image; a B-cos pass has no
    cross-image operation), cut down to what fits ~`budget_s` seconds of CPU work and flagged if below 256."""
    from bcos_hip import synth
    from oracle import bcos_oracle as O
    avail = _AVAIL_CPUS
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    if ARCHS[arch]["family"] == "vit":
        fwd = lambda xx, detach: O.simple_vit_logits(sd, xx, detach=detach)  # noqa: E731
    else:
        fwd = lambda xx, detach: O.resnet_logits(sd, xx, arch, detach=detach)  # noqa: E731
    CH = 32

    def run(x, explain=True):
        t0 = time.perf_counter()
        for lo in range(0, x.shape[0], CH):
            if explain:
                O.explain_batch(fwd, x[lo:lo + CH])
            else:
                with torch.no_grad():
                    fwd(x[lo:lo + CH], False)
        return time.perf_counter() - t0

    xs = synth.synthetic_images(4 * CH, seed=321)
    torch.set_num_threads(min(avail, 32))
    run(xs[:8])                                      # first call: oneDNN primitive creation
    env_threads = os.environ.get("BCOS_CPU_BASELINE_THREADS")
    cands = sorted({c for c in ((int(env_threads),) if env_threads else (16, 32, 48, 64, 96, 128)) if 1 <= c <= avail}) or [avail]
    # the sweep runs what the timed passes run -- four 32-image chunks of forward + explanation (a single chunk of ~1 s rides the host's
    # boost clocks: 35.7 against 26.6 images/s sustained on one node; two chunks still did on some hosts: 32.7 against 24.7) -- one chunk warm, then timed twice; a pool size
    # whose 2-image probe is more than 2.5 x slower per image than the best so far is recorded from the probe alone (torch's intra-op pool
    # collapses beyond some size on the 2 x 64-core hosts: 0.05 images/s at 256 threads)
    sweep, skipped = {}, []
    best = 0.0
    for c in cands:
        torch.set_num_threads(c)
        run(xs[:2])
        t2 = run(xs[:2])
        if best > 0.0 and t2 / 2.0 > 2.5 / best:
            sweep[c] = round(2 / t2, 2)
            skipped.append(c)
            continue
        run(xs[:CH])
        sweep[c] = round(4 * CH / min(run(xs), run(xs)), 2)
        best = max(best, sweep[c])
    cores = max((c for c in sweep if c not in skipped), key=sweep.get)
    torch.set_num_threads(cores)
    rate = sweep[cores]
    # passes: 2 timed of forward+explanation + 2 of forward-only (~1/6 of the cost each), one-chunk warm-ups: ~2.5 n / rate seconds
    n = max(CH, min(n_images, int(budget_s * rate / 2.5) // CH * CH))
    x = synth.synthetic_images(n, seed=321)
    run(x[:CH])
    t_fe = sorted(run(x) for _ in range(2))
    run(x[:CH], explain=False)
    t_f = sorted(run(x, explain=False) for _ in range(2))
    value = n / t_fe[0]
    note = None
    # the sweep entry of the winner once more, AFTER the timed passes: hosts of this pool drift by +-20 % within a minute (boost clocks,
    # page placement), so the timed pass is held against the entry measured before it and the one measured after it
    rate_after = round(4 * CH / min(run(xs), run(xs)), 2)
    if abs(value - rate) > 0.2 * rate and abs(value - rate_after) > 0.2 * rate_after:      # same chunks, same pool: they must agree
        note = (f"INCONSISTENT: the timed {n}-image pass ({value:.1f} images/s) is more than 20 % off the sweep's entry for the same "
                f"{cores} threads ({rate:.1f} images/s on four {CH}-image chunks before the timed passes, {rate_after:.1f} after them) -- the host's clocks / memory placement moved between them; "
                "treat this baseline as a range")
        print("bench.py: cpu_baseline " + note, file=sys.stderr)
    # The same restatement executed by PyTorch-ROCm ON THE DEVICE (fp32, MIOpen / rocBLAS convolutions, autograd for the explanation):
    # what running the reference's algorithm eagerly on this GPU gives -- beside the CPU figure, not instead of it.
    eager = None
    if torch.cuda.is_available() and ARCHS[arch]["family"] != "vit":
        try:
            dev = torch.device("cuda", torch.cuda.current_device())
            sd_d = {k: v.to(dev) for k, v in sd.items()}
            fwd_d = lambda xx, detach: O.resnet_logits(sd_d, xx, arch, detach=detach)  # noqa: E731
            xd = synth.synthetic_images(256, seed=321).to(dev)

            def run_d(explain):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for lo in range(0, xd.shape[0], 64):
                    if explain:
                        O.explain_batch(fwd_d, xd[lo:lo + 64])
                    else:
                        with torch.no_grad():
                            fwd_d(xd[lo:lo + 64], False)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            run_d(True); run_d(False)
            te, tf = min(run_d(True) for _ in range(3)), min(run_d(False) for _ in range(3))
            eager = dict(value=round(256 / te, 1), unit="images/s", forward_only=round(256 / tf, 1),
                         sample=f"the oracle's forward + explanation of 256 images in chunks of 64 on the device through torch {torch.__version__} "
                                "eager fp32 (timing only; the product never calls it), best of 3 after a warm-up")
            del sd_d, xd
            torch.cuda.empty_cache()
        except Exception as exc:
            eager = dict(error=f"{type(exc).__name__}: {exc}"[:200])
    return dict(value=round(value, 3), unit="images/s", cores=cores, kind="port", images=n,
                pytorch_rocm_eager_on_this_gpu=eager,
                passes_images_per_s=[round(n / t, 3) for t in t_fe],
                forward_only=dict(value=round(n / t_f[0], 3), unit="images/s", passes_images_per_s=[round(n / t, 3) for t in t_f]),
                thread_sweep_images_per_s={str(k): v for k, v in sweep.items()},
                sweep_winner_again_after_the_timed_passes=rate_after,
                thread_binding=dict(OMP_PROC_BIND=os.environ.get("OMP_PROC_BIND"), OMP_PLACES=os.environ.get("OMP_PLACES")),
                note=note,
                sample=f"forward+explanation (and, separately, forward-only) of one batch of {n} images in chunks of {CH}, best of 2 timed "
                       f"passes after a warm-up (the other pass: {n / t_fe[1]:.1f} images/s), torch {torch.__version__} CPU fp32 with "
                       f"{cores} threads = the fastest of the sweep {sweep} (four {CH}-image chunks per entry after a warm chunk, best of two timed; "
                       f"entries {skipped} from a 2-image probe only: more than 2.5 x slower than the best) on {_host_description()}"
                       + ("" if n >= 256 else f"; BASELINE.md section 4 asks for batch 256: {n} images timed to stay within ~{budget_s:.0f} s "
                                               "of CPU work, throughput is per image"))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks as a CHILD process group
    (`python -m torch.distributed.run --nproc-per-node N bench.py ...`), relay rank 0's JSON line and return the child's
    exit code.  Nothing in this parent has touched the GPU at this point (no HIP call, no torch.cuda call, the library is
    not loaded) and the parent never replaces itself (no exec): it waits for the child."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in (lines[-1:] if lines else proc.stdout.splitlines()[-20:]):
        print(ln, flush=True)
    return proc.returncode if (proc.returncode != 0 or lines) else 1


def vendor_gemm_reference(shapes, ours_ms, prod, n_ev, pipe_peak, dev):
    """Time torch.matmul in fp16 on (M, prod * K, N) for every distinct matrix-bound launch shape; -> the sum over the step's launches
    beside the sum of this repo's launch times for the same launches."""
    import collections
    count = collections.Counter(s for s in shapes if s is not None)
    ours = collections.defaultdict(float)
    for s, ms in zip(shapes, ours_ms):
        if s is not None:
            ours[s] += ms
    vend_ms = flops = 0.0
    worst = None
    classes = collections.OrderedDict()        # shape class -> [ours ms, vendor ms, launches]
    def shape_class(M, K, N):
        if K >= 1536:
            return "K >= 1536 (3x3 and K = 2048 layers)"
        if N >= 1024 and K <= 512:
            return "K <= 512 into N >= 1024 (short K, wide N: expand 1x1 at 14^2 / 7^2)"
        if N <= 64:
            return "N <= 64 (stem, 56^2 reduce / 3x3)"
        return "512 <= K < 1536, N 128-1024 (reduce 1x1, 3x3 @28^2)"
    for (M, K, N), c in sorted(count.items()):
        a = torch.randn(M, K * prod, device=dev, dtype=torch.float16)
        b = torch.randn(K * prod, N, device=dev, dtype=torch.float16)
        for _ in range(2):
            torch.matmul(a, b)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            torch.matmul(a, b)
        e1.record()
        torch.cuda.synchronize()
        one = e0.elapsed_time(e1) / 5
        vend_ms += one * c
        flops += 2.0 * M * K * prod * N * c
        ratio = (ours[(M, K, N)] / c) / one
        cl = classes.setdefault(shape_class(M, K, N), [0.0, 0.0, 0])
        cl[0] += ours[(M, K, N)]; cl[1] += one * c; cl[2] += c
        if worst is None or ratio > worst[0]:
            worst = (ratio, (M, K, N), round(1e3 * ours[(M, K, N)] / c, 1), round(1e3 * one, 1))
        del a, b
    ours_total = sum(ours.values())
    return dict(ms_per_step=round(vend_ms / n_ev, 3), ours_ms_per_step=round(ours_total / n_ev, 3), launches_per_step=sum(count.values()) // n_ev,
                distinct_shapes=len(count), tflops=round(flops / vend_ms / 1e9, 1), frac_of_executing_pipe=round(flops / vend_ms / 1e9 / pipe_peak, 4),
                ours_over_vendor_time=round(ours_total / vend_ms, 3),
                role="context (hipBLASLt's default heuristic through torch.matmul, untuned for these shapes), NOT a bound: a ratio above 1 in "
                     "ours_over_vendor marks a shape class with measured headroom, a ratio below 1 says nothing about a ceiling",
                ours_over_vendor={k: dict(ratio=round(v[0] / v[1], 3), ours_ms_per_step=round(v[0] / n_ev, 3), vendor_ms_per_step=round(v[1] / n_ev, 3),
                                          launches_per_step=v[2] // n_ev) for k, v in classes.items()},
                slowest_against_vendor=dict(ratio=round(worst[0], 3), M_K_N=list(worst[1]), ours_us=worst[2], vendor_us=worst[3]),
                note=(f"torch.matmul fp16 (fp32 accumulate) on (M, {prod} K, N) per matrix-bound launch shape, 5 timed calls each after 2, HIP "
                      "events, outside the timed region: the same matrix instructions on the same pipe with none of the launch's other work "
                      "(no fp32 -> f16 split of the operands, no patch gather for the 3x3 / 7x7 layers -- the vendor GEMM gets the unfolded "
                      "matrix for free --, no patch norms, no B-cos / BatchNorm / ReLU epilogue, no multiplier or maxima tensors)"))


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(outputs, dirname):
    """--dump-outputs: every tensor of `outputs` (name -> tensor) as dirname/<name>.npy.  float64 stays float64, other floating
    types become float32, integer / bool outputs float64 (exact).  An output larger than its share of the 64 MB budget is written
    as a sample of its flattened elements at indices drawn from a generator seeded by its name and size, so that two runs with
    the same arguments sample the same elements.  Returns name -> {shape, dtype, written elements} for the result line."""
    import zlib
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    items = [(k, v) for k, v in outputs.items() if isinstance(v, torch.Tensor)]
    share = DUMP_LIMIT_BYTES // max(len(items), 1)
    info = {}
    for name, t in items:
        t = t.detach()
        dt = torch.float64 if (t.dtype == torch.float64 or not t.is_floating_point()) else torch.float32
        flat = t.reshape(-1)
        n = flat.numel()
        itemsize = 8 if dt == torch.float64 else 4
        sampled = n * itemsize > share
        if sampled:
            rng = np.random.default_rng(zlib.crc32(f"{name}:{n}".encode()))
            idx = np.sort(rng.integers(0, n, size=share // itemsize, dtype=np.int64))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        arr = flat.to(dt).cpu().numpy()
        np.save(os.path.join(dirname, f"{name}.npy"), arr if sampled else arr.reshape(tuple(t.shape)))
        info[name] = dict(shape=list(t.shape), dtype=str(t.dtype).replace("torch.", ""), written=int(arr.size), sampled=sampled)
    return info


def train_main(args):
    """`--train`: images/s of whole training steps of the B-cosified network on the HIP kernels -- through the engines' training plans
    (bcos_hip/train_plan.py, bcos_hip/vit_train_plan.py), or per layer on the nn.Module path (--no-train-plan).  One JSON line of the same shape as the metric's; the roofline prices the
    algorithmic work of a step -- forward + input-gradient + weight-gradient contractions = 3 x the forward FLOPs -- against the whole
    step time (no per-kernel events: the parameter-gradient launches run on a second stream beside the input-gradient chain)."""
    import torch.nn.functional as F
    from bcos_hip import dist as bdist, lib, synth
    lib.load()
    if args.contraction:
        lib.set_contraction_mode(args.contraction)
    rank, local_rank, world = bdist.init()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    if os.environ.get("BCOS_SINGLE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    spec = ARCHS[args.arch]
    if spec["family"] == "vit":
        net = synth.build_bcosified_vit(seed=0).to(dev)
    elif spec["family"] == "clip":
        net = synth.build_bcosified_clip_rn50(seed=0).to(dev)
    else:
        net = synth.build_bcosified_resnet(args.arch, seed=0).to(dev)
    with torch.no_grad():
        synth.calibrate(net, synth.synthetic_images(8, seed=123).to(dev))
        replica_diff = bdist.replicate_parameters(net) if world > 1 else []
    if replica_diff:
        raise SystemExit(f"bench.py: replicas differ after the broadcast of rank 0's parameters: {replica_diff[:5]}")
    if not args.no_train_plan:           # (in eval mode: the inference plan; its layer / block list also drives the training plan)
        if spec["family"] == "vit":
            from bcos_hip import vit_engine
            vit_engine.attach(net)
        else:
            from bcos_hip import engine
            engine.attach(net)
    net.train()
    B = args.batch
    x = synth.synthetic_images(B, seed=1000 + rank).to(dev)
    n_out = 1024 if spec["family"] == "clip" else 1000          # (CLIP RN50: the 1024 embedding coordinates stand in for the classes)
    target = F.one_hot(torch.randint(0, n_out, (B,), generator=torch.Generator().manual_seed(rank)), n_out).float().to(dev)
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-4, momentum=0.9)

    path = {}
    last = {}           # what the step hands its caller (--dump-outputs)

    def step():
        opt.zero_grad(set_to_none=True)
        logits = net(x)
        path["node"] = type(logits.grad_fn).__name__
        path["plan"] = getattr(getattr(net, "_bcos_engine", None), "_train_plan", None) not in (None, False)
        loss = F.binary_cross_entropy_with_logits(logits, target)
        loss.backward()
        if world > 1:
            bdist.allreduce_gradients(params)
        opt.step()
        last.update(loss=loss.detach(), logits=logits.detach())
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        loss = step()
        marks[i + 1].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    gflop_step = 3.0 * spec["gflop_fwd"] * B
    ms = 1e3 * elapsed / args.steps
    contraction = lib.get_contraction_mode()
    result = {
        "metric": f"images/sec (training step: fwd + bwd + update) B-cos {args.arch} @224, batch {B} per GPU -- diagnostic, not the BASELINE.json metric",
        "value": round(B * world * args.steps / elapsed, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms, 3),
        "step_times": dict(unit="ms", median=round(step_ms[len(step_ms) // 2], 3), min=round(step_ms[0], 3), max=round(step_ms[-1], 3)),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (parameters, activations, gradients, accumulation; forward / input-gradient contractions: " + DTYPES[contraction].format(min_k=0)
                 + "; weight-gradient contraction: " + ("fp32 MFMA" if contraction == "f32" else "exact 3-way bf16 split of both operands, 6 bf16 MFMA products, fp32 accumulate") + ")",
        "data": "synthetic",
        "config": {"workload": f"B-cosified {args.arch} TRAINING step (train-mode forward with batch statistics, BCE-with-logits, backward, "
                               f"SGD-momentum update), batch {B} per GPU, 224x224x6, calibrated random-init weights",
                   "global_batch": B * world, "parallelism": f"dp{world}", "contraction": contraction,
                   "path": (f"training plan (bcos_hip/{'vit_' if spec['family'] == 'vit' else ''}train_plan.py): the whole network ONE autograd node whose "
                            "forward / backward walk the engine's layer list" if path.get("plan") else
                            "nn.Module path: one HIP launch sequence per layer under autograd (no training plan for this topology)"),
                   "collective": "bucketed asynchronous all_reduce of the gradients (bcos_hip.dist.allreduce_gradients)" if world > 1 else "none",
                   "final_loss": round(float(loss.detach()), 6)},
        "roofline": dict(bound="mfma", achieved=round(gflop_step / ms, 2), peak=PEAK_FP32_MFMA_TFLOPS, unit="TFLOP/s (algorithmic fp32 FLOP of "
                         "the B-cos contractions: forward + input gradient + weight gradient = 3 x forward; fp32 matrix peak as the common "
                         "denominator)", frac=round(gflop_step / ms / PEAK_FP32_MFMA_TFLOPS, 4), traffic=None,
                         algorithmic_gflop_per_step=round(gflop_step, 1),
                         note="whole training step (every kernel, the optimizer update and the Python / autograd dispatch included), not a "
                              "per-kernel time: the per-layer path is launch- and elementwise-bound at this batch size"),
        "cpu_baseline": None,
    }
    if rank == 0 and args.dump_outputs:
        result["outputs_dumped"] = dump_outputs(last, args.dump_outputs)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if args.train and args.batch == 256 and "--batch" not in " ".join(sys.argv):
        args.batch = 64          # the reference's ImageNet training batch per GPU (bcosification/experiment_parameters.py:29)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    if args.train:
        return train_main(args)
    from bcos_hip import dist as bdist, engine, lib, ops, synth
    lib.load()      # fails loudly if the HIP library was not built
    if args.contraction:
        lib.set_contraction_mode(args.contraction)
    contraction = lib.get_contraction_mode()
    rank, local_rank, world = bdist.init()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    if os.environ.get("BCOS_SINGLE_DEVICE"):     # functional check of the N > 1 control flow on a 1-GPU box (with
        local_rank = 0                           # BCOS_DIST_BACKEND=gloo); never set by the driver
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    # shader clock and socket power DURING the timed region (a child process samples every ~10 ms: bcos_hip/telemetry.py) -- the part
    # is power / clock limited under these kernels, so the roofline is also stated at the clock it actually sustained.  Started ahead
    # of the model build: the child has found its SMI source long before the timed region begins.
    sampler = None
    if rank == 0 and args.full and not args.no_telemetry:
        from bcos_hip import telemetry
        sampler = telemetry.Sampler(index=telemetry.physical_index(local_rank), interval=0.01).start()     # (SMI / sysfs count physical devices)

    # -- model + data, resident in HBM --------------------------------------------------------------------------
    spec = ARCHS[args.arch]
    if not spec["explain"]:
        args.forward_only = True
    if spec["family"] == "vit":
        from bcos_hip import vit_engine
        net = synth.build_bcosified_vit(seed=0).to(dev)
    elif spec["family"] == "clip":
        net = synth.build_bcosified_clip_rn50(seed=0).to(dev)
    else:
        net = synth.build_bcosified_resnet(args.arch, seed=0).to(dev)
    calib = synth.synthetic_images(8, seed=123).to(dev)
    with torch.no_grad():
        synth.calibrate(net, calib)            # same seeds on every rank
        # data-parallel replicas carry rank 0's parameters (what loading one checkpoint gives in deployment) and PROVE it:
        # a digest of every state-dict entry is exchanged; diverged replicas end the run instead of being averaged over
        replica_diff = bdist.replicate_parameters(net) if world > 1 else []
    if replica_diff:
        raise SystemExit(f"bench.py: replicas differ after the broadcast of rank 0's parameters: {replica_diff[:5]}")
    eng = vit_engine.attach(net) if spec["family"] == "vit" else engine.attach(net)
    x = synth.synthetic_images(args.batch, seed=1000 + rank).to(dev)
    torch.cuda.synchronize()

    pipe = bdist.OverlappedGather(depth=2) if world > 1 else None
    if world > 1:
        # what actually runs must be what the line will say: one rank per device over RCCL.  (BCOS_SINGLE_DEVICE / BCOS_DIST_BACKEND
        # are the functional checks of the control flow on a 1-GPU box or on gloo: they say so in the line and are never set by the driver.)
        seen, backend = dist.get_world_size(), dist.get_backend()
        if seen != world:
            raise SystemExit(f"bench.py: --gpus {world} but the process group has {seen} ranks")
        if backend != "nccl" and not (os.environ.get("BCOS_SINGLE_DEVICE") or os.environ.get("BCOS_DIST_BACKEND")):
            raise SystemExit(f"bench.py: --gpus {world} on real devices must run over RCCL (backend 'nccl'), got '{backend}'")

    # --graph: the step is recorded once into a hipGraph (engine.CapturedPass) and replayed; the steps that carry the
    # per-launch HIP events for the roofline run the very same launches eagerly (events cannot be read back from a graph).
    captured = None
    if args.graph:
        try:
            captured = engine.CapturedPass(eng, x, explain=not args.forward_only, want_weights=True)
        except Exception as exc:        # capture is an optimisation: fall back to eager launches, say so
            print(f"bench.py: hipGraph capture failed ({type(exc).__name__}: {exc}); running eagerly", file=sys.stderr)
            captured = None

    def step(eager=False):
        if captured is not None and not eager:
            out = captured()
            keys = ("logits",) if args.forward_only else ("logits", "contribution_map")
        elif args.forward_only:
            out = dict(logits=eng.forward(x))      # clip_rn50: the image embeddings
            keys = ("logits",)
        else:
            out = eng.explain(x, want_weights=True)
            keys = ("logits", "contribution_map")
        if world > 1:       # the single collective of the path: ONE packed all-gather per step over RCCL/xGMI, asynchronous
            pipe.submit({k: out[k] for k in keys}, copy_out=False)      # (overlaps the next step's compute; drained inside the timed region)
        return out

    if sampler is not None:
        sampler.wait_ready()

    kernel_events = args.full and not args.no_kernel_events
    for w in range(args.warmup):
        if w == 0 and kernel_events and args.warmup > 1:
            # the first warm-up step runs the way the event-carrying timed steps do (every launch on the caller's stream, over the whole
            # batch): the kernel instantiations, LDS / scratch reservations and arenas of THAT path are first-use costs too
            sub = getattr(eng, "subbatch_streams", 1)
            eng.subbatch_streams = 1
            step(eager=True)
            eng.subbatch_streams = sub
        else:
            step()
    if pipe is not None:
        pipe.flush()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    # HIP events on the launch stream around every contraction launch of a SAMPLE of the timed steps (every 20th: the
    # two events per launch cost ~7 us of stream time each, 0.9 ms per step if taken on every step)
    EVENT_STRIDE = 20
    event_steps = [i for i in range(args.steps) if i % EVENT_STRIDE == 0] if kernel_events else []
    events = []
    # one HIP event per step boundary on the caller's stream (the engine's side streams are joined into it at the end of every
    # pass): per-step times -> median / min, and the two execution modes of the timed region reported apart
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    wall0 = time.time()
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        if i in event_steps:
            # the steps that carry the per-launch HIP events run their launches on ONE stream: with the engine's two sub-batch
            # streams (bcos_hip/engine.py: _SUBBATCH_STREAMS) launches overlap and an event pair would time its neighbour too
            ops.KERNEL_TIMING = []
            sub = getattr(eng, "subbatch_streams", 1)
            eng.subbatch_streams = 1
            out = step(eager=True)
            eng.subbatch_streams = sub
            events += ops.KERNEL_TIMING
            ops.KERNEL_TIMING = None
        else:
            out = step()
        marks[i + 1].record()
    if pipe is not None:
        gathered = pipe.flush()             # the last exchanges complete inside the timed region
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    wall1 = time.time()
    clocks = sampler.window(wall0, wall1) if sampler is not None else None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # the collective by itself, outside the timed region: the packed all-gather of one step's results issued and waited for with nothing
    # to overlap it (inside the timed region it runs on RCCL's stream beside the next step's compute)
    if args.dump_outputs and rank == 0:
        # (no further step may run before the dump: the engine's output buffers can be reused by the next pass)
        dumped = dump_outputs(out, args.dump_outputs)
    gather_ms = gather_bytes = None
    if world > 1 and args.full:
        out = step()
        payload = {k: out[k] for k in (("logits",) if args.forward_only else ("logits", "contribution_map"))}
        gather_bytes = int(sum(v.numel() * v.element_size() for v in payload.values()))
        pipe.flush()
        torch.cuda.synchronize()
        dist.barrier()
        gts = []
        for _ in range(5):
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            pipe.submit(payload, copy_out=False)
            pipe.flush()
            g1.record()
            torch.cuda.synchronize()
            gts.append(g0.elapsed_time(g1))
        gt = torch.tensor([sorted(gts)[len(gts) // 2]], device=dev, dtype=torch.float64)
        dist.all_reduce(gt, op=dist.ReduceOp.MAX)
        gather_ms = round(float(gt.item()), 4)

    ms_per_step = 1e3 * elapsed / args.steps
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    plain = sorted(t for i, t in enumerate(step_ms) if i not in event_steps)
    evs = sorted(t for i, t in enumerate(step_ms) if i in event_steps)
    med = lambda v: (round(v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), 3) if v else None)  # noqa: E731
    n_streams = int(getattr(eng, "subbatch_streams", 1))
    step_times = dict(
        unit="ms", source="HIP events on the caller's stream at every step boundary (this rank)",
        all_steps=dict(median=med(sorted(step_ms)), min=round(min(step_ms), 3), max=round(max(step_ms), 3)),
        # the steps as deployed: the batch as `n_streams` contiguous sub-batches on that many HIP streams
        sub_batch_stream_steps=dict(streams=n_streams, steps=len(plain), median=med(plain), min=round(plain[0], 3) if plain else None),
        # the steps that carry the per-launch events: every launch on ONE stream over the whole batch (+ ~14 us of event records per launch)
        single_stream_event_steps=dict(steps=len(evs), median=med(evs), min=round(evs[0], 3) if evs else None))
    images = args.batch * world * args.steps
    value = images / elapsed

    shapes = [ev[4] for ev in events]                                   # (M, K, N) of the launch's implicit GEMM, or None
    per_launch = [(e0.elapsed_time(e1), fl, nb) for (e0, e1, fl, nb, _) in events]   # (ms, algorithmic flops, algorithmic bytes)
    kernel_ms = sum(ms for ms, _, _ in per_launch)                   # all contraction launches of the sampled steps
    launches = len(per_launch)
    n_ev = max(len(event_steps), 1)
    gflop_step = spec["gflop_fwd"] * (1 if args.forward_only else 2) * args.batch
    achieved = gflop_step * n_ev / kernel_ms if kernel_ms > 0 else 0.0     # GFLOP/ms == TFLOP/s
    # HBM traffic from the PMC counters (FETCH_SIZE x 2 + WRITE_SIZE, separate rocprofv3 --pmc passes over this same command:
    # scripts/collect_profiles.sh) cannot be collected by the run itself; the tracked summary of the latest passes is quoted
    traffic = traffic_step = traffic_source = None
    tfile = os.path.join(REPO, "profiles", "traffic_latest.json")
    if os.path.exists(tfile) and args.arch == "resnet50" and not args.forward_only and args.batch == 256:
        try:
            tj = json.load(open(tfile))
            traffic = tj.get("hbm_bytes_per_launch")
            traffic_step = tj.get("hbm_bytes_per_step")
            traffic_source = (f"profiles/traffic_latest.json ({tj.get('source', 'rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes')}; "
                              "not measured by this run: counters need their own profiler passes)")
        except Exception:
            traffic = None
    # both bounds of SURVEY.md section 8(d): a launch is counted HBM-bound when its algorithmic intensity is below the
    # balance of what the contraction sustains (~250 TFLOP/s fp32-equivalent against ~5 TB/s => 50 FLOP/B)
    hbm = [(ms, fl, nb) for ms, fl, nb in per_launch if fl / max(nb, 1) < 50.0]
    mfma = [(ms, fl, nb) for ms, fl, nb in per_launch if fl / max(nb, 1) >= 50.0]
    mfma_shapes = [sh for (ms, fl, nb), sh in zip(per_launch, shapes) if fl / max(nb, 1) >= 50.0]
    hbm_ms, mfma_ms = sum(m for m, _, _ in hbm), sum(m for m, _, _ in mfma)
    hbm_gbps = sum(nb for _, _, nb in hbm) / hbm_ms / 1e6 if hbm_ms > 0 else 0.0
    mfma_tf = sum(fl for _, fl, _ in mfma) / mfma_ms / 1e9 if mfma_ms > 0 else 0.0
    prod = PRODUCTS[contraction]
    # The roofline is priced on the pipe that EXECUTES: every fp32 product of the contraction is evaluated with `prod` matrix
    # instructions on the 16-bit MFMA pipe (1 on the fp32 pipe in mode f32), so achieved = prod x algorithmic FLOP / kernel time
    # against that pipe's dense peak.  Per-launch two-sided bound: the larger of (executed matrix work / pipe peak) and
    # (algorithmic bytes / HBM peak); summed over the launches and divided by the measured kernel time.
    pipe_peak = PEAK_16BIT_MFMA_TFLOPS if prod > 1 else PEAK_FP32_MFMA_TFLOPS
    pipe_name = "f16 / bf16 MFMA, dense" if prod > 1 else "fp32 MFMA, dense"
    ideal_ms = sum(max(prod * fl / (pipe_peak * 1e9), nb / (PEAK_HBM_GBPS * 1e6)) for _, fl, nb in per_launch)
    alg_bytes_step = sum(nb for _, _, nb in per_launch) / n_ev
    roofline = dict(bound="mfma", achieved=round(prod * achieved, 2), peak=pipe_peak,
                    unit=f"TFLOP/s ({pipe_name}; {prod} matrix product(s) per fp32 product)",
                    frac=round(prod * achieved / pipe_peak, 4),
                    traffic=traffic, traffic_bytes_per_step=traffic_step, algorithmic_bytes_per_step=int(alg_bytes_step),
                    traffic_over_algorithmic=round(traffic_step / alg_bytes_step, 3) if traffic_step and alg_bytes_step else None,
                    traffic_source=traffic_source,
                    kernel="tapconv_kernel (all instantiations) + skinny_kernel", launches_per_step=launches // n_ev,
                    avg_launch_us=round(1e3 * kernel_ms / max(launches, 1), 2),
                    kernel_ms_per_step=round(kernel_ms / n_ev, 3), steps_with_events=len(event_steps),
                    single_stream_kernel_ms_per_step=round(kernel_ms / n_ev, 3),
                    two_stream_ms_per_step=(step_times["sub_batch_stream_steps"]["median"] if n_streams > 1 else None),
                    execution_modes=("kernel_ms_per_step / avg_launch_us / by_bound: the event-carrying steps, every launch on ONE stream over the "
                                     "whole batch (sum of the contraction launches only); ms_per_step / value: all timed steps, of which the "
                                     f"others run as {n_streams} sub-batches on {n_streams} streams whose launches overlap -- a whole step "
                                     "(two_stream_ms_per_step, incl. the non-contraction kernels) can therefore be shorter than the "
                                     "single-stream sum of its contraction launches"),
                    algorithmic_gflop_per_step=round(gflop_step, 1), algorithmic_tflops=round(achieved, 2),
                    vs_fp32_mfma_peak=round(achieved / PEAK_FP32_MFMA_TFLOPS, 4),
                    two_sided=dict(roofline_ms_per_step=round(ideal_ms / n_ev, 3), frac=round(ideal_ms / kernel_ms, 4) if kernel_ms > 0 else None,
                                   note="sum over launches of max(matrix instructions on the executing pipe at its dense peak, algorithmic "
                                        "bytes at 8 TB/s) / measured kernel time"),
                    by_bound=dict(
                        mfma=dict(launches_per_step=len(mfma) // n_ev, ms_per_step=round(mfma_ms / n_ev, 3),
                                  algorithmic_tflops=round(mfma_tf, 1), achieved_tflops=round(prod * mfma_tf, 1), peak_tflops=pipe_peak,
                                  frac_of_executing_pipe=round(prod * mfma_tf / pipe_peak, 4)),
                        hbm=dict(launches_per_step=len(hbm) // n_ev, ms_per_step=round(hbm_ms / n_ev, 3),
                                 achieved_gbps=round(hbm_gbps, 1), peak_gbps=PEAK_HBM_GBPS, frac=round(hbm_gbps / PEAK_HBM_GBPS, 4),
                                 note="algorithmic bytes (A once, weights once, every epilogue tensor once) / launch time")),
                    note=(f"achieved / peak / frac: matrix work executed on the {pipe_name.split(',')[0]} pipe ({prod} x the algorithmic "
                          f"{gflop_step:.1f} GFLOP per step, SURVEY.md section 8(d): 17.22 GFLOP/image forward+explanation) / the time of "
                          "the contraction launches measured with HIP events on the launch stream, against that pipe's dense peak; "
                          "vs_fp32_mfma_peak = algorithmic TFLOP/s / 157.3 (the fp32 matrix pipe the contraction does not run on)"))

    # What the vendor's GEMM reaches on the same pipe at the same shapes: every matrix-bound launch of the step as ONE plain fp16 GEMM
    # (torch.matmul -> hipBLASLt / rocBLAS, fp32 accumulate) of the launch's M and N and `prod` x its K -- the matrix work the
    # split-f16 loop executes, without the split, the patch gather, the B-cos epilogue or any tensor beyond C.  Outside the timed region.
    if rank == 0 and world == 1 and args.full and prod > 1 and not args.no_vendor_ref and mfma_shapes:
        try:
            roofline["by_bound"]["mfma"]["vendor_f16_gemm"] = vendor_gemm_reference(mfma_shapes, [m for m, _, _ in mfma], prod, n_ev, pipe_peak, dev)
        except Exception as exc:           # (an allocation failure of the reference must not cost the bench line)
            roofline["by_bound"]["mfma"]["vendor_f16_gemm"] = {"error": f"{type(exc).__name__}: {exc}"[:200]}
    # ... and what a plain streaming copy reaches against the 8 TB/s the bandwidth-bound launches are priced at: THIS library's own
    # copy kernel (bcos_stream_copy: eight global_load_dwordx4 in flight per thread, non-temporal; the microarchitecture guide measures
    # 6.29 TB/s for such a kernel) on 1 GiB -> 1 GiB of fp32, read + written bytes / time, outside the timed region.  torch's
    # dst.copy_(src) on the same buffers is reported beside it (the reference of round 5: ~5.0 TB/s, a fifth below).
    if rank == 0 and world == 1 and args.full and not args.no_vendor_ref and hbm:
        try:
            src = torch.empty(1 << 28, device=dev, dtype=torch.float32).normal_()
            dst = torch.empty_like(src)

            def rate(fn, warm=3, calls=10):
                for _ in range(warm):
                    fn()
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0.record()
                for _ in range(calls):
                    fn()
                c1.record()
                torch.cuda.synchronize()
                return calls * 2 * src.numel() * 4 / c0.elapsed_time(c1) / 1e6
            own_gbps = rate(lambda: ops.stream_copy(src, dst))
            torch_gbps = rate(lambda: dst.copy_(src))
            roofline["by_bound"]["hbm"].update(
                stream_copy_gbps=round(own_gbps, 1), frac_of_stream_copy=round(hbm_gbps / own_gbps, 4),
                torch_copy_gbps=round(torch_gbps, 1), frac_of_torch_copy=round(hbm_gbps / torch_gbps, 4),
                stream_copy_note="stream_copy_gbps: read + written bytes / time of bcos_stream_copy (this library's float4 streaming kernel) on 1 GiB "
                                 "fp32 tensors, 10 calls after 3 -- the rate a kernel with nothing but one coalesced read and one coalesced write "
                                 "reaches on this part; torch_copy_gbps: dst.copy_(src) on the same tensors (round 5's reference)")
            del src, dst
        except Exception as exc:
            roofline["by_bound"]["hbm"]["stream_copy_gbps"] = None

    # the same fraction at the clock the part sustained during the timed region: the pipe's dense peak scales with the shader
    # clock (PEAK_16BIT_MFMA_TFLOPS is quoted at SPEC_SCLK_MHZ); `frac` itself stays priced at the specification clock
    if clocks is not None:
        sclk = clocks.get("sclk_mhz_mean")
        # a device under this step draws > 1 kW and clocks above 1.5 GHz: samples far below that were taken from another (idle) device or
        # from a stale source -- no re-pricing of the roofline on them
        pw = clocks.get("power_w_mean")
        clocks_plausible = bool(sclk) and sclk >= 1000.0 and (pw is None or pw >= 300.0)
        roofline.update(sclk_mhz_mean=sclk, sclk_mhz_min=clocks.get("sclk_mhz_min"), sclk_mhz_max=clocks.get("sclk_mhz_max"),
                        power_w_mean=clocks.get("power_w_mean"), power_w_max=clocks.get("power_w_max"),
                        spec_sclk_mhz=SPEC_SCLK_MHZ, clock_samples=clocks.get("samples"), clock_source=clocks.get("source"),
                        frac_at_measured_clock=(round(roofline["frac"] * SPEC_SCLK_MHZ / sclk, 4) if sclk and clocks_plausible else None),
                        clock_note=("sclk_mhz_mean / power_w_mean: samples taken every ~10 ms by a child process over the WHOLE timed region "
                                    "(all steps, both execution modes); frac_at_measured_clock = frac x spec clock / mean sampled clock, i.e. "
                                    "the matrix pipe's peak re-priced at the clock the part sustained"))
        if not clocks_plausible:
            roofline["clock_warning"] = "sampled clock / power are not those of a loaded device (wrong physical device?): frac_at_measured_clock withheld"
        if roofline["by_bound"]["mfma"].get("frac_of_executing_pipe") is not None and sclk and clocks_plausible:
            roofline["by_bound"]["mfma"]["frac_at_measured_clock"] = round(roofline["by_bound"]["mfma"]["frac_of_executing_pipe"] * SPEC_SCLK_MHZ / sclk, 4)

    result = {
        "metric": ("images/sec (fwd+explanation) B-cos ResNet-50 @224, batch 256, 1/2/4/8 MI355X"
                   if args.arch == "resnet50" and not args.forward_only and args.batch == 256 else
                   f"images/sec ({'fwd' if args.forward_only else 'fwd+explanation'}) B-cos {args.arch} @224, batch "
                   f"{args.batch} -- diagnostic, not the BASELINE.json metric"),
        "value": round(value, 2),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "step_times": step_times,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": DTYPES[contraction].format(min_k=ops.F16X2_MIN_K),
        "data": "synthetic",
        "config": {"workload": f"B-cosified {args.arch} {'forward' if args.forward_only else 'forward+explanation'}, "
                               f"batch {args.batch} per GPU, 224x224x6 (AddInverse), calibrated random-init weights",
                   "global_batch": args.batch * world, "parallelism": f"dp{world}", "contraction": contraction,
                   "launch": "hipGraph replay (event-carrying steps eager)" if captured is not None else "eager",
                   "sub_batch_streams": int(getattr(eng, "subbatch_streams", 1)),
                   "ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
                   "backend": dist.get_backend() if dist.is_initialized() else "none",
                   "replicas_identical": (not replica_diff) if world > 1 else None,
                   "collective": "one packed async all_gather(logits, contribution maps) per step, double buffered" if world > 1 else "none",
                   # the all-gather alone (median of 5 issued with nothing beside them, max over ranks) and what every rank contributes
                   "gather_ms_per_step": gather_ms, "gather_bytes_per_rank": gather_bytes},
        "roofline": roofline if args.full else None,      # (a plain run carries no per-launch events: nothing to price)
    }
    if args.dump_outputs and rank == 0:
        result["outputs_dumped"] = dumped
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline and spec["family"] != "clip" and not args.forward_only:
        result["cpu_baseline"] = cpu_baseline(net, args.arch, args.cpu_sample)
    elif rank == 0:
        result["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
