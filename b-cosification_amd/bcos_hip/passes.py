"""Pass scheduling of the fused engines: ONE copy of how a pass over a batch is issued -- once on the caller's stream, or as contiguous
sub-batches on side streams whose launches are issued interleaved -- and of the two small loops every `explain` entry point shares.

An engine describes a pass as a generator `make_gen(lo, hi)` over the images [lo, hi) that yields (nothing) between blocks of launches
and returns its result; `SideStreams.run` decides on how many streams it runs and carries out the protocol around it.  The launches
of a pass, the stream they are issued on and their order on that stream are the generator's business alone.

torch's stream API is reached through `torch.cuda.*` at call time and through `_on_device` / `_record_stream` of this module, so that a
test can put stand-ins that log in their place (tests/test_passes_cpu.py).
"""
import os
import threading

import torch

from . import ops
from .lib import BcosHipError

# Images are independent in eval mode: a batch of at least 2 x _SUBBATCH_MIN images is split into _SUBBATCH_STREAMS contiguous
# sub-batches whose passes are issued on their own HIP streams.  The launches of one sub-batch fill the tails of the other's
# (a launch ends with most CUs idle while its last tiles finish; 117 + ~15 launches per step) and its HBM-bound launches overlap
# the other's matrix-bound ones: same-node A/B at ResNet-50 batch 256: 26.13 -> 24.63 ms per step with 2 streams (4: 24.68),
# results bit-identical (an image's result does not depend on what else is in its batch: test_determinism_and_batch_independence).
_SUBBATCH_STREAMS = int(os.environ.get("BCOS_SUBBATCH_STREAMS", "2"))
_SUBBATCH_MIN = int(os.environ.get("BCOS_SUBBATCH_MIN", "32"))


def _on_device(device) -> bool:
    return torch.device(device).type == "cuda"


def _record_stream(t, stream):
    t.record_stream(stream)


def _drive(gen):
    """run a pass generator to its end and hand back its return value"""
    try:
        while True:
            next(gen)
    except StopIteration as stop:
        return stop.value


_ISSUING = threading.Lock()        # ops._ARENA is a module global switched per generator resume: ONE pass sequence is issued at a time


def _interleave(gens, streams, arenas, device):
    """Issue the passes of several sub-batches INTERLEAVED: generator i is resumed under stream i and maxima arena i, one block at a
    time, round-robin.  Issued one whole pass after the other, the second stream's first launch is queued only when the host is done
    with the first pass -- 4 ms into a ResNet-50 step that takes 23 (scripts/probe/host_bound_probe.py); back-to-back steps hide that
    behind the previous step, an isolated call does not.  The launches of a pass and their order on its stream are unchanged.
    Threading: like the reference's `explanation_mode` context (bcos/common.py:347-384 mutates module state) this is single-threaded by
    design -- the maxima arena is a module global of bcos_hip.ops; a second Python thread entering while a pass sequence is being
    issued raises instead of corrupting both passes silently.
    Errors: when one pass generator raises, the others are closed and the caller's stream is ordered behind every side stream BEFORE
    the exception propagates -- the half-issued launches write into output tensors the caller may free or reuse."""
    if not _ISSUING.acquire(blocking=False):
        raise BcosHipError("engine: explain() / forward() re-entered from a second thread while a pass sequence is being issued "
                           "(the fused plan is single-threaded, like the reference's explanation_mode context)")
    n = len(gens)
    results, live = [None] * n, list(range(n))
    prev = ops._ARENA
    try:
        for i in range(n):
            with torch.cuda.stream(streams[i]):          # (the zero fill of pass i's maxima is ordered on pass i's stream)
                arenas[i].reset(device)
        while live:
            for i in list(live):
                ops.set_absmax_arena(arenas[i])
                with torch.cuda.stream(streams[i]):
                    try:
                        next(gens[i])
                    except StopIteration as stop:
                        results[i] = stop.value
                        live.remove(i)
    except BaseException:
        for g in gens:
            g.close()
        cur = torch.cuda.current_stream()
        for st in streams[:n]:
            cur.wait_stream(st)
        raise
    finally:
        ops.set_absmax_arena(prev)
        _ISSUING.release()
    return results


def n_streams(n: int, limit: int, device) -> int:
    """On how many streams does a pass over `n` images run?  At most `limit`, fewer for batches under limit x _SUBBATCH_MIN images, and
    ONE when that leaves no second sub-batch, when the batch is not on a device, and while the caller's stream is being captured into
    a hipGraph.  The one statement of the rule: every entry point of every plan asks here (plan.FusedPlan.n_streams)."""
    S = min(int(limit), n // _SUBBATCH_MIN)
    if S <= 1 or not _on_device(device) or torch.cuda.is_current_stream_capturing():
        return 1
    return S


def cuts(n: int, S: int):
    """the S + 1 bounds of the contiguous sub-batches of n images"""
    return [(n * i) // S for i in range(S + 1)]


class SideStreams:
    """The side streams and maxima arenas of ONE engine's sub-batch passes, per device, created on first use and grown on demand."""

    def __init__(self):
        self._side = {}

    def get(self, device, S):
        key = str(device)
        if key not in self._side or len(self._side[key][0]) < S:
            self._side[key] = ([torch.cuda.Stream(device=device) for _ in range(S)], [ops.AbsmaxArena() for _ in range(S)])
        return self._side[key]

    def run(self, device, n, limit, make_gen, arena, prepare):
        """Run the pass generator make_gen(lo, hi) over n images: once on the caller's stream under the engine's own `arena`, or for
        n_streams(n, limit, device) contiguous sub-batches on side streams, their launches issued interleaved (_interleave).  -> the
        list of the generators' results, one per sub-batch.
        `prepare()` brings everything the passes cache lazily -- refreshed layer plans, the attention-pool copies, the mean / std
        constants, the positional-embedding table -- up to date on the caller's stream, which every side stream then waits for: no
        sub-batch reads a cache another one is still producing.  The caller's stream waits for every side stream before
        this returns (or raises: _interleave), and every tensor of the results is recorded on it: those a side stream's pool allocated
        are read next on the caller's stream; for the others the allocator has nothing to do."""
        S = n_streams(n, limit, device)
        if S == 1:
            with ops.absmax_arena(arena, device):
                return [_drive(make_gen(0, n))]
        prepare()
        streams, arenas = self.get(device, S)
        cur = torch.cuda.current_stream()
        for st in streams[:S]:
            st.wait_stream(cur)
        b = cuts(n, S)
        outs = _interleave([make_gen(b[i], b[i + 1]) for i in range(S)], streams, arenas, device)
        for st in streams[:S]:
            cur.wait_stream(st)
        for o in outs:
            for t in (o.values() if isinstance(o, dict) else [o]):
                if torch.is_tensor(t):
                    _record_stream(t, cur)
        return outs


def detached(x):
    """the input batch as the passes read it: cut off any autograd graph, contiguous (ONE copy at most, ahead of the sub-batch cuts)"""
    x = x.detach()
    return x if x.is_contiguous() else x.contiguous()


def explanation_outputs(x, want_weights: bool):
    """The two image-sized results of explain() for the whole batch: the sub-batches write into slices of ONE pair of tensors -- no
    concatenation pass over [N, 6, H, W] behind the step (0.3 ms of a 17.4 ms ViT-Ti step at batch 512)."""
    N, _, H, W = x.shape
    return (torch.empty((N, 6, H, W), device=x.device, dtype=torch.float32) if want_weights else None,
            torch.empty((N, H, W), device=x.device, dtype=torch.float32))


def assemble_explanation(parts, outs=None):
    """The dictionary explain() returns from the results of its sub-batches: the per-image rows concatenated, the shared output pair
    `outs` attached.  A single pass that allocated its own outputs is handed back as it is."""
    if outs is None:
        (res,) = parts
        return res
    what = "functional_value" if "functional_value" in parts[0] else "explained_class_idx"
    res = {k: (parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts])) for k in ("logits", "prediction", what)}
    res.update(dynamic_linear_weights=outs[0], contribution_map=outs[1])
    return res


def explain_repeated(x, forward, make_args, backward, want_weights: bool):
    """ONE forward in explanation mode, then one input-gradient pass per argument: the dynamic weights of the forward do not depend on
    what is explained, so its state is kept and only the backward is repeated; the last pass consumes the state.
    forward() -> (logits, state); make_args(logits) -> the T per-pass arguments; backward(state, arg, consume) -> (weights, map).
    -> logits, contribution_maps [N, T, H, W] and, if requested, dynamic_linear_weights [N, T, 6, H, W]"""
    logits, st = forward()
    args = make_args(logits)
    N, T, (H, W) = x.shape[0], len(args), x.shape[2:]
    maps = torch.empty((N, T, H, W), device=x.device, dtype=torch.float32)
    wall = torch.empty((N, T, 6, H, W), device=x.device, dtype=torch.float32) if want_weights else None
    for k, arg in enumerate(args):
        wts, contrib = backward(st, arg, k == T - 1)
        maps[:, k] = contrib
        if want_weights:
            wall[:, k] = wts
    out = dict(logits=logits, contribution_maps=maps)
    if want_weights:
        out["dynamic_linear_weights"] = wall
    return out
