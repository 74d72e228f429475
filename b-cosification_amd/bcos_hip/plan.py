"""What the fused plans share: the base class `FusedPlan` of engine.ResNetEngine, vit_engine.ViTEngine and densenet_engine.DenseNetEngine,
and the input sources their forward generators read.

A plan supplies its topology and nothing else: `_run_forward_gen(src, keep, gates=None)`, `_backward_gen(x, st, cls, want_weights,
consume, outs=None, functional=None, g_head=None)`, `n_logits()`, `_ensure_fresh()` / `refresh()`, and the hooks below where the plans
truly differ.  The base owns the per-engine state (mean / std constants, maxima arena, side streams, logit bias / temperature), how a
pass is handed to the scheduler (bcos_hip/passes.py) and every entry point: forward(), explain() and the two repeated-backward ones.

The repeated entry points live here under private names; a plan that offers one binds the public name in its class body
(`explain_targets = FusedPlan._explain_targets`), because callers ask `hasattr(engine, "explain_targets")`.
"""
import contextlib
import copy
from typing import Dict, Optional

import torch

from . import ops, passes
from .functional import LogitFunctional, as_functional
from .passes import _SUBBATCH_STREAMS, _drive


class Images:
    """The input of a forward pass: the batch x itself.  Every source holds the images `x` its prepared input is made from, the number
    `n` of images the plan then runs and `add_inverse`; cut(lo, hi) is the source of the sub-batch [lo, hi) of those n, and
    prepare(mean, std, want_absmax) its normalised NHWC input."""

    def __init__(self, x):
        if x.dim() != 4 or x.shape[1] not in (3, 6):
            raise ValueError(f"expected [N,6,H,W] (or [N,3,H,W] to be AddInverse-encoded), got {tuple(x.shape)}")
        self.x = passes.detached(x)      # cut off any autograd graph, contiguous: ONE copy at most, ahead of the sub-batch cuts
        self.n, self.add_inverse = x.shape[0], x.shape[1] == 3

    def cut(self, lo, hi):
        part = copy.copy(self)
        part.x, part.n = self.x[lo:hi], hi - lo
        return part

    def prepare(self, mean, std, want_absmax):
        return ops.prep_input(self.x, mean, std, cpad=8, add_inverse=self.add_inverse, want_absmax=want_absmax)


class OccludedCopies(Images):
    """forward(x, occlude=rects): the n copies `x * mask_i` of the ONE 6-channel device image x, rects a device bank [n, 4] of int32
    rectangles (include/bcos_hip.h).  The copies are never built: ops.prep_input_occluded prepares them from x and the bank."""
    add_inverse = False

    def __init__(self, x, rects):
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 6:
            raise ValueError(f"forward(x, occlude=...): expected ONE 6-channel image [1,6,H,W] (the masks multiply the network input; "
                             f"masking before AddInverse is a different operator), got {tuple(x.shape)}")
        ops.require_device(x, "bcos_hip.engine")
        if not (torch.is_tensor(rects) and rects.device == x.device and rects.dtype == torch.int32 and rects.dim() == 2      # (x is on a device)
                and rects.shape[1] == 4 and rects.is_contiguous() and rects.shape[0] > 0):
            raise ValueError("forward(x, occlude=...): the mask bank is a contiguous int32 tensor [n, 4] of rectangles on the image's device")
        self.x, self.rects, self.first, self.n = passes.detached(x), rects, 0, rects.shape[0]

    def cut(self, lo, hi):
        part = copy.copy(self)
        part.first, part.n = self.first + lo, hi - lo
        return part

    def prepare(self, mean, std, want_absmax):
        return ops.prep_input_occluded(self.x, self.rects, mean, std, first=self.first, n=self.n, cpad=8, want_absmax=want_absmax)


class PerturbedCopies(OccludedCopies):
    """forward(x, perturb=plan): the B * K copies, image-major, of the 6-channel device images x [B,6,H,W] with the first k_j pixels of
    every image's ranking removed; plan a bcos_hip.perturbation.PerturbPlan (scores [B, H*W], thr [B, K], descending, K) on their
    device.  Prepared by ops.prep_input_perturbed, cut along the copy index."""

    def __init__(self, x, plan):
        if x.dim() != 4 or x.shape[1] != 6:
            raise ValueError(f"forward(x, perturb=...): expected 6-channel images [B,6,H,W] (pixels are removed from the network input; "
                             f"masking before AddInverse is a different operator), got {tuple(x.shape)}")
        ops.require_device(x, "bcos_hip.engine")
        B, _, H, W = x.shape
        scores, thr, K = getattr(plan, "scores", None), getattr(plan, "thr", None), getattr(plan, "K", None)
        if not (torch.is_tensor(scores) and scores.device == x.device and scores.dtype == torch.float32 and tuple(scores.shape) == (B, H * W)
                and scores.is_contiguous() and torch.is_tensor(thr) and thr.device == x.device and thr.dtype == torch.int64
                and isinstance(K, int) and K > 0 and tuple(thr.shape) == (B, K) and thr.is_contiguous() and hasattr(plan, "descending")):
            raise ValueError("forward(x, perturb=...): the plan holds contiguous scores [B, H*W] (float32) and thr [B, K] (int64, from "
                             "ops.perturb_select) on the images' device, `descending` and K")
        self.x, self.plan, self.first, self.n = passes.detached(x), plan, 0, B * K

    def prepare(self, mean, std, want_absmax):
        return ops.prep_input_perturbed(self.x, self.plan.scores, self.plan.thr, mean, std, descending=self.plan.descending,
                                        first=self.first, n=self.n, cpad=8, want_absmax=want_absmax)


class RiseCopies(OccludedCopies):
    """forward(x, rise=bank): the n copies `x * m_i` of the ONE 6-channel device image x under the RISE masks of bank, an ops.RiseBank
    (`rows`: a device int32 tensor [n, 4] of (bits_lo, bits_hi, shift_r, shift_c), and the grid side `s`; include/bcos_hip.h).  Neither
    the masks nor the copies are built: ops.prep_input_rise prepares the input from x and the bank.  Cut along the copy index."""

    def __init__(self, x, bank):
        if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 6:
            raise ValueError(f"forward(x, rise=...): expected ONE 6-channel image [1,6,H,W] (the masks multiply the network input; "
                             f"masking before AddInverse is a different operator), got {tuple(x.shape)}")
        ops.require_device(x, "bcos_hip.engine")
        rows, s = getattr(bank, "rows", None), getattr(bank, "s", None)
        if not (torch.is_tensor(rows) and rows.device == x.device and rows.dtype == torch.int32 and rows.dim() == 2      # (x is on a device)
                and rows.shape[1] == 4 and rows.is_contiguous() and rows.shape[0] > 0 and isinstance(s, int) and 2 <= s <= 8):
            raise ValueError("forward(x, rise=...): the mask bank is an ops.RiseBank: contiguous int32 rows [n, 4] of (bits_lo, bits_hi, "
                             "shift_r, shift_c) on the image's device, and the grid side s in 2..8")
        self.x, self.bank, self.first, self.n = passes.detached(x), bank, 0, rows.shape[0]

    def prepare(self, mean, std, want_absmax):
        return ops.prep_input_rise(self.x, self.bank, mean, std, first=self.first, n=self.n, cpad=8, want_absmax=want_absmax)


def input_source(x, occlude=None, perturb=None, rise=None):
    """the source forward(x, occlude=..., perturb=..., rise=...) reads, validated on the host before anything else happens"""
    if occlude is not None and perturb is not None and rise is None:
        raise ValueError("forward(x, occlude=..., perturb=...): one of the two at a time")
    if rise is not None:
        if occlude is not None or perturb is not None:
            raise ValueError("forward(x, occlude=..., perturb=..., rise=...): one of the three at a time")
        return RiseCopies(x, rise)
    if perturb is not None:
        return PerturbedCopies(x, perturb)
    return Images(x) if occlude is None else OccludedCopies(x, occlude)


class FusedPlan:
    """Base of the launch plans: per-engine state, pass plumbing and the entry points (see the module docstring)."""
    who = "engine"                       # how the plan names itself in its messages

    def __init__(self, net, subbatch_streams=_SUBBATCH_STREAMS):
        self.net = net
        norm = getattr(net, "bcosifynormalize", None)
        # (a native B-cos network takes the 6-channel image as it is: mean 0 / std 1 leave every value's bits alone)
        self._mean, self._std = (tuple(norm.mean), tuple(norm.std)) if norm is not None else ((0.0,) * 6, (1.0,) * 6)
        self._dev_consts = {}
        ll = net.logit_layer
        self.logit_bias = ll.logit_bias if ll is not None else None
        self.logit_temperature = ll.logit_temperature if ll is not None else None
        self._absmax_arena = ops.AbsmaxArena()      # per-pixel / per-row operand maxima of one pass: one zero fill instead of one per tensor
        self.subbatch_streams = subbatch_streams    # 1 = every pass on the caller's stream
        self._side = passes.SideStreams()           # (streams, arenas) of the sub-batch passes, created on first use

    # ---------------------------------------------------------------------------------------------- hooks
    def _stream_limit(self, cotangent=None) -> int:
        return self.subbatch_streams

    def _pass_context(self):
        """what every pass of the plan is issued under"""
        return contextlib.nullcontext()

    def _prepare_extra(self, x):
        """whatever else the passes over the images x cache lazily (see _prepare)"""

    def _check_targets(self, targets, logits=None):
        """class indices range-checked on the host (IndexError like the reference's out[0, idx]; negative indices wrap; None stays
        None): called before any launch (`logits` None) and again behind the forward, for a head whose width is known only then"""
        return ops.check_targets(targets, self.n_logits()) if logits is None else targets

    # ---------------------------------------------------------------------------------------------- state and pass plumbing
    def _consts(self, device):
        key = str(device)
        if key not in self._dev_consts:
            self._dev_consts[key] = (torch.tensor(self._mean, dtype=torch.float32, device=device),
                                     torch.tensor(self._std, dtype=torch.float32, device=device))
            ops.publish_cached(self._dev_consts[key][1])
        return self._dev_consts[key]

    def _prepare(self, x):
        """everything the passes cache lazily, brought up to date on the current stream (passes.SideStreams.run)"""
        self._ensure_fresh()
        self._consts(x.device)
        self._prepare_extra(x)

    def _passes(self, x, n, make_gen, cotangent=None):
        """make_gen(lo, hi) over n images as sub-batches on side streams, or once on the caller's (bcos_hip/passes.py: images are
        independent, the sub-batches fill each other's launch tails)"""
        with self._pass_context():
            return self._side.run(x.device, n, self._stream_limit(cotangent), make_gen, self._absmax_arena, lambda: self._prepare(x))

    def n_streams(self, x, cotangent=None) -> int:
        """On how many sub-batch streams does explain(x, ...) run?  `subbatch_streams` for a batch of at least that many times
        _SUBBATCH_MIN images on a device -- replayed `gates` included: they are cut along the batch like the images -- and ONE where
        _stream_limit says so or a pass is being captured into a hipGraph.  Results do not depend on the answer: an image's bits are a
        function of the image alone."""
        return passes.n_streams(x.shape[0], self._stream_limit(cotangent), x.device)

    def _begin(self, src, want_absmax=True, prepare=True):
        """head of every forward generator: the plan brought up to date, then -> (images, prepared NHWC input) of the source
        (`prepare` = False: None in its place -- the caller's first launch reads the images themselves)"""
        ops.require_device(src.x, type(self).__module__)
        self._ensure_fresh()
        mean, std = self._consts(src.x.device)
        return src.x, (src.prepare(mean, std, want_absmax) if prepare else None)

    def _run_forward(self, x, keep, gates=None):
        return _drive(self._run_forward_gen(Images(x), keep, gates))

    # ---------------------------------------------------------------------------------------------- entry points
    @torch.no_grad()
    def forward(self, x: torch.Tensor, occlude: Optional[torch.Tensor] = None, perturb=None, rise=None) -> torch.Tensor:
        """The head output of the batch x.
        `occlude` (a device bank [n, 4] of int32 rectangles, include/bcos_hip.h): x is ONE 6-channel image [1, 6, H, W] and the result
        the head output [n, ...] of its n occluded copies `x * mask_i` (occlusion.py:80-90) -- the copies are never built: the prepared
        input comes from ops.prep_input_occluded, everything behind it is the plan of an n-image batch, sub-batch streams included.
        `perturb` (bcos_hip.perturbation.PerturbPlan: scores [B, H*W], thr [B, K], descending, K): x is [B, 6, H, W] and the result the
        head output [B * K, ...], image-major, of the copies with the first k_j pixels of every image's ranking removed -- prepared by
        ops.prep_input_perturbed, then the plan of a B * K-image batch, cut along the copy index.
        `rise` (ops.RiseBank: device rows [n, 4] and the grid side s): x is ONE 6-channel image and the result the head output [n, ...]
        of its copies `x * m_i` under the bank's RISE masks (rise.py:79-88) -- prepared by ops.prep_input_rise from the image and the
        four integers of every mask, then the plan of an n-image batch.  At most one of the three."""
        src = input_source(x, occlude, perturb, rise)

        def one(lo, hi):
            return (yield from self._run_forward_gen(src.cut(lo, hi), keep=False))[0]
        parts = self._passes(src.x, src.n, one)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    @torch.no_grad()
    def explain(self, x: torch.Tensor, targets: Optional[torch.Tensor] = None, want_weights: bool = True,
                gates=None, cotangent=None, functional: Optional[LogitFunctional] = None) -> Dict[str, torch.Tensor]:
        """Forward in explanation mode + input-gradient pass of the explained logit of every image
        (batched bcos/common.py:163-181).  `targets` [N] int64 selects the logits (default: arg-max).
        `gates` (ResNet plan): optional list of NHWC 0/1 tensors, one per ReLU in execution order, that REPLACE the v > 0
        decisions (replay of gates recorded elsewhere; used by the gate-pinned parity test).
        `cotangent` (attention-pool heads): a callable that receives the head output -- the embeddings [N, D], or [(HW), N, D']
        for an `attn_unpool` head -- and returns d(scalar to explain) / d(head output) of the same shape; the input-gradient
        pass then starts from it instead of from a one-hot coordinate (the zero-shot text logit of
        interpretability/analyses/text_localisation.py:68-126: bcos_hip.clip_head.zeroshot_attribution).
        `functional` (bcos_hip.functional.LogitFunctional, instead of `targets`): explain a linear functional sum_k c_k y_k of the logits --
        a contrast y_a - y_b, the mean-corrected y_t - mean_k y_k -- at the cost of one ordinary pass (the network is linear in the head
        cotangent); the result carries `functional_value` [N] (sum_k c_k logit_k) in place of `explained_class_idx`."""
        functional = self._checked_functional(x, functional, targets, cotangent)
        targets = self._check_targets(targets)
        src = Images(x)
        x, outs = src.x, None
        if self.n_streams(x, cotangent=cotangent) > 1:
            # sub-batches write into ONE set of output tensors and read ONE device copy of the targets; a single pass allocates its
            # outputs and moves its targets behind its forward
            outs = passes.explanation_outputs(x, want_weights)
            targets = None if targets is None else targets.to(device=x.device, dtype=torch.int64).contiguous()

        def one(lo, hi):
            cut = lambda t: None if t is None else t[lo:hi]      # noqa: E731
            return self._explain_gen(src.cut(lo, hi), cut(targets), want_weights,
                                     None if gates is None else [gt[lo:hi] for gt in gates],       # (replayed ReLU decisions: [N, ...] like the activations)
                                     cotangent, outs=None if outs is None else (cut(outs[0]), outs[1][lo:hi]),
                                     functional=None if functional is None else functional[lo:hi].to(x.device))
        return passes.assemble_explanation(self._passes(x, src.n, one, cotangent), outs)

    def _explain_gen(self, src, targets, want_weights, gates, cotangent, outs=None, functional=None):
        """forward + input-gradient pass of one (sub-)batch as a generator (yields behind every block of either pass); the caller owns
        the stream and the maxima arena the launches are issued under"""
        logits, st = yield from self._run_forward_gen(src, keep=True, gates=gates)
        x = src.x
        if cotangent is not None:
            g_head = cotangent(logits)
            if tuple(g_head.shape) != tuple(logits.shape):
                raise ValueError(f"cotangent: expected shape {tuple(logits.shape)}, got {tuple(g_head.shape)}")
            wts, contrib = yield from self._backward_gen(x, st, None, want_weights, True, outs, g_head=g_head)
            return dict(logits=logits, embedding=logits, dynamic_linear_weights=wts, contribution_map=contrib)
        targets = self._check_targets(targets, logits)
        pred, _ = ops.argmax_rows(logits)
        if functional is not None:
            wts, contrib = yield from self._backward_gen(x, st, None, want_weights, True, outs, functional)
            return dict(logits=logits, prediction=pred, functional_value=functional.value(logits), dynamic_linear_weights=wts,
                        contribution_map=contrib)
        cls = pred if targets is None else targets.to(device=logits.device, dtype=torch.int64).contiguous()
        wts, contrib = yield from self._backward_gen(x, st, cls, want_weights, True, outs)
        return dict(logits=logits, prediction=pred, explained_class_idx=cls, dynamic_linear_weights=wts,
                    contribution_map=contrib)

    def _checked_functional(self, x, functional, targets=None, cotangent=None):
        """a `functional` argument validated on the host before any launch and moved to x's device (None stays None)"""
        functional = as_functional(functional)
        if functional is None:
            return None
        if targets is not None or cotangent is not None:
            raise ValueError(f"{self.who}: `functional` replaces `targets` / `cotangent`: pass one of them")
        return functional.checked(x.shape[0], self.n_logits()).to(x.device)

    def _explain_repeated(self, x, make_args, backward_gen, want_weights):
        """ONE forward in explanation mode over the detached batch x, then backward_gen(st, arg, last) for every argument of
        make_args(logits) (passes.explain_repeated)"""
        with self._pass_context(), ops.absmax_arena(self._absmax_arena, x.device):
            return passes.explain_repeated(x, lambda: self._run_forward(x, keep=True), make_args,
                                           lambda st, arg, last: _drive(backward_gen(st, arg, last)), want_weights)

    @torch.no_grad()
    def _explain_targets(self, x: torch.Tensor, targets: torch.Tensor, want_weights: bool = False) -> Dict[str, torch.Tensor]:
        """ONE forward in explanation mode, then one input-gradient pass per target column: `targets` [N, T] (or [T],
        shared by all images).  The reference's `attribute_selection` (interpretability/explanation_methods/utils.py:84-99,
        bcos/common.py:319-344) re-runs the forward for every target; the dynamic weights of the forward do not depend on
        the explained logit, so they are kept and only the backward is repeated.
        Returns logits [N,K], contribution_maps [N,T,H,W] and, if requested, dynamic_linear_weights [N,T,6,H,W]."""
        targets = self._check_targets(targets)
        x = passes.detached(x)

        def columns(logits):
            tg = self._check_targets(targets, logits).to(device=logits.device, dtype=torch.int64)
            return (tg.view(1, -1).expand(x.shape[0], -1) if tg.dim() == 1 else tg).unbind(1)
        return self._explain_repeated(x, columns, lambda st, cls, last: self._backward_gen(x, st, cls.contiguous(), want_weights, last), want_weights)

    @torch.no_grad()
    def _explain_functionals(self, x: torch.Tensor, functionals, want_weights: bool = False) -> Dict[str, torch.Tensor]:
        """ONE forward in explanation mode, then one input-gradient pass per LogitFunctional of `functionals` (each over the whole
        batch) -- explain_targets for functionals: the kept forward does not depend on what is explained.
        Returns logits [N, K], functional_values [N, T], contribution_maps [N, T, H, W] and, if requested, dynamic_linear_weights
        [N, T, 6, H, W]."""
        x = passes.detached(x)
        fs = [self._checked_functional(x, f) for f in functionals]
        if not fs or any(f is None for f in fs):
            raise ValueError("explain_functionals: a non-empty list of LogitFunctional objects")
        out = self._explain_repeated(x, lambda logits: fs, lambda st, f, last: self._backward_gen(x, st, None, want_weights, last, functional=f),
                                     want_weights)
        out["functional_values"] = torch.stack([f.value(out["logits"]) for f in fs], 1)
        return out


def attach(net, cls):
    """Compile `net` into the launch plan `cls` and make `net(x)` (under no_grad, eval mode) and `net.explain_batch(x)` use it.  Raises
    BcosHipError, with the reason, for a network outside the plan's scope.  Call `net._bcos_engine.refresh()` after changing
    parameters through `.data`."""
    eng = cls(net)
    object.__setattr__(net, "_bcos_engine", eng)
    return eng


def detach(net):
    if hasattr(net, "_bcos_engine"):
        object.__delattr__(net, "_bcos_engine")
