"""Pixel-perturbation (deletion) curves on the fused engines -- the second quantitative evaluation of the B-cos papers beside the grid
pointing game (bcos_hip/localisation.py).

An image's pixels are ranked by their attribution; for K removal levels the first k_j pixels of the ranking are removed -- all six
channels of the [r,g,b,1-r,1-g,1-b] network input set to 0, as inside an Occlusion rectangle -- and the explained class's score is
recorded.  The ranking (key32 / key64 / thr(k), ties by ascending pixel index) is defined once, in include/bcos_hip.h.  With a fused
engine attached the B * K perturbed copies are never built: ops.perturb_select finds every image's K thresholds in one call,
`engine.forward(x, perturb=plan)` prepares the copies from the source images (bcos_prep_input_perturbed), and ops.class_scores reads
the class's score out of logits that stay on the device.  Without an engine the copies are materialised with torch ops from the same
thresholds and run through the module; select and scores are the same kernels.
"""
import math
from typing import Dict, Optional

import torch

from . import ops

__all__ = ["PerturbPlan", "removed_pixels", "materialise", "removal_counts", "pixel_perturbation", "DEFAULT_FRACTIONS"]

DEFAULT_FRACTIONS = tuple(i * 0.025 for i in range(11))       # 0, 2.5 %, ..., 25 % of the pixels


class PerturbPlan:
    """What `engine.forward(x, perturb=plan)` needs of a ranking: scores [B, H*W] (float32), thr [B, K] (int64 holding the uint64
    thresholds ops.perturb_select returned for these scores) and the order they were selected in."""

    def __init__(self, scores: torch.Tensor, thr: torch.Tensor, descending: bool = False):
        self.scores, self.thr, self.descending, self.K = scores, thr, bool(descending), int(thr.shape[1])

    def images(self, lo: int, hi: int) -> "PerturbPlan":
        return PerturbPlan(self.scores[lo:hi], self.thr[lo:hi], self.descending)


def removed_pixels(scores: torch.Tensor, thr: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """-> bool [B, K, H*W]: is pixel p of image b removed in copy j, i.e. key64_b(p) < thr[b, j] as unsigned 64-bit numbers
    (include/bcos_hip.h), from torch ops on the tensors' device"""
    B, HW = scores.shape
    bits = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = bits ^ torch.where(bits >> 31 != 0, 0xFFFFFFFF, 0x80000000)
    if descending:
        key = key ^ 0xFFFFFFFF
    hi, lo = (thr >> 32) & 0xFFFFFFFF, thr & 0xFFFFFFFF          # (an arithmetic shift: the mask drops the sign's copies)
    p = torch.arange(HW, device=scores.device, dtype=torch.int64)
    key = key[:, None, :]
    return (key < hi[:, :, None]) | ((key == hi[:, :, None]) & (p[None, None, :] < lo[:, :, None]))


def materialise(x: torch.Tensor, scores: torch.Tensor, thr: torch.Tensor, descending: bool = False) -> torch.Tensor:
    """-> [B * K, 6, H, W], image-major: the perturbed copies as tensors (what the fused engines never build)"""
    B, Cx, H, W = x.shape
    gone = removed_pixels(scores, thr, descending).view(B, -1, 1, H, W)
    return torch.where(gone, torch.zeros((), dtype=x.dtype, device=x.device), x[:, None]).reshape(-1, Cx, H, W)


def removal_counts(fractions, HW: int):
    """k_j = floor(f_j * HW + 0.5) in Python integers"""
    fr = [float(f) for f in fractions]
    if not fr or any(not (0.0 <= f <= 1.0) for f in fr):
        raise ValueError(f"pixel_perturbation: fractions are numbers in [0, 1], got {list(fractions)}")
    return [min(HW, int(math.floor(f * HW + 0.5))) for f in fr]


def _resolve(engine_or_model):
    """-> (engine or None, module or None): the fused path is taken with an engine that is attached and whose module is in eval mode"""
    if isinstance(engine_or_model, torch.nn.Module):
        model = engine_or_model
        engine = getattr(model, "_bcos_engine", None)
        if engine is not None and (getattr(model, "training", False) or not hasattr(engine, "forward")):
            engine = None
        return engine, model
    return engine_or_model, None


@torch.no_grad()
def pixel_perturbation(engine_or_model, x: torch.Tensor, targets=None, *, attributions: Optional[torch.Tensor] = None, explainer=None,
                       fractions=DEFAULT_FRACTIONS, order: str = "least", score: str = "logit",
                       copies_per_call: int = 256) -> Dict[str, object]:
    """x [B, 6, H, W], targets [B] (default: the predicted classes) ->
        curves      [B, K] on x's device: the score of image b's class with the first counts[j] pixels of its ranking removed,
        counts      the K removal counts k_j = floor(f_j * H*W + 0.5),
        fractions   the K fractions as given,
        targets     [B] int64, the explained classes,
        thresholds  [B, K] int64: the uint64 thresholds of the ranking (ops.perturb_select).
    The pixel scores come from `attributions` ([B, H, W], or [B, C, H, W] summed over the channels), from
    `explainer.attribute(img, target).sum(1)` per image (any explainer of interpretability.explanation_methods, as
    localisation.grid_pointing_game takes one), or by default from the contribution maps of `engine.explain(x, targets)`.
    order = "least": the least important pixels go first; "most": deletion of the most important first.  Ties break by ascending
    pixel index in either order.  The INSERTION game is order = "least" with the counts H*W - k: what is left of the image are its k most
    important pixels.  score: "logit", "sigmoid" (BcosMixin.to_probabilities) or "softmax".
    Each engine call carries max(1, copies_per_call // K) images; the result does not depend on it.  Without an attached engine, or in
    train() mode, the copies are materialised with torch ops from the same thresholds and run through the module."""
    if order not in ("least", "most"):
        raise ValueError(f"pixel_perturbation: order must be 'least' or 'most', got {order!r}")
    if score not in ops.CLASS_SCORE_MODES:
        raise ValueError(f"pixel_perturbation: score must be one of {sorted(ops.CLASS_SCORE_MODES)}, got {score!r}")
    if x.dim() != 4 or x.shape[1] != 6:
        raise ValueError(f"pixel_perturbation: expected 6-channel images [B,6,H,W] (pixels are removed from the network input), got {tuple(x.shape)}")
    engine, model = _resolve(engine_or_model)
    run = engine.forward if engine is not None else model
    x = x.detach().contiguous()
    B, _, H, W = x.shape
    HW = H * W
    descending = order == "most"
    counts = removal_counts(fractions, HW)
    K = len(counts)

    tg, maps = None, None
    if targets is not None:
        tg = torch.as_tensor(targets).reshape(-1).to(torch.int64)
        if tg.numel() == 1 and B > 1:
            tg = tg.expand(B)
        if tg.numel() != B:
            raise ValueError(f"pixel_perturbation: need one target per image: got {tg.numel()} targets for {B} images")
    if attributions is not None:
        maps = attributions.sum(1) if attributions.dim() == 4 else attributions
    elif explainer is None:
        if engine is None or not hasattr(engine, "explain"):
            raise ValueError("pixel_perturbation: without a fused engine the pixel scores come from `attributions` or an `explainer`")
        res = engine.explain(x, tg, want_weights=False)
        maps = res["contribution_map"]
        if tg is None:
            tg = res["explained_class_idx"].reshape(-1).to(torch.int64)
    if tg is None:                                               # the predicted classes
        tg = torch.cat([run(x[lo:lo + max(1, copies_per_call)]).detach().argmax(1) for lo in range(0, B, max(1, copies_per_call))])
    checked = targets is None                                    # (predicted classes are indices of the logits already)
    if maps is None and not checked:                             # an explainer never sees an index the logits do not have
        tg, checked = ops.check_targets(tg, int(run(x[:1]).shape[1]), "pixel_perturbation: targets"), True
    tg = tg.to(x.device)
    if maps is None:
        maps = torch.cat([explainer.attribute(x[b:b + 1], int(t)).sum(1) for b, t in enumerate(tg.tolist())])
    if tuple(maps.shape) != (B, H, W):
        raise ValueError(f"pixel_perturbation: attributions {tuple(maps.shape)} for images {tuple(x.shape)}: expected [{B}, {H}, {W}]")
    scores = maps.detach().to(device=x.device, dtype=torch.float32).reshape(B, HW).contiguous()

    thr = ops.perturb_select(scores, counts, descending=descending)
    plan = PerturbPlan(scores, thr, descending)
    tg32 = tg.to(torch.int32) if checked else None               # (otherwise validated against the first logits below)
    curves = torch.empty((B, K), device=x.device, dtype=torch.float32)
    step = max(1, int(copies_per_call) // K)
    for lo in range(0, B, step):
        hi = min(B, lo + step)
        if engine is not None:
            out = engine.forward(x[lo:hi], perturb=plan.images(lo, hi))
        else:
            out = model(materialise(x[lo:hi], scores[lo:hi], thr[lo:hi], descending)).detach()
        if out.dim() != 2 or out.shape[0] != (hi - lo) * K:
            raise ValueError(f"pixel_perturbation: the model must map {(hi - lo) * K} images to [{(hi - lo) * K}, classes], got {tuple(out.shape)}")
        if tg32 is None:                                         # IndexError like the reference's out[0, idx]; negative indices wrap
            tg = ops.check_targets(tg, out.shape[1], "pixel_perturbation: targets").to(x.device)
            tg32 = tg.to(torch.int32)
        curves[lo:hi] = ops.class_scores(out.float().contiguous(), tg32[lo:hi], group=K, mode=score).view(hi - lo, K)
    return dict(curves=curves, counts=counts, fractions=[float(f) for f in fractions], targets=tg, thresholds=thr)
