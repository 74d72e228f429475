"""CPU restatements of the pixel-perturbation entry points (TEST INFRASTRUCTURE, beside occlusion_emulation.py): what include/bcos_hip.h
documents for bcos_perturb_select, bcos_prep_input_perturbed and bcos_class_scores -- the ranking through a stable numpy sort of the
key32 values -- the float64 evaluation of sigmoid and softmax, and the header's rounding bounds as formulas of the INPUTS.  The
`-m "not gpu"` tests monkeypatch bcos_hip.ops with the first three; the GPU tests judge the kernels against all of it."""
import math

import numpy as np
import torch

import occlusion_emulation as OE

U = 2.0 ** -24
TINY = 2.0 ** -126
UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def key32(scores, descending=False):
    """m(s) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000), complemented for "most important first"; -> uint32 array of scores' shape"""
    bits = np.ascontiguousarray(torch.as_tensor(scores).detach().cpu().numpy().astype(np.float32, copy=False)).view(np.uint32)
    m = bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)
    return ~m if descending else m


def thresholds(scores, counts, descending=False):
    """-> uint64 [B, K]: thr_b(k) = key64 of the k-th pixel of a STABLE sort by key32 (ties keep ascending p), UINT64_MAX for k = HW"""
    keys = key32(scores, descending)
    B, HW = keys.shape
    out = np.empty((B, len(counts)), dtype=np.uint64)
    for b in range(B):
        order = np.argsort(keys[b], kind="stable")
        for j, k in enumerate(counts):
            if not 0 <= k <= HW:
                raise ValueError("count outside [0, HW]")
            out[b, j] = UINT64_MAX if k == HW else (np.uint64(keys[b, order[k]]) << np.uint64(32)) | np.uint64(order[k])
    return out


def perturb_select(scores, counts, descending=False):
    """ops.perturb_select: the thresholds as an int64 tensor holding the uint64 bit patterns"""
    return torch.from_numpy(thresholds(scores, [int(k) for k in counts], descending).view(np.int64))


def removed(scores, thr, descending=False):
    """-> bool array [B, K, HW]: key64_b(p) < thr[b, j] as unsigned numbers"""
    keys = key32(scores, descending).astype(np.uint64)
    B, HW = keys.shape
    key64 = (keys << np.uint64(32)) | np.arange(HW, dtype=np.uint64)[None]
    t = np.ascontiguousarray(torch.as_tensor(thr).detach().cpu().numpy()).view(np.uint64)
    return key64[:, None, :] < t[:, :, None]


def materialise(x, scores, thr, descending=False):
    """-> [B * K, 6, H, W], image-major: image b with the removed pixels of copy j set to 0 in every channel"""
    x = torch.as_tensor(x).detach().cpu()
    B, Cx, H, W = x.shape
    gone = torch.from_numpy(removed(scores, thr, descending)).view(B, -1, 1, H, W)
    return torch.where(gone, torch.zeros((), dtype=x.dtype), x[:, None]).reshape(-1, Cx, H, W).contiguous()


def prep_input_perturbed(x_nchw, scores, thr, mean6, std6, descending=False, first=0, n=None, cpad=8, want_absmax=False):
    copies = materialise(x_nchw, scores, thr, descending)
    n = copies.shape[0] - first if n is None else n
    return OE.prep_input(copies[first:first + n], torch.as_tensor(mean6).cpu(), torch.as_tensor(std6).cpu(), cpad)


def _rows(logits, targets, group, dtype):
    x = torch.as_tensor(logits).detach().cpu().to(dtype)
    t = torch.as_tensor(targets).detach().cpu().reshape(-1).long().repeat_interleave(int(group))
    assert t.numel() == x.shape[0]
    return x, t


def class_scores(logits, targets, group=1, mode="logit"):
    """ops.class_scores in torch float32 (the logit exactly; sigmoid and softmax to fp32 accuracy, not to the kernel's bits)"""
    x, t = _rows(logits, targets, group, torch.float32)
    if mode == "logit":
        return x.gather(1, t[:, None])[:, 0]
    return class_scores64(logits, targets, group, mode).float()


def class_scores64(logits, targets, group=1, mode="logit"):
    x, t = _rows(logits, targets, group, torch.float64)
    xt = x.gather(1, t[:, None])[:, 0]
    if mode == "logit":
        return xt
    if mode == "sigmoid":
        return torch.sigmoid(xt)
    return torch.exp(xt - torch.logsumexp(x, dim=1))


def sigmoid_bound(logits, targets, group=1):
    """include/bcos_hip.h, mode 1: |out - sigma(x_t)| <= 6 u sigma(x_t) + 2^-126"""
    return 6 * U * class_scores64(logits, targets, group, "sigmoid") + TINY


def softmax_bound(logits, targets, group=1):
    """include/bcos_hip.h, mode 2: |out - p| <= (|x_t - M| + D + ceil(CL / 64) + 12) u p + 2^-126, D = sum_c softmax_c |x_c - M|"""
    x, t = _rows(logits, targets, group, torch.float64)
    M = x.amax(1, keepdim=True)
    soft = torch.softmax(x, dim=1)
    D = (soft * (x - M).abs()).sum(1)
    dt = (x.gather(1, t[:, None]) - M).abs()[:, 0]
    return (dt + D + math.ceil(x.shape[1] / 64) + 12) * U * class_scores64(logits, targets, group, "softmax") + TINY
