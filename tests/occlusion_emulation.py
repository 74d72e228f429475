"""CPU restatements of the two Occlusion entry points (TEST INFRASTRUCTURE, beside cpu_emulation.py): what include/bcos_hip.h documents
for bcos_prep_input_occluded and bcos_occlusion_accumulate, the float64 evaluation of the same formula, and the rounding bound of the
fp32 chain.  The `-m "not gpu"` tests monkeypatch bcos_hip.ops with the first two; the GPU tests judge the kernels against the rest."""
import numpy as np
import torch


def keep_masks(rects, H, W, dtype=torch.float32):
    """int [n, 4] rectangles -> [n, 1, H, W]: 0 inside rows [r0, r1) x columns [c0, c1), 1 outside (occlusion.py:44-50)"""
    r = torch.as_tensor(rects).long().cpu()
    m = torch.ones((r.shape[0], 1, H, W), dtype=dtype)
    for i, (r0, r1, c0, c1) in enumerate(r.tolist()):
        m[i, 0, r0:r1, c0:c1] = 0
    return m


def prep_input(x_nchw, mean6, std6, cpad=8):
    """bcos_prep_input for a 6-channel input: (x - mean) / std, NCHW -> NHWC, channels padded with zeros"""
    N, _, H, W = x_nchw.shape
    out = torch.zeros((N, H, W, cpad), dtype=torch.float32)
    out[..., :6] = ((x_nchw - mean6.view(1, 6, 1, 1)) / std6.view(1, 6, 1, 1)).permute(0, 2, 3, 1)
    return out


def prep_input_occluded(x_nchw, rects, mean6, std6, first=0, n=None, cpad=8, want_absmax=False):
    n = rects.shape[0] - first if n is None else n
    _, _, H, W = x_nchw.shape
    return prep_input(x_nchw * keep_masks(rects[first:first + n], H, W), mean6, std6, cpad)


def _select(org, pert, targets, dtype):
    org, pert = torch.as_tensor(org).reshape(-1).cpu().to(dtype).numpy(), torch.as_tensor(pert).cpu().to(dtype).numpy()
    if targets is not None:
        t = np.asarray(torch.as_tensor(targets).cpu()).reshape(-1)
        org, pert = org[t], pert[:, t]
    return org, pert


def occlusion_accumulate(org, pert, rects, H, W, targets=None, only_positive=False, rects_host=None):
    """the kernel's arithmetic in numpy float32: per element one chain over the covering masks in ascending m of fl(fl(org - pert) / n_part)"""
    o, p = _select(org, pert, targets, torch.float32)
    out = np.zeros((o.shape[0], H, W), dtype=np.float32)
    for m, (r0, r1, c0, c1) in enumerate(torch.as_tensor(rects).cpu().tolist()):
        if r0 >= r1 or c0 >= c1:
            raise ValueError("empty rectangle")
        d = o - p[m]
        if only_positive:
            d = np.where(d < 0, np.float32(0), d)
        term = (d / np.float32((r1 - r0) * (c1 - c0))).astype(np.float32)
        out[:, r0:r1, c0:c1] += term[:, None, None]
    return torch.from_numpy(out)


def formula64(org, pert, rects, H, W, targets=None, only_positive=False):
    """-> (sum_m [pixel in rect_m] d / n_part, sum_m [pixel in rect_m] |d / n_part|, covering masks per pixel) in float64 from the given logits"""
    o, p = _select(org, pert, targets, torch.float64)
    out = np.zeros((o.shape[0], H, W))
    mag = np.zeros_like(out)
    cover = np.zeros((H, W), dtype=np.int64)
    for m, (r0, r1, c0, c1) in enumerate(torch.as_tensor(rects).cpu().tolist()):
        d = o - p[m]
        if only_positive:
            d = np.maximum(d, 0.0)
        term = d / float((r1 - r0) * (c1 - c0))
        out[:, r0:r1, c0:c1] += term[:, None, None]
        mag[:, r0:r1, c0:c1] += np.abs(term)[:, None, None]
        cover[r0:r1, c0:c1] += 1
    return torch.from_numpy(out), torch.from_numpy(mag), torch.from_numpy(cover)


def chain_bound(mag, cover):
    """|fp32 chain - exact| <= (k + 2) 2^-24 sum |d / n_part| for a pixel under k masks: one rounding each for the subtraction and the
    division of every term and k - 1 additions whose partial sums are bounded by the sum of magnitudes (first order in 2^-24)"""
    return (cover.double() + 2.0)[None] * 2.0 ** -24 * mag
