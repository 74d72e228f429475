"""CPU restatements of the three RISE entry points (TEST INFRASTRUCTURE, beside occlusion_emulation.py): the mask of include/bcos_hip.h
("RISE baseline explainer") and the summation order of bcos_rise_accumulate in numpy float32, one rounding per operation as the kernels
(no fused multiply-add), plus the float64 evaluation and the rounding bound the GPU test holds the accumulate kernel to.  The
`-m "not gpu"` tests monkeypatch bcos_hip.ops with rise_masks / prep_input_rise / rise_accumulate / class_scores; the GPU tests compare
the kernels with them bit for bit."""
import numpy as np
import torch

import occlusion_emulation as OE

F32 = np.float32


def pack_rows(grid, shifts):
    """bool grids [n, s, s] and shifts [n, 2] -> int32 bank rows [n, 4] (bits_lo, bits_hi, shift_r, shift_c)"""
    n, s, _ = grid.shape
    rows = np.zeros((n, 4), dtype=np.int64)
    for i in range(n):
        bits = 0
        for a in range(s):
            for b in range(s):
                bits |= int(bool(grid[i, a, b])) << (a * s + b)
        rows[i, 0], rows[i, 1] = bits & 0xFFFFFFFF, bits >> 32
    rows[:, 2:] = shifts
    return np.where(rows >= 2 ** 31, rows - 2 ** 32, rows).astype(np.int32)      # (the words as two's-complement int32)


def unpack_grid(rows, s):
    """int32 rows [n, 4] -> float32 grids [n, s, s]"""
    rows = np.asarray(rows).astype(np.int64) & 0xFFFFFFFF
    out = np.zeros((rows.shape[0], s, s), dtype=F32)
    for i, (lo, hi) in enumerate(rows[:, :2].tolist()):
        bits = lo | (hi << 32)
        for a in range(s):
            for b in range(s):
                out[i, a, b] = (bits >> (a * s + b)) & 1
    return out


def axis(size, shift, s, U):
    """-> (k0, k1, f) for the pixels 0..size-1 of one axis at `shift`: integer floor division, one fp32 division, mirrored indices"""
    p = np.arange(size, dtype=np.int64) + int(shift)
    num = (2 * p + 1) * s - U
    i0 = np.floor_divide(num, 2 * U)
    f = (num - i0 * 2 * U).astype(F32) / F32(2 * U)
    assert f.dtype == F32

    def mirror(k):
        k = np.abs(k)
        return np.where(k >= s, 2 * (s - 1) - k, k)
    return mirror(i0), mirror(i0 + 1), f


def mask(grid, shift_r, shift_c, H, W):
    """one mask [H, W] in float32: top = g00 + fc (g01 - g00), bot = g10 + fc (g11 - g10), m = top + fr (bot - top)"""
    s = grid.shape[0]
    cell_h, cell_w = -(-H // s), -(-W // s)
    assert 0 <= shift_r < cell_h and 0 <= shift_c < cell_w
    a0, a1, fr = axis(H, shift_r, s, (s + 1) * cell_h)
    b0, b1, fc = axis(W, shift_c, s, (s + 1) * cell_w)
    g = grid.astype(F32)
    fr, fc = fr[:, None], fc[None, :]
    g00, g01, g10, g11 = g[a0][:, b0], g[a0][:, b1], g[a1][:, b0], g[a1][:, b1]
    top = g00 + fc * (g01 - g00)
    bot = g10 + fc * (g11 - g10)
    m = top + fr * (bot - top)
    assert m.dtype == F32
    return m


def masks(rows, s, H, W):
    """bank rows [n, 4] -> float32 masks [n, H, W]"""
    rows = np.asarray(torch.as_tensor(rows).cpu())
    grids = unpack_grid(rows, s)
    return np.stack([mask(grids[i], int(rows[i, 2]), int(rows[i, 3]), H, W) for i in range(rows.shape[0])])


# ---------------------------------------------------------------------------------------------- stand-ins for bcos_hip.ops
def rise_masks(bank, H, W, first=0, n=None):
    n = len(bank) - first if n is None else n
    return torch.from_numpy(masks(bank.rows[first:first + n], bank.s, int(H), int(W)))


def prep_input_rise(x_nchw, bank, mean6, std6, first=0, n=None, cpad=8, want_absmax=False):
    _, _, H, W = x_nchw.shape
    return OE.prep_input(x_nchw.cpu() * rise_masks(bank, H, W, first, n)[:, None], mean6.cpu(), std6.cpu(), cpad)


def accumulate(scores, m, p1):
    """the kernel's order in numpy float32: chunks of 64 masks; a chunk sum starts at 0 and adds the separately rounded products in
    ascending i; the total adds the chunk sums in ascending order; then / float(n) / p1"""
    scores, m = np.asarray(scores, dtype=F32), np.asarray(m, dtype=F32)
    n, T = scores.shape
    tot = np.zeros((T,) + m.shape[1:], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for base in range(0, n, 64):
            acc = np.zeros_like(tot)
            for i in range(base, min(n, base + 64)):
                acc += scores[i][:, None, None] * m[i][None]
            tot += acc
        out = tot / F32(n) / F32(p1)
    assert out.dtype == F32
    return out


def rise_accumulate(scores, bank, H, W, p1):
    return torch.from_numpy(accumulate(scores.detach().cpu().numpy(), masks(bank.rows, bank.s, int(H), int(W)), p1))


def class_scores(logits, targets, group=1, mode="logit"):
    """bcos_class_scores in torch float32 on the host (the kernel's own bounds are tested in tests/test_perturbation_*.py)"""
    t = torch.as_tensor(targets).reshape(-1).long().repeat_interleave(group)
    x = logits.float()
    p = x if mode == "logit" else torch.sigmoid(x) if mode == "sigmoid" else torch.softmax(x, dim=1)
    return p.gather(1, t.view(-1, 1))[:, 0]


# ---------------------------------------------------------------------------------------------- float64 and the bound
def accumulate64(scores, m, p1):
    """-> (the same sum in float64 over the SAME fp32 mask values and fp32 scores, sum_i |score * m| / (n p1))"""
    s64, m64 = np.asarray(scores, dtype=np.float64), np.asarray(m, dtype=np.float64)
    n = s64.shape[0]
    out = np.einsum("it,ihw->thw", s64, m64) / n / float(F32(p1))
    mag = np.einsum("it,ihw->thw", np.abs(s64), np.abs(m64)) / n / float(F32(p1))
    return out, mag


def accumulate_bound(mag, n):
    """|out - out64| <= (2 * 64 + ceil(n / 64) + 4) 2^-24 sum_i |score m| / (n p1): two roundings per term of a chunk (product, addition),
    one per chunk sum, two divisions and second order"""
    return (2 * 64 + -(-n // 64) + 4) * 2.0 ** -24 * mag
