"""Case table, fp64 reference and PER-ELEMENT bounds of the depthwise 7x7 B-cos convolution (csrc/bcos_dwconv.hip; include/bcos_hip.h:
bcos_dwconv7_fwd / bcos_dwconv7_bwd).

Reference: the documented expressions in fp64 from the fp32 inputs promoted; the two epsilons are the fp32 constant 1e-6f the kernel
adds, promoted (on an all-zero patch the norm IS sqrt(eps)).

Bounds, u = 2^-24.  Every output element is one chain of 49 FMAs over the taps (one rounding each; a tap outside the image adds an exact
zero), so with A = sum_t |w x| the standard forward analysis gives |lin - lin64| <= gamma_49 A, gamma_49 = 49 u / (1 - 49 u).  The constant
used is K_LIN = 49 + 8: the chain, and 8 u for everything a compiler may legally do to it short of reordering (nothing today).
    lin    dl = K_LIN u A
    norm   ss is a chain of 49 FMAs of non-negative terms: relative error <= 49 u; + eps (u), the square root halves the relative error
           and rounds once more (u):   |norm - n64| <= RHO n64,  RHO = (49 + 1) / 2 u + u = 26 u
    scale  B = 2:  s = |lin| / norm, one IEEE division:   ds = (dl / n64 + s64 (RHO + u)) (1 + 1e-5)
           (the factor covers 1 / (1 - RHO) of the inverted norm)
           otherwise:  c = |lin / norm| (dc as ds above), t = c + eps (dt = dc + u t64), s = t^(B-1):
           ds = (B - 1) t64^(B-2) dt (1 + 1e-5) + K_POW u s64, K_POW = 4: the accuracy the HIP math API documents for powf, not a measurement
    y      y = s lin, one product:   dy = s64 dl + (|lin64| + dl) ds + u (|y64| + that);   B = 1: y = lin, dy = dl
    gx     z = mul gy is rounded once before the chain (u |z|, inside the 8 u above), the chain as lin with A = sum_t |w mul gy|, then one
           addition:   dgx = K_LIN u A + u (|gx64| + K_LIN u A)     (addend or not)
A dropped or misplaced tap moves lin by a term of the size of A / 49, five decades outside K_LIN u A (test_convnext_cpu.py holds the bound
to that on every case).

Cases: the issue's seven shapes; the smallest H and W that span two 8 x 8 spatial tiles, one per direction (9 rows x 3, 3 x 9); C = 68:
two channel slices of 64 with a tail of one float4 lane.  A plain module (no fixtures, no collection hooks).
"""
import numpy as np
import torch

U = 2.0 ** -24
EPS32 = float(np.float32(1e-6))
K_LIN = 49 + 8
RHO = 26 * U
K_POW = 4
TILE, SLICE = 8, 64          # csrc/bcos_dwconv.hip: TILE, CL * 4

SHAPES = [(1, 1, 1, 4), (1, 2, 3, 40), (3, 5, 9, 40), (2, 7, 7, 96), (1, 8, 8, 260), (2, 19, 13, 64), (1, 33, 34, 16),
          (1, TILE + 1, 3, 8), (1, 3, TILE + 1, 8), (1, 4, 5, SLICE + 4)]
KINDS = ("normal", "zero", "hot")


def case_id(shape, kind):
    return "n%dh%dw%dc%d-%s" % (*shape, kind)


CASES = [(s, k) for s in SHAPES for k in KINDS]


def make_inputs(shape, kind):
    """x / gy [N,H,W,C], w [7,7,C] (unit-norm filters, as the module supplies them), mul >= 0 and addend [N,H,W,C]; fp32, CPU"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + C + 7 * KINDS.index(kind))
    x = torch.randn(N, H, W, C, generator=g)
    gy = torch.randn(N, H, W, C, generator=g)
    if kind == "zero":
        x.zero_()
        gy.zero_()
    elif kind == "hot":       # one hot pixel per image, everything else ten decades below it, a quarter of the pixels exactly zero
        mag = torch.full((1, H, W, 1), 1e-4)
        mag[0, H // 3, W // 2, 0] = 1e6
        mag = mag * (torch.rand(N, H, W, 1, generator=g) > 0.25)
        x, gy = x * mag, gy * mag
    w = torch.randn(7, 7, C, generator=g)
    w = w / w.flatten(0, 1).norm(dim=0)
    mul = torch.rand(N, H, W, C, generator=g)
    addend = torch.randn(N, H, W, C, generator=g)
    return dict(x=x, gy=gy, w=w, mul=mul, addend=addend)


def _taps(t, w, flip=False, drop=None, shift=None):
    """(sum_t w t_tap, sum_t |w t_tap|, sum_t t_tap^2) over the 49 taps, fp64, by explicit shifts of the zero-padded tensor.
    `drop`: a tap left out; `shift`: (tap, other tap) -- the first reads the second's pixel (the mutations the bound must notice)."""
    N, H, W, C = t.shape
    tp = torch.nn.functional.pad(t, (0, 0, 3, 3, 3, 3))
    lin, A, ss = (torch.zeros_like(t) for _ in range(3))
    for r in range(7):
        for s in range(7):
            if drop == (r, s):
                continue
            rr, sc = shift[1] if shift is not None and shift[0] == (r, s) else (r, s)
            if flip:
                rr, sc = 6 - rr, 6 - sc
            v = tp[:, rr:rr + H, sc:sc + W, :]
            lin += w[r, s] * v
            A += (w[r, s] * v).abs()
            ss += v * v
    return lin, A, ss


def scale_of(lin, n, b):
    if b == 2.0:
        return lin.abs() / n
    return ((lin / n).abs() + EPS32) ** (b - 1.0)


def reference_fwd(inp, b, **mut):
    """fp64: lin, A, norm, scale, y"""
    x, w = inp["x"].double(), inp["w"].double()
    lin, A, ss = _taps(x, w, **mut)
    n = (ss + EPS32).sqrt()
    if b == 1.0:
        return dict(lin=lin, A=A, norm=n, scale=torch.ones_like(lin), y=lin.clone())
    s = scale_of(lin, n, b)
    return dict(lin=lin, A=A, norm=n, scale=s, y=s * lin)


def bounds_fwd(ref, b):
    dl = K_LIN * U * ref["A"]
    n, s, lin = ref["norm"], ref["scale"], ref["lin"]
    out = dict(norm=RHO * n)
    if b == 1.0:
        out.update(y=dl)
        return out
    dc = (dl / n + (lin.abs() / n) * (RHO + U)) * (1 + 1e-5)
    if b == 2.0:
        ds = dc
    else:
        t = (lin / n).abs() + EPS32
        ds = (b - 1.0) * t ** (b - 2.0) * (dc + U * t) * (1 + 1e-5) + K_POW * U * s
    err = s * dl + (lin.abs() + dl) * ds
    out.update(scale=ds, y=err + U * (ref["y"].abs() + err))
    return out


def reference_bwd(inp, use_mul, use_addend, **mut):
    """fp64: gx, A"""
    z = inp["gy"].double() * (inp["mul"].double() if use_mul else 1.0)
    lin, A, _ = _taps(z, inp["w"].double(), flip=True, **mut)
    return dict(gx=lin + (inp["addend"].double() if use_addend else 0.0), A=A)


def bounds_bwd(ref):
    dl = K_LIN * U * ref["A"]
    return dict(gx=dl + U * (ref["gx"].abs() + dl))


def worst_ratio(out, ref, bound):
    """max over the elements of |out - ref| / bound (0 / 0 = 0: an exact result under a zero bound passes, anything else is inf)"""
    err = (out.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0
