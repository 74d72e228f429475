"""Case table, fp64 reference and PER-ELEMENT bounds of the training-mode gradients of the depthwise 7x7 B-cos convolution
(csrc/bcos_dwconv_train.hip; include/bcos_hip.h: bcos_dwconv7_train_bwd / bcos_dwconv7_wgrad), in the style of dwconv_cases.py, whose
inputs, tap walk and constants are imported.

Reference: the documented expressions in fp64 from the fp32 inputs promoted.  The backward's inputs y, scale, norm are GIVEN: the GPU
tests hand the kernel the fp64 forward reference rounded to fp32 and the reference below starts from those same fp32 values, so no bound
carries forward error.  (test_dwconv_train_cpu.py calls the same functions on the UNROUNDED forward, where they must equal torch's
float64 autograd.)
    glin = 2 scale g        r = -(g y) / norm^2        acc(q) = sum_t w_t glin(q - t + 3)        box(q) = sum_t r(q - t + 3)
    gx = acc + x box [+ addend]                        gw(t, c) = sum_{n,p} glin_c(n, p) x_c(n, p + t - 3)

Bounds, u = 2^-24, from the operation count of the header's arithmetic -- not from a run.
  glin  one rounded product (the doubling is exact):               |glin - glin64| <= u |glin64|
  acc   the 49-FMA chain over rounded operands, exactly bcos_dwconv7_bwd's gx with z = glin: with A_g = sum_t |w_t glin64|
            d_acc = K_LIN u A_g            (K_LIN = 49 + 8 of dwconv_cases.py: the chain, the operand's rounding, the same allowance)
  r     two rounded products and one IEEE division:                |r - r64| <= 3 u |r64| (1 + 1e-5)
  box   49 additions from 0 (the first is exact, 48 round) over operands that carry 3 u each: with A_r = sum_t |r64|
            d_box = (48 + 3) u A_r (1 + 1e-4) <= K_BOX u A_r,  K_BOX = 49 + 8    (the rest of K_BOX is the allowance K_LIN has)
  gx    the product with x and the additions, each allowed a rounding of its own (the kernel's single FMA commits fewer):
            t = x box:          dt = |x| d_box + u (|x box64| + |x| d_box)
            s = acc + t:        ds = d_acc + dt + u (|acc64 + x box64| + d_acc + dt)
            + addend:           dgx = ds + u (|gx64| + ds)                       (without an addend dgx = ds)
  B = 1 gx = acc over glin = g [+ addend]: reference_bwd / bounds_bwd of dwconv_cases.py without mul, as they stand.
  gw    glin carries u (mul gy) + u (gain; exact for 1 and 2) <= 2 u.  The summation order of the header: per (tap, channel) a
        workgroup's part is ONE FMA chain over L = ceil(P / 256) pairs x 3 tile rows x 8 columns = 24 L terms, and the second launch
        adds the 2 G partials in a chain of 2 G - 1 additions.  Every term passes through at most 24 L + 2 G - 1 roundings, so with
        S = sum_{n,p} |glin64 x| and K_GW = 24 L + 2 G + 6 (the two chains, 2 for glin, 5 allowance as above):
            dgw = gamma(K_GW) S,   gamma(k) = k u / (1 - k u)
        P = N ceil(H / 6) ceil(W / 8),  G = ceil(P / L)  (the header's work assignment).
A dropped tap moves acc by a term of the size of A_g / 49, a dropped norm term moves gx by |x box|, a missing factor 2 halves acc, a
shifted tap replaces one of gw's 49 correlations by its neighbour's: all decades outside these bounds (test_dwconv_train_cpu.py holds
each to 100 x on every normal case).

Cases: the issue's shapes -- the smallest ones, two tiles per direction of BOTH kernels' tilings (9 rows: 8 + 1 and 6 + 3; 9 columns:
8 + 1), C = 68: a slice of 64 and a tail of one float4 lane, (3,17,9,68): several partials per slice along images, tile rows, tile
columns and parts -- and (9,33,41,4): P = 324 > 256 pairs, the one shape at which a workgroup owns more than one pair (L = 2).  The
slice is 64 channels in both kernels, so there is no C = 36 case.  A plain module (no fixtures, no collection hooks).
"""
import torch

from dwconv_cases import EPS32, K_LIN, KINDS, U, _taps, make_inputs, reference_fwd, worst_ratio  # noqa: F401  (re-exported)

K_BOX = 49 + 8
WTH, WTW, WG_MAX, PARTS = 6, 8, 256, 2          # csrc/bcos_dwconv_train.hip: stage 1 of the weight gradient

SHAPES = [(1, 1, 1, 4), (1, 2, 3, 40), (3, 5, 9, 40), (2, 7, 7, 96), (1, 9, 3, 8), (1, 3, 9, 8), (1, 4, 5, 68), (2, 19, 13, 64),
          (3, 17, 9, 68), (9, 33, 41, 4)]
CASES = [(s, k) for s in SHAPES for k in KINDS]


def case_id(shape, kind):
    return "n%dh%dw%dc%d-%s" % (*shape, kind)


def wgrad_plan(shape):
    """(P, L, G) of the header's work assignment"""
    N, H, W, _ = shape
    P = N * (-(-H // WTH)) * (-(-W // WTW))
    L = -(-P // WG_MAX)
    return P, L, -(-P // L)


def workspace_bytes(shape):
    """include/bcos_hip.h: bytes = 4 * 49 * C * 2 * G"""
    return 4 * 49 * shape[3] * PARTS * wgrad_plan(shape)[2]


def forward_given(inp, rounded=True):
    """y, scale, norm of the B = 2 forward in fp64: rounded to fp32 and promoted again (what the kernels are handed), or as they are"""
    f = reference_fwd(inp, 2.0)
    return {k: (f[k].float().double() if rounded else f[k]) for k in ("y", "scale", "norm")}


def reference_gx(inp, given, use_addend, drop=None, no_r=False, factor=2.0):
    """fp64 input gradient and the sums its bound needs.  Mutations: `drop` a tap of the weighted sum, `no_r` no norm term, `factor` != 2"""
    x, g, w = inp["x"].double(), inp["gy"].double(), inp["w"].double()
    glin = factor * given["scale"] * g
    r = -(g * given["y"]) / (given["norm"] * given["norm"])
    acc, A_g, _ = _taps(glin, w, flip=True, drop=drop)
    box, A_r, _ = _taps(r, torch.ones_like(w), flip=True)
    if no_r:
        box = torch.zeros_like(box)
    gx = acc + x * box + (inp["addend"].double() if use_addend else 0.0)
    return dict(gx=gx, acc=acc, box=box, A_g=A_g, A_r=A_r, x=x, addend=use_addend)


def bounds_gx(ref):
    x = ref["x"].abs()
    d_acc = K_LIN * U * ref["A_g"]
    d_box = K_BOX * U * ref["A_r"]
    xb = (ref["x"] * ref["box"]).abs()
    dt = x * d_box + U * (xb + x * d_box)
    ds = d_acc + dt + U * ((ref["acc"] + ref["x"] * ref["box"]).abs() + d_acc + dt)
    return dict(gx=ds + U * (ref["gx"].abs() + ds) if ref["addend"] else ds)


def reference_gw(inp, mul, gain, shift=None):
    """fp64 weight gradient [7,7,C] and S = sum |glin x|.  `mul`: fp64 [N,H,W,C] or None.  Mutation `shift`: (tap, other tap) -- the first
    correlates with the second's pixels"""
    x, g = inp["x"].double(), inp["gy"].double()
    glin = gain * (mul * g if mul is not None else g)
    N, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 3, 3, 3, 3))
    gw, S = torch.zeros(7, 7, C, dtype=torch.float64), torch.zeros(7, 7, C, dtype=torch.float64)
    for r in range(7):
        for s in range(7):
            rr, sc = shift[1] if shift is not None and shift[0] == (r, s) else (r, s)
            v = glin * xp[:, rr:rr + H, sc:sc + W, :]
            gw[r, s] = v.sum((0, 1, 2))
            S[r, s] = v.abs().sum((0, 1, 2))
    return dict(gw=gw, S=S)


def bounds_gw(ref, shape):
    _, L, G = wgrad_plan(shape)
    k = (WTH // PARTS) * WTW * L + PARTS * G + 6
    return dict(gw=k * U / (1 - k * U) * ref["S"])
