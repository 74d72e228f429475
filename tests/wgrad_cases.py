"""The case table of the training-mode weight gradient (include/bcos_hip.h: bcos_conv2d_wgrad / bcos_conv2d_wgrad_ordered), the input
families every case runs with, the fp64 reference and the PER-ELEMENT bound every element of gw is held to.

Reference, from the fp32 operands promoted to fp64, over the USED channels only (the pad channels up to the pitches hold NaN):
    gw64[co, tap, ci] = sum_m glin[m, co] x[pix(m, tap), ci],       m = (n, i, j),  pix = (n, i sh - ph + th dh, j sw - pw + tw dw)
Bound, with u = 2^-24:
    form[co, tap, ci] = sum_m |glin[m, co]| |x[pix(m, tap), ci]|    (the L1 form of the column sums)
    |gw - gw64| <= K_fam u form,   and an element whose sum is empty (a tap that only ever meets padding) is exactly 0.
K_fam = max(4 x FP32_WORST_fam, 16): FP32_WORST_fam is the worst use of the form by PyTorch's own fp32 weight gradient over the table
(tests/test_wgrad_cases_cpu.py re-measures it); the floor of 16 u is twice the provable cost of the three dropped products of an exact
three-way truncation split, |m_a l_b + l_a m_b + l_a l_b| <= 2^-21 |a b| = 8 u.
The bf16 matrix pipe adds one term for the family `full` alone (operands of ONE sign, where no rounding error cancels another):
    |gw - gw64| <= (K_full + D) u form,   D = 6 ceil(chunk / 16) + split - 1,
the accumulations behind an element: six matrix instructions per 16 pixels of a chunk, then the chunks' partial sums.  Measured on the
MI355X (both bf16x3 kernels, same figures): the error of `full` grows with D and with nothing else -- 2.0 u at D = 6 (the dropped
products alone), 5.7 - 5.8 u at D = 12, 13.6 u at D = 36, 18.1 u at D = 42, 19.0 and 23.8 u at D = 90 -- i.e. 0.2 - 0.5 u per
accumulation, never more; K_full = 16 alone is exceeded from D = 42 on and only there.  The fp32 pipe (mode f32) stays at 1.0 u on
every case of `full` and gets no such term, and neither does any other family (they stay under a quarter of K on every kernel).

The table holds the smallest shapes that reach each route of wgrad3_plan (csrc/bcos_train.hip); `plan` is what
bcos_conv2d_wgrad_plan_query answers for the case (the CPU test pins it) and the coverage assertions at the end of this module read it.

A plain module (no fixtures, no collection hooks): the test files import it.
"""
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FAMILIES = ("normal", "full", "imgrange", "hot")
HOT = 4096.0

# worst |fp32 PyTorch conv weight gradient - fp64| / form over CASES, in units of u, as test_wgrad_cases_cpu.py measures and prints it
# (one thread; rounded UP to the next tenth that leaves 2 %; the CPU test holds the measurement inside (want - tol, want] with
# tol = max(0.3, 5 % of want): another oneDNN build blocks the pixel sum differently):
#     normal 5.078 (linear_rows)   full 1.037 (shortcut_1x1_s2)   imgrange 6.396 (stem7x7_c6)   hot 63.547 (thin_combine)
# so K = 20.8 (normal), 16 (full: the floor), 26.4 (imgrange), 259.6 (hot: fp32 itself loses the sum of the ordinary pixels behind a
# pixel 2^12 above them)
FP32_WORST = {"normal": 5.2, "full": 1.1, "imgrange": 6.6, "hot": 64.9}
K_FLOOR = 16.0
K = {fam: max(4 * w, K_FLOOR) for fam, w in FP32_WORST.items()}


PIPE_TERM_FAMILIES = ("full",)


def chain(chunk, split):
    """accumulations behind one element: six matrix instructions per 16 pixels of a chunk, plus the sum over the chunks"""
    return 6 * ((chunk + 15) // 16) + split - 1


def bound_k(family, steps):
    """the constant of the bound of a bf16x3 launch whose elements have `steps` accumulations behind them (mode f32: steps = 0)"""
    return K[family] + (steps if family in PIPE_TERM_FAMILIES else 0)


def fp32_tolerance(want):
    return max(0.3, 0.05 * want)


def _r4(v):
    return (v + 3) & ~3


@dataclass(frozen=True)
class Case:
    id: str
    geom: tuple                    # N, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw
    plan: dict = field(compare=False, hash=False)      # the fields of bcos_wgrad_plan this case is in the table for
    wgs: int = 0                   # BCOS_OPT_WGRAD_WGS for the case (0: the default)
    why: str = ""

    def __getattr__(self, name):
        names = ("N", "C", "H", "W", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")
        if name in names:
            return self.geom[names.index(name)]
        raise AttributeError(name)

    @property
    def P(self):
        return (self.H + 2 * self.ph - self.dh * (self.kh - 1) - 1) // self.sh + 1

    @property
    def Q(self):
        return (self.W + 2 * self.pw - self.dw * (self.kw - 1) - 1) // self.sw + 1

    @property
    def M(self):
        return self.N * self.P * self.Q

    @property
    def taps(self):
        return self.kh * self.kw

    @property
    def x_pitch(self):
        return _r4(self.C)

    @property
    def g_pitch(self):
        return _r4(self.Cout)

    def ints(self, gw_cin=0):
        """the 18 geometry integers of the C entry points, in their order"""
        return (self.N, self.H, self.W, self.C, self.x_pitch, self.P, self.Q, self.Cout, self.g_pitch, self.kh, self.kw,
                self.sh, self.sw, self.ph, self.pw, self.dh, self.dw, gw_cin)

    @property
    def steps(self):
        """accumulations behind one element on the ordered route"""
        return chain(self.plan["chunk"], self.plan["split"])


def _plan(fused, direct, tco, tci, gy, split, combine, chunk, last, ws):
    return dict(fused_taps=fused, direct=direct, tiles_co=tco, tiles_ci=tci, grid_y=gy, split=split, combine=combine, chunk=chunk,
                last=last, ws_floats=ws)


CASES = [
    Case("stem7x7_c6", (5, 6, 16, 12, 12, 7, 7, 2, 2, 3, 3, 1, 1), _plan(1, 0, 1, 4, 1, 1, 0, 240, 240, 0),
         why="C = 6 in a pitch of 8, 49 taps over 4 column tiles"),
    Case("fused3x3_c36", (3, 36, 9, 11, 20, 3, 3, 1, 1, 1, 1, 1, 1), _plan(1, 0, 1, 3, 1, 2, 1, 160, 137, 2 * 20 * 9 * 36),
         why="cf = 36, a chunk edge inside an image row"),
    Case("pertap_rect_c132", (2, 132, 7, 5, 30, 3, 2, 2, 1, 1, 0, 1, 2), _plan(0, 0, 1, 2, 6, 1, 0, 32, 24, 0),
         why="everything rectangular, Cout % 4 != 0, M = 24: a ragged last stage"),
    Case("pertap_c130_scalar", (2, 130, 6, 7, 30, 3, 3, 1, 1, 1, 1, 1, 1), _plan(0, 0, 1, 2, 9, 1, 0, 96, 84, 0),
         why="C % 4 != 0 beyond 128: scalar loads and stores, gw_cin & 3"),
    Case("direct_1x1_co136", (1, 256, 28, 36, 136, 1, 1, 1, 1, 0, 0, 1, 1), _plan(0, 1, 2, 2, 1, 4, 1, 256, 240, 4 * 136 * 256),
         why="the second co tile has one live wave with 8 rows"),
    Case("shortcut_1x1_s2", (3, 128, 14, 10, 256, 1, 1, 2, 2, 0, 0, 1, 1), _plan(0, 0, 2, 1, 1, 1, 0, 112, 105, 0),
         why="the downsample shortcut: 1 x 1 but not direct"),
    Case("tinyQ_multiwrap", (40, 16, 5, 7, 12, 3, 3, 2, 2, 0, 0, 1, 1), _plan(1, 0, 1, 2, 1, 1, 0, 240, 240, 0),
         why="P Q = 6 < 16: one stage advance wraps several rows and images"),
    Case("thin_combine", (2, 64, 40, 37, 64, 3, 3, 1, 1, 1, 1, 1, 1), _plan(1, 0, 1, 5, 1, 12, 1, 256, 144, 12 * 64 * 9 * 64),
         why="the unrolled-by-4 loop of the thin combine plus its remainder"),
    Case("wide_combine", (2, 8, 92, 93, 8, 3, 3, 1, 1, 1, 1, 1, 1), _plan(1, 0, 1, 1, 1, 67, 2, 256, 216, 67 * 8 * 9 * 8),
         why="the by-64 unrolled loop of the wide combine plus its remainder"),
    Case("wide_combine_wgs64", (2, 8, 92, 93, 8, 3, 3, 1, 1, 1, 1, 1, 1), _plan(1, 0, 1, 1, 1, 63, 2, 272, 248, 63 * 8 * 9 * 8), wgs=64,
         why="the option changes the chunking, not the answer"),
    Case("linear_rows", (1, 512, 1, 300, 1000, 1, 1, 1, 1, 0, 0, 1, 1), _plan(0, 1, 8, 4, 1, 2, 1, 160, 140, 2 * 1000 * 512),
         why="the linear layer as a 1 x 1 convolution, ragged Cout"),
    Case("dil2_pad2", (1, 16, 5, 5, 12, 3, 3, 1, 1, 2, 2, 2, 2), _plan(1, 0, 1, 2, 1, 1, 0, 32, 25, 0),
         why="dilation 2 under padding 2: the outer taps meet the image at a few pixels only"),
    Case("single_pixel", (1, 4, 1, 1, 4, 1, 1, 1, 1, 0, 0, 1, 1), _plan(0, 1, 1, 1, 1, 1, 0, 16, 1, 0), why="M = 1"),
    # (every tap of dil2_pad2 meets the image somewhere; here only the centre tap does: eight taps whose sums are empty)
    Case("pad_only_taps", (1, 4, 2, 2, 4, 3, 3, 1, 1, 2, 2, 2, 2), _plan(1, 0, 1, 1, 1, 1, 0, 16, 4, 0),
         why="taps that only ever meet padding: elements that must be exactly 0"),
]
SHORT_CHAIN = ("pertap_rect_c132", "dil2_pad2", "single_pixel")        # <= 12 accumulations behind an element


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def hot_pixels(case):
    """(pixel of x in image 0, pixel of glin in the last image) that the family `hot` multiplies by HOT.  The pixel of x is the one the
    centre tap meets at the middle output pixel: a pixel the layer reads (a strided 1 x 1 layer skips most of its input)"""
    c = case
    i, j = c.P // 2, c.Q // 2
    ih, iw = i * c.sh - c.ph + (c.kh // 2) * c.dh, j * c.sw - c.pw + (c.kw // 2) * c.dw
    assert 0 <= ih < c.H and 0 <= iw < c.W
    return (0, ih, iw), (c.N - 1, i, j)


def make_inputs(case, family):
    """(x [N, H, W, x_pitch], glin [N, P, Q, g_pitch]) fp32 on the CPU, the same tensors on every call; the pad channels hold NaN"""
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + 17 * [c.geom for c in CASES].index(case.geom) + 3)
    xs, gs = (case.N, case.H, case.W, case.C), (case.N, case.P, case.Q, case.Cout)
    if family == "full":
        # every value positive with an all-ones significand: all three bf16 planes non-zero and of one sign
        one = torch.tensor(2.0 - 2.0 ** -23)
        x = torch.ldexp(one, torch.randint(-2, 3, xs, generator=g))
        gl = torch.ldexp(one, torch.randint(-2, 3, gs, generator=g))
    else:
        x, gl = torch.randn(xs, generator=g), torch.randn(gs, generator=g)
    if family == "imgrange":            # (the exponents 12 ((n mod 3) - 1) + 9 (n mod 2) of the products differ from image to image)
        n = torch.arange(case.N)
        x = x * torch.ldexp(torch.tensor(1.0), 12 * (n % 3 - 1)).view(-1, 1, 1, 1)
        gl = gl * torch.ldexp(torch.tensor(1.0), 9 * (n % 2)).view(-1, 1, 1, 1)
    elif family == "hot":
        hx, hg = hot_pixels(case)
        x[hx] *= HOT
        gl[hg] *= HOT
    elif family not in ("normal", "full"):
        raise ValueError(family)
    xp = torch.full((case.N, case.H, case.W, case.x_pitch), float("nan"))
    gp = torch.full((case.N, case.P, case.Q, case.g_pitch), float("nan"))
    xp[..., :case.C] = x
    gp[..., :case.Cout] = gl
    return xp, gp


def xcol(x, case, ph=None, pw=None, decode_kw=None):
    """[M, taps, C]: row m = (n, i, j) holds, per tap, the input pixel the tap meets there (zeros where it meets padding), used channels
    only.  ph / pw / decode_kw override the case's padding and the divisor of the tap decode th = tap / kw: the mutants of the CPU tier."""
    c = case
    ph = c.ph if ph is None else ph
    pw = c.pw if pw is None else pw
    dk = c.kw if decode_kw is None else decode_kw
    tap = torch.arange(c.taps, device=x.device)
    th = tap // dk
    tw = tap - th * dk
    ih = torch.arange(c.P, device=x.device)[:, None] * c.sh - ph + th[None, :] * c.dh          # [P, taps]
    iw = torch.arange(c.Q, device=x.device)[:, None] * c.sw - pw + tw[None, :] * c.dw          # [Q, taps]
    ok = ((ih >= 0) & (ih < c.H))[:, None, :] & ((iw >= 0) & (iw < c.W))[None, :, :]             # [P, Q, taps]
    idx = ih.clamp(0, c.H - 1)[:, None, :] * c.W + iw.clamp(0, c.W - 1)[None, :, :]
    xf = x[..., :c.C].reshape(c.N, c.H * c.W, c.C)
    cols = xf[:, idx.reshape(-1), :].reshape(c.N, c.P, c.Q, c.taps, c.C)
    cols = torch.where(ok[None, :, :, :, None], cols, torch.zeros((), dtype=x.dtype, device=x.device))
    return cols.reshape(c.M, c.taps, c.C)


def xcol_unfold(x, case):
    """the same by F.unfold"""
    c = case
    xn = x[..., :c.C].permute(0, 3, 1, 2)
    u = F.unfold(xn, (c.kh, c.kw), dilation=(c.dh, c.dw), padding=(c.ph, c.pw), stride=(c.sh, c.sw))      # [N, C taps, P Q]
    return u.reshape(c.N, c.C, c.taps, c.P * c.Q).permute(0, 3, 2, 1).reshape(c.M, c.taps, c.C)


def contract(g2, cols):
    """[Cout, taps, C] = g2^T cols   (g2 [M, Cout], cols [M, taps, C])"""
    M, taps, Cc = cols.shape
    return (g2.t() @ cols.reshape(M, taps * Cc)).reshape(g2.shape[1], taps, Cc)


def reference(x, glin, case):
    """(gw64, form), both [Cout, taps, C] fp64, on the device of the operands"""
    cols = xcol(x.double(), case)
    g2 = glin[..., :case.Cout].double().reshape(case.M, case.Cout)
    return contract(g2, cols), contract(g2.abs(), cols.abs())


def conv_weight_grad(x, glin, case, dtype):
    """PyTorch's own weight gradient of the convolution in `dtype`, as [Cout, taps, C]"""
    c = case
    xn = x[..., :c.C].permute(0, 3, 1, 2).to(dtype).contiguous()
    g = glin[..., :c.Cout].permute(0, 3, 1, 2).to(dtype).contiguous()
    with torch.enable_grad():
        w = torch.zeros(c.Cout, c.C, c.kh, c.kw, dtype=dtype, requires_grad=True)
        (gw,) = torch.autograd.grad(F.conv2d(xn, w, None, (c.sh, c.sw), (c.ph, c.pw), (c.dh, c.dw)), w, g)
    return gw.permute(0, 2, 3, 1).reshape(c.Cout, c.taps, c.C)


def worst(err, form):
    """max over EVERY element of err / form in units of u; an exact element counts as 0 whatever its form (an empty sum must be exactly
    0: any error over a zero form is inf), a NaN anywhere gives NaN"""
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (form * U))
    return float("nan") if bool(torch.isnan(ratio).any()) else float(ratio.max())


def ratio(gw, ref):
    """worst |gw - gw64| / (u form) of a result [Cout, taps, C] (any float type) against ref = reference(...)"""
    return worst((gw.double().reshape(ref[0].shape) - ref[0]).abs(), ref[1])


def fp32_ratio(case, family):
    x, gl = make_inputs(case, family)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        gw32 = conv_weight_grad(x, gl, case, torch.float32)
    finally:
        torch.set_num_threads(threads)
    return ratio(gw32, reference(x, gl, case))


def planes(t):
    """the exact three-way bf16 split of the kernels: (h, m, l) fp32 tensors with h + m + l == t, each of 8 significand bits, by truncation"""
    def top(v):
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    h = top(t)
    r1 = t - h
    m = top(r1)
    l = r1 - m
    assert torch.equal(top(l), l) and torch.equal((h.double() + m.double() + l.double()).float(), t)
    return h, m, l


DROPPED = (("m", "l"), ("l", "m"), ("l", "l"))           # (plane of glin, plane of x) of the products the kernels leave out


def six_products(x, glin, case, also_drop=(), cols_fn=xcol):
    """the documented arithmetic in fp64: the exact product sum minus the three dropped plane products (and minus `also_drop`, more
    (plane of glin, plane of x) pairs: the mutants)"""
    c = case
    xs = dict(zip("hml", planes(x[..., :c.C].contiguous())))
    gs = dict(zip("hml", planes(glin[..., :c.Cout].contiguous())))
    out = contract(glin[..., :c.Cout].double().reshape(c.M, c.Cout), cols_fn(x.double(), c))
    for a, b in DROPPED + tuple(also_drop):
        out = out - contract(gs[a].double().reshape(c.M, c.Cout), cols_fn(xs[b].double(), c))
    return out


# ---- what the table is shown to cover (no device, no library: the `plan` column, which the CPU test pins to the query) -------------------
def kind(c):
    return "fused" if c.plan["fused_taps"] else ("1x1" if c.taps == 1 else "pertap")


def dead_wave(c):
    """a wave of the last co tile whose 32 rows lie beyond Cout"""
    return c.Cout - 128 * (c.plan["tiles_co"] - 1) <= 96


def empty_taps(c):
    """taps that meet padding at every output pixel: their elements of gw are empty sums"""
    def misses(k, n_out, s, p, d, size):
        return [all(not 0 <= i * s - p + t * d < size for i in range(n_out)) for t in range(k)]
    mh, mw = misses(c.kh, c.P, c.sh, c.ph, c.dh, c.H), misses(c.kw, c.Q, c.sw, c.pw, c.dw, c.W)
    return [th * c.kw + tw for th in range(c.kh) for tw in range(c.kw) if mh[th] or mw[tw]]


assert len({c.id for c in CASES}) == len(CASES)
assert any(empty_taps(c) for c in CASES)
# fused and per-tap launches have several taps and are never direct; a 1 x 1 layer is direct or (strided: the shortcut) indexed
assert {(kind(c), c.plan["direct"]) for c in CASES} == {("fused", 0), ("pertap", 0), ("1x1", 1), ("1x1", 0)}
assert {c.plan["combine"] for c in CASES} == {0, 1, 2}
assert any(c.plan["split"] > 1 and c.plan["last"] < c.plan["chunk"] for c in CASES)
assert any(c.plan["last"] % 16 for c in CASES)                                      # a ragged last stage
assert any(dead_wave(c) for c in CASES) and any(c.Cout % 4 for c in CASES)
assert any(c.C % 4 == 0 for c in CASES) and any(c.C % 4 and c.C >= 128 for c in CASES) and any(c.C % 4 and c.C < 128 for c in CASES)
assert any(c.wgs for c in CASES) and any(c.H != c.W and c.kh != c.kw and c.sh != c.sw and c.ph != c.pw and c.dh != c.dw for c in CASES)
assert all(by_id(i).steps <= 12 for i in SHORT_CHAIN)
