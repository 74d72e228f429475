"""The case tables of the token-path entry points of csrc/bcos_vit.hip and csrc/bcos_norms.hip (include/bcos_hip.h: bcos_layernorm_fwd /
_stats / _bwd_detached / _bwd / _bwd_add, bcos_groupnorm_fwd / _bwd_detached / _bwd, bcos_gelu_gate / bcos_gelu_bwd, bcos_add_rows_bcast,
bcos_finalize_explanation_patches), the fp64 reference of what they compute and the PER-ELEMENT bounds every output is held to.

Reference: the documented expressions in fp64 from the fp32 inputs promoted (eps is the fp32 value the entry point receives, promoted).
The BACKWARD entry points take rstd as an INPUT: their reference uses the fp32 rstd of the fp32 forward formula (make_inputs: "rstd"),
promoted to fp64 -- not an fp64 recomputation; only mean(x) of the full backward is recomputed, in fp64.

LayerNorm row / GroupNorm (image, group) with n values; u = 2^-24, A = max |x| of the row or group, sd = sqrt(var64 + eps), xh = x_hat64,
E(xh, q) = |xh| + q (1 + |xh|)  (the error of an x_hat in units of u: |xh| its own roundings; q = A / sd the error u A of `x - mean`
divided by sd, and q |xh| the relative error u A / sd that the same error leaves in the centred second moment, i.e. in sd):
    y         |y - y64|      <= K_y    u ( |w| E(xh, A / sd) + |y64| )              F_y: the x_hat error through w; the affine's roundings
    rstd      |rstd sd - 1|  <= K_rstd u ( 1 + A / sd )                             sqrt / reciprocal roundings; the relative error of sd
    zss       |zss - zss64|  <= K_zss  u ( zss64 + 2 sum_c |y64| F_y[c] )           the sum's roundings; d(y^2) = 2 |y| dy per column
    det       |o - o64|      <= K_det  u ( |h| + mean_c |h| + |addend| + |o64| )    h = gy w rstd: products; the mean's sum; the two adds
              |o2 - o2_64|   <= K_det  u ( (that form) |mul2| + |o2_64| )           the error of o carried by mul2; the product's rounding
    full      |gx - gx64|    <= K_full u ( rs (|h| + mean|h|) + rs ( E mean|h xh| + |xh| mean(|h| E) ) + |addend| + |gx64| )
              h = gy w, rs = rstd, xh = (x - mean64) rs, E = E(xh, A rs): the products and the first mean; the x_hat error in
              `xh mean(h xh)` -- in the factor xh and inside the mean --, no credit for cancellation; the adds
    xhat_out  |xh' - xh|     <= K_y    u ( E(xh, A rs) + |xh| )                     F_y with w = 1, b = 0
    x_absmax is bit-equal to max |x| of the row; y_absmax / out2_absmax are bit-equal to the row maximum of the y / out2 written.
GELU, with Phi = 0.5 erfc(-x / sqrt 2), phi the normal density, z = |x| / sqrt 2, t = 1 / (1 + p z), the condition number of the
formula's alternating polynomial c(t) = sum_k |a_k| t^k / sum_k a_k t^k (1.7 .. 4.5) and G = (c(t) + 2 z^2) min(Phi, 1 - Phi) + Phi:
    gate      |gate - Phi|   <= E_AS + K_gelu u G            E_AS = 0.75e-7: half the 1.5e-7 Abramowitz-Stegun 7.1.26 states for erf (not
                                                             tuned); c(t) min(..): the roundings of the Horner sum, whose terms cancel,
                                                             and of t, carried by the tail = min(Phi, 1 - Phi); 2 z^2 min(..): z is
                                                             rounded before it is squared, and the exponential carries an absolute
                                                             error of its argument as a relative one; Phi: the final 1 - tail / 2
    y         |y - x Phi|    <= |x| (gate's bound) + u |y64|
    gx        |gx - gx64|    <= |gy| ( E_AS + K_gelu_gx u ( G + |x| phi (1 + x^2) ) ) + u |gx64|      phi's exponent argument and product
add_rows_bcast is exact: bit-equal to x + pe[i % period] in fp32.
Un-patchify:  |W - W64| <= K_fin_w u |W64|  (one division);  |c - c64| <= K_fin_c u sum_ch |x6 W64|, x6 = [x, 1 - x] under add_inverse
(the six products and their sum, no credit for cancellation).

tests/test_token_cases_cpu.py evaluates the same expressions in plain fp32 PyTorch (two-pass formulae, torch's own summation order; the
GELU as a restatement of bcos_gelu_gate with an exact division and torch.exp) for every case, prints the worst use of each form and pins
the constants: K = 4 x that worst use.  The 4 covers the kernels' lane-tree and 16-lane summation orders, the workgroup reduction of
GroupNorm and the hardware's 1-ulp reciprocal, exp and division, nothing more.  For the GELU forms the fp32 restatement is measured
against the SAME polynomial in fp64 (its rounding error alone); that the polynomial stays within 1.5e-7 of erf -- E_AS on the gate -- is
a separate fp64 assertion there, and the two add up to the bound above.
tests/test_token_kernels_gpu.py launches every case through the C ABI and judges every element.

A plain module (no fixtures, no collection hooks): the two test files import it.
"""
import math
from dataclasses import dataclass, replace

import torch

U = 2.0 ** -24
E_AS = 0.75e-7

# worst |fp32 PyTorch - fp64| / form over the case tables, in units of u, as test_token_cases_cpu.py measures and prints it:
#     y 2.905   zss 1.464   det 1.809   full 1.965   (all four: ln-offset-r8229d5-w-e5)      rstd 1.329 (ln-normal-r131093d4-wb-e5)
#     gelu 1.699   gelu_gx 2.386   (gelu-gate-n524365)
#     fin_w 1.000   fin_c 4.792   (fin-n65h256w256p16c8-inv1)
# FP32_WORST is that, rounded UP to the next tenth that leaves 2 % (another build of PyTorch sums a row in another order; the CPU test
# holds the measurement inside (FP32_WORST - 0.3, FP32_WORST]), and the constants are 4 x FP32_WORST:
#     K_y 12.0   K_rstd 5.6   K_zss 6.0   K_det 7.6   K_full 8.4   K_gelu 7.2   K_gelu_gx 10.0   K_fin_w 4.4   K_fin_c 19.6
FP32_WORST = {"y": 3.0, "rstd": 1.4, "zss": 1.5, "det": 1.9, "full": 2.1, "gelu": 1.8, "gelu_gx": 2.5, "fin_w": 1.1, "fin_c": 4.9}
K = {k: 4 * v for k, v in FP32_WORST.items()}

LN_FAMILIES = ("normal", "offset", "rowrange", "outlier", "constant")
GN_FAMILIES = ("normal", "offset", "grouprange")
AFFINES = ("wb", "w", "none")
LN_OPS = ("fwd", "stats", "bwd_detached", "bwd")
GN_OPS = ("fwd", "bwd_detached", "bwd")
DET_KEYS = ("--", "a-", "-m", "am")            # (addend given, mul2 given) of bcos_layernorm_bwd_detached


def _eps_tag(eps):
    return {1e-5: "e5", 1e-6: "e6"}[eps]


@dataclass(frozen=True)
class LN:
    family: str
    rows: int
    D: int
    affine: str = "wb"
    eps: float = 1e-5
    ops: tuple = LN_OPS
    kind = "ln"

    @property
    def id(self):
        return f"ln-{self.family}-r{self.rows}d{self.D}-{self.affine}-{_eps_tag(self.eps)}"


@dataclass(frozen=True)
class GN:
    family: str
    N: int
    HW: int
    C: int
    G: int
    affine: str = "wb"
    eps: float = 1e-5
    ops: tuple = GN_OPS
    kind = "gn"

    @property
    def id(self):
        return f"gn-{self.family}-n{self.N}hw{self.HW}c{self.C}g{self.G}-{self.affine}"


@dataclass(frozen=True)
class GELU:
    op: str           # "gate" (bcos_gelu_gate) or "bwd" (bcos_gelu_bwd)
    n: int
    kind = "gelu"

    @property
    def ops(self):
        return (self.op,)

    @property
    def id(self):
        return f"gelu-{self.op}-n{self.n}"


@dataclass(frozen=True)
class ADD:
    B: int
    T: int
    D: int
    kind = "add"
    ops = ("add",)

    @property
    def id(self):
        return f"add-b{self.B}t{self.T}d{self.D}"


@dataclass(frozen=True)
class FIN:
    N: int
    H: int
    W: int
    ps: int
    Cpad: int
    add_inverse: int
    gp_offset: int = 0                                   # gp is a view this many floats into its buffer
    outputs: tuple = ("both", "weights", "contrib")      # the launches of the GPU test
    kind = "fin"
    ops = ("finalize",)

    @property
    def id(self):
        return f"fin-n{self.N}h{self.H}w{self.W}p{self.ps}c{self.Cpad}-inv{self.add_inverse}" + ("-mis" if self.gp_offset else "")


# widths of the one-float4-per-lane kernels and of the strided loop (vec_ok: D % 4 == 0 and D <= 256), NV of layernorm_stats16_kernel
VEC_WIDTHS = (4, 64, 68, 192, 252, 256)
STRIDED_WIDTHS = (1, 3, 50, 65, 260, 384, 768, 1000)
FIRST_PASS_ROWS = 8192               # grid_rows: 2048 workgroups of four rows
FIRST_PASS_ROWS_STATS16 = 131072     # 8192 workgroups of sixteen rows
GELU_GATE_FIRST_PASS = 2048 * 256
GELU_BWD_FIRST_PASS = 8192 * 256


def _ln_table():
    t = []
    normal = [(4, 1), (4, 5), (4, 333), (64, 1), (64, 17), (68, 1), (68, 5), (68, 50), (68, 3), (192, 1), (192, 5), (192, 50), (192, 333),
              (252, 5), (252, 17), (256, 1), (256, 3), (256, 333),
              (1, 5), (3, 17), (50, 3), (65, 5), (65, 333), (260, 17), (384, 50), (768, 5), (1000, 3)]
    for i, (D, rows) in enumerate(normal):
        t.append(LN("normal", rows, D, AFFINES[i % 3], (1e-5, 1e-6)[i % 2]))
    i = 0
    for fam in LN_FAMILIES[1:]:
        for D, rows in ((68, 17), (192, 50), (65, 17), (1000, 5), (256, 5)):
            t.append(LN(fam, rows, D, AFFINES[i % 3], (1e-5, 1e-6)[(i // 3) % 2]))
            i += 1
    t.append(LN("constant", 17, 1, "wb"))
    # the second pass of the grid-stride loops
    t.append(LN("normal", FIRST_PASS_ROWS + 37, 8, "wb"))
    t.append(LN("offset", FIRST_PASS_ROWS + 37, 5, "w"))
    t.append(LN("normal", FIRST_PASS_ROWS_STATS16 + 21, 4, "wb", ops=("stats",)))
    t.append(LN("rowrange", FIRST_PASS_ROWS_STATS16 + 21, 68, "w", 1e-6, ops=("stats",)))
    return t


def _gn_table():
    geoms = [(1, 1, 2, 1), (2, 1, 4, 4), (2, 49, 12, 4), (3, 196, 48, 8), (2, 196, 64, 1), (2, 37, 32, 32), (1, 3136, 24, 4),
             (2, 85, 3, 1), (2, 64, 4, 1), (2, 257, 1, 1)]
    t = [GN("normal", *g, affine=("wb", "none")[i % 2]) for i, g in enumerate(geoms)]
    i = 0
    for fam in GN_FAMILIES[1:]:
        for g in ((2, 49, 12, 4), (3, 196, 48, 8), (2, 37, 32, 32), (2, 85, 3, 1), (2, 1, 4, 4), (2, 257, 1, 1)):
            t.append(GN(fam, *g, affine=("none", "wb")[i % 2]))
            i += 1
    return t


LN_CASES = _ln_table()
GN_CASES = _gn_table()
GELU_CASES = [GELU("gate", 77), GELU("gate", GELU_GATE_FIRST_PASS + 77), GELU("bwd", 77), GELU("bwd", GELU_BWD_FIRST_PASS + 77)]
ADD_CASES = [ADD(1, 1, 4), ADD(3, 5, 8), ADD(2, 197, 192), ADD(512, 1, 4104)]
FIN_CASES = [FIN(1, 4, 4, 1, 8, 1), FIN(2, 8, 12, 2, 8, 0), FIN(2, 12, 8, 4, 8, 1), FIN(1, 32, 48, 16, 8, 1),
             FIN(2, 8, 12, 2, 6, 1), FIN(2, 8, 12, 2, 12, 0), FIN(2, 8, 12, 2, 8, 1, gp_offset=1),
             FIN(65, 256, 256, 16, 8, 1, outputs=("contrib",))]
CASES = LN_CASES + GN_CASES + GELU_CASES + ADD_CASES + FIN_CASES
STD6 = (0.229, 0.224, 0.225, 0.231, 0.226, 0.222)


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def _seed(case):
    return sum((i + 1) * b for i, b in enumerate(case.id.encode())) % (2 ** 31)


def _pow10(g, shape, lo, hi):
    return 10.0 ** (torch.rand(shape, generator=g) * (hi - lo) + lo)


def _affine(g, case, C):
    """w with negative entries and one exact zero (w[1]; a single column keeps its negative entry), b; None where the case passes NULL"""
    w = torch.randn(C, generator=g)
    w[0] = -w[0].abs() - 0.25
    if C > 1:
        w[1] = 0.0
    b = torch.randn(C, generator=g)
    return (w if case.affine in ("wb", "w") else None), (b if case.affine == "wb" else None)


def eps32(case):
    """the eps the entry point receives (a float), promoted"""
    return float(torch.tensor(case.eps, dtype=torch.float32))


# ---- the Gaussian gate -------------------------------------------------------------------------------------------------------------
def _deriv(x):
    return 0.5 * math.erfc(-x / math.sqrt(2)) + x * math.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _deriv_zero():
    lo, hi = -0.8, -0.7            # Phi + x phi changes sign once in between
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _deriv(mid) < 0 else (lo, mid)
    return 0.5 * (lo + hi)


GELU_DERIV_ZERO = _deriv_zero()          # -0.75179...
GELU_HEAD = 6 + 29 + 200 + 8001


def gelu_vector(n, g):
    """specials, the integers, 200 points around the zero of the derivative, a dense grid over [-14, 14], then randn * 2; a shorter n
    takes the head of the same vector"""
    head = torch.cat([torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-6, -1e-6], dtype=torch.float64),
                      torch.arange(-14, 15, dtype=torch.float64),
                      GELU_DERIV_ZERO + torch.linspace(-2e-3, 2e-3, 200, dtype=torch.float64),
                      torch.linspace(-14, 14, 8001, dtype=torch.float64)]).float()
    assert head.numel() == GELU_HEAD
    if n <= GELU_HEAD:
        return head[:n].clone()
    return torch.cat([head, torch.randn(n - GELU_HEAD, generator=g) * 2])


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _ln_x(g, fam, rows, D):
    x = torch.randn(rows, D, generator=g)
    if fam == "offset":                  # |mean| = 100 .. 1000 x the row's spread, both signs
        spread = _pow10(g, (rows, 1), -1, 1)
        sign = (torch.randint(0, 2, (rows, 1), generator=g) * 2 - 1).float()
        x = spread * (x + sign * _pow10(g, (rows, 1), 2.1, 3))
    elif fam == "rowrange":              # every row at its own magnitude
        x = x * _pow10(g, (rows, 1), -3, 3)
    elif fam == "outlier":
        x = torch.where(torch.rand(x.shape, generator=g) < 0.02, x * 300, x)
    elif fam == "constant":              # every third row (every row of a single column) is one value
        vals = torch.tensor([-1000.0, 0.0, 1.0])
        for r in range(rows):
            if D == 1 or r % 3 == 0:
                x[r] = vals[(r // 3 if D > 1 else r) % 3]
    elif fam != "normal":
        raise ValueError(fam)
    return x


def constant_rows(case):
    return [r for r in range(case.rows) if case.D == 1 or r % 3 == 0]


def make_inputs(case):
    """the inputs of a case, fp32 on the CPU, a dict; the same tensors on every call"""
    g = torch.Generator().manual_seed(_seed(case))
    if case.kind == "ln":
        rows, D = case.rows, case.D
        x = _ln_x(g, case.family, rows, D)
        w, b = _affine(g, case, D)
        gy, addend, mul2 = (torch.randn(rows, D, generator=g) for _ in range(3))
        if case.family == "rowrange":
            gy = gy * _pow10(g, (rows, 1), -3, 3)
        inp = {"x": x, "w": w, "b": b, "gy": gy, "addend": addend, "mul2": mul2}
        inp["rstd"] = _ln_eval(x, w, b, gy, None, addend, mul2, eps32(case), torch.float32, fwd_only=True)["rstd"]
        return inp
    if case.kind == "gn":
        N, HW, C, G = case.N, case.HW, case.C, case.G
        x = torch.randn(N, HW, C, generator=g)
        if case.family == "offset":
            x = x + (torch.randint(0, 2, (N, 1, C), generator=g) * 2 - 1).float() * _pow10(g, (N, 1, 1), 2.1, 3)
        elif case.family == "grouprange":        # every (image, group) at its own magnitude and offset, decades apart
            k = torch.randperm(N * G, generator=g).float().reshape(N, 1, G, 1)
            mag = 10.0 ** (-3 + 6 * k / max(N * G - 1, 1))
            off = mag * 3 * (torch.randint(0, 2, (N, 1, G, 1), generator=g) * 2 - 1).float()
            x = (x.reshape(N, HW, G, C // G) * mag + off).reshape(N, HW, C)
        w, b = _affine(g, case, C)
        gy = torch.randn(N, HW, C, generator=g)
        inp = {"x": x, "w": w, "b": b, "gy": gy}
        inp["rstd"] = _gn_eval(case, inp, torch.float32, fwd_only=True)["rstd"]
        return inp
    if case.kind == "gelu":
        return {"x": gelu_vector(case.n, g), "gy": torch.randn(case.n, generator=g)}
    if case.kind == "add":
        return {"x": torch.randn(case.B, case.T, case.D, generator=g), "pe": torch.randn(case.T, case.D, generator=g)}
    if case.kind == "fin":
        N, H, W, ps, Cpad = case.N, case.H, case.W, case.ps, case.Cpad
        gh, gw = H // ps, W // ps
        gp = torch.randn(N, gh, gw, ps, ps, Cpad, generator=g) * _pow10(g, (N, gh, gw, ps, ps, 1), -3, 3)     # every pixel its own decade
        gp[..., 6:] = float("nan")               # the padding channels must not reach any output
        x = torch.rand(N, 3 if case.add_inverse else 6, H, W, generator=g)
        return {"gp": gp, "x": x, "std6": torch.tensor(STD6)}
    raise ValueError(case.kind)


# ---- the expressions, in a given precision (fp64: the reference; fp32: what the constants are measured with) ---------------------------
def _ln_eval(x, w, b, gy, rstd, addend, mul2, eps, dt, mut=None, fwd_only=False):
    """x, gy, addend, mul2 [R, n]; w, b None or broadcastable to [R, n]; rstd [R], the fp32 forward's (an input of the backward)"""
    x = x.to(dt)
    n = x.shape[1]
    pad = (n + 63) // 64 * 64
    wd = w.to(dt) if w is not None else None
    xs = x[:, :-1] if mut == "droplast" else x
    mean = xs.sum(1, keepdim=True) / n
    d = x - mean
    ds = d[:, :-1] if mut == "droplast" else d
    ss = (ds * ds).sum(1, keepdim=True)
    if mut == "maskedlane":              # the lanes past the row contribute (0 - mean)^2
        ss = ss + (pad - n) * mean * mean
    var = ss / (pad if mut == "padded" else n)
    if mut == "onepass":
        var = ((x * x).sum(1, keepdim=True) / n - mean * mean).clamp_min(0)
    sd = (var + eps).sqrt()
    xh = d / sd
    y = xh if wd is None else xh * wd
    if b is not None:
        y = y + b.to(dt)
    r = {"y": y, "rstd": (1.0 / sd).reshape(-1), "zss": (y * y).sum(1), "x_absmax": x.abs().amax(1)}
    if fwd_only:
        return r
    rs = rstd.to(dt).reshape(-1, 1)
    gy = gy.to(dt)
    h = (gy if wd is None else gy * wd) * rs
    o = h if mut == "det_nomean" else h - h.sum(1, keepdim=True) / n
    for key in DET_KEYS:
        oa = o + addend.to(dt) if key[0] == "a" else o
        r["out/" + key] = oa
        r["out2/" + key] = oa * mul2.to(dt) if key[1] == "m" else oa
    xhb = (x - x.sum(1, keepdim=True) / n) * rs
    hb = gy if wd is None else gy * wd
    mhx = (hb * xhb).sum(1, keepdim=True) / n
    gx = rs * (hb - hb.sum(1, keepdim=True) / n - (0 if mut == "full_nomhx" else xhb * mhx))
    r.update({"gx/-": gx, "gx/a": gx + addend.to(dt), "xhat": xhb})
    return r


def _ln_forms(x, w, gy, rstd, addend, mul2, eps, ref):
    x = x.double()
    A = x.abs().amax(1, keepdim=True)
    mean = x.mean(1, keepdim=True)
    sd = (((x - mean) ** 2).mean(1, keepdim=True) + eps).sqrt()
    xh = ((x - mean) / sd).abs()
    aw = w.double().abs() if w is not None else torch.ones_like(x)
    q = A / sd
    Fy = aw * (xh + q * (1 + xh)) + ref["y"].abs()
    f = {"y": ("y", U * Fy), "rstd": ("rstd", U * (1 + q.reshape(-1)) * ref["rstd"]),
         "zss": ("zss", U * (ref["zss"] + 2 * (ref["y"].abs() * Fy).sum(1)))}
    if "xhat" not in ref:
        return f
    rs = rstd.double().reshape(-1, 1)
    gy = gy.double()
    h = (gy * aw * rs).abs()
    base = h + h.mean(1, keepdim=True)
    for key in DET_KEYS:
        fo = base + (addend.double().abs() if key[0] == "a" else 0) + ref["out/" + key].abs()
        f["out/" + key] = ("det", U * fo)
        f["out2/" + key] = ("det", U * (fo * (mul2.double().abs() if key[1] == "m" else 1) + ref["out2/" + key].abs()))
    xhb = ref["xhat"].abs()
    E = xhb + A * rs * (1 + xhb)
    hb = (gy * aw).abs()
    fb = rs * (hb + hb.mean(1, keepdim=True)) + rs * (E * (hb * xhb).mean(1, keepdim=True) + xhb * (hb * E).mean(1, keepdim=True))
    f["gx/-"] = ("full", U * (fb + ref["gx/-"].abs()))
    f["gx/a"] = ("full", U * (fb + addend.double().abs() + ref["gx/a"].abs()))
    f["xhat"] = ("y", U * (E + xhb))
    return f


def _gn_channels(case, device, mut=None):
    cg = case.C // case.G
    gi, ci = torch.arange(case.G, device=device).reshape(-1, 1), torch.arange(cg, device=device).reshape(1, -1)
    return ((gi if mut == "gn_goffset" else gi * cg) + ci).reshape(-1)


def _gn_rows(t, case, ch):
    """[N, HW, C] -> [N G, HW cg]: one row per (image, group)"""
    N, HW, G, cg = case.N, case.HW, case.G, case.C // case.G
    return t[:, :, ch].reshape(N, HW, G, cg).permute(0, 2, 1, 3).reshape(N * G, HW * cg)


def _gn_vec(v, case, ch):
    """[C] -> [N G, HW cg]"""
    N, HW, G, cg = case.N, case.HW, case.G, case.C // case.G
    return v[ch].reshape(1, G, 1, cg).expand(N, G, HW, cg).reshape(N * G, HW * cg)


def _gn_back(r, case, ch):
    N, HW, G, cg = case.N, case.HW, case.G, case.C // case.G
    out = torch.zeros(N, HW, case.C, dtype=r.dtype, device=r.device)
    out[:, :, ch] = r.reshape(N, G, HW, cg).permute(0, 2, 1, 3).reshape(N, HW, case.C)
    return out


GN_NAMES = {"y": "y", "out/--": "gx_det", "gx/-": "gx", "xhat": "xhat"}       # row-matrix result -> output of the GroupNorm entry points


def _gn_eval(case, inp, dt, mut=None, fwd_only=False):
    if mut == "gn_whole":                # normalised over the whole image; the affine stays per channel
        return {"y": _gn_eval(replace(case, G=1), inp, dt, fwd_only=True)["y"]}
    dev = inp["x"].device
    ch, good = _gn_channels(case, dev, mut), _gn_channels(case, dev)
    w = _gn_vec(inp["w"], case, good) if inp["w"] is not None else None
    b = _gn_vec(inp["b"], case, good) if inp["b"] is not None else None
    zero = torch.zeros(case.N * case.G, case.HW * (case.C // case.G), device=dev)
    r = _ln_eval(_gn_rows(inp["x"], case, ch), w, b, _gn_rows(inp["gy"], case, ch), inp.get("rstd"), zero, zero, eps32(case), dt,
                 fwd_only=fwd_only)
    out = {"rstd": r["rstd"]}
    for k, name in GN_NAMES.items():
        if k in r:
            out[name] = _gn_back(r[k], case, ch)
    return out


def _gn_forms(case, inp, ref):
    ch = _gn_channels(case, inp["x"].device)
    rows = {k: _gn_rows(ref[name], case, ch) for k, name in GN_NAMES.items()}
    rows["rstd"] = ref["rstd"]
    rows["zss"] = (rows["y"] ** 2).sum(1)
    for key in DET_KEYS:
        rows["out/" + key] = rows["out2/" + key] = rows["out/--"]
    rows["gx/a"] = rows["gx/-"]
    w = _gn_vec(inp["w"], case, ch) if inp["w"] is not None else None
    x = _gn_rows(inp["x"], case, ch)
    zero = torch.zeros_like(x)
    f = _ln_forms(x, w, _gn_rows(inp["gy"], case, ch), inp["rstd"], zero, zero, eps32(case), rows)
    out = {"rstd": f["rstd"]}
    for k, name in GN_NAMES.items():
        out[name] = (f[k][0], _gn_back(f[k][1], case, ch))
    return out


AS_COEFFS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)        # a1 .. a5 of 7.1.26, p = 0.3275911


def gate_poly(x, dt):
    """bcos_gelu_gate (csrc/bcos_internal.h) restated: the same polynomial, an exact division, torch.exp"""
    x = x.to(dt)
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    poly = 1.061405429 * t + -1.453152027
    poly = poly * t + 1.421413741
    poly = poly * t + -0.284496736
    poly = poly * t + 0.254829592
    half = 0.5 * (poly * t * torch.exp(-z * z))
    return torch.where(x >= 0, 1.0 - half, half)


def _gelu_eval(inp, dt, mut=None, exact=False):
    x, gy = inp["x"].to(dt), inp["gy"].to(dt)
    if exact:
        gate = 0.5 * torch.erfc(-x / math.sqrt(2))
    elif mut == "tanh":
        gate = 0.5 * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    else:
        gate = gate_poly(x, dt)
    phi = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return {"gate": gate, "y": gate * x, "gx": gy * (gate + x * phi)}


def _gelu_forms(inp, ref):
    x, gy = inp["x"].double().abs(), inp["gy"].double().abs()
    Phi = ref["gate"]
    z = x * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    powers = [t ** (k + 1) for k in range(5)]
    cond = sum(abs(a) * p for a, p in zip(AS_COEFFS, powers)) / sum(a * p for a, p in zip(AS_COEFFS, powers))
    G = (cond + 2 * z * z) * torch.minimum(Phi, 1 - Phi) + Phi
    phi = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return {"gate": ("gelu", U * G, torch.full_like(G, E_AS)),
            "y": ("gelu", U * x * G, x * E_AS + U * ref["y"].abs()),
            "gx": ("gelu_gx", U * gy * (G + x * phi * (1 + x * x)), gy * E_AS + U * ref["gx"].abs())}


def _fin_eval(case, inp, dt, mut=None):
    N, H, W, ps, Cpad = case.N, case.H, case.W, case.ps, case.Cpad
    gh, gw = H // ps, W // ps
    gp, x, std6 = inp["gp"], inp["x"].to(dt), inp["std6"].to(dt)
    if mut == "gw_from_h":               # the patch row pitch taken from the image height
        dev = gp.device
        n, hh, ww = (torch.arange(k, device=dev).reshape(s) for k, s in ((N, (-1, 1, 1)), (H, (1, -1, 1)), (W, (1, 1, -1))))
        idx = ((((n * gh + hh // ps) * gh + ww // ps) * ps + hh % ps) * ps + ww % ps) % (N * H * W)
        g = gp.reshape(N * H * W, Cpad)[idx.reshape(-1)][:, :6].to(dt).reshape(N, H, W, 6).permute(0, 3, 1, 2)
    else:
        g = gp.reshape(N, gh, gw, ps, ps, Cpad)[..., :6].to(dt).permute(0, 5, 1, 3, 2, 4).reshape(N, 6, H, W)
    wt = g / std6.reshape(1, 6, 1, 1)
    x6 = torch.cat([x, 1.0 - x], 1) if case.add_inverse else x
    return {"weights": wt, "contrib": (x6 * wt).sum(1)}


def _fin_forms(case, inp, ref):
    x = inp["x"].double()
    x6 = torch.cat([x, 1.0 - x], 1) if case.add_inverse else x
    return {"weights": ("fin_w", U * ref["weights"].abs()), "contrib": ("fin_c", U * (x6 * ref["weights"]).abs().sum(1))}


def evaluate(case, inp, dt, mut=None):
    """every output of the case's entry points by the documented expressions in `dt`; `mut` names a deliberate mistake"""
    if case.kind == "ln":
        return _ln_eval(inp["x"], inp["w"], inp["b"], inp["gy"], inp["rstd"], inp["addend"], inp["mul2"], eps32(case), dt, mut)
    if case.kind == "gn":
        return _gn_eval(case, inp, dt, mut)
    if case.kind == "gelu":
        return _gelu_eval(inp, dt, mut)
    if case.kind == "add":
        return {"x": (inp["x"].reshape(case.B, -1) + inp["pe"].reshape(1, -1)).reshape(inp["x"].shape)}       # fp32: exact, no `dt`
    return _fin_eval(case, inp, dt, mut)


def reference(case, inp):
    """fp64, from the fp32 inputs promoted; the backward outputs from inp["rstd"], the fp32 forward's, promoted -- not recomputed"""
    if case.kind == "gelu":
        return _gelu_eval(inp, torch.float64, exact=True)
    return evaluate(case, inp, torch.float64)


def forms(case, inp, ref):
    """output name -> (constant's name, per-element form that K multiplies, per-element additive term or None)"""
    if case.kind == "ln":
        f = _ln_forms(inp["x"], inp["w"], inp["gy"], inp["rstd"], inp["addend"], inp["mul2"], eps32(case), ref)
    elif case.kind == "gn":
        f = _gn_forms(case, inp, ref)
    elif case.kind == "gelu":
        return _gelu_forms(inp, ref)
    elif case.kind == "fin":
        f = _fin_forms(case, inp, ref)
    else:
        return {}
    return {k: (v[0], v[1], None) for k, v in f.items()}


def bounds(case, inp, ref):
    """output name -> per-element bound on |output - ref[name]|"""
    return {k: K[key] * form + (0 if add is None else add) for k, (key, form, add) in forms(case, inp, ref).items()}


def use(out, ref, form, add=None):
    """(worst over EVERY element of (|out - ref| - add) / form -- to be compared with K --, the flat index of that element); an exact
    element counts as 0 whatever its form, a NaN anywhere gives NaN"""
    err = (out.double() - ref).abs()
    if add is not None:
        err = (err - add).clamp_min(0)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / form).reshape(-1)
    if bool(torch.isnan(ratio).any()) or bool(torch.isnan(out).any()):
        return float("nan"), int(torch.isnan(ratio).to(torch.int8).argmax())
    i = int(ratio.argmax())
    return float(ratio[i]), i


def fp32_uses(case, inp=None):
    """the worst use of every form by the plain fp32 evaluation: {constant's name: (use, output name)}.  The GELU's fp32 restatement
    is measured against the same polynomial in fp64 (module docstring)."""
    inp = make_inputs(case) if inp is None else inp
    ref = reference(case, inp)
    f = forms(case, inp, ref)
    r32 = evaluate(case, inp, torch.float32)
    if case.kind == "gelu":
        ref = evaluate(case, inp, torch.float64)
        # (below the smallest normal, 2^-126, fp32 resolves 2^-149 only: an absolute error that E_AS covers 10^30 times over)
        tiny = 2.0 ** -126 * (1 + inp["x"].double().abs())
        f = {k: (key, form, tiny * (inp["gy"].double().abs() if k == "gx" else 1)) for k, (key, form, _) in f.items()}
    res = {}
    for name, (key, form, add) in f.items():
        v = use(r32[name], ref[name], form, add)[0]
        if key not in res or not v <= res[key][0]:
            res[key] = (v, name)
    return res
