"""The case table of the uncentered-norm entry points of csrc/bcos_norms.hip (include/bcos_hip.h: bcos_layernorm_unc_fwd / _bwd_detached /
_bwd, bcos_groupnorm_unc_fwd / _bwd_detached / _bwd), the fp64 reference of what they compute and the PER-ELEMENT bounds every output is
held to.  The manner is that of tests/token_cases.py, whose input families, affine vectors, (image, group) <-> row mapping and `use` this
module shares.

Over a set S of n values (a row; an (image, group)):  m = mean x, var = mean (x - m)^2, sd = sqrt(var + eps), r = 1 / sd,
    y = w x / sd + b                         (posnorm_uncentered.py:39-58, groupnorm_uncentered.py:21-61: the value divided is x, not x - m)
    detached (var a constant)    out = h r + addend, h = gy w;   out2 = out mul2
    full                         gx = r h - r^3 (x - m) (sum_S h x) / n (+ addend);   xr = x r  (for the weight gradient)
Reference: those expressions in fp64 from the fp32 inputs promoted (eps the fp32 value the entry point receives).  The BACKWARD entry
points take rstd as an INPUT: their reference uses the fp32 rstd of the fp32 forward formula (make_inputs: "rstd"), promoted -- only the
mean of the full backward is recomputed, in fp64.

Bounds, with u = 2^-24, A = max_S |x|, q = A / sd (`x - m` is exact only to u A: that is a relative u A / sd in the centred second moment's
root -- the only place the mean enters the forward) and d = x - m64:
    y         |y - y64|      <= K_y    u ( |w| |x / sd| (1 + q) + |y64| )           the division and the error of sd through w; the affine
    rstd      |rstd sd - 1|  <= K_rstd u ( 1 + q )                                  sqrt / reciprocal roundings; the relative error of sd
    det       |o - o64|      <= K_det  u ( |h r| + |addend| + |o64| )               two products; the add
              |o2 - o2_64|   <= K_det  u ( (that form) |mul2| + |o2_64| )           the error of o carried by mul2; the product's rounding
    full      |gx - gx64|    <= K_full u ( r |h| + r^3 (|d| + A) mean_S |h x| + |addend| + |gx64| )
              the first product; in the second term the roundings of r^3, of the sum (mean |h x|: no credit for cancellation in sum h x)
              and of its products scale with |d|, and the error u A of `x - m` with A -- in units of sd that is the (A / sd) of the
              existing LayerNorm lines; the adds
    xr        |xr - xr64|    <= K_xr   u |xr64|                                      one product
No term takes credit for cancellation: a row whose mean is 1000 x its spread, or a constant row (sd = sqrt(eps)), is held to the q term
and no closer.

tests/test_unorm_cases_cpu.py evaluates the same expressions in plain fp32 PyTorch for every case, prints the worst use of each form and
pins the constants: K = 4 x that worst use (the project's rule; the 4 covers the kernels' lane-tree and workgroup summation orders and the
fused multiply-adds of the device compiler, nothing more).  tests/test_unorm_gpu.py launches every case through the C ABI and judges every
element.

A plain module (no fixtures, no collection hooks): the two test files import it.
"""
from dataclasses import dataclass

import torch

import token_cases as tc

U = tc.U
DET_KEYS = tc.DET_KEYS             # (addend given, mul2 given) of bcos_layernorm_unc_bwd_detached: "--", "a-", "-m", "am"

# worst |fp32 PyTorch - fp64| / form over the case table, in units of u, as test_unorm_cases_cpu.py measures and prints it:
#     y 1.015   rstd 1.046   det 1.222 (out/a-)   (all three: row-normal-r8229d8-wb-e5)
#     full 2.391 (row-offset-r8229d5-w-e5, gx/-)   xr 0.999 (grp-offset-n3hw196c48g8-none)
# FP32_WORST is that, rounded UP to the next tenth that leaves 2 % (another build of PyTorch sums a row in another order; the CPU test
# holds the measurement inside (FP32_WORST - 0.3, FP32_WORST]), and the constants are 4 x FP32_WORST:
#     K_y 4.4   K_rstd 4.4   K_det 5.2   K_full 10.0   K_xr 4.4
FP32_WORST = {"y": 1.1, "rstd": 1.1, "det": 1.3, "full": 2.5, "xr": 1.1}
K = {k: 4 * v for k, v in FP32_WORST.items()}

ROW_FAMILIES = tc.LN_FAMILIES      # normal, offset (|mean| = 100 .. 1000 x spread), rowrange, outlier, constant
GRP_FAMILIES = tc.GN_FAMILIES      # normal, offset, grouprange
AFFINES = tc.AFFINES               # wb, w, none
OPS = ("fwd", "bwd_detached", "bwd")
MUTATIONS = ("centred", "full_nomean", "n_off")


@dataclass(frozen=True)
class ROW:
    family: str
    rows: int
    D: int
    affine: str = "wb"
    eps: float = 1e-5
    misaligned: bool = False       # the GPU test passes x / gy / y / out as views one float into their buffers
    kind = "row"

    @property
    def id(self):
        return f"row-{self.family}-r{self.rows}d{self.D}-{self.affine}-{tc._eps_tag(self.eps)}" + ("-mis" if self.misaligned else "")


@dataclass(frozen=True)
class GRP:
    family: str
    N: int
    HW: int
    C: int
    G: int
    affine: str = "wb"
    eps: float = 1e-5
    kind = "grp"

    @property
    def id(self):
        return f"grp-{self.family}-n{self.N}hw{self.HW}c{self.C}g{self.G}-{self.affine}"


# widths of the one-float4-per-lane kernels and of the strided loop (vec_ok: D % 4 == 0, D <= 256, 16-byte aligned)
VEC_WIDTHS = (4, 64, 68, 96, 252, 256)
STRIDED_WIDTHS = (1, 3, 50, 65, 260, 1000)
FIRST_PASS_ROWS = 8192               # grid_rows: 2048 workgroups of four rows


def _row_table():
    t = []
    # (D, rows): rows of 1, 3, 5, 17 leave a wavefront group of four partly empty
    normal = [(4, 1), (4, 333), (64, 17), (68, 5), (96, 3), (96, 50), (252, 17), (256, 1), (256, 333),
              (1, 5), (3, 17), (50, 3), (65, 333), (260, 17), (1000, 3)]
    for i, (D, rows) in enumerate(normal):
        t.append(ROW("normal", rows, D, AFFINES[i % 3], (1e-5, 1e-6)[i % 2]))
    i = 0
    for fam in ROW_FAMILIES[1:]:
        for D, rows in ((68, 17), (65, 17), (1000, 5), (256, 5)):
            t.append(ROW(fam, rows, D, AFFINES[i % 3], (1e-5, 1e-6)[(i // 3) % 2]))
            i += 1
    t.append(ROW("constant", 17, 1, "wb"))
    # a width divisible by 4 on the strided kernels: every large operand one float off a 16-byte boundary
    t.append(ROW("normal", 17, 68, "wb", misaligned=True))
    t.append(ROW("offset", 5, 256, "w", misaligned=True))
    # the second pass of the grid-stride loops, both kernel forms
    t.append(ROW("normal", FIRST_PASS_ROWS + 37, 8, "wb"))
    t.append(ROW("offset", FIRST_PASS_ROWS + 37, 5, "w"))
    return t


def _grp_table():
    # (N, HW, C, G): groups of 1 .. 18 816 values; HW = 85 (5 x 17) and 37 are rectangular images; G = 1, G = C and in between
    geoms = [(1, 1, 2, 1), (2, 1, 4, 4), (2, 49, 12, 4), (3, 196, 48, 8), (2, 196, 64, 1), (2, 37, 32, 32), (1, 3136, 24, 4),
             (2, 85, 3, 1), (2, 64, 4, 1), (2, 257, 1, 1)]
    t = [GRP("normal", *g, affine=AFFINES[i % 3]) for i, g in enumerate(geoms)]
    i = 0
    for fam in GRP_FAMILIES[1:]:
        for g in ((2, 49, 12, 4), (3, 196, 48, 8), (2, 37, 32, 32), (2, 85, 3, 1), (2, 1, 4, 4)):
            t.append(GRP(fam, *g, affine=AFFINES[(i + 1) % 3]))
            i += 1
    return t


ROW_CASES = _row_table()
GRP_CASES = _grp_table()
CASES = ROW_CASES + GRP_CASES


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


eps32 = tc.eps32


def make_inputs(case):
    """the inputs of a case, fp32 on the CPU, a dict; the same tensors on every call"""
    g = torch.Generator().manual_seed(tc._seed(case))
    if case.kind == "row":
        rows, D = case.rows, case.D
        x = tc._ln_x(g, case.family, rows, D)
        w, b = tc._affine(g, case, D)
        gy, addend, mul2 = (torch.randn(rows, D, generator=g) for _ in range(3))
        if case.family == "rowrange":
            gy = gy * tc._pow10(g, (rows, 1), -3, 3)
        inp = {"x": x, "w": w, "b": b, "gy": gy, "addend": addend, "mul2": mul2}
        inp["rstd"] = _row_eval(x, w, b, gy, None, addend, mul2, eps32(case), torch.float32, fwd_only=True)["rstd"]
        return inp
    N, HW, C, G = case.N, case.HW, case.C, case.G
    x = torch.randn(N, HW, C, generator=g)
    if case.family == "offset":
        x = x + (torch.randint(0, 2, (N, 1, C), generator=g) * 2 - 1).float() * tc._pow10(g, (N, 1, 1), 2.1, 3)
    elif case.family == "grouprange":        # every (image, group) at its own magnitude and offset, decades apart
        k = torch.randperm(N * G, generator=g).float().reshape(N, 1, G, 1)
        mag = 10.0 ** (-3 + 6 * k / max(N * G - 1, 1))
        off = mag * 3 * (torch.randint(0, 2, (N, 1, G, 1), generator=g) * 2 - 1).float()
        x = (x.reshape(N, HW, G, C // G) * mag + off).reshape(N, HW, C)
    w, b = tc._affine(g, case, C)
    gy = torch.randn(N, HW, C, generator=g)
    inp = {"x": x, "w": w, "b": b, "gy": gy}
    inp["rstd"] = _grp_eval(case, inp, torch.float32, fwd_only=True)["rstd"]
    return inp


# ---- the expressions, in a given precision (fp64: the reference; fp32: what the constants are measured with) ---------------------------
def _row_eval(x, w, b, gy, rstd, addend, mul2, eps, dt, mut=None, fwd_only=False):
    """x, gy, addend, mul2 [R, n]; w, b None or broadcastable to [R, n]; rstd [R], the fp32 forward's (an input of the backward).
    `mut`: a deliberate mistake -- "centred" (the mean subtracted from the value that is divided), "full_nomean" (the mean term dropped
    from the full gradient), "n_off" (n wrong by one)"""
    x = x.to(dt)
    n = x.shape[1]
    nn = n + 1 if mut == "n_off" else n
    wd = w.to(dt) if w is not None else None
    mean = x.sum(1, keepdim=True) / nn
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / nn
    sd = (var + eps).sqrt()
    xr = (d if mut == "centred" else x) / sd
    y = xr if wd is None else xr * wd
    if b is not None:
        y = y + b.to(dt)
    r = {"y": y, "rstd": (1.0 / sd).reshape(-1)}
    if fwd_only:
        return r
    rs = rstd.to(dt).reshape(-1, 1)
    gy = gy.to(dt)
    h = gy if wd is None else gy * wd
    o = h * rs
    for key in DET_KEYS:
        oa = o + addend.to(dt) if key[0] == "a" else o
        r["out/" + key] = oa
        r["out2/" + key] = oa * mul2.to(dt) if key[1] == "m" else oa
    db = x if mut == "full_nomean" else x - x.sum(1, keepdim=True) / nn
    coef = rs * rs * rs * ((h * x).sum(1, keepdim=True) / nn)
    gx = rs * h - coef * db
    r.update({"gx/-": gx, "gx/a": gx + addend.to(dt), "xr": x * rs})
    return r


def _row_forms(x, w, gy, rstd, addend, mul2, eps, ref):
    x = x.double()
    A = x.abs().amax(1, keepdim=True)
    mean = x.mean(1, keepdim=True)
    d = (x - mean).abs()
    sd = ((d ** 2).mean(1, keepdim=True) + eps).sqrt()
    aw = w.double().abs() if w is not None else torch.ones_like(x)
    q = A / sd
    f = {"y": ("y", U * (aw * (x.abs() / sd) * (1 + q) + ref["y"].abs())), "rstd": ("rstd", U * (1 + q.reshape(-1)) * ref["rstd"])}
    if "xr" not in ref:
        return f
    rs = rstd.double().reshape(-1, 1)
    h = (gy.double() * aw).abs()
    for key in DET_KEYS:
        fo = h * rs + (addend.double().abs() if key[0] == "a" else 0) + ref["out/" + key].abs()
        f["out/" + key] = ("det", U * fo)
        f["out2/" + key] = ("det", U * (fo * (mul2.double().abs() if key[1] == "m" else 1) + ref["out2/" + key].abs()))
    fb = rs * h + rs ** 3 * (d + A) * (h * x.abs()).mean(1, keepdim=True)
    f["gx/-"] = ("full", U * (fb + ref["gx/-"].abs()))
    f["gx/a"] = ("full", U * (fb + addend.double().abs() + ref["gx/a"].abs()))
    f["xr"] = ("xr", U * ref["xr"].abs())
    return f


GRP_NAMES = {"y": "y", "out/--": "gx_det", "gx/-": "gx", "xr": "xr"}       # row-matrix result -> output of the group entry points


def _grp_eval(case, inp, dt, mut=None, fwd_only=False):
    ch = tc._gn_channels(case, inp["x"].device)
    w = tc._gn_vec(inp["w"], case, ch) if inp["w"] is not None else None
    b = tc._gn_vec(inp["b"], case, ch) if inp["b"] is not None else None
    zero = torch.zeros(case.N * case.G, case.HW * (case.C // case.G), device=inp["x"].device)
    r = _row_eval(tc._gn_rows(inp["x"], case, ch), w, b, tc._gn_rows(inp["gy"], case, ch), inp.get("rstd"), zero, zero, eps32(case), dt,
                  mut, fwd_only=fwd_only)
    out = {"rstd": r["rstd"]}
    for k, name in GRP_NAMES.items():
        if k in r:
            out[name] = tc._gn_back(r[k], case, ch)
    return out


def _grp_forms(case, inp, ref):
    ch = tc._gn_channels(case, inp["x"].device)
    rows = {k: tc._gn_rows(ref[name], case, ch) for k, name in GRP_NAMES.items()}
    rows["rstd"] = ref["rstd"]
    for key in DET_KEYS:
        rows["out/" + key] = rows["out2/" + key] = rows["out/--"]
    rows["gx/a"] = rows["gx/-"]
    w = tc._gn_vec(inp["w"], case, ch) if inp["w"] is not None else None
    x = tc._gn_rows(inp["x"], case, ch)
    zero = torch.zeros_like(x)
    f = _row_forms(x, w, tc._gn_rows(inp["gy"], case, ch), inp["rstd"], zero, zero, eps32(case), rows)
    out = {"rstd": f["rstd"]}
    for k, name in GRP_NAMES.items():
        out[name] = (f[k][0], tc._gn_back(f[k][1], case, ch))
    return out


def evaluate(case, inp, dt, mut=None):
    """every output of the case's entry points by the documented expressions in `dt`; `mut` names a deliberate mistake"""
    if case.kind == "row":
        return _row_eval(inp["x"], inp["w"], inp["b"], inp["gy"], inp["rstd"], inp["addend"], inp["mul2"], eps32(case), dt, mut)
    return _grp_eval(case, inp, dt, mut)


def reference(case, inp):
    """fp64, from the fp32 inputs promoted; the backward outputs from inp["rstd"], the fp32 forward's, promoted -- not recomputed"""
    return evaluate(case, inp, torch.float64)


def forms(case, inp, ref):
    """output name -> (constant's name, per-element form that K multiplies)"""
    if case.kind == "row":
        return _row_forms(inp["x"], inp["w"], inp["gy"], inp["rstd"], inp["addend"], inp["mul2"], eps32(case), ref)
    return _grp_forms(case, inp, ref)


def bounds(case, inp, ref):
    """output name -> per-element bound on |output - ref[name]|"""
    return {k: K[key] * form for k, (key, form) in forms(case, inp, ref).items()}


use = tc.use


def uses(case, out, inp=None, ref=None):
    """the worst use of every form by `out` (output name -> tensor): {constant's name: (use, output name)}"""
    inp = make_inputs(case) if inp is None else inp
    ref = reference(case, inp) if ref is None else ref
    res = {}
    for name, (key, form) in forms(case, inp, ref).items():
        v = use(out[name], ref[name], form)[0]
        if key not in res or not v <= res[key][0]:
            res[key] = (v, name)
    return res


def fp32_uses(case, mut=None):
    """the worst use of every form by the plain fp32 evaluation (with `mut`: by the deliberately mistaken one)"""
    inp = make_inputs(case)
    return uses(case, evaluate(case, inp, torch.float32, mut), inp)
