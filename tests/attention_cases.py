"""The case table of the attention entry points (include/bcos_hip.h: bcos_attention_fwd / bcos_attention_bwd_v), the fp64 reference
of what they compute and the PER-ELEMENT bounds every output is held to.

Reference, per (image, head), from the fp32 inputs promoted to fp64:
    s = scale q k^T,  m = rowmax(s),  l = sum_k exp(s - m),  p = exp(s - m) / l,  out = p v,  gv = p^T gout.
Bounds, with u = 2^-24 and delta[q] = scale ||q||_2 max_k ||k||_2 (the Cauchy-Schwarz size of a score of row q):
    |out - out64|[q, d]   <= K_OUT  u ( (2 delta[q] + 4) (p64 |v|)[q, d] + max_k |v[k, d]| )
    |gv - gv64|[k, d]     <= K_GV   u ( sum_q p64[q, k] (2 delta[q] + 4) |gout[q, d]| + max(1, sum_q p64[q, k]) max_q |gout[q, d]| )
    |stats[..., 0] - m64| <= K_MAX  u ( delta + |m64| )
    |stats[..., 1] l64 - 1| <= K_RSUM u ( 2 delta + 4 )
2 delta is a score error carried through the softmax, + 4 the exponential and the normalisation, and the column-maximum term the
per-feature scaling of the value operand of the f16 kernels: the error of an element of v / gout is relative to its column's
maximum, not to itself.

tests/test_attention_cases_cpu.py evaluates the same expression in plain fp32 PyTorch for every case, prints the worst use of each
form and pins the constants: K = 4 x that worst use (the 4 covers the kernels' chunked summation order with online rescaling, the
hardware's 1-ulp exp2 and the 2^-22 = 4 u element resolution of a two-way fp16 split, nothing more).
tests/test_attention_gpu.py launches every case on both kernel families and judges every element.

A plain module (no fixtures, no collection hooks): the two test files import it.
"""
from dataclasses import dataclass

import torch

U = 2.0 ** -24
DH = 64
SCALE = 0.125

# worst |fp32 PyTorch - fp64| / form over CASES, in units of u, as test_attention_cases_cpu.py measures and prints it:
#     out 1.732 (hot-b2h3t197)   gv 1.933 (offset-b2h3t33)   row max 5.506 (outlier-b2h3t288)   1 / row sum 3.580 (negscore-b2h3t197)
# FP32_WORST is that, rounded UP to the next tenth that leaves 2 % (another BLAS sums the 64 products of a score in another order; the
# CPU test holds the measurement inside (FP32_WORST - 0.3, FP32_WORST]), and the constants are 4 x FP32_WORST:
#     K_OUT = 7.2   K_GV = 8.0   K_MAX = 22.8   K_RSUM = 14.8
FP32_WORST = {"out": 1.8, "gv": 2.0, "max": 5.7, "rsum": 3.7}
K_OUT = 4 * FP32_WORST["out"]
K_GV = 4 * FP32_WORST["gv"]
K_MAX = 4 * FP32_WORST["max"]
K_RSUM = 4 * FP32_WORST["rsum"]
K = {"out": K_OUT, "gv": K_GV, "max": K_MAX, "rsum": K_RSUM}

FAMILIES = ("normal", "spread", "hot", "tokrange", "colrange", "outlier", "offset", "negscore")


@dataclass(frozen=True)
class Case:
    family: str
    T: int
    B: int = 2
    H: int = 3

    @property
    def id(self):
        return f"{self.family}-b{self.B}h{self.H}t{self.T}"


def _table():
    cases = [Case("normal", T) for T in (1, 31, 32, 33, 64, 65, 197, 256, 257, 288)]
    cases += [Case("normal", 50, B=1, H=32), Case("normal", 17, B=3, H=1)]           # the CLIP attention pool; one head
    for fam in FAMILIES[1:]:
        cases += [Case(fam, T) for T in (33, 197, 288)]
    return cases


CASES = _table()


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def make_inputs(case):
    """(qkv [B, T, 3 H 64] laid out "(three h d)", gout [B, T, H 64]) of a case, fp32 on the CPU; the same tensors on every call.
    Batches and heads carry different data."""
    B, T, H = case.B, case.T, case.H
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(case.family) + 7 * T + 131 * B + H)
    x = torch.randn(B, T, 3, H, DH, generator=g)
    go = torch.randn(B, T, H, DH, generator=g)
    fam = case.family

    def pow10(shape, lo, hi):
        return 10.0 ** (torch.rand(shape, generator=g) * (hi - lo) + lo)

    if fam == "spread":                 # a peaked softmax
        x, go = x * 4, go * 4
    elif fam == "hot":                  # row maxima of the scores far beyond 88: exp overflows fp32 unless the maximum is subtracted first
        x[:, :, :2] *= 8
    elif fam == "tokrange":             # every token of q, k and v (per head) at its own magnitude: the per-row scales of X and Y
        x = x * pow10((B, T, 3, H, 1), -2, 1)
    elif fam == "colrange":             # every feature at its own magnitude: the per-feature scale of Z, and where it is undone
        x[:, :, :2] *= pow10((1, 1, 2, H, DH), -1, 1)
        x[:, :, 2] *= pow10((1, 1, H, DH), -4, 4)
        go = go * pow10((1, 1, H, DH), -4, 4)
    elif fam == "outlier":              # elements far below their row's maximum live in the low plane of a split
        x = torch.where(torch.rand(x.shape, generator=g) < 0.02, x * 300, x)
        go = torch.where(torch.rand(go.shape, generator=g) < 0.02, go * 300, go)
    elif fam == "offset":               # strong cancellation in gv
        x[:, :, :2] += 3
        x[:, :, 2] += 100
    elif fam == "negscore":
        # q = c + noise with |c_d| = 3 (one sign pattern per image and head), k = -q moved on by one token: every real score is
        # -0.125 (|c|^2 = 576) +- a few units, i.e. <= -50, while a zero-padded key has the raw score 0
        c = 3.0 * (torch.randint(0, 2, (B, 1, H, DH), generator=g) * 2 - 1).float()
        x[:, :, 0] = c + 0.25 * x[:, :, 0]
        x[:, :, 1] = -torch.roll(x[:, :, 0], 1, dims=1)
    elif fam != "normal":
        raise ValueError(fam)
    return x.reshape(B, T, 3 * H * DH).contiguous(), go.reshape(B, T, H * DH).contiguous()


def heads(t, H):
    """[B, T, H 64] -> [B, H, T, 64]"""
    B, T, _ = t.shape
    return t.reshape(B, T, H, DH).transpose(1, 2)


def tokens(t):
    """[B, H, T, 64] -> [B, T, H 64]"""
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B, T, H * DH)


def split_qkv(qkv, H):
    return tuple(heads(t, H) for t in qkv.split(H * DH, dim=-1))


def evaluate(qkv, gout, H, dtype, scale=SCALE, q_override=None):
    """the reference expression in `dtype` (fp64: the reference; fp32: what the constants are measured with).  Returns a dict of
    out, gv [B, T, H 64] and m, l [B, H, T], and p [B, H, T, T]."""
    q, k, v = (t.to(dtype) for t in split_qkv(qkv, H))
    if q_override is not None:
        q = q_override.to(dtype)
    go = heads(gout, H).to(dtype)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(-1)
    e = torch.exp(s - m.unsqueeze(-1))
    l = e.sum(-1)
    p = e / l.unsqueeze(-1)
    return {"out": tokens(p @ v), "gv": tokens(p.transpose(-1, -2) @ go), "m": m, "l": l, "p": p}


def reference(qkv, gout, H, scale=SCALE):
    """fp64 values and the four bound FORMS (without their constants K): {"out": (value, form), "gv": ..., "max": ..., "rsum": ...}.
    The value of "rsum" is l64: the quantity judged is stats[..., 1] l64 - 1."""
    r = evaluate(qkv, gout, H, torch.float64, scale)
    q, k, v = (t.double() for t in split_qkv(qkv, H))
    go = heads(gout, H).double()
    p = r["p"]
    delta = scale * q.norm(dim=-1) * k.norm(dim=-1).amax(-1, keepdim=True)               # [B, H, T]
    w = 2 * delta + 4
    f_out = U * (w.unsqueeze(-1) * (p @ v.abs()) + v.abs().amax(-2, keepdim=True))
    colsum = p.sum(-2)                                                                   # sum_q p[q, k]   [B, H, T]
    f_gv = U * (p.transpose(-1, -2) @ (w.unsqueeze(-1) * go.abs()) + colsum.clamp_min(1.0).unsqueeze(-1) * go.abs().amax(-2, keepdim=True))
    return {"out": (r["out"], tokens(f_out)), "gv": (r["gv"], tokens(f_gv)),
            "max": (r["m"], U * (delta + r["m"].abs())), "rsum": (r["l"], U * w), "p": p, "delta": delta}


def worst(err, form):
    """max over EVERY element of err / form; an exact element counts as 0 whatever its form, a NaN anywhere gives NaN"""
    ratio = torch.where(err == 0, torch.zeros_like(err), err / form)
    return float("nan") if bool(torch.isnan(ratio).any()) else float(ratio.max())


def ratios(ref, out=None, stats=None, gv=None):
    """worst error / form (in units of the bound form, WITHOUT K) of the results given, each against `ref` = reference(...)"""
    r = {}
    if out is not None:
        r["out"] = worst((out.double() - ref["out"][0]).abs(), ref["out"][1])
    if stats is not None:
        st = stats.double()
        r["max"] = worst((st[..., 0] - ref["max"][0]).abs(), ref["max"][1])
        r["rsum"] = worst((st[..., 1] * ref["rsum"][0] - 1).abs(), ref["rsum"][1])
    if gv is not None:
        r["gv"] = worst((gv.double() - ref["gv"][0]).abs(), ref["gv"][1])
    return r


def fp32_ratios(case):
    """the worst use of the four forms by the plain fp32 PyTorch evaluation of the reference expression"""
    qkv, gout = make_inputs(case)
    ref = reference(qkv, gout, case.H)
    r32 = evaluate(qkv, gout, case.H, torch.float32)
    return ratios(ref, out=r32["out"], stats=torch.stack([r32["m"], 1.0 / r32["l"]], dim=-1), gv=r32["gv"])
