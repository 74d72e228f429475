"""The SigLIP distillation loss (include/bcos_hip.h: bcos_siglip_loss) three times over, for the tests of tests/test_siglip_*.py and the
fixture generator tests/golden/make_golden_siglip.py:

  case_inputs      the seeded inputs of the recorded cases (the fixture stores results, not the inputs);
  reference64      the definition in fp64 (torch autograd over the formula of the header), with the magnitudes the bounds need;
  emulate32        the kernel's arithmetic restated in numpy fp32: the same operations in the same orders (64 lane chains and the xor
                   butterfly for every wave sum, FMA where the kernel has one);
  bounds           per-element bounds on |kernel - reference64|, derived below.

THE BOUNDS.  u = 2^-24.  Every fp32 operation (+, *, /, sqrt, FMA) is correctly rounded: relative error <= u; expf and log1pf of the device
library are accurate to 1 ulp: relative error <= 2u.  A wave sum over n terms is ceil(n / 64) chain steps and 6 butterfly levels:
k(n) = ceil(n / 64) + 6 roundings, each at most u times the sum of the terms' magnitudes.  Written for NORMALIZE; without it the
normalisation terms drop out (e_u = 0, inv = 1).
  norm             sumsq: k(D) u (non-negative terms); sqrt halves that and adds u:  (k(D) / 2 + 1) u; the bounds carry one rounding more,
                   e_inv = (k(D) / 2 + 2) u, which also covers the fp32 value of the clamp 1e-12.
  unit element     u_d = x_d / norm: e_u = e_inv + u.
  cosine           c = (sum_d us_d t_d) / norm_t, with A = sum_d |us_d| |ut_d| (<= 1, Cauchy-Schwarz):
                   eps_c = (k(D) + e_u/u + e_inv/u + 1) u A.
  power            f = c |c|^(p-1), p - 1 products: |df| <= F1 eps_c + (p - 1) u |f|, F1 = p |c|^(p-1) its derivative (p <= 1: df = eps_c).
  mean             L - 1 additions and a division:  dq <= (sum_l df_l + L u sum_l |f_l|) / L.
  logit            z = fma(scale, q, bias):  dz <= |scale| dq + u |z|.
  logsigmoid       Lipschitz constant 1 in z; e = expf(-|x|) 2u, log1pf 2u more, and d log1p(e) = e / (1 + e) <= log1p(e), the
                   subtraction u:  dls <= dz + 6 u |ls|.
  loss             per row k(M) roundings, over the rows k(N), the division by N:
                   dloss <= (sum dls + (k(M) + k(N) + 1) u sum |ls|) / N.
  sigmoid          sg = (e or 1) / (1 + e): 2u + u + u, and |d sg / dz| <= 1/4:  dsg <= dz / 4 + 4 u sg;  G = -y sg / N one rounding more:
                   dG <= (dz / 4 + 5 u sg) / N.
  gbias            sum G:  sum dG + (k(M) + k(N)) u sum |G|.
  gscale           sum fma(G, q):  sum (dG |q| + |G| dq) + (k(M) + k(N)) u sum |G q|.
  coefficient      coef = (G scale) / L:  dcoef <= (dG |scale| + 2 u |G scale|) / L;
                   dc_l = coef * (p * w) with w = |c|^(p-1) (p - 2 products), F2 = |f''| = p (p - 1) |c|^(p-2) (DETACH_POW: F1 = |c|^(p-1),
                   F2 = (p - 1) |c|^(p-2)):  ddc <= dcoef F1 + |coef| (F2 eps_c + p u F1)     (p <= 1: ddc = dcoef).
  gs[r, d]         acc = sum_j fma(dc_j, ut_jd):          E_acc = sum_j ddc_j |ut_jd| + (M + e_u/u) u sum_j |dc_j| |ut_jd|;
                   rho = sum_j dc_j c_j (wave sum):       E_rho = sum_j (ddc_j |c_j| + |dc_j| eps_c) + k(M) u sum_j |dc_j c_j|;
                   v = fma(-us_d, rho, acc), g = v / norm (inv = 1 / norm below):
                   dg <= (E_acc + |us_d| E_rho + e_u |us_d| |rho| + u |v|) inv + (e_inv + u) |g|.
                   A row below the clamp: g = acc / 1e-12f, the constant off by u from 1e-12:       dg <= E_acc inv + 3 u |g|.
  gt[j, d]         the same with the sum over the R = L N student rows as ONE chain (R roundings) and
                   kappa = sum_i (sum_l fma(dc, c)):   E_kappa = sum_li (ddc |c| + |dc| eps_c) + (L + N) u sum_li |dc c|.
All of it first order in u; the bounds are multiplied by 1.01 for the second-order terms (the largest: the curvature of the sigmoid,
|sg''| <= 0.1, times dz^2, below 1e-3 of dz / 4 while dz <= 1e-2 -- bounds() asserts that) and get 2^-126 for results that underflow.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
NORM_EPS = 1e-12


# ---------------------------------------------------------------------------------------------------------------- recorded cases
def _pooled():
    out = []
    for (n, d) in ((1, 1), (2, 8), (5, 65), (64, 1024)):
        for (sc, bi) in ((10.0, -10.0), (100.0, -10.0)):
            out.append(dict(name=f"pooled_n{n}_d{d}_s{int(sc)}", L=0, N=n, M=n, D=d, scale=sc, bias=bi, p=0, detach=False, pos_offset=0))
    return out


def _unpooled():
    out = []
    for (l, n, d) in ((1, 3, 64), (4, 5, 65), (49, 8, 63)):
        for p in (1, 2, 3):
            for detach in (False, True):
                out.append(dict(name=f"unpool_l{l}_n{n}_d{d}_p{p}_{'detach' if detach else 'grad'}", L=l, N=n, M=n, D=d, scale=10.0, bias=-10.0,
                                p=p, detach=detach, pos_offset=0))
    return out


# L = 0: image features [N, D] (the pooled head); L >= 1: [L, N, D].  "zero_row": student row 1 is all zeros.  The two-rank case is M = 2 N with
# pos_offset = rank * N: the reference's local term plus its negative_only term against the other rank's text features.
CASES = _pooled() + _unpooled() + [
    dict(name="zero_row", L=0, N=4, M=4, D=24, scale=10.0, bias=-10.0, p=0, detach=False, pos_offset=0, zero_row=1),
    dict(name="two_ranks_rank0", L=0, N=4, M=8, D=16, scale=10.0, bias=-10.0, p=0, detach=False, pos_offset=0, world=2, rank=0),
    dict(name="two_ranks_rank1", L=0, N=4, M=8, D=16, scale=10.0, bias=-10.0, p=0, detach=False, pos_offset=4, world=2, rank=1),
]
for _k, _c in enumerate(CASES):
    _c["seed"] = 7100 + _k
FULL_MAX = 4096          # gradients of more elements are recorded on KEEP_ROWS rows, with every row's norm


def case_by_name(name):
    return next(c for c in CASES if c["name"] == name)


def keep_rows(rows: int):
    return sorted({0, 1 % rows, rows // 2, rows - 1})


def case_inputs(case):
    """-> raw (un-normalised) student features, teacher features (fp32 CPU tensors), log of the scale (fp32 0-d), bias (fp32 0-d).
    The student is the teacher plus noise, so the positive pairs are the larger cosines, as in a distillation run.  The two ranks of the
    two-rank case share one seed: rank r's students are rows [r N, (r + 1) N) of the world's batch."""
    n, m, d, l = case["N"], case["M"], case["D"], case["L"]
    seed = case["seed"] - case.get("rank", 0)
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(m, d, generator=gen)
    lead = (max(l, 1), m)
    s = t.unsqueeze(0) * (0.5 + torch.rand(lead + (1,), generator=gen)) + 0.8 * torch.randn(lead + (d,), generator=gen)
    po = max(case["pos_offset"], 0)
    s = s[:, po:po + n].contiguous()
    if "zero_row" in case:
        s[:, case["zero_row"]] = 0.0
    if l == 0:
        s = s[0]
    log_scale = torch.tensor(math.log(case["scale"]), dtype=torch.float32)
    bias = torch.tensor(case["bias"], dtype=torch.float32)
    return s, t, log_scale, bias


# ---------------------------------------------------------------------------------------------------------------- fp64 definition
def _normalize64(x):
    n = x.norm(dim=-1, keepdim=True)
    return x / n.clamp_min(NORM_EPS)


def reference64(s, t, scale, bias, *, pos_offset=0, p=0, normalize=False, detach_pow=False):
    """The definition of include/bcos_hip.h in fp64 on the given (fp32-valued) inputs.  s [L, N, D] or [N, D], t [M, D]; scale, bias: Python
    floats.  -> dict(loss, gs, gt, gscale, gbias) as fp64 numpy arrays plus `aux`, the magnitudes bounds() needs."""
    s64 = torch.as_tensor(s).double().clone().requires_grad_(True)
    t64 = torch.as_tensor(t).double().clone().requires_grad_(True)
    sc = torch.tensor(float(scale), dtype=torch.float64, requires_grad=True)
    bi = torch.tensor(float(bias), dtype=torch.float64, requires_grad=True)
    s3 = s64 if s64.dim() == 3 else s64.unsqueeze(0)
    us, ut = (_normalize64(s3), _normalize64(t64)) if normalize else (s3, t64)
    c = us @ ut.T                                                    # [L, N, M]
    L, N, M = c.shape
    if p >= 2:
        w = c.abs() ** (p - 1)
        f = c * (w.detach() if detach_pow else w)
    else:
        f = c
    q = f.mean(0)
    z = sc * q + bi
    y = -torch.ones(N, M, dtype=torch.float64)
    if pos_offset >= 0:
        y[torch.arange(N), torch.arange(N) + pos_offset] = 1.0
    ls = torch.nn.functional.logsigmoid(y * z)
    loss = -ls.sum() / N
    gs, gt, gsc, gb = torch.autograd.grad(loss, (s64, t64, sc, bi))
    with torch.no_grad():
        sg = torch.sigmoid(-y * z)
        G = -y * sg / N
        ca = c.abs()
        if p >= 2:
            F1 = ca ** (p - 1) * (1 if detach_pow else p)
            F2 = ca ** (p - 2) * ((p - 1) if detach_pow else p * (p - 1))
        else:
            F1, F2 = torch.ones_like(c), torch.zeros_like(c)
        coef = G * sc / L
        dc = coef.unsqueeze(0) * F1
        aux = dict(us=us, ut=ut, c=c, f=f, q=q, z=z, ls=ls, sg=sg, G=G, F1=F1, F2=F2, coef=coef, dc=dc,
                   inv_s=1.0 / s3.norm(dim=-1).clamp_min(NORM_EPS), inv_t=1.0 / t64.norm(dim=-1).clamp_min(NORM_EPS),
                   clamp_s=s3.norm(dim=-1) < NORM_EPS, clamp_t=t64.norm(dim=-1) < NORM_EPS)
        aux = {k: v.detach().numpy() for k, v in aux.items()}
    return dict(loss=loss.detach().numpy(), gs=gs.numpy(), gt=gt.numpy(), gscale=gsc.numpy(), gbias=gb.numpy(), aux=aux)


# ---------------------------------------------------------------------------------------------------------------- per-element bounds
def _k(n):
    return math.ceil(n / 64) + 6


def bounds(ref, scale, *, p=0, normalize=False, detach_pow=False):
    """Per-element bounds on |kernel - reference64| for loss, gs, gt, gscale, gbias (the derivation is the module docstring)."""
    a = ref["aux"]
    us, ut, c = a["us"], a["ut"], a["c"]                           # [L, N, D], [M, D], [L, N, M]
    L, N, M = c.shape
    D = us.shape[-1]
    u = U
    kD, kM, kN = _k(D), _k(M), _k(N)
    e_inv = (kD / 2 + 2) * u if normalize else 0.0
    e_u = e_inv + u if normalize else 0.0
    A = np.einsum("lnd,md->lnm", np.abs(us), np.abs(ut))
    eps_c = (kD * u + e_u + e_inv + (u if normalize else 0.0)) * A
    f = a["f"]
    df = a["F1"] * eps_c + (p - 1) * u * np.abs(f) if p >= 2 else eps_c
    dq = (df.sum(0) + L * u * np.abs(f).sum(0)) / L
    dz = abs(scale) * dq + u * np.abs(a["z"])
    assert dz.max() <= 1e-2, dz.max()
    ls, sg, G, q = a["ls"], a["sg"], a["G"], a["q"]
    dls = dz + 6 * u * np.abs(ls)
    b_loss = (dls.sum() + (kM + kN + 1) * u * np.abs(ls).sum()) / N
    dG = (dz / 4 + 5 * u * sg) / N
    b_gbias = dG.sum() + (kM + kN) * u * np.abs(G).sum()
    b_gscale = (dG * np.abs(q) + np.abs(G) * dq).sum() + (kM + kN) * u * np.abs(G * q).sum()
    dcoef = (dG * abs(scale) + 2 * u * np.abs(G * scale)) / L
    coef, dc = a["coef"], a["dc"]
    if p >= 2:
        ddc = dcoef[None] * a["F1"] + np.abs(coef)[None] * (a["F2"] * eps_c + p * u * a["F1"])
    else:
        ddc = np.broadcast_to(dcoef[None], c.shape)
    adc, aus, aut = np.abs(dc), np.abs(us), np.abs(ut)
    dcc = ddc * np.abs(c) + adc * eps_c                            # error of one product dc * c
    # gs
    E_acc = np.einsum("lnm,md->lnd", ddc, aut) + (M * u + e_u) * np.einsum("lnm,md->lnd", adc, aut)
    acc = np.einsum("lnm,md->lnd", dc, ut)
    inv_s = a["inv_s"][..., None]
    g_s = ref["gs"].reshape(us.shape)
    if normalize:
        rho = (dc * c).sum(-1)[..., None]
        E_rho = dcc.sum(-1)[..., None] + kM * u * np.abs(dc * c).sum(-1)[..., None]
        v = acc - us * rho
        b_proj = (E_acc + aus * E_rho + e_u * aus * np.abs(rho) + u * np.abs(v)) * inv_s + (e_inv + u) * np.abs(g_s)
        b_clamp = E_acc * inv_s + 3 * u * np.abs(g_s)
        b_gs = np.where(a["clamp_s"][..., None], b_clamp, b_proj)
    else:
        b_gs = E_acc
    # gt
    R = L * N
    E_acc = np.einsum("lnm,lnd->md", ddc, aus) + (R * u + e_u) * np.einsum("lnm,lnd->md", adc, aus)
    acc = np.einsum("lnm,lnd->md", dc, us)
    inv_t = a["inv_t"][..., None]
    g_t = ref["gt"]
    if normalize:
        kap = (dc * c).sum((0, 1))[:, None]
        E_kap = dcc.sum((0, 1))[:, None] + (L + N) * u * np.abs(dc * c).sum((0, 1))[:, None]
        v = acc - ut * kap
        b_proj = (E_acc + aut * E_kap + e_u * aut * np.abs(kap) + u * np.abs(v)) * inv_t + (e_inv + u) * np.abs(g_t)
        b_clamp = E_acc * inv_t + 3 * u * np.abs(g_t)
        b_gt = np.where(a["clamp_t"][..., None], b_clamp, b_proj)
    else:
        b_gt = E_acc
    tiny = 2.0 ** -126
    out = dict(loss=b_loss, gs=b_gs.reshape(ref["gs"].shape), gt=b_gt, gscale=b_gscale, gbias=b_gbias)
    return {k: 1.01 * np.asarray(v) + tiny for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------- fp32 restatement
F32 = np.float32


def _fma(a, b, c):
    """fp32 FMA: the product of two fp32 numbers is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding differs
    from the fused operation only on exact ties of the second rounding)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


_LANES = np.arange(64)


def _butterfly(v):
    """v [..., 64] -> the wave sum [...]: xor 32, 16, 8, 4, 2, 1, every lane adding its partner's value"""
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., _LANES ^ o]).astype(F32)
    return v[..., 0]


def _lanes(x):
    """[..., n] -> [..., ceil(n / 64), 64]: element d sits in lane d % 64, chain step d // 64; the padding zeros leave the chains unchanged"""
    n = x.shape[-1]
    k = -(-n // 64)
    pad = np.zeros(x.shape[:-1] + (k * 64 - n,), F32)
    return np.concatenate([x.astype(F32), pad], -1).reshape(x.shape[:-1] + (k, 64))


def _wave_dot(a, b):
    al, bl = np.broadcast_arrays(_lanes(a), _lanes(b))
    acc = np.zeros(al.shape[:-2] + (64,), F32)
    for k in range(al.shape[-2]):
        acc = _fma(al[..., k, :], bl[..., k, :], acc)
    return _butterfly(acc)


def _wave_add(x):
    xl = _lanes(x)
    acc = np.zeros(xl.shape[:-2] + (64,), F32)
    for k in range(xl.shape[-2]):
        acc = (acc + xl[..., k, :]).astype(F32)
    return _butterfly(acc)


def _clamped_norm(x):
    """-> (max(||row||, eps), below the clamp) of every row"""
    n = np.sqrt(_wave_dot(x, x)).astype(F32)
    clamp = n < F32(NORM_EPS)
    return np.where(clamp, F32(NORM_EPS), n).astype(F32), clamp


def _abs_pow(c, p):
    a = np.abs(c)
    w = a
    for _ in range(2, p):
        w = (w * a).astype(F32)
    return w


def emulate32(s, t, scale, bias, *, pos_offset=0, p=0, normalize=False, detach_pow=False):
    """bcos_siglip_loss restated: fp32 numpy, the kernel's operations and orders.  -> dict(loss, gs, gt, gscale, gbias), fp32."""
    s = np.asarray(s, F32)
    t = np.asarray(t, F32)
    shape_s = s.shape
    s3 = s if s.ndim == 3 else s[None]
    L, N, D = s3.shape
    M = t.shape[0]
    scale, bias = F32(scale), F32(bias)
    if normalize:
        n_s, clamp_s = _clamped_norm(s3)
        n_t, clamp_t = _clamped_norm(t)
    else:
        n_s, clamp_s = np.ones((L, N), F32), np.zeros((L, N), bool)
        n_t, clamp_t = np.ones((M,), F32), np.zeros((M,), bool)
    us = (s3 / n_s[..., None]).astype(F32)
    c = _wave_dot(us[:, :, None, :], t[None, None, :, :])            # [L, N, M]: the dot with the RAW teacher row, divided by its norm
    if normalize:
        c = (c / n_t).astype(F32)
    # pairs
    total = np.zeros((N, M), F32)
    for l in range(L):
        term = (c[l] * _abs_pow(c[l], p)).astype(F32) if p >= 2 else c[l]
        total = (total + term).astype(F32)
    q = (total / F32(L)).astype(F32)
    z = _fma(scale, q, bias)
    y = -np.ones((N, M), F32)
    if pos_offset >= 0:
        y[np.arange(N), np.arange(N) + pos_offset] = 1.0
    x = y * z
    e = np.exp(-np.abs(x).astype(np.float64)).astype(F32)
    ls = (np.minimum(x, F32(0)) - np.log1p(e.astype(np.float64)).astype(F32)).astype(F32)
    sg = (np.where(x >= 0, e, F32(1)) / (F32(1) + e)).astype(F32)
    G = ((-y * sg) / F32(N)).astype(F32)
    coef = ((G * scale).astype(F32) / F32(L)).astype(F32)
    dc = np.empty_like(c)
    rdot = np.zeros((N, M), F32)
    for l in range(L):
        if p >= 2:
            w = _abs_pow(c[l], p)
            dc[l] = (coef * w).astype(F32) if detach_pow else (coef * (F32(p) * w).astype(F32)).astype(F32)
        else:
            dc[l] = coef
        rdot = _fma(dc[l], c[l], rdot)
    # the row partials: lane chains over j (plain additions; the G q products enter by FMA), then the rows likewise
    def row_chain(terms, fma_with=None):
        tl = _lanes(terms)
        ql = _lanes(fma_with) if fma_with is not None else None
        acc = np.zeros(tl.shape[:-2] + (64,), F32)
        for k in range(tl.shape[-2]):
            acc = _fma(tl[..., k, :], ql[..., k, :], acc) if ql is not None else (acc + tl[..., k, :]).astype(F32)
        return _butterfly(acc)
    loss = (-_wave_add(row_chain(ls)) / F32(N)).astype(F32)
    gscale = _wave_add(row_chain(G, q))
    gbias = _wave_add(row_chain(G))
    # gs
    ut = (t / n_t[:, None]).astype(F32)
    acc = np.zeros((L, N, D), F32)
    for j in range(M):
        acc = _fma(dc[:, :, j, None], ut[j][None, None, :], acc)
    if normalize:
        rho = _wave_dot(dc, c)[..., None]
        proj = (_fma(-us, rho, acc) / n_s[..., None]).astype(F32)
        gs = np.where(clamp_s[..., None], (acc / n_s[..., None]).astype(F32), proj)
    else:
        gs = acc
    # gt
    acc = np.zeros((M, D), F32)
    for l in range(L):
        for i in range(N):
            acc = _fma(dc[l, i, :, None], us[l, i][None, :], acc)
    if normalize:
        kap = np.zeros((M,), F32)
        for i in range(N):
            kap = (kap + rdot[i]).astype(F32)
        proj = (_fma(-ut, kap[:, None], acc) / n_t[:, None]).astype(F32)
        gt = np.where(clamp_t[:, None], (acc / n_t[:, None]).astype(F32), proj)
    else:
        gt = acc
    return dict(loss=loss, gs=gs.reshape(shape_s), gt=gt, gscale=gscale, gbias=gbias)
