"""Cases, fp64 reference and per-element bound of bcos_patch_norm_bwd_add (include/bcos_hip.h) on RECTANGULAR geometry: every pair of
(H, W), (kh, kw), (sh, sw), (ph, pw), (dh, dw) differs, so that a swapped pair or a mixed-up `hn % sh` / `hn / sh` cannot pass.

    out[n,h,w,c] = x[n,h,w,c] T[n,h,w] + addend[n,h,w,c],     T[n,h,w] = sum of r[n,i,j] over the output pixels whose patch holds (h, w)
    |out - exact| <= (kh kw + 2) u (|x| S + |addend|),        S = the same sum over |r|,   u = 2^-24
derived, not measured: at most kh kw - 1 additions for T in any order, one product, one sum.  A pixel that no patch holds gives exactly
the addend (0 without one).

VARIANTS name the kernel of csrc/bcos_train.hip each one reaches (the choice is bcos_patch_norm_bwd_add's, by C, the tap count and the
alignment); tests/test_wgrad_cases_cpu.py checks the bound against an fp32 evaluation and against two index mutants, and
tests/test_wgrad_gpu.py runs every case.

A plain module: the test files import it.
"""
from dataclasses import dataclass

import torch

U = 2.0 ** -24
SHAPES = ((2, 7, 5), (3, 9, 11))                 # N, H, W
# kh, kw, sh, sw, ph, pw, dh, dw
KERNELS = {"3x2": (3, 2, 2, 1, 1, 0, 1, 2), "2x3": (2, 3, 1, 2, 0, 1, 2, 1)}
KERNELS_20 = {"5x4": (5, 4, 2, 1, 1, 0, 1, 1), "4x5": (4, 5, 1, 2, 0, 1, 1, 1)}       # 20 taps > 16: no room in a 16-lane pixel group
KERNELS_GAPS = {"1x1s23": (1, 1, 2, 3, 0, 0, 1, 1)}                                  # most pixels lie in no patch
# name -> (C, x_pitch, kernels, addend offset in floats, the kernel it reaches)
VARIANTS = {
    "c64_group16": (64, 64, KERNELS, 0, "patch_norm_bwd_group_kernel<16>"),
    "c128_group32": (128, 128, KERNELS, 0, "patch_norm_bwd_group_kernel<32>"),
    "c64_taps20_wave": (64, 64, KERNELS_20, 0, "patch_norm_bwd_kernel, vector form"),
    "c36_wave": (36, 36, KERNELS, 0, "patch_norm_bwd_kernel, vector form"),
    "c6_pitch8_scalar": (6, 8, KERNELS, 0, "patch_norm_bwd_kernel, scalar form"),
    "c64_misaligned_addend": (64, 64, KERNELS, 1, "patch_norm_bwd_kernel, scalar form"),
    "c36_gaps": (36, 36, KERNELS_GAPS, 0, "patch_norm_bwd_kernel, vector form"),
}


@dataclass(frozen=True)
class Case:
    variant: str
    shape: tuple
    kname: str

    @property
    def id(self):
        return f"{self.variant}-{self.kname}-n{self.shape[0]}h{self.shape[1]}w{self.shape[2]}"

    @property
    def kernel(self):
        return VARIANTS[self.variant][2][self.kname]

    @property
    def C(self):
        return VARIANTS[self.variant][0]

    @property
    def x_pitch(self):
        return VARIANTS[self.variant][1]

    @property
    def addend_offset(self):
        return VARIANTS[self.variant][3]

    @property
    def PQ(self):
        _, H, W = self.shape
        kh, kw, sh, sw, ph, pw, dh, dw = self.kernel
        return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1

    def ints(self):
        """N, H, W, C, x_pitch, P, Q, kh, kw, sh, sw, ph, pw, dh, dw: the 15 integers of the C entry point"""
        return self.shape + (self.C, self.x_pitch) + self.PQ + self.kernel


CASES = [Case(v, s, k) for v, spec in VARIANTS.items() for k in spec[2] for s in SHAPES]
assert all(min(c.PQ) >= 1 for c in CASES)
assert all(c.kernel[0] * c.kernel[1] <= 16 for c in CASES if "group" in c.variant)
assert all(c.kernel[0] * c.kernel[1] > 16 for c in CASES if "taps20" in c.variant)


def make_inputs(case):
    """(x [N,H,W,x_pitch] with NaN pad channels, r [N,P,Q], addend [N,H,W,C]) fp32 on the CPU, the same on every call"""
    N, H, W = case.shape
    P, Q = case.PQ
    g = torch.Generator().manual_seed(77 + CASES.index(case))
    x = torch.full((N, H, W, case.x_pitch), float("nan"))
    x[..., :case.C] = torch.randn(N, H, W, case.C, generator=g)
    r = torch.randn(N, P, Q, generator=g) * torch.ldexp(torch.tensor(1.0), torch.randint(-6, 7, (N, P, Q), generator=g))
    return x, r, torch.randn(N, H, W, case.C, generator=g)


def patch_sum_scatter(r, case):
    """T [N,H,W] in the dtype of r, walking the OUTPUT pixels and their taps (the forward indexing) -- and the number of patches that
    hold each input pixel"""
    N, H, W = case.shape
    P, Q = case.PQ
    kh, kw, sh, sw, ph, pw, dh, dw = case.kernel
    T = torch.zeros(N, H, W, dtype=r.dtype, device=r.device)
    cnt = torch.zeros(H, W, dtype=torch.int64, device=r.device)
    for th in range(kh):
        for tw in range(kw):
            for i in range(P):
                ih = i * sh - ph + th * dh
                if not 0 <= ih < H:
                    continue
                for j in range(Q):
                    iw = j * sw - pw + tw * dw
                    if 0 <= iw < W:
                        T[:, ih, iw] += r[:, i, j]
                        cnt[ih, iw] += 1
    return T, cnt


def patch_sum_gather(r, case, swap_pad=False, mix_strides=False):
    """the same walking the INPUT pixels (the kernels' transposed arithmetic: hn = h + ph - th dh, patch row hn / sh where hn % sh == 0).
    swap_pad exchanges ph and pw; mix_strides tests and divides hn by sw and wn by sh: the mutants of the CPU tier"""
    N, H, W = case.shape
    P, Q = case.PQ
    kh, kw, sh, sw, ph, pw, dh, dw = case.kernel
    if swap_pad:
        ph, pw = pw, ph
    s_h, s_w = (sw, sh) if mix_strides else (sh, sw)
    T = torch.zeros(N, H, W, dtype=r.dtype, device=r.device)
    for h in range(H):
        for w in range(W):
            for tap in range(kh * kw):
                th, tw = tap // kw, tap % kw
                hn, wn = h + ph - th * dh, w + pw - tw * dw
                if hn >= 0 and wn >= 0 and hn % s_h == 0 and wn % s_w == 0 and hn // s_h < P and wn // s_w < Q:
                    T[:, h, w] += r[:, hn // s_h, wn // s_w]
    return T


def reference(x, r, addend, case):
    """(exact, bound, covered): fp64 value and per-element bound [N,H,W,C], and the [H,W] mask of pixels that some patch holds"""
    T, cnt = patch_sum_scatter(r.double(), case)
    S, _ = patch_sum_scatter(r.double().abs(), case)
    xs = x[..., :case.C].double()
    ad = addend.double() if addend is not None else torch.zeros_like(xs)
    taps = case.kernel[0] * case.kernel[1]
    return xs * T[..., None] + ad, (taps + 2) * U * (xs.abs() * S[..., None] + ad.abs()), cnt > 0


def worst(out, ref):
    """max over every element of |out - exact| / bound (<= 1 passes; exact elements count as 0, NaN anywhere gives NaN)"""
    err = (out.double() - ref[0]).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / ref[1])
    return float("nan") if bool(torch.isnan(ratio).any()) else float(ratio.max())
