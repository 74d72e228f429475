"""The case table of the bcos_tapconv_ops dispatcher: (route case) x (epilogue feature set), each with the tile launcher
(`route`), contraction loop and epilogue kind it is EXPECTED to take (include/bcos_hip.h: bcos_tapconv_route_query).

tests/test_tapconv_routes_cpu.py asks the library's route query for every case (no device needed) and checks that the table
is complete: every (route, loop, direction, epilogue kind) the library can report is reached by a case or listed in
UNREACHABLE with the source line that makes it so.  tests/test_tapconv_routes_gpu.py launches every case and judges every
output element against fp64.

A plain module (no fixtures, no collection hooks): the two test files import it.
"""
import ctypes as C
import math
from dataclasses import dataclass

import torch

N_KINDS = 8          # specialised epilogue kinds per direction (csrc/bcos_tapconv_plan.h: N_EPI_KINDS; bcos_tapconv_epilogue_kinds())

EPI_NORM_ONLY, EPI_FORCE_POW, EPI_SCALE_GATE_LSB, EPI_GATE2_FROM_MUL, EPI_MUL_FROM_ACT, EPI_UNIT_NORM_W = 1, 2, 4, 8, 16, 32


@dataclass(frozen=True)
class Epi:
    """An epilogue feature set.  `kind`: the epilogue kind the dispatcher is expected to pick (0 = general, k = specialised kind k
    of the direction: csrc/bcos_tapconv_plan.h EPI_KINDS_FWD / EPI_KINDS_BWD, in their order)."""
    name: str
    kind: int
    bcos_mode: int = 0            # 0 plain / gradient launch, 1 BCOS_CONV_EPS, 2 BCOS_LINEAR_EPS
    b: float = 2.0
    relu: int = 0                 # 0 / 1 ReLU / 2 constant-gate GELU
    flags: int = 0
    max_out: int = 0
    addend_sub: int = 0
    bias: bool = False
    ch_scale: bool = False
    ch_shift: bool = False
    addend: bool = False
    mul: bool = False
    mul2: bool = False
    out2: bool = False
    gate2: bool = False
    relu_gate: bool = False
    scale_out: bool = False
    norm_out: bool = False
    absmax: bool = False          # out_absmax (and out2_absmax with out2)
    col_scale: bool = False
    row_scale: bool = False
    a_sumsq: bool = False
    rowadd: bool = False
    misalign: bool = False        # the addend tensor starts 4 bytes off a 16-byte boundary (vec_ok = 0)
    generic_opt: bool = False     # BCOS_OPT_EPI_GENERIC = 1

    @property
    def norm(self):
        return self.bcos_mode != 0


# the eight forward kinds (B-cos launches, B = 2) in the order of EPI_KINDS_FWD, bias / channel affine / norm_out / out_absmax spread over them
FWD_KINDS = [
    Epi("f1_relu_scale", 1, bcos_mode=1, relu=1, scale_out=True, ch_scale=True, ch_shift=True, norm_out=True, absmax=True),
    Epi("f2_relu_scale_addend", 2, bcos_mode=1, relu=1, scale_out=True, addend=True, ch_scale=True),
    Epi("f3_scale", 3, bcos_mode=2, scale_out=True, bias=True, norm_out=True),
    Epi("f4_relu", 4, bcos_mode=1, relu=1, bias=True, ch_scale=True, ch_shift=True, absmax=True),
    Epi("f5_relu_addend", 5, bcos_mode=2, relu=1, addend=True, norm_out=True),
    Epi("f6_bare", 6, bcos_mode=1, norm_out=True),
    Epi("f7_gelu_scale", 7, bcos_mode=2, relu=2, scale_out=True, bias=True),
    Epi("f8_gelu", 8, bcos_mode=2, relu=2, ch_scale=True, ch_shift=True, norm_out=True),
]
# the eight backward kinds in the order of EPI_KINDS_BWD
BWD_KINDS = [
    Epi("b1_mul", 1, mul=True, absmax=True),
    Epi("b2_mul_addend_out2", 2, mul=True, addend=True, out2=True, absmax=True),
    Epi("b3_mul_addend_out2_mul2", 3, mul=True, addend=True, out2=True, mul2=True),
    Epi("b4_bare", 4),
    Epi("b5_addend", 5, addend=True),
    Epi("b6_mul_out2", 6, mul=True, out2=True),
    Epi("b7_mul_from_act", 7, mul=True, flags=EPI_MUL_FROM_ACT),
    # b8: the bound of this set carries two fp32 ulps for the row-scaled term (tests/test_tapconv_routes_gpu.py, module docstring).  For the
    # audit, the worst error on the fp32-MFMA loop in units of the bound WITHOUT them, what twice that measurement would allow, and the
    # worst error in units of the bound as asserted (MI355X; the GPU file prints the pair for every b8 case):
    #   cfg128_f32-b8_rowadd   4.95   (twice: 9.9)    0.43
    #   cfg64_f32-b8_rowadd    2.09   (twice: 4.2)    0.33
    #   cfg32_f32-b8_rowadd    2.30   (twice: 4.6)    0.34
    #   cfg32_fewrow-b8_rowadd 4.24   (twice: 8.5)    0.42
    # The derived allowance is the tighter of the two everywhere (error / allowance 0.33 .. 0.48 over all b8 cases; 0.5 is what "twice the
    # measurement" would give by construction), and unlike a measured factor it does not grow with the worst cancellation a case happens to
    # hold (d256x32-b8_rowadd: 34 x the bare bound over 6.3 M elements, 0.48 of the asserted one).
    Epi("b8_rowadd", 8, rowadd=True, addend=True),
]
GENERAL = Epi("g_b2p5", 0, bcos_mode=1, b=2.5, scale_out=True, norm_out=True, bias=True)
GENERAL_BWD = Epi("g_gate2", 0, mul=True, out2=True, mul2=True, gate2=True)            # the general epilogue of a plain / gradient launch
ALL_KINDS = FWD_KINDS + BWD_KINDS + [GENERAL, GENERAL_BWD]

# the reasons the dispatcher falls back to the general epilogue for (csrc/bcos_tapconv_dispatch.hip: select_epilogue_kind, the "specialised epilogue" stage of the dispatch);
# spread over the routes, one or two per route
GENERAL_REASONS = [
    Epi("g_force_pow", 0, bcos_mode=1, flags=EPI_FORCE_POW, scale_out=True),
    Epi("g_maxout2", 0, bcos_mode=1, max_out=2, scale_out=True, norm_out=True, bias=True),
    Epi("g_maxout4", 0, bcos_mode=2, max_out=4, scale_out=True),
    Epi("g_col_scale", 0, bcos_mode=1, col_scale=True, relu=1, scale_out=True),
    Epi("g_plain_relu", 0, relu=1, addend=True, mul=True),                               # (no backward kind has a ReLU)
    Epi("g_relu_gate", 0, bcos_mode=1, relu=1, relu_gate=True, scale_out=True, ch_scale=True, ch_shift=True),
    Epi("g_misaligned", 0, addend=True, mul=True, misalign=True),
    Epi("g_generic_opt", 0, bcos_mode=1, relu=1, scale_out=True, generic_opt=True),
    Epi("g_gelu_addend", 0, bcos_mode=1, relu=2, addend=True, scale_out=True),          # (no forward kind has GELU + addend)
    Epi("g_plain_scale_out", 0, scale_out=True, mul=True),                               # (a plain launch with scale_out)
]
G_UNIT_NORM_W = Epi("g_unit_norm_w", 0, bcos_mode=1, flags=EPI_UNIT_NORM_W, col_scale=True, scale_out=True, norm_out=True)
G_ROW_SCALE = Epi("g_row_scale", 0, bcos_mode=2, row_scale=True, a_sumsq=True, bias=True, scale_out=True, norm_out=True)     # general on a loop other than f16x2
F_ROW_SCALE = Epi("f3_row_scale", 3, bcos_mode=2, row_scale=True, a_sumsq=True, bias=True, scale_out=True, norm_out=True)    # rides in the operand scale on f16x2
B_ROW_SCALE = Epi("b4_row_scale", 4, row_scale=True)
G_B_ROW_SCALE = Epi("g_b_row_scale", 0, row_scale=True)                                # ... and the plain form, likewise
B_ADDEND_SUB = Epi("b5_addend_sub2", 5, addend=True, addend_sub=2)
# Cout % 4 != 0: no specialised kind, an odd output pitch (vec_ok = 0: the scalar path of the general epilogue) and a column guard at a
# width that is not a multiple of 4.  Whatever the feature set, the kind is 0.
ODD_SETS = (Epi("g_odd_fwd", 0, bcos_mode=1, relu=1, scale_out=True, norm_out=True, bias=True, ch_scale=True, ch_shift=True),
            Epi("g_odd_fwd_bare", 0, bcos_mode=2, scale_out=True, addend=True),
            Epi("g_odd_bwd", 0, mul=True, addend=True, out2=True, mul2=True),
            Epi("g_odd_bwd_bare", 0))
SKINNY_SETS = [Epi("s_bare", 0), Epi("s_addend", 0, addend=True), Epi("s_mul", 0, mul=True), Epi("s_addend_mul", 0, addend=True, mul=True)]


@dataclass(frozen=True)
class Route:
    """A route case: a geometry (forward-convolution parameters; the row grid is the convolution's output grid), a contraction
    mode and the options that steer the dispatcher to `route` / `loop`."""
    name: str
    route: str
    loop: str                     # bcos_hip.lib.LOOP_NAMES
    mode: str                     # "f32" / "bf16x3" / "f16x2" (bf16x3 with presplit = True: the bcos_split_weights image is passed)
    N: int
    H: int
    W: int
    C: int
    Cout: int
    k: int = 1
    st: int = 1
    pd: int = 0
    dil: int = 1
    opts: tuple = ()              # ((option name, value), ...)
    presplit: bool = False
    imgmax: bool = False          # pass a_imgmax / a_imgmin (the input-patch loop)
    a_pitch_x: int = 0            # extra channels of the tensor A is a slice of
    out_pitch_x: int = 0          # ... of the output tensor
    out_s: int = 1                # strided / offset output mapping
    out_0: int = 0
    cgroup: bool = False          # depth-to-space: Cout = 2 * 2 * G columns, out_sh = out_sw = 2
    groups: int = 0
    chunks: int = 1
    ch_pass: int = 0              # skinny: expected channels per pass
    aligned: bool = False         # a case that is there FOR its aligned channel count (C % 32 == 0: the uniform_tap = 1 walk; C % 16 == 0 with
                                  # 2 .. 16 taps: the channel-chunk-major K walk of the LDS-DMA loop), exempt from the table's ragged-K rule
    sets: tuple = ()              # the epilogue feature sets run on it (default: ALL_KINDS)

    @property
    def P(self):
        return (self.H + 2 * self.pd - self.dil * (self.k - 1) - 1) // self.st + 1

    @property
    def Q(self):
        return (self.W + 2 * self.pd - self.dil * (self.k - 1) - 1) // self.st + 1

    @property
    def M(self):
        return self.N * self.P * self.Q


F16 = dict(mode="f16x2")
TALL1 = (("h2_tall_min", 1),)
REGS = (("h2_loop", 1),)
SPREAD = (FWD_KINDS[0], FWD_KINDS[5], BWD_KINDS[1], BWD_KINDS[7], GENERAL, GENERAL_BWD)      # reduced list for the variants of a route already swept in full


def _r(name, route, loop, **kw):
    return Route(name=name, route=route, loop=loop, **kw)


ROUTES = [
    # -- fp32 MFMA / bf16x3 / bf16x3 pre-split: the three loops of the cfg launchers --------------------------------------------------
    #    128 x 128 needs >= 64 tiles (few-row branch below that): 8 281 rows; ragged Cout 100; C = 24 (uniform_tap = 0), K = 216
    _r("cfg128_f32", "cfg_128x128", "f32", mode="f32", N=1, H=91, W=91, C=24, Cout=100, k=3, pd=1, sets=tuple(ALL_KINDS + GENERAL_REASONS[:2] + [G_ROW_SCALE, G_B_ROW_SCALE])),
    _r("cfg128_x3", "cfg_128x128", "bf16x3", mode="bf16x3", N=2, H=65, W=63, C=72, Cout=200, sets=tuple(ALL_KINDS + GENERAL_REASONS[2:4] + [G_UNIT_NORM_W, G_ROW_SCALE])),
    _r("cfg128_x3p", "cfg_128x128", "bf16x3_presplit", mode="bf16x3", presplit=True, N=2, H=65, W=63, C=72, Cout=200, sets=tuple(ALL_KINDS + GENERAL_REASONS[4:6])),
    _r("cfg64_f32", "cfg_128x64", "f32", mode="f32", N=3, H=27, W=23, C=24, Cout=52, k=3, st=2, pd=1, sets=tuple(ALL_KINDS + GENERAL_REASONS[6:8])),
    _r("cfg64_x3", "cfg_128x64", "bf16x3", mode="bf16x3", N=3, H=11, W=13, C=72, Cout=52, sets=tuple(ALL_KINDS + GENERAL_REASONS[8:10] + [B_ADDEND_SUB])),
    _r("cfg64_x3p", "cfg_128x64", "bf16x3_presplit", mode="bf16x3", presplit=True, N=3, H=11, W=13, C=72, Cout=52, a_pitch_x=8, out_pitch_x=12),
    _r("cfg32_f32", "cfg_128x32", "f32", mode="f32", N=3, H=11, W=13, C=72, Cout=24, out_s=2, out_0=1),
    _r("cfg32_x3", "cfg_128x32", "bf16x3", mode="bf16x3", N=3, H=13, W=11, C=20, Cout=24, k=3, pd=2, dil=2, sets=tuple(ALL_KINDS + GENERAL_REASONS[0:2])),
    _r("cfg32_x3p", "cfg_128x32", "bf16x3_presplit", mode="bf16x3", presplit=True, N=3, H=11, W=13, C=72, Cout=24),
    # few-row launches of wide outputs: narrower column tiles
    _r("cfg64_fewrow", "cfg_128x64", "bf16x3", mode="bf16x3", N=3, H=10, W=11, C=72, Cout=100, sets=SPREAD),
    _r("cfg32_fewrow", "cfg_128x32", "f32", mode="f32", N=3, H=10, W=11, C=72, Cout=132, sets=SPREAD),
    # grouped launches (fp32 / bf16x3 only): C and Cout per group
    _r("cfg64_groups", "cfg_128x64", "bf16x3", mode="bf16x3", N=3, H=11, W=13, C=24, Cout=40, k=3, pd=1, groups=3,
       sets=(FWD_KINDS[0], FWD_KINDS[5], BWD_KINDS[0], BWD_KINDS[3], GENERAL)),
    _r("cfg128_groups_presplit", "cfg_128x128", "bf16x3_presplit", mode="bf16x3", presplit=True, N=3, H=11, W=13, C=24, Cout=96, groups=2,
       sets=(FWD_KINDS[2], BWD_KINDS[4])),
    # the chunked path (BCOS_OPT_SPLIT_LIMIT): 5 images of 41 184 bytes cut into chunks of 2, 2, 1
    _r("cfg64_chunks", "cfg_128x64", "bf16x3", mode="bf16x3", N=5, H=11, W=13, C=72, Cout=52, opts=(("split_limit", 100000),), chunks=3,
       sets=(FWD_KINDS[1], BWD_KINDS[2], B_ADDEND_SUB, BWD_KINDS[7], BWD_KINDS[6])),

    # -- split-f16, LDS-DMA staged (the default loop) -------------------------------------------------------------------------------
    _r("d192_132", "d_128x192", "f16x2_dma", N=3, H=37, W=37, C=72, Cout=132, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[0:2] + [F_ROW_SCALE, B_ROW_SCALE])),
    _r("d192_188", "d_128x192", "f16x2_dma", N=2, H=91, W=93, C=24, Cout=188, k=3, st=2, pd=1, **F16, sets=SPREAD + (GENERAL_REASONS[2],)),     # stride-2 input; 4 324 rows (>= 64 tiles of 128 x 128, few-row branch below that)
    _r("d192_576", "d_128x192", "f16x2_dma", N=3, H=23, W=23, C=72, Cout=576, **F16, sets=SPREAD),                 # whole 192-column tiles (Cout % 192 == 0)
    _r("d256", "d_128x256", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=200, opts=(("h2_tile", 2),), **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[2:4])),
    _r("d256_cost", "d_128x256", "f16x2_dma", N=2, H=33, W=31, C=72, Cout=456, opts=(("h2_wide_cost", 4),), **F16, sets=SPREAD),      # chosen by the cost model (a wide tile priced as one narrow one)
    _r("d128", "d_128x128", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=100, opts=(("h2_tile", 1),), **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[4:6])),
    _r("d128_cost", "d_128x128", "f16x2_dma", N=1, H=91, W=91, C=24, Cout=100, k=3, pd=1, **F16, sets=SPREAD),    # 3 x 3 WITHOUT image maxima: per-tap loop
    _r("d64", "d_128x64", "f16x2_dma", N=3, H=27, W=23, C=24, Cout=52, k=3, st=2, pd=1, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[6:8] + [B_ADDEND_SUB])),
    _r("d64_fewrow", "d_128x64", "f16x2_dma", N=3, H=10, W=11, C=72, Cout=100, **F16, sets=SPREAD),
    _r("d64_pitch", "d_128x64", "f16x2_dma", N=3, H=11, W=13, C=72, Cout=52, a_pitch_x=8, out_pitch_x=12, **F16, sets=SPREAD + (F_ROW_SCALE,)),
    _r("d32", "d_128x32", "f16x2_dma", N=3, H=11, W=13, C=72, Cout=24, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[8:10])),
    _r("d32_fewrow", "d_128x32", "f16x2_dma", N=3, H=10, W=11, C=72, Cout=132, **F16, sets=SPREAD),
    _r("d32_d2s", "d_128x32", "f16x2_dma", N=3, H=11, W=13, C=24, Cout=16, k=4, pd=2, cgroup=True, **F16,
       sets=(BWD_KINDS[0], BWD_KINDS[1], BWD_KINDS[3], BWD_KINDS[5], GENERAL_BWD)),                        # depth to space, per-tap loop (no image maxima)
    _r("d32_7x7", "d_128x32", "f16x2_dma", N=2, H=29, W=33, C=8, Cout=24, k=7, st=2, pd=3, imgmax=True, **F16, sets=SPREAD),       # >= 25 taps: image maxima as row scales
    _r("d256x64", "d_256x64", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=52, opts=TALL1, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[0:2])),
    _r("d256x64_mapped", "d_256x64", "f16x2_dma", N=3, H=21, W=23, C=24, Cout=52, k=3, pd=2, dil=2, out_s=2, out_0=1, opts=TALL1, **F16, sets=SPREAD),
    _r("d256x32", "d_256x32", "f16x2_dma", N=2, H=363, W=362, C=8, Cout=24, **F16),                                # hard-coded M >= 2 * 256 * 512: 262 812 rows
    _r("d64_chunks", "d_128x64", "f16x2_dma", N=5, H=11, W=13, C=72, Cout=52, opts=(("split_limit", 100000),), chunks=3, **F16,
       sets=(FWD_KINDS[0], BWD_KINDS[1])),

    # -- split-f16, register-staged (BCOS_OPT_H2_LOOP = 1) ---------------------------------------------------------------------------
    _r("h256", "h2_128x256", "f16x2_regs", N=3, H=21, W=23, C=72, Cout=200, opts=REGS + (("h2_tile", 2),), **F16),
    _r("h256_cost", "h2_128x256", "f16x2_regs", N=2, H=33, W=31, C=72, Cout=456, opts=REGS + (("h2_wide_cost", 4),), **F16, sets=SPREAD),
    _r("h128", "h2_128x128", "f16x2_regs", N=3, H=21, W=23, C=24, Cout=100, k=3, st=2, pd=1, opts=REGS, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[2:4])),
    _r("h64", "h2_128x64", "f16x2_regs", N=3, H=11, W=13, C=72, Cout=52, opts=REGS, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[4:6] + [F_ROW_SCALE])),
    _r("h32", "h2_128x32", "f16x2_regs", N=3, H=11, W=13, C=72, Cout=24, opts=REGS, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[6:8])),
    _r("h256x64", "h2_256x64", "f16x2_regs", N=3, H=21, W=23, C=72, Cout=52, opts=REGS + TALL1, **F16),
    _r("h256x32", "h2_256x32", "f16x2_regs", N=2, H=363, W=362, C=8, Cout=24, opts=REGS, **F16),

    # -- split-f16 over an LDS-resident input patch (3 x 3 / 4 x 4 taps, stride 1, C % 16 == 0, image maxima) ---------------------------
    _r("p256a", "p_128x256_a", "f16x2_patch", N=3, H=14, W=14, C=48, Cout=200, k=3, pd=1, imgmax=True, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[0:2])),
    _r("p128a", "p_128x128_a", "f16x2_patch", N=3, H=13, W=14, C=48, Cout=100, k=3, pd=1, imgmax=True, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[2:4])),
    _r("p128a_narrow_opt", "p_128x128_a", "f16x2_patch", N=3, H=14, W=14, C=48, Cout=200, k=3, pd=1, imgmax=True, opts=(("patch_wide", 0),), **F16, sets=SPREAD),
    _r("p128b", "p_128x128_b", "f16x2_patch", N=5, H=7, W=7, C=48, Cout=100, k=3, pd=1, imgmax=True, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[4:6])),
    _r("p128c", "p_128x128_c", "f16x2_patch", N=2, H=27, W=28, C=48, Cout=132, k=3, pd=1, imgmax=True, out_pitch_x=12, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[6:8])),
    _r("p256x64a", "p_256x64_a", "f16x2_patch", N=2, H=56, W=55, C=16, Cout=52, k=3, pd=1, imgmax=True, **F16, sets=tuple(ALL_KINDS + GENERAL_REASONS[8:10])),
    _r("p2_b32", "p2_256x64_b32", "f16x2_patch", N=2, H=19, W=70, C=16, Cout=52, k=3, pd=1, imgmax=True, **F16),
    _r("p2_t9", "p2_256x32_t9", "f16x2_patch", N=2, H=19, W=70, C=16, Cout=24, k=3, pd=1, imgmax=True, a_pitch_x=16, **F16),
    _r("p2_t16", "p2_256x32_t16", "f16x2_patch", N=3, H=20, W=22, C=16, Cout=24, k=4, pd=2, imgmax=True, **F16),
    _r("p2_t16_d2s", "p2_256x32_t16", "f16x2_patch", N=3, H=20, W=22, C=16, Cout=16, k=4, pd=2, imgmax=True, cgroup=True, **F16,
       sets=(BWD_KINDS[0], BWD_KINDS[1], BWD_KINDS[2], BWD_KINDS[3], BWD_KINDS[4], BWD_KINDS[5], GENERAL_BWD)),

    # -- Cout % 4 != 0 on every family (general epilogue, scalar stores, odd pitch) -----------------------------------------------------
    _r("cfg128_odd", "cfg_128x128", "bf16x3", mode="bf16x3", N=2, H=65, W=63, C=72, Cout=130, sets=ODD_SETS),
    _r("cfg64_odd", "cfg_128x64", "f32", mode="f32", N=3, H=11, W=13, C=72, Cout=50, sets=ODD_SETS),
    _r("cfg32_odd_presplit", "cfg_128x32", "bf16x3_presplit", mode="bf16x3", presplit=True, N=3, H=11, W=13, C=24, Cout=30, k=3, pd=1, sets=ODD_SETS),
    _r("d192_odd", "d_128x192", "f16x2_dma", N=3, H=37, W=37, C=72, Cout=130, **F16, sets=ODD_SETS),
    _r("d256_odd", "d_128x256", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=130, opts=(("h2_tile", 2),), **F16, sets=ODD_SETS),
    _r("d128_odd", "d_128x128", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=130, opts=(("h2_tile", 1),), **F16, sets=ODD_SETS),
    _r("d64_odd", "d_128x64", "f16x2_dma", N=3, H=27, W=23, C=24, Cout=50, k=3, st=2, pd=1, **F16, sets=ODD_SETS),
    _r("d32_odd", "d_128x32", "f16x2_dma", N=3, H=11, W=13, C=72, Cout=30, **F16, sets=ODD_SETS),
    _r("d256x64_odd", "d_256x64", "f16x2_dma", N=3, H=21, W=23, C=72, Cout=50, opts=TALL1, **F16, sets=ODD_SETS),
    _r("h128_odd", "h2_128x128", "f16x2_regs", N=3, H=21, W=23, C=72, Cout=130, opts=REGS, **F16, sets=ODD_SETS),
    _r("h64_odd", "h2_128x64", "f16x2_regs", N=3, H=11, W=13, C=72, Cout=50, opts=REGS, **F16, sets=ODD_SETS),
    _r("h256x64_odd", "h2_256x64", "f16x2_regs", N=3, H=21, W=23, C=24, Cout=50, k=3, pd=1, opts=REGS + TALL1, **F16, sets=ODD_SETS),
    _r("p256a_odd", "p_128x256_a", "f16x2_patch", N=3, H=14, W=14, C=48, Cout=130, k=3, pd=1, imgmax=True, **F16, sets=ODD_SETS),
    _r("p128b_odd", "p_128x128_b", "f16x2_patch", N=5, H=7, W=7, C=48, Cout=130, k=3, pd=1, imgmax=True, **F16, sets=ODD_SETS),
    _r("p256x64a_odd", "p_256x64_a", "f16x2_patch", N=2, H=56, W=55, C=16, Cout=50, k=3, pd=1, imgmax=True, **F16, sets=ODD_SETS),
    _r("p2_t9_odd", "p2_256x32_t9", "f16x2_patch", N=2, H=19, W=70, C=16, Cout=30, k=3, pd=1, imgmax=True, **F16, sets=ODD_SETS),
    _r("p2_t16_odd", "p2_256x32_t16", "f16x2_patch", N=3, H=20, W=22, C=16, Cout=30, k=4, pd=2, imgmax=True, **F16, sets=ODD_SETS),

    # -- aligned channel counts: the uniform_tap = 1 walk (C % 32 == 0) and the channel-chunk-major K walk of the LDS-DMA loop (2 .. 16 taps,
    #    C % 16 == 0, NO image maxima: the per-tap loop), which the ragged cases above never take ----------------------------------------
    _r("cfg128_c64", "cfg_128x128", "bf16x3", mode="bf16x3", N=2, H=65, W=63, C=64, Cout=200, aligned=True, sets=SPREAD),
    _r("cfg64_c64_f32", "cfg_128x64", "f32", mode="f32", N=3, H=11, W=13, C=64, Cout=52, aligned=True, sets=SPREAD),
    _r("cfg64_3x3_c32", "cfg_128x64", "bf16x3_presplit", mode="bf16x3", presplit=True, N=3, H=27, W=23, C=32, Cout=52, k=3, st=2, pd=1, aligned=True, sets=SPREAD),
    _r("d192_c64", "d_128x192", "f16x2_dma", N=3, H=37, W=37, C=64, Cout=132, aligned=True, **F16, sets=SPREAD),
    _r("d128_3x3_c48", "d_128x128", "f16x2_dma", N=3, H=21, W=23, C=48, Cout=100, k=3, pd=1, opts=(("h2_tile", 1),), aligned=True, **F16, sets=SPREAD),
    _r("d256_3x3_c32", "d_128x256", "f16x2_dma", N=3, H=43, W=45, C=32, Cout=200, k=3, st=2, pd=1, opts=(("h2_tile", 2),), aligned=True, **F16, sets=SPREAD),
    _r("d64_c64", "d_128x64", "f16x2_dma", N=3, H=11, W=13, C=64, Cout=52, aligned=True, **F16, sets=SPREAD),
    _r("d64_3x3_c48", "d_128x64", "f16x2_dma", N=3, H=27, W=23, C=48, Cout=52, k=3, st=2, pd=1, aligned=True, **F16, sets=SPREAD),
    _r("d256x64_2x2_c32", "d_256x64", "f16x2_dma", N=3, H=21, W=23, C=32, Cout=52, k=2, pd=0, opts=TALL1, aligned=True, **F16, sets=SPREAD),
    _r("d32_3x3_c16", "d_128x32", "f16x2_dma", N=3, H=11, W=13, C=16, Cout=24, k=3, pd=1, aligned=True, **F16, sets=SPREAD),
    _r("h128_c64", "h2_128x128", "f16x2_regs", N=3, H=21, W=23, C=64, Cout=100, opts=REGS, aligned=True, **F16, sets=SPREAD),
    _r("h64_3x3_c48", "h2_128x64", "f16x2_regs", N=3, H=27, W=23, C=48, Cout=52, k=3, st=2, pd=1, opts=REGS, aligned=True, **F16, sets=SPREAD),
    _r("h256_3x3_c32", "h2_128x256", "f16x2_regs", N=3, H=21, W=23, C=32, Cout=200, k=3, pd=1, opts=REGS + (("h2_tile", 2),), aligned=True, **F16, sets=SPREAD),

    # -- launches that ASK for f16x2 and are sent elsewhere: the unit-norm projection runs on the bf16x3 loop of the cfg launchers (side tensors
    #    of the split-f16 loop passed and ignored); a row_scale keeps a 3 x 3 launch with image maxima off the patch kernels ------------------
    _r("cfg128_from_f16x2", "cfg_128x128", "bf16x3", N=3, H=37, W=37, C=72, Cout=132, **F16, sets=(G_UNIT_NORM_W,)),
    _r("d64_from_patch", "d_128x64", "f16x2_dma", N=3, H=13, W=14, C=48, Cout=100, k=3, pd=1, imgmax=True, aligned=True, **F16, sets=(F_ROW_SCALE, B_ROW_SCALE)),

    # -- the narrow-output kernel (Cout <= 8, plain / addend / mul): one pass over all channels, and a C whose channels are sliced --------
    _r("skinny4", "skinny", "f32", mode="f16x2", N=3, H=11, W=13, C=12, Cout=4, k=3, pd=1, ch_pass=12, sets=tuple(SKINNY_SETS)),
    _r("skinny8", "skinny", "f32", mode="bf16x3", N=3, H=11, W=13, C=16, Cout=8, k=3, pd=1, ch_pass=16, out_pitch_x=4, sets=tuple(SKINNY_SETS)),
    _r("skinny4_sliced", "skinny", "f32", mode="f32", N=2, H=11, W=13, C=256, Cout=4, k=3, pd=1, ch_pass=16, sets=tuple(SKINNY_SETS)),
    _r("skinny6", "skinny", "f32", mode="bf16x3", N=3, H=11, W=13, C=12, Cout=6, k=3, pd=1, ch_pass=12, sets=tuple(SKINNY_SETS)),
    _r("skinny8_sliced", "skinny", "f32", mode="f16x2", N=2, H=11, W=13, C=24, Cout=8, k=3, pd=1, ch_pass=12, out_s=2, out_0=0, sets=tuple(SKINNY_SETS)),
]

# (route, direction, kind) triples the dispatcher itself makes unreachable, each with the source line that makes it so.  direction: 1 = B-cos
# (forward kinds), 0 = plain.  The completeness test fails for a triple that is neither reached by a case nor listed here -- and for one that
# is listed here and reached.
UNREACHABLE = (
    [("skinny", 1, k, "csrc/bcos_skinny.hip skinny_decide: `if (e.bcos_mode != BCOS_NONE || ...) return false` -- a B-cos launch never takes the narrow kernel")
     for k in range(0, N_KINDS + 1)] +
    [("skinny", 0, k, "csrc/bcos_tapconv_dispatch.hip bcos_tapconv_route_query: the narrow kernel has its own plain epilogue; the query reports epi_kind 0 for it")
     for k in range(1, N_KINDS + 1)])

# features the dispatcher keeps off a launcher family (asked per feature, not per kind): (route prefix, epilogue set, where the launch goes instead, source)
FEATURE_DETOURS = [
    ("p128a", F_ROW_SCALE, "d_128x64", "csrc/bcos_tapconv_dispatch.hip choose_route: `if (dma && geom_ok && p.a_imgmax && !e.row_scale && !e.a_sumsq)`"),
    ("p128a", B_ROW_SCALE, "d_128x64", "the same condition: the patch kernels compile row_scale out"),
    ("d192_132", G_UNIT_NORM_W, "cfg_128x128", "csrc/bcos_tapconv_dispatch.hip select_operands: `if (mode == 2 && G == 1 && h2_pays && !unit_w ...` -- BCOS_EPI_UNIT_NORM_W runs on the fp32 / bf16x3 loops"),
]


# Per-element bounds against fp64.  LIN: what include/bcos_hip.h states for the contraction loops (comment on bcos_operands.a_imgmax),
# |lin - lin64| <= 2e-6 ||a_row|| ||w_col||; Y / S / N: what follows from it for the B-cos output y = lin |lin| / norm (two factors of lin),
# its scale s = |lin| / norm and the patch norm, as tests/test_gpu_parity.py::test_patch_loop_dynamic_range_inside_an_image asserts them.
LIN_BOUND, Y_BOUND, S_BOUND, N_BOUND = 2e-6, 4e-6, 3e-6, 5e-6


def bcos_forward_errors(y, s, n, y64, s64, n64, norm_y, norm_s, tiny=1e-30):
    """Worst per-element errors of a B-cos forward launch against fp64, each in the unit of its bound: (y - y64) / norm_y (norm_y = the
    upper bound of |lin|^2 / norm: ||patch|| ||w_c||^2 without a bias), (s - s64) / norm_s (||w_c||), (n - n64) / n64.  Every element counts."""
    e_y = ((y.double() - y64).abs() / (norm_y + tiny)).max().item()
    e_s = ((s.double() - s64).abs() / (norm_s + tiny)).max().item()
    e_n = ((n.double() - n64).abs() / n64).max().item()
    return e_y, e_s, e_n


def loops_of(route_name):
    """The contraction loops a launcher can run (csrc/bcos_tapconv_plan.h family_loop: launch_cfg picks among three, the others instantiate one)."""
    if route_name == "skinny":
        return ["f32"]
    fam = route_name.split("_")[0]
    return {"cfg": ["f32", "bf16x3", "bf16x3_presplit"], "h2": ["f16x2_regs"], "d": ["f16x2_dma"], "p": ["f16x2_patch"], "p2": ["f16x2_patch"]}[fam]


def rejected(r, e):
    """Pairs bcos_tapconv_ops' argument validation (csrc/bcos_tapconv_dispatch.hip: validate) rejects (include/bcos_hip.h): nothing is asked of them."""
    if r.cgroup and (e.norm or e.max_out or e.absmax or e.norm_out or e.bias or e.ch_scale or e.ch_shift or (e.flags & EPI_MUL_FROM_ACT)
                     or e.rowadd or e.addend_sub > 1 or e.row_scale or e.misalign):
        return True                                          # out_cgroup launches are plain gradient launches
    if r.groups > 1 and (e.max_out or e.absmax or e.row_scale or e.a_sumsq or e.addend_sub > 1):
        return True
    if e.max_out and r.Cout % 4 != 0:
        return True
    return False


@dataclass(frozen=True)
class Case:
    r: Route
    e: Epi

    @property
    def id(self):
        return f"{self.r.name}-{self.e.name}"

    @property
    def kind(self):
        """expected epilogue kind: the set's, 0 on the narrow kernel"""
        return 0 if self.r.route == "skinny" else self.e.kind

    @property
    def absmax(self):
        return self.e.absmax and not (self.r.cgroup or self.r.groups > 1 or self.r.route == "skinny")


def all_cases():
    out = []
    for r in ROUTES:
        for e in (r.sets or tuple(ALL_KINDS)):
            if not rejected(r, e):
                out.append(Case(r, e))
    return out


CASES = all_cases()


# ---------------------------------------------------------------------------------------------------------------------------------
# building the three structs of a case

def _image_scales(N):
    """per-image magnitudes a few decades apart"""
    return torch.tensor([10.0 ** (3 * ((n * 2) % 3) - 3) for n in range(N)]).view(N, 1, 1, 1)


class Built:
    """Tensors and the three structs of one case on `device`.  On the CPU the side tensors the library's own kernels produce
    (a_absmax, a_imgmax, weight images) are buffers of the right size with no meaning: the route query does not read them."""

    def __init__(self, case, device, blib):
        r, e = case.r, case.e
        self.case = case
        dev = torch.device(device)
        real = dev.type != "cpu"
        g = torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(case.id)))
        G = max(r.groups, 1)
        N, H, W, Cg, P, Q = r.N, r.H, r.W, r.C, r.P, r.Q
        Ctot = G * Cg
        taps = r.k * r.k
        self.G, self.taps = G, taps
        # A: a channel slice of a wider tensor; the channels beyond it hold large finite values (a leak shows, K padding does not poison)
        a_pitch = Ctot + r.a_pitch_x
        a_full = torch.randn(N, H, W, a_pitch, generator=g) * 1e3
        a_full[..., :Ctot] = torch.randn(N, H, W, Ctot, generator=g) * _image_scales(N)
        self.a_full = a_full.to(dev)
        # weights [G Cout][taps][C], rows one decade apart
        cols = G * r.Cout
        w = torch.randn(cols, taps, Cg, generator=g) / math.sqrt(taps * Cg) * (10.0 ** (torch.rand(cols, 1, 1, generator=g) - 0.5))
        if r.cgroup:      # a class's unused taps carry zero weights, as DgradPlan builds them: class (dh, dw) uses taps of its own parity
            Gc = r.Cout // 4
            for cls in range(4):
                for t in range(taps):
                    if ((t // r.k) % 2, (t % r.k) % 2) != (cls // 2, cls % 2):
                        w[cls * Gc:(cls + 1) * Gc, t] = 0
        self.w = w.to(dev)
        # output tensor [N, OH, OW, out_pitch] and the mapping of the row grid into it
        div = e.max_out if e.max_out > 1 else 1
        if r.cgroup:
            self.out_c = r.Cout // 4
            out_sh = 2
            OH, OW = P * 2 + 1, Q * 2
            h0 = 0
        else:
            self.out_c = cols // div
            out_sh, h0 = r.out_s, r.out_0
            OH, OW = (P - 1) * out_sh + h0 + 1 + (1 if out_sh > 1 else 0), (Q - 1) * out_sh + h0 + 1
        self.OH, self.OW, self.out_sh, self.h0 = OH, OW, out_sh, h0
        out_pitch = self.out_c + r.out_pitch_x
        self.out_pitch = out_pitch
        assert div == 1 or r.out_pitch_x == 0
        self.pitch_s = cols if div > 1 else out_pitch          # scale_out of a MaxOut launch keeps the contraction's width, densely (pitch Cout)
        npx = N * OH * OW
        self.npx = npx
        self.keep = []
        self.guards = {}

        def canary(name, shape, extra=64):
            n = int(torch.Size(shape).numel())
            buf = torch.full((n + 2 * extra,), float("nan"), device=dev)
            self.guards[name] = (buf, extra)
            return buf[extra:extra + n].view(shape)

        def rnd(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g) * scale).to(dev)

        def like_out(scale=1.0, misalign=False):
            t = torch.randn(npx * out_pitch + 4, generator=g) * scale
            t = t.to(dev)
            off = 1 if misalign else 0
            self.keep.append(t)
            return t[off:off + npx * out_pitch].view(N, OH, OW, out_pitch)

        geom = blib.TapconvGeom()
        for k_, v in dict(N=N, H=H, W=W, C=Cg, P=P, Q=Q, in_sh=r.st, in_sw=r.st, dh0=-r.pd, dw0=-r.pd, dstep_h=r.dil, dstep_w=r.dil,
                          TH=r.k, TW=r.k, OH=OH, OW=OW, out_sh=out_sh, out_sw=out_sh, out_h0=h0, out_w0=h0, Cout=r.Cout,
                          a_pitch=a_pitch if (r.a_pitch_x or G > 1) else 0, out_pitch=out_pitch if (r.out_pitch_x or G > 1) else 0,
                          norm_pitch=0, out_cgroup=(r.Cout // 4 if r.cgroup else 0), groups=r.groups).items():
            setattr(geom, k_, int(v))
        self.geom = geom

        ep = blib.Epilogue()
        self.t = {}
        T = self.t
        if e.bias: T["bias"] = rnd(cols, scale=0.5)
        if e.ch_scale: T["ch_scale"] = (torch.randn(cols, generator=g) * 0.5 + 1.5).to(dev) * (1 - 2 * (torch.arange(cols, device=dev) % 3 == 0).float())
        if e.ch_shift: T["ch_shift"] = rnd(cols, scale=0.3)
        if e.col_scale: T["col_scale"] = (torch.rand(cols, generator=g) + 0.5).to(dev)
        if e.addend:
            if e.addend_sub > 1:
                s_ = e.addend_sub
                T["addend"] = rnd(N, (OH + s_ - 1) // s_, (OW + s_ - 1) // s_, out_pitch, scale=0.7)
            else:
                T["addend"] = like_out(0.7, misalign=e.misalign)
        if e.mul: T["mul"] = like_out(1.0).abs() if (e.flags & EPI_MUL_FROM_ACT) else like_out(1.0)
        if e.flags & EPI_MUL_FROM_ACT:
            T["mul"] = T["mul"] * (T["mul"] > 0.3)                     # a kept activation: relu output, zeros included
            T["mul_norm"] = (torch.rand(npx, generator=g) + 0.5).to(dev)
            T["mul_csc"] = (torch.randn(r.Cout, generator=g) * 0.5 + 1.5).to(dev)
            T["mul_csh"] = rnd(r.Cout, scale=0.1)
        if e.mul2: T["mul2"] = like_out(1.0)
        if e.gate2: T["gate2"] = like_out(1.0)
        if e.relu_gate: T["relu_gate"] = like_out(1.0)
        if e.row_scale: T["row_scale"] = (10.0 ** (torch.rand(npx, generator=g) * 2 - 1)).to(dev)
        if e.a_sumsq: T["a_sumsq"] = (torch.rand(npx, generator=g) * 4 + 0.5).to(dev) * float(Cg)
        if e.rowadd:
            T["rowadd"] = like_out(1.0)
            T["rowadd_scale"] = rnd(npx, scale=0.5)
        T["out"] = canary("out", (N, OH, OW, out_pitch))
        if e.out2: T["out2"] = canary("out2", (N, OH, OW, out_pitch))
        if e.scale_out: T["scale_out"] = canary("scale_out", (N, OH, OW, self.pitch_s))
        if e.norm_out: T["norm_out"] = canary("norm_out", (N, OH, OW, G))
        if case.absmax:
            T["out_absmax"] = torch.zeros(npx, dtype=torch.int32, device=dev)
            if e.out2: T["out2_absmax"] = torch.zeros(npx, dtype=torch.int32, device=dev)
        for k_, t in T.items():
            setattr(ep, k_, t.data_ptr())
        ep.bcos_mode, ep.relu, ep.b, ep.flags, ep.max_out, ep.addend_sub = e.bcos_mode, e.relu, e.b, e.flags, e.max_out, e.addend_sub
        self.epi = ep

        ops = blib.Operands()
        ops.a, ops.wt = self.a_full.data_ptr(), self.w.data_ptr()
        ops.contraction = {"f32": blib.CONTRACT_F32, "bf16x3": blib.CONTRACT_BF16X3, "f16x2": blib.CONTRACT_F16X2}[r.mode]
        lib = blib.load()
        ktot = taps * Cg
        nbytes = C.c_int64(0)
        if r.mode == "f16x2" and G == 1:
            am = torch.zeros(N * H * W, dtype=torch.int32, device=dev)
            blib.check(lib.bcos_split_weights_f16x2_bytes(cols, ktot, C.byref(nbytes)), "bcos_split_weights_f16x2_bytes")
            image = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
            rng = torch.zeros(2, N, dtype=torch.int32, device=dev)
            if real:
                blib.check(lib.bcos_rows_absmax(self.a_full.data_ptr(), am.data_ptr(), N * H * W, Ctot, a_pitch, None), "bcos_rows_absmax")
                blib.check(lib.bcos_split_weights_f16x2_conv(self.w.data_ptr(), image.data_ptr(), cols, taps, Cg, None), "bcos_split_weights_f16x2_conv")
                blib.check(lib.bcos_image_absrange(am.data_ptr(), rng[0].data_ptr(), rng[1].data_ptr(), N, H * W, None), "bcos_image_absrange")
            ops.a_absmax, ops.wt_f16x2 = am.data_ptr(), image.data_ptr()
            if r.imgmax:
                ops.a_imgmax, ops.a_imgmin = rng[0].data_ptr(), rng[1].data_ptr()
            self.keep += [am, image, rng]
        if r.presplit:
            blib.check(lib.bcos_split_weights_bytes(cols, ktot, C.byref(nbytes)), "bcos_split_weights_bytes")
            image3 = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
            if real:
                blib.check(lib.bcos_split_weights(self.w.data_ptr(), image3.data_ptr(), cols, ktot, None), "bcos_split_weights")
            ops.wt_bf16x3 = image3.data_ptr()
            self.keep.append(image3)
        self.ops = ops

    def options(self):
        o = dict(self.case.r.opts)
        if self.case.e.generic_opt:
            o["epi_generic"] = 1
        return o


def with_options(blib, opts):
    """context manager stack: every option of `opts` set for the block"""
    from contextlib import ExitStack
    st = ExitStack()
    for k_, v in opts.items():
        st.enter_context(blib.option(k_, v))
    return st
