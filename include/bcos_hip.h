/*
 * bcos_hip.h -- C ABI of the MI355X (gfx950) B-cos forward / explanation hot path.
 *
 * The reference (shrebox/B-cosification) has no FFI for this path: the boundary is the
 * Python nn.Module API of bcos/modules.  Every entry point below
 * therefore names the reference *function* whose ATen launch sequence it replaces
 * (paths relative to the reference root), and the Python host layer in
 * b-cosification_amd/bcos/ binds them with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer to fp32 data unless the name says otherwise;
 *     the caller owns every buffer; the library never allocates or frees device memory.
 *   - all work is enqueued on the hipStream_t passed as `void* stream` (NULL = default
 *     stream); calls are asynchronous and re-entrant; the only global mutable state is the
 *     thread-local last-error string, the process-wide DEFAULT contraction mode (which a call
 *     overrides through bcos_operands.contraction) and the option table of bcos_set_option.
 *     The library never reads the process environment.
 *   - return value: 0 = ok, negative = error (BCOS_E_*); never throws.
 *   - activations are NHWC ("channels-last": pixel-major, channels contiguous).  The
 *     logical NCHW shape of the reference is kept by the Python layer through
 *     torch.channels_last strides, so no copies are involved.
 *   - weights are [Cout][taps][Cin] (K-contiguous, "KRSC"); Cin must be a multiple of 4.
 */
#ifndef BCOS_HIP_H
#define BCOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCOS_ABI_VERSION 12

enum {
    BCOS_OK = 0,
    BCOS_E_INVAL = -22,   /* bad shape / alignment / NULL where required */
    BCOS_E_NOSUP = -95,   /* combination not supported by the kernels   */
    BCOS_E_LAUNCH = -5    /* hip launch error (see bcos_last_error_string) */
};

/* B-cos scaling flavour applied to the contraction result `lin` of one output row.
 *   BCOS_NONE        y = lin                                (b == 1: bcosconv2d.py:172-174)
 *   BCOS_CONV_EPS    norm = sqrt(sum_patch x^2 + 1e-6)       (bcosconv2d.py:212-221)
 *   BCOS_LINEAR_EPS  norm = sqrt(sum x^2) + 1e-12            (bcoslinear.py:113)
 * with  b == 2 : s = |lin| / norm                            (bcosconv2d.py:186-187)
 *       b != 2 : s = (|lin / norm| + 1e-6)^(b-1)             (bcosconv2d.py:188-190)
 * and   y = s * lin.                                                                  */
enum { BCOS_NONE = 0, BCOS_CONV_EPS = 1, BCOS_LINEAR_EPS = 2 };

/*
 * Generic "tap convolution" descriptor: one implicit GEMM
 *     acc[m, co] = sum_{t < TH*TW} sum_{c < C} A[n, i*in_sh + dh(t), j*in_sw + dw(t), c] * Wt[co, t, c]
 * over rows m = (n, i, j), n < N, i < P, j < Q, with dh(t) = dh0 + (t / TW) * dstep_h,
 * dw(t) = dw0 + (t % TW) * dstep_w, taps outside [0,H)x[0,W) contributing zero
 * (zero padding).  Row m is written to pixel (n, i*out_sh + out_h0, j*out_sw + out_w0)
 * of an NHWC tensor [N, OH, OW, Cout].
 *
 * A forward convolution (stride s, padding p, dilation d) is
 *     in_s = s, dh0 = -p, dstep = d, TH x TW = kernel, P x Q = OH x OW, out_s = 1, out_0 = 0.
 * The input-gradient ("dgrad") of a strided convolution is one launch per output parity
 * class with the matching sub-kernel, in_s = 1 and out_s = stride (bcos_hip/ops.py: DgradPlan),
 * or -- narrow outputs -- ONE launch whose columns are (parity class, channel), see out_cgroup.
 */
typedef struct bcos_tapconv_geom {
    int32_t N, H, W, C;          /* A operand: NHWC, C % 4 == 0                      */
    int32_t P, Q;                /* row grid per image                              */
    int32_t in_sh, in_sw;        /* input coordinate step per row-grid step         */
    int32_t dh0, dw0;            /* first tap offset                                */
    int32_t dstep_h, dstep_w;    /* tap-to-tap offset (dilation)                    */
    int32_t TH, TW;              /* tap grid                                        */
    int32_t OH, OW;              /* output tensor spatial size                      */
    int32_t out_sh, out_sw;      /* output pixel step per row-grid step             */
    int32_t out_h0, out_w0;      /* output pixel offset                             */
    int32_t Cout;                /* GEMM N; output channel count                    */
    int32_t a_pitch;             /* floats between consecutive pixels of A (0 = C): lets a launch
                                    read a channel slice (grouped convolution)      */
    int32_t out_pitch;           /* floats between consecutive output pixels (0 = Cout); every
                                    per-element epilogue tensor uses the same pitch  */
    int32_t norm_pitch;          /* floats between consecutive pixels of norm_out (0 = 1) */
    int32_t out_cgroup;          /* 0: off.  G > 0 ("depth to space"): Cout = out_sh * out_sw * G and column
                                    (dh * out_sw + dw) * G + c of row (n, i, j) is channel c of output pixel
                                    (n, i*out_sh + dh, j*out_sw + dw): ALL parity classes of a strided input
                                    gradient in one launch over the union of their taps (weights of taps a class
                                    does not use are zero; bcos_hip/ops.py: DgradPlan).  Needs G % 4 == 0,
                                    out_h0 == out_w0 == 0, 16-byte addressable tensors, no max_out, no *_absmax */
    int32_t groups;              /* 0 / 1: off.  G > 1 (grouped convolution, bcosconv2d.py:84-140 `groups`): one launch for all
                                    groups.  C and Cout are PER GROUP: group g reads channels [g C, (g+1) C) of every pixel of A
                                    (a_pitch 0 = G C), contracts them with weight rows [g Cout, (g+1) Cout) of wt [G Cout][taps][C]
                                    and writes output columns g Cout + co (out_pitch 0 = G Cout; bias / ch_scale / ch_shift are
                                    indexed by that global column); norm_out holds one patch norm per pixel AND group
                                    ([pixels][norm_pitch], norm_pitch 0 = G).  Runs on the fp32 / bf16x3 loops (no f16x2, no
                                    *_absmax, no out_cgroup, no fused MaxOut); the pre-split bf16x3 image is used when
                                    Cout % 32 == 0. */
} bcos_tapconv_geom;

/*
 * Fused epilogue, applied per output element (row m -> output pixel index `pix`,
 * channel c, idx = pix*out_pitch + c).  NULL pointers / zero flags switch a stage off.
 * Stages run in this order:
 *     v = acc
 *     v *= col_scale[c]                              unit-norm projection of NormedConv2d / NormedLinear folded into the contraction:
 *                                                    conv(x, w / ||w||) = conv(x, w) / ||w_c|| per output channel (bcosconv2d.py:26-35,
 *                                                    bcoslinear.py:25-27); col_scale from bcos_weight_row_invnorm (ABI v5)
 *     v += bias[c]                                   nn.Conv2d bias (bcosifyconv2d.py:18-31)
 *     s = bcos_scale(v, norm[m]); v *= s             B-cos transform (bcos_mode, b)
 *     v *= ch_scale[c]; s *= ch_scale[c]             BatchNormUncentered2d eval: weight/sqrt(var+eps)
 *                                                    (batchnorm_uncentered.py:46-60)
 *     v += ch_shift[c]                               ... its bias
 *     v += addend[idx]                               residual add (fwd) / gradient accumulation (dgrad)
 *     relu == 2: gate = 0.5 (1 + erf(v / sqrt 2)); s *= gate; v *= gate   (MyGELU, bcosify_vit.py:27-32)
 *     relu == 1: s = v > 0 ? s : 0; v = max(v, 0)    (relu_gate != NULL: the decision is relu_gate[idx] > 0 instead of
 *                                                    v > 0 -- replay of recorded gates, see tests/ gate-pinned parity)
 *     out [idx] = mul  ? v * mul [idx] : v           dgrad: multiply by the stored scale of the layer below
 *     out2[idx] = v [* mul2[idx]] [* (gate2[idx] > 0)]   second product of the same v (shortcut gradient)
 *     scale_out[idx] = s                             d out / d lin with the dynamic scale detached
 *                                                    (explanation mode: bcosconv2d.py:181-184)
 *     norm_out[pix] = norm[m]                        (only written by blocks of the first Cout tile)
 *     out_absmax[pix]  = max(out_absmax[pix],  bits(max_c |out [idx]|))   atomically; the caller zeroes the buffer.
 *     out2_absmax[pix] = ... of out2                  "bits" = the fp32 bit pattern (monotonic for non-negative values).
 *                                                    These per-pixel maxima are the `a_absmax` of the launch that reads
 *                                                    the tensor as its A operand (f16x2 contraction, see bcos_operands).
 */
typedef struct bcos_epilogue {
    const float* bias;
    const float* ch_scale;
    const float* ch_shift;
    const float* addend;
    const float* mul;
    const float* mul2;
    const float* gate2;
    const float* relu_gate;
    float* out;
    float* out2;
    float* scale_out;
    float* norm_out;
    uint32_t* out_absmax;   /* NULL or [N*OH*OW] */
    uint32_t* out2_absmax;  /* NULL or [N*OH*OW] */
    const float* mul_norm;  /* BCOS_EPI_MUL_FROM_ACT: patch norms [N*OH*OW] of the layer whose activation `mul` holds */
    const float* mul_csc;   /* ... its ch_scale [Cout] (NULL = 1) */
    const float* mul_csh;   /* ... its ch_shift [Cout] (NULL = 0) */
    const float* col_scale; /* NULL or [Cout] (grouped launches: [G Cout]): factor of every accumulator column, applied first (ABI v5) */
    const float* row_scale; /* NULL or [N*OH*OW]: factor of every accumulator ROW, applied with col_scale ahead of the bias (ABI v7)         */
    const float* a_sumsq;   /* NULL or [N*OH*OW] (B-cos launches): sum of squares of the row's EFFECTIVE operand, taken in place of the sum
                               the loop collects from A.  The two fields fold a LayerNorm into the contraction that reads it
                               (centered_norms.py:197-224 in front of a linear layer): with z = gamma (x - mean(x)) r + beta,
                                   W z = r (W' x) + W beta,   W'[j,k] = gamma[k] W[j,k] - mean_k'(gamma[k'] W[j,k'])
                               -- A = x, wt = W' (built once per weight), row_scale = r = 1 / sqrt(var + eps), bias = W beta,
                               a_sumsq = |z|^2 (both per row from bcos_layernorm_stats) -- and the gradient of the detached-variance
                               form, gx = r (gamma gz - mean(gamma gz)), is the input-gradient launch over W'^T with the same row_scale. */
    uint32_t* out_imgmax;   /* NULL or [N] (ABI v9), ZERO-FILLED by the caller before the first launch that writes the tensor: the launch folds
                               every row maximum it emits through out_absmax into max over the pixels of image n -- what
                               bcos_image_absrange computes from out_absmax in a pass of its own -- so that a 3 x 3 launch reading `out`
                               (bcos_operands.a_imgmax) needs no such pass.  Several launches filling disjoint pixels of one tensor
                               accumulate.  Only for launches bcos_tapconv_fuses_image_range() answers 1 for; with out_imgmin_c.      */
    uint32_t* out_imgmin_c; /* ... and a LOWER BOUND of the min over the NONZERO pixels of image n, stored complemented (~v; 0 = no nonzero
                               pixel): exact when a tile owns its pixels (one column tile), the minimum over the column tiles' own maxima
                               otherwise.  Handed on as bcos_operands.a_imgmin_c.                                                     */
    const float* rowadd;    /* NULL or a tensor indexed like `out` (ABI v9), with rowadd_scale [output pixels]: a plain gradient launch
                               (bcos_mode BCOS_NONE, no mul / out2, addend_sub <= 1) writes out = acc + (rowadd_scale[pixel] * rowadd + addend)
                               -- the patch-norm term of a 1 x 1 / stride-1 B-cos layer's input gradient, x * (sum over the patches that
                               contain the pixel of r) = x[pixel] * r[pixel], which bcos_patch_norm_bwd_add otherwise writes as a tensor of
                               its own for this launch to read back as `addend`.  Specialised epilogues only: BCOS_E_NOSUP otherwise
                               (the caller falls back to bcos_patch_norm_bwd_add).                                                    */
    const float* rowadd_scale;
    int32_t bcos_mode;      /* BCOS_NONE / BCOS_CONV_EPS / BCOS_LINEAR_EPS */
    int32_t relu;           /* 0 none, 1 ReLU, 2 GELU with constant gate  */
    float b;                /* the B-cos exponent B (2 = fast path)       */
    int32_t flags;          /* BCOS_EPI_* bits                            */
    int32_t max_out;        /* 0 / 1: off.  2 or 4 (Cout % 4 == 0): MaxOut fused (bcosconv2d.py:166-170): the Cout accumulator
                               columns are the M adjacent filters of Cout / M units; v = max over each unit before the B-cos
                               scale; out is [pixels, Cout / M] (out_pitch 0 = Cout / M); scale_out keeps width Cout and holds s at
                               the winning filter (first maximum) and 0 elsewhere, i.e. d out / d lin.  Only with bias, the scale,
                               out, scale_out, norm_out.                                                          */
    int32_t addend_sub;     /* 0 / 1: `addend` is indexed like `out`.  s > 1 (ABI v4): `addend` is the dense tensor
                               [N, ceil(OH / s), ceil(OW / s), out_pitch] of the output pixels (h % s == 0, w % s == 0); nothing is
                               added at the other pixels.  This is the input gradient of a 1x1 / stride-s shortcut convolution
                               (zero off its s-grid) handed to the main branch's gradient launch without being scattered into a
                               zero-filled full-size tensor first.  Gradient launches only (bcos_mode BCOS_NONE, no out_cgroup, no groups). */
} bcos_epilogue;

/* compute the patch norms (norm_out) but leave v unscaled: used by the MaxOut / grouped
 * general path, where bcos_maxout_scale applies the scaling afterwards. */
#define BCOS_EPI_NORM_ONLY 1
/* use the general (|lin/norm| + 1e-6)^(b-1) form even when b == 2: the reference takes that branch for
 * its learnable-B variants (bcosifyconv2d.py:91-98 with b_loss). */
#define BCOS_EPI_FORCE_POW 2
/* ReLU launches with scale_out: store the gate decision in the least significant mantissa bit of the stored
 * multiplier t = s * ch_scale * gate (1 = open; a closed gate stores exactly 0).  The one-ulp change of t (6e-8
 * relative) is far below the fp32 rounding of the products it enters, and the explanation pass then needs no
 * separate gate tensor: */
#define BCOS_EPI_SCALE_GATE_LSB 4
/* out2 = v [* mul2] gated by that bit of `mul` (instead of gate2 > 0): saves one output-sized read per launch. */
#define BCOS_EPI_GATE2_FROM_MUL 8

/* `mul` holds the kept forward ACTIVATION a = relu(lin s ch_scale + ch_shift) of the layer below (B = 2, s = |lin| / norm, no
 * residual addend) instead of its stored multiplier t = s ch_scale gate; the epilogue rebuilds
 *     t = ch_scale sqrt(|a - ch_shift| / (|ch_scale| norm))  where a > 0, else 0
 * from mul_norm / mul_csc / mul_csh.  The forward launch of such a layer then writes out + norm_out only: one
 * output-sized HBM write less (the explanation pass reads `a` where it would have read t). */
#define BCOS_EPI_MUL_FROM_ACT 16
/* Unit-norm weight projection fused into the contraction (NormedConv2d / NormedLinear, bcos/modules/bcosconv2d.py:26-35,
 * bcoslinear.py:25-27: w_hat = w / ||w||_2 per output unit, recomputed on every call): `wt` holds the RAW weights; the launch
 * gathers sum_k w[c,k]^2 of its tile's weight rows from the staging registers they pass through and multiplies every
 * accumulator column by 1 / ||w_c|| (times col_scale[c], the optional trainable `scale`) ahead of the other stages --
 * conv(x, w / ||w||) = conv(x, w) / ||w_c||.  No projected weight tensor is written or read.  Runs on the fp32 / bf16x3 loops
 * with on-the-fly operand splits (weights that change every step have no pre-split image); inference keeps a cached
 * col_scale from bcos_weight_row_invnorm and the pre-split image of the raw weights instead.  (ABI v5) */
#define BCOS_EPI_UNIT_NORM_W 32

/* -- library -------------------------------------------------------------------------- */

/* ABI version (BCOS_ABI_VERSION of the build).  A library compiled with -DBCOS_DEV_BUILD -- the only builds in which the kernels'
 * timing knock-outs and unvalidated code paths can be switched on (csrc/bcos_internal.h: BCOS_DEV_SWITCH) -- returns the version
 * with BCOS_VERSION_DEV_FLAG set: such a library may compute wrong results and must not be used as the product. */
#define BCOS_VERSION_DEV_FLAG 0x40000000
int bcos_version(void);

/* Human-readable description of the last error on this thread ("" if none). */
const char* bcos_last_error_string(void);

/* Arithmetic of the contraction inside bcos_tapconv.  Inputs, outputs, accumulation and every stored tensor are fp32 in
 * all modes; the mode only chooses how an fp32 product is evaluated on the matrix pipe:
 *   f32     v_mfma_f32_32x32x2_f32: exact fp32 FMA chain (64 cycles per 32x32x2).
 *   bf16x3  every fp32 operand is split exactly into three bf16 slices (x = h + m + l, 3 x 8 significand bits, fp32
 *           exponent range) and a*b is evaluated with the 6 leading products on v_mfma_f32_32x32x16_bf16 (products of
 *           bf16 numbers are exact in fp32; dropped terms <= 2^-21 |a b|).  Needs nothing from the caller.
 *   f16x2   every operand is scaled by a power of two (exact) and split into two fp16 numbers, x 2^e = h + l
 *           (|x 2^e - h - l| <= 2^-22 |x|), a*b = l_a h_b + h_a l_b + h_a h_b on v_mfma_f32_32x32x16_f16: 3 matrix
 *           instructions per 16 k.  The scales are per GEMM row (taken from `a_absmax`, the per-pixel max |A| side tensor
 *           that the producer of A emitted through bcos_epilogue.out_absmax or bcos_rows_absmax) and per weight row
 *           (stored in the image made by bcos_split_weights_f16x2), and are undone exactly in the epilogue.  A call that
 *           lacks either falls back to bf16x3.  All three agree with an fp64 reference to fp32-rounding level
 *           (relL2 ~8e-7 at K = 2304); tests/test_gpu_parity.py runs every parity case in every mode.
 * The mode is chosen PER CALL by bcos_operands.contraction; BCOS_CONTRACT_DEFAULT defers to a process-wide default
 * (the only process-wide setting of the library; initial value f16x2) that bcos_set_contraction_mode changes:
 * 0 = f32, 1 = bf16x3, 2 = f16x2. */
int bcos_set_contraction_mode(int mode);
int bcos_get_contraction_mode(void);

enum { BCOS_CONTRACT_DEFAULT = 0, BCOS_CONTRACT_F32 = 1, BCOS_CONTRACT_BF16X3 = 2, BCOS_CONTRACT_F16X2 = 3 };

/* Process-wide development / test switches (ABI v7; rounds 1-3 read them from the environment on every launch).  Every
 * option selects between code paths that compute the SAME operator -- none changes what an entry point means -- and each
 * has the default a deployment wants; tests and the A/B scripts flip them through bcos_set_option.  Values are plain
 * integers held in atomics: a launch reads the table once, without locks and without touching the environment. */
enum bcos_option {
    BCOS_OPT_TAIL_SPLIT = 0,      /* 1 (default): half-height tiles fill the last round of a launch of 2-8 rounds; 0: off          */
    BCOS_OPT_D_ONE_WG = 1,        /* 0 (default): off; n > 0: LDS request of the LDS-DMA kernels that leaves room for n workgroups per CU */
    BCOS_OPT_EPI_GENERIC = 2,     /* 0 (default): specialised epilogues where a launch's feature set has one; 1: general epilogue  */
    BCOS_OPT_H2_LOOP = 3,         /* 0 (default): LDS-DMA staged split-f16 loop (tile_body_d); 1: register-staged loop (same bits) */
    BCOS_OPT_PATCH = 4,           /* 1 (default): 3 x 3 / 4 x 4-union launches with per-image maxima run over an LDS-resident input
                                     patch; 0: per-tap loops with per-row operand scales everywhere                               */
    BCOS_OPT_PATCH_WIDE = 5,      /* 1 (default): 128 x 256 patch tiles for 129..256 output columns; 0: 128 x 128                 */
    BCOS_OPT_H2_TILE = 6,         /* 0 (default): tile width by cost model; 1: force 128 x 128; 2: force 128 x 256                */
    BCOS_OPT_H2_TALL = 7,         /* 1 (default): 256-row tiles for <= 64-column launches of >= H2_TALL_MIN rows; 0: 128-row tiles */
    BCOS_OPT_H2_TALL_MIN = 8,     /* row count from which the 256 x 64 tiles are used (default 2 * 256 * 512)                      */
    BCOS_OPT_ATTENTION_F32 = 9,   /* 0 (default): attention on the f16 matrix pipe (exact 2-way splits); 1: fp32 MFMA kernel       */
    BCOS_OPT_SPLIT_LIMIT = 10,    /* bytes of A from which a split-operand launch is cut into batch chunks (default and maximum
                                     2^31: the 32-bit buffer offsets); tests lower it to exercise the chunked path                */
    BCOS_OPT_LDS_MIN_KB = 11,     /* 0 (default): off; n (<= 160): the split-f16 LDS-DMA / input-patch launches request at least n KiB of
                                     LDS -- > 80 keeps two workgroups of such a launch off one CU while a launch with a smaller request
                                     can still sit beside it (round 5 probe of matrix-bound beside bandwidth-bound launches:
                                     scripts/probe/corun2_probe.py, profiles/r05_corun_probe.txt).  (Number of an option measured in
                                     round 4 and not adopted.)                                                                            */
    BCOS_OPT_RESERVED_12 = 12,    /* reserved (value fixed at 0; any other value is BCOS_E_INVAL): number of the 2-way split of K,
                                     measured in round 4 and not adopted                                                  */
    BCOS_OPT_PATCH_LEVELS = 13,   /* 1 (default): the input-patch loop runs one pass per operand-scale level present in a tile
                                     (bcos_operands.a_imgmax); 0: level 0 only, the single per-image scale of ABI v6 -- kept so that
                                     tests can show what the ladder is for (rows far darker than their image lose accuracy)      */
    BCOS_OPT_H2_WIDE_COST = 14,   /* cost of a 128 x 256 tile in quarters of a 128 x 128 tile in the tile-width choice of the f16x2 loop
                                     (rounds of tiles on 512 slots are compared): 8 = two narrow tiles (rounds 2-3), default 7            */
    BCOS_OPT_WGRAD_WGS = 15,      /* workgroups the ordered weight gradient (bcos_conv2d_wgrad_ordered) aims for when it cuts the pixels into
                                     chunks (default 768 = 3 per CU; 64 .. 4096): more chunks = more parallel work, a larger workspace and
                                     a longer combine (ABI v9)                                                                        */
    BCOS_OPT_COUNT = 16
};
/* 0, or BCOS_E_INVAL for an unknown option or a value outside its range. */
int bcos_set_option(int option, int64_t value);
int bcos_get_option(int option, int64_t* value);

/* Operands of one bcos_tapconv launch. */
typedef struct bcos_operands {
    const float* a;             /* A: activations (forward) or gradients (dgrad), NHWC fp32                          */
    const uint32_t* a_absmax;   /* NULL or [N*H*W]: fp32 bit pattern of max_c |a[pixel, c]| (any value >= the true max
                                   and < 2^8 times it keeps full precision)                                        */
    const float* wt;            /* [Cout][taps][C] fp32; always required (fallback paths read it)                  */
    const void* wt_bf16x3;      /* NULL or the image made by bcos_split_weights                                    */
    const void* wt_f16x2;       /* NULL or the image made by bcos_split_weights_f16x2                              */
    int32_t contraction;        /* BCOS_CONTRACT_*                                                                  */
    const uint32_t* a_imgmax;   /* NULL or [N]: max over the pixels of image n of a_absmax (bcos_image_absrange; ABI v6).  With it,
                                   stride-1 3 x 3 launches (and the 4 x 4 tap union of a depth-to-space gradient) of the f16x2
                                   contraction run over an LDS-resident input patch: every input element is loaded and split once
                                   per 16 channels instead of once per tap.  A pixel then serves rows with different tap windows,
                                   so the operand scales are per IMAGE, on a ladder (ABI v7): row r of image n is contracted with
                                   the scale 2^(16 l) above the image's, l = floor((E_n - E_r) / 16) for the exponents E of the image
                                   maximum and of the row's maximum over its taps (from a_absmax; exact maxima as the epilogues and
                                   bcos_rows_absmax emit them); a tile whose rows span several levels is contracted once per level,
                                   each pass writing its own rows.  Every row is therefore computed with a scale within 2^16 of its
                                   own window's maximum: no element of it is off by more than 2^-23 of that maximum, and
                                   |lin - exact| <= 2e-6 ||patch|| ||w|| per output row -- as with the per-row scales of the other
                                   f16x2 loops -- whatever the dynamic range inside the image
                                   (tests/test_gpu_parity.py::test_patch_loop_dynamic_range_inside_an_image: measured ~2e-7).  Level,
                                   scale and result of a row are functions of its image alone: an image's bits do not depend on its
                                   batch neighbours or position.                                                              */
    const uint32_t* a_imgmin;   /* NULL or [N]: min over the NONZERO pixels of image n of a_absmax (0xffffffff: all zero;
                                   bcos_image_absrange; ABI v7).  Images whose [a_imgmin, a_imgmax] span at most 2^16 have level 0
                                   everywhere and skip the level bookkeeping; launches with >= 25 taps (7 x 7 stem) take the image
                                   maximum as the scale of such an image's rows instead of scanning every row's taps.  NULL: the
                                   range is unknown -- every tile derives its rows' levels, >= 25-tap launches scan.          */
    const uint32_t* a_imgmin_c; /* NULL or [N] (ABI v9; read only when a_imgmin is NULL): a lower bound of a_imgmin stored complemented, as
                                   the launch that produced A left it in bcos_epilogue.out_imgmin_c.  It can switch the level
                                   bookkeeping of the input-patch loop on for an image that would not have needed it, never off for one
                                   that does, and decides no bit of any result; >= 25-tap launches ignore it (they scan).              */
} bcos_operands;

/* -- contraction kernels (LDS-tiled implicit GEMM on the matrix cores) ---------------------------------------- */

/* The generic fused implicit GEMM every entry point below lowers to (bcos_tapconv / bcos_tapconv_presplit are the
 * same call with only `a`, `wt` [, `wt_bf16x3`] set). */
int bcos_tapconv_ops(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi, void* stream);

/* Would bcos_tapconv_ops(ops, geom, epi, ...) fold the per-image range of its out_absmax into epi->out_imgmax / out_imgmin_c (1), or
 * not (0: the call then rejects the two fields), or are the arguments invalid (< 0)?  Launches nothing.  (ABI v9) */
int bcos_tapconv_fuses_image_range(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi);
int bcos_tapconv(const float* a, const float* wt, const bcos_tapconv_geom* geom,
                 const bcos_epilogue* epi, void* stream);

/* Which tile launcher, contraction loop and epilogue would bcos_tapconv_ops(ops, geom, epi, ...) run?  (ABI v11)  Launches nothing and needs no
 * device: the query and the launch share the same planning functions (argument validation, operand and epilogue selection, route choice) and
 * only the launch goes on to a launcher -- the answer holds under the option table and default contraction mode of the moment.  Returns 0 and
 * fills *out, or the error code bcos_tapconv_ops returns for the same arguments (out == NULL: BCOS_E_INVAL).  Every compiled launcher has an
 * id in [0, bcos_tapconv_route_count()); the ids are not stable across versions, the names are.  bcos_tapconv_group's fused narrow-output
 * form (several tap sets in one launch) is outside the query: it reports what each entry would take on its own. */
enum { BCOS_LOOP_F32 = 0,             /* v_mfma_f32_32x32x2_f32 (also the narrow-output kernel)    */
       BCOS_LOOP_BF16X3 = 1,          /* 3-way bf16 split of both operands on the fly              */
       BCOS_LOOP_BF16X3_PRESPLIT = 2, /* ... weights from the bcos_split_weights image             */
       BCOS_LOOP_F16X2_REGS = 3,      /* split-f16, register-staged (BCOS_OPT_H2_LOOP = 1)         */
       BCOS_LOOP_F16X2_DMA = 4,       /* split-f16, LDS-DMA staged                                 */
       BCOS_LOOP_F16X2_PATCH = 5 };   /* split-f16 over an LDS-resident input patch (a_imgmax)     */
typedef struct bcos_tapconv_route {
    int32_t route;        /* id; bcos_tapconv_route_name(route) names it, e.g. "d_128x192", "p_128x128_b", "skinny"                   */
    int32_t epi_kind;     /* 0 = general epilogue (always for "skinny": its own plain epilogue), k + 1 = specialised kind k of its direction */
    int32_t norm;         /* 1 = B-cos launch (forward kinds), 0 = plain / gradient launch (backward kinds)                           */
    int32_t loop;         /* BCOS_LOOP_*                                                                                               */
    int32_t bm, bn;       /* tile rows / columns (0 for the narrow-output kernel)                                                      */
    int32_t chunks;       /* 1, or the number of batch chunks of the BCOS_OPT_SPLIT_LIMIT path (the route is the first chunk's)        */
    int32_t ch_pass;      /* narrow-output kernel: input channels staged per pass (< C: the channels are walked in slices); 0 otherwise */
} bcos_tapconv_route;
int bcos_tapconv_route_query(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi, bcos_tapconv_route* out);
const char* bcos_tapconv_route_name(int route);   /* NULL outside [0, bcos_tapconv_route_count()) */
int bcos_tapconv_route_count(void);
/* Number of specialised epilogue kinds per direction (epi_kind runs over 0 .. this). */
int bcos_tapconv_epilogue_kinds(void);

/* Pre-split, pre-scaled weights for the f16x2 contraction: wt [rows][Ktot] fp32 -> image
 * [32-row tile][16-k step][plane h|l][lane][8 f16] (B fragments of v_mfma_f32_32x32x16_f16; rows padded to a multiple of
 * 128, k to a multiple of 16) followed by float[padded rows] inverse row scales.  Copied verbatim into LDS by the kernel. */
int bcos_split_weights_f16x2_bytes(int rows, int Ktot, int64_t* bytes);
int bcos_split_weights_f16x2(const float* wt, void* image, int rows, int Ktot, void* stream);
/* ... of convolution weights [rows][taps][C] (Ktot = taps * C).  For 1 < taps <= 16 and C % 16 == 0 the image stores K
 * channel-chunk-major (16-k step ks = tap ks % taps of channel chunk ks / taps), the order in which the kernel then walks
 * the taps so that a workgroup's input pixels stay cache-resident across the taps; a launch must be given the image
 * made with ITS tap count and C (bcos_tapconv_geom.TH * TW, C). */
int bcos_split_weights_f16x2_conv(const float* wt, void* image, int rows, int taps, int C, void* stream);

/* The weight banks and f16x2 images of MANY layers from ONE call -- two launches (ABI v9; a training step rebuilds every layer's forward
 * bank, its transposed / tap-reversed input-gradient banks and their images from the updated weights: ~350 small launches per ResNet-50 step).
 * Job j gathers bank[r][t][c] = c < channels ? src[r * row_stride + c * ch_stride + tap_offset[t]] : 0 (r < rows, t < taps, c < Cp) into
 * `bank` ([rows][taps][Cp] fp32) and writes `image` = what bcos_split_weights_f16x2_conv(bank, image, rows, taps, Cp) would make of it, bit
 * for bit (bcos_split_weights_f16x2_bytes(rows, taps * Cp) bytes, 16-byte aligned; NULL: the bank only).  `jobs` is a DEVICE array of
 * `njobs` descriptors -- the caller uploads it once and reuses it while the pointers in it stay valid; `max_rows` / `max_ktot` >= every
 * job's rows / taps * Cp (they size the grids); `row_max`: DEVICE scratch, ZERO-FILLED by the caller before every call, in which job j
 * owns the words [row_offset, row_offset + rows).
 *   forward bank of OIHW weights [Cout][Cin][kh][kw]:   rows = Cout, channels = Cin, row_stride = Cin kh kw, ch_stride = kh kw, tap_offset[t] = t
 *   a parity class of the input gradient:               rows = Cin, channels = Cout, row_stride = kh kw, ch_stride = Cin kh kw,
 *                                                        tap_offset[a TW + b] = rs_h[a] kw + rs_w[b] (the class's tap lists, bcos_hip/ops.py: DgradPlan)
 *   a linear layer [Cout][Cin] / its transpose:         rows = Cout / Cin, channels = Cin / Cout, strides (Cin, 1) / (1, Cin), one tap at offset 0 */
#define BCOS_PREP_MAX_TAPS 49
typedef struct bcos_weight_prep_job {
    const float* src;
    float* bank;
    void* image;
    int32_t rows, channels, Cp, taps;
    int32_t row_stride, ch_stride;
    int32_t tap_offset[BCOS_PREP_MAX_TAPS];
    int32_t row_offset;          /* the job's first word in row_max */
} bcos_weight_prep_job;
int bcos_weight_prep_batch(const bcos_weight_prep_job* jobs, int njobs, int max_rows, int max_ktot, uint32_t* row_max, void* stream);

/* out[r] = fp32 bit pattern of max_c |x[r*pitch + c]|, c < C (C % 4 == 0; pitch 0 = C): the `a_absmax` of a tensor whose
 * producer is not a bcos_tapconv epilogue (network input, pooling, attention ...).  One pass over x. */
int bcos_rows_absmax(const float* x, uint32_t* out, int64_t rows, int C, int pitch, void* stream);
/* out[n] = max over p < pixels_per_image of absmax[n * pixels_per_image + p]: bcos_operands.a_imgmax from a_absmax (ABI v6). */
int bcos_image_absmax(const uint32_t* absmax, uint32_t* out, int n_images, int pixels_per_image, void* stream);
/* ... and out_min[n] = the smallest NONZERO absmax of image n, 0xffffffff if every pixel is zero (bcos_operands.a_imgmin; ABI v7;
 * out_min may be NULL). */
int bcos_image_absrange(const uint32_t* absmax, uint32_t* out_max, uint32_t* out_min, int n_images, int pixels_per_image, void* stream);
/* The same range by several workgroups per image (ABI v9): out_max [N] and out_min_c [N] are ZERO-FILLED by the caller; out_min_c[n] receives
 * the COMPLEMENT of the minimum over the nonzero pixels (~v; 0 = no nonzero pixel) -- the form of bcos_epilogue.out_imgmin_c, handed to the
 * reading launch as bcos_operands.a_imgmin_c. */
int bcos_image_absrange_c(const uint32_t* absmax, uint32_t* out_max, uint32_t* out_min_c, int n_images, int pixels_per_image, void* stream);

/* Pre-split weights for the bf16x3 contraction.  Weights are constant at inference (NormedConv2d / BcosifyConv2d
 * weights only change in training, bcosconv2d.py:26-35), so their exact 3-way bf16 split is done once:
 *   wt [rows][Ktot] fp32 -> wt3, laid out [32-row tile][16-k step][plane h|m|l][lane][8 bf16], which is exactly the B
 *   fragment a wavefront feeds to v_mfma_f32_32x32x16_bf16 (rows padded to a multiple of 128, k to a multiple of 16).
 * bcos_tapconv_presplit then loads B straight into registers (six coalesced 16-byte loads per lane and 16-k step): no
 * conversion, no LDS traffic and no barrier participation for the weights.  Results are bit-identical to bcos_tapconv.
 * wt3 == NULL, contraction mode 0 or a narrow-output launch fall back to wt (which must always be passed). */
int bcos_split_weights_bytes(int rows, int Ktot, int64_t* bytes);
int bcos_split_weights(const float* wt, void* wt3, int rows, int Ktot, void* stream);
int bcos_tapconv_presplit(const float* a, const float* wt, const void* wt3, const bcos_tapconv_geom* geom,
                          const bcos_epilogue* epi, void* stream);

/* `count` tapconv launches over the SAME input `a` (e.g. the parity classes of a strided input gradient, one tap set,
 * weight tensor and output offset each): same result as calling bcos_tapconv once per entry.  Narrow outputs
 * (Cout <= 8, count <= 4, identical shapes, plain / addend / mul epilogue on one output tensor) run as ONE launch in
 * which every workgroup stages its input patch once for all tap sets (the ResNet stem gradient: 4 launches -> 1). */
int bcos_tapconv_group(const float* a, const float* const* wts, const bcos_tapconv_geom* geoms,
                       const bcos_epilogue* epis, int count, void* stream);

/*
 * Replaces BcosConv2d.forward_impl (bcos/modules/bcosconv2d.py:153-194) and
 * BcosifyConv2d.forward_impl (bcos/modules/bcosifyconv2d.py:50-102) for groups == 1,
 * max_out == 1: conv2d + calc_patch_norms (bcosconv2d.py:196-231) + |cos|^(B-1) scaling in
 * one pass.  x [N,H,W,Cin] NHWC, w [Cout,kh,kw,Cin], y [N,Ho,Wo,Cout] NHWC.
 * `bias` may be NULL.  `scale_out` (NULL or [N,Ho,Wo,Cout]) receives the detached dynamic
 * scale s = dy/dlin used by the explanation pass; `norm_out` (NULL or [N,Ho,Wo]) the patch
 * norms.  Unit-norm weights (NormedConv2d, bcosconv2d.py:26-35) are obtained by running
 * bcos_weight_rownorm_scale on `w` first (the projection is input independent).
 */
int bcos_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                    float* scale_out, float* norm_out,
                    int N, int Cin, int H, int W, int Cout, int kh, int kw,
                    int sh, int sw, int ph, int pw, int dh, int dw,
                    float b, void* stream);

/*
 * Replaces BcosLinear.forward (bcos/modules/bcoslinear.py:88-130) and BcosifyLinear.forward
 * (bcos/modules/bcosifylinear.py:42-95), max_out == 1.  x [rows,Cin], w [Cout,Cin],
 * y [rows,Cout].
 */
int bcos_linear_fwd(const float* x, const float* w, const float* bias, float* y,
                    float* scale_out, float* norm_out,
                    int64_t rows, int Cin, int Cout, float b, void* stream);

/*
 * Input gradient of bcos_conv2d_fwd in explanation mode (scale detached): replaces the
 * autograd convolution_backward + mul of bcos/common.py:177.
 *     gx = conv_transpose(gy * s, w)
 * gy, s: [N,Ho,Wo,Cout]; wT: [Cin,kh,kw,Cout] = w with the spatial taps flipped and
 * Cout/Cin swapped (stride 1) -- produced by bcos_hip/ops.py: DgradPlan; for
 * stride > 1 the Python layer issues one bcos_tapconv per parity class instead.
 * `gylin` is gy*s precomputed by the caller (bcos_mul) or fused into the producer.
 */
int bcos_conv2d_dgrad_s1(const float* gylin, const float* wT, float* gx,
                         int N, int Cin, int H, int W, int Cout, int kh, int kw,
                         int ph, int pw, void* stream);

/* Input gradient of bcos_linear_fwd in explanation mode: gx[rows,Cin] = gylin[rows,Cout] @ w. */
int bcos_linear_dgrad(const float* gylin, const float* wT, float* gx,
                      int64_t rows, int Cin, int Cout, void* stream);

/* -- HBM-bound helper kernels ---------------------------------------------------------- */

/* w[r,:] *= gain[r] / ||w[r,:]||_2  (gain NULL = 1): NormedConv2d / NormedLinear unit-norm
 * projection (bcosconv2d.py:28-35, bcoslinear.py:25-27).  One wavefront per row. */
int bcos_weight_rownorm_scale(const float* w, const float* gain, float* w_out,
                              int rows, int64_t cols, void* stream);

/* inv[r] = gain[r] / ||w[r,:]||_2  (gain NULL = 1): the per-filter factor bcos_epilogue.col_scale takes when the unit-norm
 * projection is folded into the contraction instead of being written out as a projected weight tensor (one read of w, `rows`
 * floats written).  (ABI v5) */
int bcos_weight_row_invnorm(const float* w, const float* gain, float* inv, int rows, int64_t cols, void* stream);

/* out[i] = a[i] * b[i] */
int bcos_mul(const float* a, const float* b, float* out, int64_t n, void* stream);

/* dst[i] = src[i], n floats, 16-byte aligned, as the plainest streaming kernel this library can issue: every thread keeps eight
 * global_load_dwordx4 in flight and stores them with global_store_dwordx4 (non-temporal both ways), 2048 workgroups walking the
 * buffers with a grid stride.  It exists as the REFERENCE the bandwidth-bound launches are priced against (bench.py:
 * roofline.by_bound.hbm.stream_copy_gbps -- /opt/skills/guides/MI355X_MICROARCH.md measures 6.29 TB/s for such a copy), and as the
 * device-to-device copy of the engines where one is needed on a given stream.  (ABI v9) */
int bcos_stream_copy(const float* src, float* dst, int64_t n, void* stream);

/* Row-wise L2 normalisation y[r,:] = x[r,:] / ||x[r,:]||_2 and / or its inverse norms inv_norm[r] (either may be NULL): the
 * `attn_unpool` head of BcosAttentionPool2d (bcos/modules/bcosattnpool.py:23-32: x / x.norm(dim=-1), norm detached in
 * explanation mode) and `outa / outa.norm(dim=-1)` of the zero-shot attribution
 * (interpretability/analyses/text_localisation.py:76).  One wavefront per row.  (ABI v5) */
int bcos_rows_normalize(const float* x, float* y, float* inv_norm, int64_t rows, int C, void* stream);

/* Gradient of a cosine logit w.r.t. the un-normalised feature row f (text_localisation.py:76-78, 101:
 * `img_features = outa / outa.norm(...)`, `logits = img_features @ zeroshot_weight`, `logits.max(1).values.backward`):
 *   out[r,:] = coef[r] * inv_norm[r] * (w[r,:] - l[r] * u[r,:])
 * with u = f / ||f|| (given), w[r,:] = the text embedding of the explained class of row r, l[r] = u[r,:] . w[r,:], coef[r] the
 * (detached) pooling weight of the row (NULL = 1).  (ABI v5) */
int bcos_cosine_grad(const float* u, const float* w, const float* l, const float* inv_norm, const float* coef, float* out,
                     int64_t rows, int C, void* stream);

/* Backward of the fused MaxOut: glin[r, c] = gy[r, c / M] * t[r, c] with t = the scale_out of a max_out launch
 * (gy [rows, Cout / M], t and glin [rows, Cout], Cout % 4 == 0): routes the gradient to the winning filter. */
int bcos_maxout_expand(const float* gy, const float* t, float* glin, int64_t rows, int Cout, int max_out, void* stream);

/* MaxOut + B-cos scaling for the non-fused general path (max_out > 1, groups > 1):
 * lin [rows, Cout*max_out] -> y [rows, Cout] with per-row norms given (bcosconv2d.py:166-194). */
int bcos_maxout_scale(const float* lin, const float* norm, float* y, float* scale_out,
                      int32_t* argmax_out, int64_t rows, int Cout, int max_out,
                      int norm_stride, float b, void* stream);

/*
 * Network input: AddInverse (bcos/data/transforms.py:54-55, if add_inverse) + the 6-channel
 * Normalize of BcosifyNetwork (bcosify.py:38-43) + NCHW -> NHWC with channel padding.
 * x: [N,Cx,H,W] NCHW with Cx = 3 (add_inverse) or 6; out: [N,H,W,Cpad], channels >= 6 zero.
 * absmax_out (NULL or [N*H*W]): per-pixel max |out| bit patterns, the operand-scale side tensor of the f16x2
 * contraction (see bcos_operands.a_absmax) -- saves the separate bcos_rows_absmax pass over the tensor.
 */
int bcos_prep_input(const float* x, float* out, const float* mean6, const float* std6, uint32_t* absmax_out,
                    int N, int Cx, int H, int W, int Cpad, int add_inverse, void* stream);

/*
 * End of the explanation pass (bcos/common.py:180-181): from the gradient w.r.t. the
 * normalised NHWC input gxn [N,H,W,Cpad] produce the dynamic linear weights
 * W(x) = d logit / d x  [N,6,H,W] NCHW (chain rule through Normalize: / std) and the
 * contribution map sum_c x_c * W_c  [N,H,W].  x6 is the 6-channel network input
 * ([N,6,H,W], or [N,3,H,W] with add_inverse).
 */
int bcos_finalize_explanation(const float* gxn, const float* x, const float* std6,
                              float* weights_out, float* contrib_out,
                              int N, int Cx, int H, int W, int Cpad, int add_inverse,
                              void* stream);

/* (x * gx).sum(channel) for NCHW tensors: bcos/common.py:181. */
int bcos_contrib_map(const float* x, const float* gx, float* out,
                     int N, int C, int H, int W, void* stream);

/* AvgPool2d(k, s, p), count_include_pad = True (torchvision maxpool swapped for
 * nn.AvgPool2d(3,2,1): bcosification/experiment_parameters.py:99), NHWC. */
int bcos_avgpool2d_fwd(const float* x, float* y, int N, int H, int W, int C,
                       int k, int s, int p, int OH, int OW, void* stream);
/* ... also writing the per-pixel max |y| bit patterns of the pooled tensor (absmax_out [N*OH*OW], may be NULL) for the f16x2 contraction
 * that reads it: k in {2, 3}, C / 4 a power of two <= 64.  (ABI v9) */
int bcos_avgpool2d_fwd_absmax(const float* x, float* y, uint32_t* absmax_out, int N, int H, int W, int C, int k, int s, int p,
                              int OH, int OW, void* stream);
/* ... its input gradient, optionally multiplied elementwise by `mul` ([N,H,W,C]); absmax_out (NULL or [N*H*W], needs
 * C / 4 a power of two <= 64): per-pixel max |gx| bit patterns for the f16x2 contraction that reads gx. */
int bcos_avgpool2d_bwd(const float* gy, const float* mul, float* gx, uint32_t* absmax_out, int N, int H, int W, int C,
                       int k, int s, int p, int OH, int OW, void* stream);

/* AdaptiveAvgPool2d(1) + flatten + LogitLayer (bcos/modules/logitlayer.py:22-27):
 * y[n,c] = mean_hw x[n,hw,c] / T + bias. */
int bcos_global_avgpool_logits(const float* x, float* y, int N, int HW, int C,
                               float inv_temperature, float logit_bias, void* stream);

/* Start of the explanation backward for a GAP head: for every image n with explained class
 * cls[n],  glin[n,hw,c] = (c == cls[n]) * scale[n,hw,c] * inv_temperature / HW
 * (the gradient of logit cls[n] w.r.t. the head's `lin`, bcos/common.py:166-177). */
int bcos_head_onehot_grad(const int64_t* cls, const float* scale, float* glin,
                          int N, int HW, int C, float inv_temperature, void* stream);
/* The same gradient carried THROUGH the head layer in one launch: it is rank one per image (only column cls[n] of the one-hot tensor
 * is non-zero), so the input gradient of the head's linear map is  v[n, r, :] = inv_temperature / R * scale[n, r, cls[n]] *
 * row_scale[n r] * w[cls[n], :]  -- bcos_head_onehot_grad followed by the K-long input-gradient contraction, without the [N, R, K]
 * tensor.  scale [N, R, K] (the head's stored multiplier), w [K, D] (its weight rows, D % 4 == 0), row_scale [N R] or NULL (the rstd of
 * a LayerNorm folded into the head), mul [N R, D] or NULL.  out = v * mul (mul NULL: v), out2 = v (may be NULL), out_absmax [N R] or
 * NULL: per-row max |out| bit patterns.  16-byte aligned tensors.  An image whose cls[n] is outside [0, K) gets a ZERO gradient
 * (what the one-hot tensor gave; nothing is read out of range).  (ABI v8; gap-reordered SimpleViT head, vit.py:197-199) */
int bcos_head_rank1_grad(const int64_t* cls, const float* scale, const float* w, const float* row_scale, const float* mul, float* out,
                         float* out2, uint32_t* out_absmax, int N, int R, int K, int D, float inv_temperature, void* stream);
/* ... with the whole second output of the gradient epilogue (bcos_epilogue.out2, the shortcut's share behind a residual block):
 * out2 = v [* mul2], zeroed where the producing block's ReLU was closed -- gate2 [N R, D] > 0, or (gate2_from_mul) the low mantissa
 * bit of mul, as BCOS_EPI_GATE2_FROM_MUL reads it -- and its row maxima.  The GAP + fc head of the ResNets (N x 7 x 7 x 1000 one-hot
 * tensor and a K = 1000 contraction in rounds 1-4).  (ABI v8) */
int bcos_head_rank1_grad_ex(const int64_t* cls, const float* scale, const float* w, const float* row_scale, const float* mul,
                            const float* mul2, const float* gate2, int gate2_from_mul, float* out, float* out2, uint32_t* out_absmax,
                            uint32_t* out2_absmax, int N, int R, int K, int D, float inv_temperature, void* stream);
/* The start of the explanation pass for a LINEAR FUNCTIONAL of the logits, f = sum_k c_k y_k, instead of one logit.  In explanation mode
 * the network is linear in the head cotangent (scales, gates and variances are detached, the LogitLayer bias is a constant:
 * bcos/common.py:163-181), so W_f(x) = sum_k c_k W_k(x) and only this launch knows about the functional -- "why class a rather than b"
 * (y_a - y_b), the mean-corrected y_t - mean_k y_k of OursRelative (interpretability/explanation_methods/explainers/ours.py:28-33).
 * Additive entry points of ABI v12: a binding recognises them by the presence of the symbols.
 *
 * SPARSE form: bcos_head_rank1_grad_ex with J classes cls [N, J] (int64) and coefficients coef [N, J] (fp32) per image, 1 <= J <= 8:
 *   v[n, r, :] = sum_{j < J} a_j * w[cls[n, j], :],   a_j = ((inv_temperature / R * scale[n, r, cls[n, j]]) * row_scale[n r]) * coef[n, j]
 * -- one fp32 chain in ascending j of separately rounded products.  Every output of the _ex form: out = v * mul (mul NULL: v),
 * out2 = v [* mul2] gated by gate2 > 0 or by the low mantissa bit of mul, both row maxima.  A class outside [0, K) contributes ZERO and
 * nothing is read out of range.  J = 1 with coef = 1 gives the bits of bcos_head_rank1_grad_ex.
 * BCOS_E_INVAL: a NULL cls / coef / scale / w / out, N / R / K / D <= 0, D % 4 != 0, J < 1, out2's companions without out2,
 * gate2_from_mul without mul or with gate2, w / mul / mul2 / gate2 / out / out2 not 16-byte aligned, cls / coef not aligned to their
 * element.  BCOS_E_NOSUP: J > 8 (use the dense form).  The library never reads device memory. */
int bcos_head_rankm_grad(const int64_t* cls, const float* coef, int J, const float* scale, const float* w, const float* row_scale,
                         const float* mul, const float* mul2, const float* gate2, int gate2_from_mul, float* out, float* out2,
                         uint32_t* out_absmax, uint32_t* out2_absmax, int N, int R, int K, int D, float inv_temperature, void* stream);
/* DENSE form: bcos_head_onehot_grad with a cotangent row per image, cot [N, K], instead of a one-hot one:
 *   glin[n, r, k] = (cot[n, k] * scale[n, r, k]) * (inv_temperature / R)      scale [N, R, K] -> glin [N, R, Kp],
 * Kp = K rounded up to a multiple of 4, the pad columns written as zeros (the input-gradient contraction of the head reads glin with
 * bcos_tapconv_geom.a_pitch = Kp); out_absmax [N R] or NULL: the bit patterns of the row maxima of |glin| (that contraction's a_absmax).
 * BCOS_E_INVAL: a NULL cot / scale / glin, N / R / K <= 0, glin not 16-byte aligned, cot / scale / out_absmax not 4-byte aligned. */
int bcos_head_cotangent_grad(const float* cot, const float* scale, float* glin, uint32_t* out_absmax, int N, int R, int K,
                             float inv_temperature, void* stream);

/* Row-wise arg-max over logits [N,C] -> idx [N] (int64), val [N]; ties -> lowest index
 * (torch.max semantics used at bcos/common.py:166). */
int bcos_argmax_rows(const float* x, int64_t* idx, float* val, int N, int C, void* stream);

/* BatchNormUncentered2d eval as a standalone op (module API path), NHWC:
 * y = x * scale[c] + shift[c] (shift may be NULL) (batchnorm_uncentered.py:46-60). */
int bcos_channel_affine(const float* x, const float* scale, const float* shift, float* y,
                        int64_t pixels, int C, int relu, void* stream);
/* y = [relu](x * scale[c] + shift[c] + addend): normalisation + affine + residual add + ReLU of a training-mode unit in one pass
 * (BatchNormUncentered2d with batch statistics followed by `out += identity; relu`, torchvision BasicBlock / Bottleneck.forward);
 * out = act > 0 ? g : 0, the gate of that ReLU on the way back.  (ABI v7; bcos_hip/train_plan.py) */
int bcos_channel_affine_add(const float* x, const float* scale, const float* shift, const float* addend, float* y, int64_t pixels,
                            int C, int relu, void* stream);
int bcos_relu_bwd(const float* g, const float* act, float* out, int64_t n, void* stream);

/* The same map row by row with the per-row max |y| (fp32 bit pattern, like bcos_epilogue.out_absmax) written to y_absmax [rows]:
 * a training-mode unit's output carries the operand scale of the contraction that reads it, so that the forward and input-gradient
 * contractions of a training step run the 3-product split-f16 loop.  addend / shift may be NULL; tensors 16-byte aligned.  (ABI v8) */
int bcos_channel_affine_rows(const float* x, const float* scale, const float* shift, const float* addend, float* y,
                             uint32_t* y_absmax, int64_t rows, int C, int relu, void* stream);

/* -- densely connected plans (bcos_dense.hip; additive entry points of ABI v12, recognised by symbol presence) ----- */
/* Pre-activation of a consumer of a concatenated feature buffer: torchvision's _DenseLayer / _Transition / norm5 apply their own
 * BatchNormUncentered2d (eval: a per-channel affine map, batchnorm_uncentered.py:46-60) and ReLU to cat(features) in front of the
 * contraction (reference standard_models.py:56-63 runs `features` and a functional ReLU behind norm5).  With the features of a block
 * stored once, raw, as channel slices of one NHWC buffer, that is a row-wise map from a slice of pitched rows to a dense operand:
 *     y[r * y_pitch + c] = act(x[r * x_pitch + c] * scale[c] + shift[c]) [* mul[r * C + c]],   r < rows, c < C,
 * act = max(., 0) for relu = 1, the identity for relu = 0.  scale, shift and mul may each be NULL (the stage is skipped: with all of
 * them NULL and relu = 0 the call copies a dense tensor into a slice or a slice out of one, bit for bit).  A pitch of 0 means C.
 * x * scale + shift is two roundings (product, then sum), the arithmetic of bcos_channel_affine_rows: with mul == NULL and
 * y_pitch in {0, C}, y and y_absmax carry the bits bcos_channel_affine_rows writes for a contiguous copy of the slice.  mul is one
 * more rounding.  y_absmax[r] (may be NULL) = fp32 bit pattern of max_c |y[r, c]|, written plainly (no atomics, no zero fill needed).
 * Nothing outside [0, C) of a pitched row is read or written.
 * BCOS_E_INVAL: NULL x / y, rows <= 0, C <= 0, C % 4 != 0, relu outside {0, 1}, a nonzero pitch < C or not a multiple of 4, a tensor
 * that is not 16-byte aligned (y_absmax: 4-byte).  BCOS_E_NOSUP: C > 8192 with C / 4 not a divisor of 64. */
int bcos_slice_affine_rows(const float* x, int64_t x_pitch, const float* scale, const float* shift, const float* mul, float* y,
                           int64_t y_pitch, uint32_t* y_absmax, int64_t rows, int C, int relu, void* stream);

/* Its input gradient in explanation mode (the norm's variance is a constant, batchnorm_uncentered.py:46-60, so the map is linear up to
 * the ReLU gate), added into the consumer's slice of the block's gradient buffer:
 *     g[r * g_pitch + c] = (accumulate ? g[r * g_pitch + c] : 0) + d[r * C + c] * scale[c] * gate,
 * gate = (x[r * x_pitch + c] * scale[c] + shift[c] > 0) for relu = 1 -- the SAME expression with the same two roundings as
 * bcos_slice_affine_rows, so gate <=> (the forward's y > 0) bit for bit -- and 1 for relu = 0 (x may then be NULL).  Per element one
 * product and one sum, in that order: |g - exact| <= 2^-23 (|g_old| + |d scale|).  accumulate = 0 never reads g (it may hold anything,
 * NaN included): the first consumer handled on the way back covers every channel of its block, so no zero fill is needed.
 * scale / shift may be NULL as above; d is dense [rows, C].  Nothing outside [0, C) of a pitched row is read or written.
 * BCOS_E_INVAL: NULL d / g, relu = 1 without x, rows / C / pitches / alignment as above, accumulate outside {0, 1}.  BCOS_E_NOSUP as above. */
int bcos_slice_affine_bwd_acc(const float* d, const float* x, int64_t x_pitch, const float* scale, const float* shift, float* g,
                              int64_t g_pitch, int64_t rows, int C, int relu, int accumulate, void* stream);

/* -- the same consumers in TRAINING mode (bcos_dense.hip; additive entry points of ABI v12, recognised by symbol presence) ----------
 * BatchNormUncentered2d with batch statistics (reference bcos/modules/norms/uncentered_norms/batchnorm_uncentered.py:36-44) as torchvision's
 * _DenseLayer.norm1, _Transition.norm and norm5 apply it to cat(features): var = x.var((0, 2, 3), unbiased=False) -- the centred second
 * moment although nothing is centred --, running_var <- (1 - momentum) running_var + momentum var, y = x weight / sqrt(var + eps) + bias.
 * Every reader of a channel of the concatenation sees the same column, so (mean, var) of a channel are computed ONCE, when its slice of
 * the block buffer is complete, and shared; a reader adds its own weight / eps / momentum / running_var (bcos_bn_reader_finish).
 * Throughout, x is a slice [rows, C] of pitched rows, C % 4 == 0, a pitch of 0 means C; nothing outside [0, C) of a pitched row is read
 * or written; nothing uses atomics.
 *
 * The column reductions (bcos_slice_batch_stats, bcos_slice_relu_bwd_colsums) split the rows into nblk blocks of rpb rows,
 *     nblk0 = min(ceil(rows / 128), 1024), rpb = ceil(rows / nblk0), nblk = ceil(rows / rpb)
 * -- a function of `rows` alone --, and take a caller-owned workspace of bcos_slice_col_ws_floats(rows, C) = 3 nblk C floats (16-byte
 * aligned).  Inside a block a column's rows r_lo + t, r_lo + t + 32, ... are added in order by lane t < 32, the 32 lanes in lane order,
 * the blocks in block order by a second launch: the summation order of a column depends on `rows` alone, NOT on C, the pitch, the slice
 * offset or which other columns are in the call.  The results of a 96-channel slice are bit for bit those of three calls of 32 channels.
 * No addend passes through more than D(rows) = ceil(rpb / 32) + ceil(nblk / 16) + 56 additions.
 *
 * bcos_slice_batch_stats: ONE pass over x.  mean[c], var[c] = the centred second moment, from per-block sums of (x - c_b) and (x - c_b)^2
 * shifted by the block's first row c_b and combined as (n_b, mean_b, M2_b) (Chan et al.).  With A = max_r |x[r, c]| and
 * R = max_r |x[r, c] - mean[c]| (exact mean):   |mean - exact| <= 2^-23 * 3 D A,   |var - exact| <= 2^-23 * D (16 R^2 + 2 R A).
 * BCOS_E_INVAL: NULL x / mean / var / workspace, rows <= 0, C <= 0, C % 4 != 0, a nonzero pitch < C or not a multiple of 4, x or the
 * workspace not 16-byte aligned (mean, var: 4-byte), a workspace smaller than the query's.  BCOS_E_NOSUP: C > 2097120. */
int bcos_slice_col_ws_floats(int64_t rows, int C, int64_t* floats);
int bcos_slice_batch_stats(const float* x, int64_t x_pitch, float* mean, float* var, float* workspace, int64_t workspace_floats,
                           int64_t rows, int C, void* stream);

/* One reader's share, ONE launch on [C] vectors: rstd = 1 / sqrt(var + eps), g = weight * rstd (weight NULL: rstd) and -- running_var not
 * NULL -- running_var = (1 - momentum) running_var + momentum var in place.  var is the reader's range of a block's shared vector.
 * |rstd - exact| <= 2^-22 exact (the sum's rounding and rsqrtf's), |g - weight exact rstd| <= 3 * 2^-23 |g|,
 * |running_var - exact| <= 2^-22 ((1 - momentum) |running_var_old| + momentum |var|).
 * BCOS_E_INVAL: NULL var / rstd / g, C <= 0, eps < 0, momentum outside [0, 1], a vector that is not 4-byte aligned. */
int bcos_bn_reader_finish(const float* var, const float* weight, float* running_var, float* rstd, float* g, int C, float eps, float momentum,
                          void* stream);

/* The column sums of that norm's backward pass from the dense incoming gradient d [rows, C] (w.r.t. the OUTPUT of norm + ReLU) and the raw
 * slice x, without writing a per-element tensor:   sgx[c] = sum_r gate d x,   sg[c] = sum_r gate d (sg may be NULL),
 * gate = (x * gvec[c] + shift[c] > 0) with the two roundings of bcos_slice_affine_rows (shift may be NULL), so gate <=> (the forward's
 * y > 0) bit for bit.  Its finish also writes gw = sgx * rstd (the norm's weight gradient; may be NULL) and
 * coef = -(gvec * sgx) * rstd^2 / rows (the variance-term coefficient of bcos_slice_bn_bwd_acc; may be NULL) -- the formulas of
 * bcos_relu_bwd_colsums.  Order and workspace as above (2 nblk C floats are used):
 *     |sgx - exact| <= 2^-23 D sum_r |gate d x|,   |sg - exact| <= 2^-23 D sum_r |gate d|;
 * gw is one rounding from sgx * rstd, coef four from its formula (|coef - formula(sgx)| <= 5 * 2^-24 |coef|).
 * BCOS_E_INVAL: NULL d / x / gvec / sgx / workspace, gw or coef without rstd, rows / C / pitch as above, d / x / gvec / shift / workspace
 * not 16-byte aligned (the other vectors: 4-byte), a workspace smaller than the query's.  BCOS_E_NOSUP as above. */
int bcos_slice_relu_bwd_colsums(const float* d, const float* x, int64_t x_pitch, const float* gvec, const float* shift, const float* rstd,
                                float* sgx, float* sg, float* gw, float* coef, float* workspace, int64_t workspace_floats, int64_t rows,
                                int C, void* stream);

/* The training form of bcos_slice_affine_bwd_acc (relu = 1): the norm's input gradient added into the reader's slice of the block's
 * gradient buffer,
 *     g[r * g_pitch + c] = (accumulate ? g[r * g_pitch + c] : 0) + gate * d[r * C + c] * scale[c] + (x[r * x_pitch + c] - mean[c]) * coef[c],
 * gate as above, scale = weight / std, coef from bcos_slice_relu_bwd_colsums.  coef NULL (then mean must be NULL too): the variance is a
 * constant -- a norm in eval() inside net.train(), or `detach` -- and the call writes the bits of bcos_slice_affine_bwd_acc; mean NULL
 * with coef: 0.  Roundings in this order: d scale; x - mean; (.) coef; their sum; the sum with the old g.  Per element
 *     |g - exact| <= 2^-23 (|g_old| + 2 |d scale| + 2 |(x - mean) coef|)      (coef NULL: 2^-23 (|g_old| + |d scale|), as there).
 * accumulate = 0 never reads g.  BCOS_E_INVAL: NULL d / x / g, mean without coef, rows / C / pitches / alignment (every tensor 16-byte) /
 * accumulate as for bcos_slice_affine_bwd_acc.  BCOS_E_NOSUP: C > 8192 with C / 4 not a divisor of 64. */
int bcos_slice_bn_bwd_acc(const float* d, const float* x, int64_t x_pitch, const float* scale, const float* shift, const float* mean,
                          const float* coef, float* g, int64_t g_pitch, int64_t rows, int C, int accumulate, void* stream);

/* -- training-mode backward (bcos_train.hip) ------------------------------------------ */
/* Outside explanation mode the dynamic scale is not detached (bcosconv2d.py:176-194), so with lin = conv(x, W) (+ bias),
 * y = s(lin, norm) * lin:   gx = dgrad(gy * dy/dlin, W) + x (.) PatchSum^T(dL/dnorm / norm),   gW = wgrad(gy * dy/dlin, x).
 *
 * bcos_train_scale_bwd: per output pixel m (rows) and channel c, from the forward's y, s (scale_out) and norm (norm_out):
 *     glin[m,c] = gy[m,c] * dy/dlin            B == 2: 2 s                  else: s (1 + (B-1) q / (q + 1e-6)), q = |lin| / norm
 *     rnorm[m]  = sum_c gy[m,c] * dy/dnorm / (d norm / d x denominator)
 *                                              B == 2: dy/dnorm = -y / norm   else: -(B-1) y q / ((q + 1e-6) norm)
 *   with the denominator norm (BCOS_CONV_EPS: sqrt(S + 1e-6)) or norm - 1e-12 (BCOS_LINEAR_EPS: ||x|| + 1e-12).
 *   force_pow selects the general form at B == 2 (the b_loss variants, bcosifyconv2d.py:91-98).
 *   bgrad (NULL = off; general form only): *bgrad += sum_{m,c} gy y ln(q + 1e-6) = dL/dB_eff, the gradient of a learnable
 *   exponent (the reference makes `b` an nn.Parameter, bcos/training/trainer.py:451-463; bcosifyconv2d.py:60-65,91-98); the
 *   caller zeroes it and applies d B_eff / d b (clamping: [b >= 1 + 1e-6]; b_loss: 1). */
int bcos_train_scale_bwd(const float* gy, const float* y, const float* s, const float* norm, float* glin, float* rnorm,
                         float* bgrad, int64_t rows, int C, int bcos_mode, float b, int force_pow, void* stream);
/* The same with glin_absmax [rows] (may be NULL): the per-row max |glin| for the input-gradient launch that reads glin.  (ABI v8) */
int bcos_train_scale_bwd_absmax(const float* gy, const float* y, const float* s, const float* norm, float* glin, float* rnorm,
                                float* bgrad, uint32_t* glin_absmax, int64_t rows, int C, int bcos_mode, float b, int force_pow,
                                void* stream);
/* The same behind a BatchNormUncentered2d (batchnorm_uncentered.py:36-44): g_out is the gradient w.r.t. the NORM's output and the launch
 * forms the gradient w.r.t. y itself on the way -- gy = g_out * bn_g[c] + (y - bn_mean[c]) * bn_coef[c] with bn_g = weight / std and
 * bn_coef the variance-term coefficient of bcos_relu_bwd_colsums (NULL: the variance is a constant -- explanation mode or a layer in
 * eval(); bn_mean NULL: 0) -- what bcos_channel_axpby would write and this launch read back.  Channel vectors 16-byte aligned.  (ABI v8) */
int bcos_train_scale_bwd_bn(const float* g_out, const float* y, const float* s, const float* norm, const float* bn_g,
                            const float* bn_mean, const float* bn_coef, float* glin, float* rnorm, uint32_t* glin_absmax, int64_t rows,
                            int C, int bcos_mode, float b, int force_pow, void* stream);

/* Backward of bcos_weight_rownorm_scale (NormedConv2d / NormedLinear in training mode, bcosconv2d.py:26-35,
 * bcoslinear.py:25-27): with w_hat = w / ||w|| per row and w_eff = gain * w_hat,
 *     gw[r,:] = gain[r] / ||w[r]|| * (g_eff[r,:] - w_hat[r,:] <w_hat[r], g_eff[r]>),   ggain[r] = <w_hat[r], g_eff[r]>.
 * gain NULL = 1; gw or ggain may be NULL. */
int bcos_weight_rownorm_bwd(const float* w, const float* g_eff, const float* gain, float* gw, float* ggain, int rows,
                            int64_t cols, void* stream);

/* MaxOut backward by index (training mode): full[r, c * M + argmax[r, c]] = g[r, c], zero at the other filters of the unit
 * (g [rows, Cout], argmax from bcos_maxout_scale, full [rows, Cout * M]; bcosconv2d.py:166-170). */
int bcos_maxout_scatter(const float* g, const int32_t* argmax, float* full, int64_t rows, int Cout, int max_out, void* stream);

/* out[n,h,w,c] = x[n,h,w,c] * sum of rnorm[n,i,j] over the output pixels (i,j) whose patch (kernel kh x kw, stride,
 * padding, dilation) contains (h,w): the input gradient through calc_patch_norms (bcosconv2d.py:196-231).  x [N,H,W,x_pitch]
 * (C channels used, x_pitch 0 = C), rnorm [N,P,Q], out [N,H,W,C]; handed to the dgrad launch as its epilogue addend. */
int bcos_patch_norm_bwd(const float* x, const float* rnorm, float* out, int N, int H, int W, int C, int x_pitch, int P, int Q,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, void* stream);
/* The same plus a gradient that reaches the same tensor by another path: out = x * PatchSum^T(rnorm) + addend (addend [N,H,W,C] dense,
 * may be NULL) -- the shortcut gradient of a residual block folded into the patch-norm term of the block's first convolution, one
 * elementwise pass less per block and training step.  (ABI v8)
 * Accuracy, every element, with u = 2^-24, T the patch sum and S the same sum over |rnorm|:
 *     |out - exact| <= (kh kw + 2) u (|x| S + |addend|)
 * (at most kh kw - 1 additions in any order, one product, one sum); a pixel that no patch contains gives exactly the addend, or 0.
 * Pad channels C .. x_pitch-1 of x are not read.  tests/test_wgrad_gpu.py: every kernel variant on rectangular geometry. */
int bcos_patch_norm_bwd_add(const float* x, const float* rnorm, const float* addend, float* out, int N, int H, int W, int C, int x_pitch,
                            int P, int Q, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, void* stream);

/* Weight gradient of a convolution / linear layer: gw[co][th][tw][ci] += sum over output pixels (n,i,j) of
 * glin[n,i,j,co] * x[n, i*sh - ph + th*dh, j*sw - pw + tw*dw, ci]   (the autograd convolution_backward weight branch).
 * glin [N,P,Q,g_pitch] (Cout used), x [N,H,W,x_pitch] (C used), gw [Cout][kh][kw][gw_cin] fp32, ZEROED BY THE CALLER
 * (partial sums of pixel chunks are combined with atomics).  Pitches 0 = dense.  Exact fp32 products on
 * v_mfma_f32_32x32x2_f32 in contraction mode f32, the six leading products of exact 3-way bf16 splits otherwise; a linear layer is the
 * 1x1 case with N = 1, H = 1, W = rows.  gw_cin >= C (0 = C): columns C .. gw_cin-1 of gw are not touched.
 * Only channels 0 .. C-1 of x and 0 .. Cout-1 of glin enter the result: the pad channels up to the pitches may hold anything, NaN
 * included (the fused-tap route loads x up to C rounded up to 4, into tile columns whose sums are never stored).
 * Accuracy, every element, for this entry point in either mode and for bcos_conv2d_wgrad_ordered: with u = 2^-24 and
 *     form[co,th,tw,ci] = sum over output pixels (n,i,j) of |glin[n,i,j,co]| * |x[n, i*sh-ph+th*dh, j*sw-pw+tw*dw, ci]|
 * (the L1 form of the column sums below),
 *     |gw - exact| <= K u form,
 * K = max(4 x the worst use of the form by PyTorch's own fp32 weight gradient, 16) per family of inputs of tests/wgrad_cases.py:
 * 20.8 for normal data, 26.4 with images 2^24 apart in magnitude, 259.6 with single pixels 2^12 above the rest (fp32 itself loses the
 * ordinary pixels behind them), and the floor 16 -- twice the 2^-21 |a b| = 8 u that the three dropped products of a split cost -- for
 * operands of ONE sign.  For those, and only on the bf16 matrix pipe (modes bf16x3 / f16x2), the bound grows with the accumulations
 * D behind an element: |gw - exact| <= (16 + D) u form, D = 6 ceil(chunk / 16) + chunks - 1 (six matrix instructions per 16 pixels of
 * a pixel chunk, then the sum over the chunks): the pipe's fp32 accumulation costs 0.2 - 0.5 u of the running sum per instruction
 * (measured: the error of one-signed data is linear in D and depends on nothing else), which cancels on data of mixed sign and does
 * not where every term has the same sign.  Mode f32 needs no such term (1.0 u measured on the same data).
 * An element whose sum is empty (a tap that only ever meets padding) is exactly 0.
 * tests/test_wgrad_gpu.py holds every route of both entry points to this, element by element. */
int bcos_conv2d_wgrad(const float* glin, const float* x, float* gw, int N, int H, int W, int C, int x_pitch, int P, int Q,
                      int Cout, int g_pitch, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int gw_cin,
                      void* stream);

/* The same weight gradient with a FIXED summation order (ABI v9): reproducible bit for bit from call to call.  Both operands of a
 * 16-pixel stage are split into their three bf16 planes once, at staging (pixel-contiguous LDS planes, one ds_read_b128 per fragment),
 * six v_mfma_f32_32x32x16_bf16 per product as in bcos_conv2d_wgrad; every (tile, tap, pixel chunk) workgroup stores its partial tile into
 * slab `chunk` of the workspace `ws`, and a second launch adds the slabs of every element in chunk order.  gw need NOT be zeroed (it is
 * written, not accumulated into); gw_cin must equal C (0 = C) and gw hold a multiple of 4 floats; contraction modes bf16x3 / f16x2 (mode
 * f32: BCOS_E_NOSUP -- use bcos_conv2d_wgrad).  ws: bcos_conv2d_wgrad_ws_floats() floats, 16-byte aligned (0 floats: NULL is fine). */
int bcos_conv2d_wgrad_ws_floats(int N, int H, int W, int C, int x_pitch, int P, int Q, int Cout, int g_pitch, int kh, int kw, int sh,
                                int sw, int ph, int pw, int dh, int dw, int gw_cin, int64_t* floats);
int bcos_conv2d_wgrad_ordered(const float* glin, const float* x, float* gw, float* ws, int N, int H, int W, int C, int x_pitch, int P,
                              int Q, int Cout, int g_pitch, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int gw_cin,
                              void* stream);

/* What bcos_conv2d_wgrad_ordered would launch for a geometry (additive, ABI v12; host only: nothing is launched, no device is needed).
 * The launch reads the same plan, so the two cannot disagree.  out == NULL: BCOS_E_INVAL; otherwise the codes of the launch's geometry
 * validation (BCOS_E_INVAL for sizes and pitches, BCOS_E_NOSUP for a gw that is not dense or no multiple of 4 floats).  The plan depends
 * on BCOS_OPT_WGRAD_WGS. */
typedef struct bcos_wgrad_plan {
    int32_t fused_taps;   /* 1: C < 128 with several taps -- the tile's columns run over (tap, channel) pairs; 0: one tap per workgroup   */
    int32_t direct;       /* 1: 1x1 / stride 1 / unpadded over the whole image: input pixel = output pixel; 0: (n, i, j) counters        */
    int32_t tiles_co;     /* 128-row tiles over Cout                                                                                     */
    int32_t tiles_ci;     /* 128-column tiles over C, or over kh kw (C rounded up to 4) when fused_taps                                  */
    int32_t grid_y;       /* taps per launch dimension: kh kw, or 1 when fused_taps                                                      */
    int32_t split;        /* pixel chunks (= slabs of the workspace when > 1)                                                            */
    int32_t combine;      /* 0: one chunk stored into gw; 1: wgrad_combine_kernel; 2: wgrad_combine_wide_kernel                          */
    int32_t reserved;     /* 0                                                                                                           */
    int64_t chunk;        /* output pixels per chunk (a multiple of 16)                                                                  */
    int64_t last;         /* output pixels of the last chunk (1 .. chunk)                                                                */
    int64_t ws_floats;    /* what bcos_conv2d_wgrad_ws_floats returns                                                                    */
} bcos_wgrad_plan;
int bcos_conv2d_wgrad_plan_query(int N, int H, int W, int C, int x_pitch, int P, int Q, int Cout, int g_pitch, int kh, int kw, int sh,
                                 int sw, int ph, int pw, int dh, int dw, int gw_cin, bcos_wgrad_plan* out);

/* out[c] += sum_r (a[r,c] - shift_a[c]) * (b ? b[r,c] - shift_b[c] : 1), C % 4 == 0, `out` zeroed by the caller: bias
 * gradients (sum of glin) and the batch statistics / parameter gradients of BatchNormUncentered2d in training mode
 * (batchnorm_uncentered.py:36-44: var = x.var((0,2,3), unbiased=False), two passes: mean, then centred squares). */
int bcos_colsum(const float* a, const float* b, const float* shift_a, const float* shift_b, float* out, int64_t rows, int C,
                void* stream);
/* The same sums at full bandwidth AND in a fixed order, given a caller-owned workspace of bcos_colsum_ws_floats(rows, C) floats
 * (16-byte aligned): every workgroup writes its partial sums there, a second launch adds them in workgroup order and WRITES `out`
 * (no zeroing by the caller, no atomics).  The order depends on (rows, C) alone: results are bit-identical from run to run and from
 * process to process.  What the training path (BatchNormUncentered2d batch statistics, bias gradients) and synth.calibrate use.
 * (ABI v7) */
int bcos_colsum_ws_floats(int64_t rows, int C, int64_t* floats);
int bcos_colsum_ws(const float* a, const float* b, const float* shift_a, const float* shift_b, float* out, float* workspace,
                   int64_t workspace_floats, int64_t rows, int C, void* stream);
/* The same sums in a FIXED order (no atomics: one workgroup owns 64 channels over all rows, every thread walks its rows in order,
 * the partial sums meet in a fixed tree) written -- not added -- to `out`: bit-identical from run to run and from process to
 * process, at a fraction of bcos_colsum's bandwidth.  What replicas that must agree bit for bit derive their statistics with
 * (bcos_hip/synth.py: calibrate).  (ABI v7) */
int bcos_colsum_ordered(const float* a, const float* b, const float* shift_a, const float* shift_b, float* out, int64_t rows, int C,
                        void* stream);

/* BatchNormUncentered2d in training mode without separate statistics passes (ABI v8; reference batchnorm_uncentered.py:36-44,
 * trainer step bcos/training/trainer.py:666-784).  Both entry points take a caller-owned workspace of bcos_bn_train_ws_floats(rows, C)
 * floats (16-byte aligned) and sum in one fixed order per (rows, C): bit-identical from run to run.
 *   bcos_bn_batch_stats: ONE pass over y [rows, C]: mean[c], var[c] = the centred variance y.var(unbiased=False) (per-workgroup shifted
 *     sums combined as (n, mean, M2) triples), rstd = 1 / sqrt(var + eps), g = weight * rstd (weight NULL: rstd), and -- running_var not
 *     NULL -- running_var = (1 - momentum) running_var + momentum var in place.
 *   bcos_relu_bwd_colsums: ga = act > 0 ? g : 0 (act NULL: ga = g and nothing is written) together with sgx[c] = sum_r ga y and
 *     (sg not NULL) sg[c] = sum_r ga; with the forward's rstd / gvec = g also gw = sgx rstd (the weight gradient) and
 *     coef = -(gvec sgx) rstd^2 / rows (the coefficient bcos_channel_axpby takes for the variance term of the input gradient). */
int bcos_bn_train_ws_floats(int64_t rows, int C, int64_t* floats);
int bcos_bn_batch_stats(const float* y, const float* weight, float* running_var, float* mean, float* var, float* rstd, float* g,
                        float* workspace, int64_t workspace_floats, int64_t rows, int C, float eps, float momentum, void* stream);
int bcos_relu_bwd_colsums(const float* g, const float* act, const float* y, float* ga, const float* rstd, const float* gvec,
                          float* sgx, float* sg, float* gw, float* coef, float* workspace, int64_t workspace_floats, int64_t rows,
                          int C, void* stream);

/* out[r,c] = a[r,c] * sa[c] + (b[r,c] - mb[c]) * sb[c]   (b / mb / sb may be NULL: out = a * sa): the input gradient of the
 * training-mode uncentered batch norm, gx = gy * w / std + (x - mean) * coef. */
int bcos_channel_axpby(const float* a, const float* sa, const float* b, const float* mb, const float* sb, float* out,
                       int64_t rows, int C, void* stream);

/* -- transformer pieces (bcos_vit.hip; the LayerNorm / GroupNorm entry points: bcos_norms.hip) ---- */

/* Accuracy, per element, of the LayerNorm / GroupNorm / GELU / un-patchify entry points of this section and of their training-mode
 * gradients further down (tests/token_cases.py, tests/test_token_kernels_gpu.py).  Against the same expressions in fp64 from the fp32
 * inputs (eps as the float passed; the gradients from the fp32 rstd they are GIVEN, not from an fp64 recomputation), with u = 2^-24,
 * a LayerNorm row / GroupNorm (image, group) of n values, A = max |x| over it, sd = sqrt(var + eps), xh = x_hat and
 * E(xh, q) = |xh| + q (1 + |xh|) -- `x - mean` is exact only to u A, which is u A / sd in x_hat and a relative u A / sd in sd:
 *     |y - y64|        <= 12.0 u ( |weight| E(xh, A / sd) + |y64| )
 *     |rstd sd - 1|    <=  5.6 u ( 1 + A / sd )
 *     |zsumsq - z64|   <=  6.0 u ( z64 + 2 sum_c |y64| (the bracket of the first line) )
 *     detached gradients, h = gy weight rstd:
 *     |out - out64|    <=  7.6 u ( |h| + mean |h| + |addend| + |out64| ),     out2: that form times |mul2|, plus |out2_64|
 *     full gradients, h = gy weight, rs = rstd, xh = (x - mean) rs, E = E(xh, A rs):
 *     |gx - gx64|      <=  8.4 u ( rs (|h| + mean |h|) + rs (E mean |h xh| + |xh| mean (|h| E)) + |addend| + |gx64| )
 *     |xhat_out - xh|  <= 12.0 u ( E + |xh| )
 * No term takes credit for cancellation: a row whose mean is 1000 x its spread, or a constant row (sd = sqrt(eps)), is held to the
 * A / sd term and no closer -- a constant row of 1000s may come out as 0.02.  x_absmax is bit-equal to max |x| of the row;
 * y_absmax / out2_absmax are bit-equal to the row maximum of the y / out2 the same launch wrote.
 * GELU, with Phi = 0.5 erfc(-x / sqrt 2), phi the normal density, z = |x| / sqrt 2, t = 1 / (1 + 0.3275911 z), the condition number
 * c(t) = sum_k |a_k| t^k / sum_k a_k t^k of the alternating polynomial of Abramowitz-Stegun 7.1.26 (1.7 .. 4.5) and
 * G = (c(t) + 2 z^2) min(Phi, 1 - Phi) + Phi:
 *     |gate - Phi|     <= 0.75e-7 + 7.2 u G           (0.75e-7: half the 1.5e-7 that 7.1.26 states for erf -- an ABSOLUTE error: below
 *                                                      x ~ -5.3 the gate itself is smaller)
 *     |y - x Phi|      <= |x| (that bound) + u |x Phi|
 *     |gx - gx64|      <= |gy| ( 0.75e-7 + 10.0 u ( G + |x| phi (1 + x^2) ) ) + u |gx64|           (bcos_gelu_bwd)
 * bcos_gelu_gate may be called in place (y = x) with the same bits.  bcos_add_rows_bcast is exact (x + pe[i % period] in fp32).
 * bcos_finalize_explanation_patches:  |W - W64| <= 4.4 u |W64|,  |contrib - c64| <= 19.6 u sum_ch |x6 W64|  (x6 = [x, 1 - x] under
 * add_inverse); channels c >= 6 of a gp record are never used (they are loaded on the 16-byte path: Cpad = 8, gp 16-byte aligned).
 * Each constant is 4 x the worst use of its form by a plain fp32 evaluation of the same expression over the test's case tables
 * (LayerNorm widths 1 .. 1000 on both kernel forms and every NV of the statistics kernel, rows that leave wavefront groups partly
 * empty, second passes of every grid-stride loop, misaligned views, offset / constant / outlier rows and rows decades apart; groups
 * of 1 .. 18816 values; GELU over [-14, 14]; rectangular images and patch sizes 1 .. 16).  None of these kernels has atomics:
 * a call repeated gives the same bits, and no output depends on which optional outputs were requested. */

/* LayerNorm over the last dimension D of x [rows, D] (weight / bias may be NULL); rstd_out (NULL or [rows]) keeps
 * 1/sqrt(var+eps) for the backward.  Forward of DetachableLayerNorm (bcos/modules/norms/centered_norms.py:197-224;
 * the value does not depend on explanation mode).  y_absmax (NULL or [rows], ABI v5): the fp32 bit pattern of max_c |y[r,c]|,
 * the operand scale source of the split-f16 contraction that reads y (bcos_operands.a_absmax). */
int bcos_layernorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, uint32_t* y_absmax,
                       int64_t rows, int D, float eps, void* stream);

/* Row statistics of the same LayerNorm WITHOUT writing y: what a contraction needs to read x in place of y (bcos_epilogue.row_scale /
 * a_sumsq).  rstd_out [rows] = 1 / sqrt(var + eps); zsumsq_out (NULL or [rows]) = sum_c (weight[c] (x[r,c] - mean) rstd + bias[c])^2,
 * the squared norm of the LayerNorm output the B-cos scale of the reading layer divides by; x_absmax (NULL or [rows]): bit
 * pattern of max_c |x[r,c]| (the operand maxima of x for the split-f16 contraction).  One read of x, nothing output-sized
 * written.  (ABI v7) */
int bcos_layernorm_stats(const float* x, const float* weight, const float* bias, float* rstd_out, float* zsumsq_out,
                         uint32_t* x_absmax, int64_t rows, int D, float eps, void* stream);

/* Input gradient of DetachableLayerNorm in explanation mode (variance constant, mean differentiable,
 * centered_norms.py:204-215):  g = gy * weight * rstd - mean_D(gy * weight * rstd)  (+ addend);
 * out = g, out2 = g * mul2 (either may be NULL; mul2 NULL -> out2 = g); out2_absmax (NULL or [rows], ABI v5): row maxima of
 * out2 as in bcos_layernorm_fwd. */
int bcos_layernorm_bwd_detached(const float* gy, const float* weight, const float* rstd, const float* addend,
                                const float* mul2, float* out, float* out2, uint32_t* out2_absmax, int64_t rows, int D,
                                void* stream);

/* DetachableGroupNorm2d (bcos/modules/norms/centered_norms.py:93-160; the conv stems of the ViT-C models) on NHWC tensors
 * x [N, HW, C]: group g owns channels [g C/G, (g+1) C/G) of every pixel; per (image, group): biased variance, eps inside the
 * square root, then the per-channel affine (weight / bias may be NULL).  rstd_out (NULL or [N*G]): 1 / std per (image, group)
 * for the gradient. */
int bcos_groupnorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out,
                       int N, int HW, int C, int G, float eps, void* stream);
/* ... its explanation-mode input gradient (variance detached, mean not: centered_norms.py:118-124):
 * gx = h - mean_group(h), h = gy * weight / std. */
int bcos_groupnorm_bwd_detached(const float* gy, const float* weight, const float* rstd, float* gx,
                                int N, int HW, int C, int G, void* stream);

/* MyGELU (bcosify_vit.py:27-32): y = gate * x with gate = 0.5 (1 + erf(x / sqrt 2)); gate_out may be NULL. */
int bcos_gelu_gate(const float* x, float* y, float* gate_out, int64_t n, void* stream);

/* x[i] += pe[i % period]: sin-cos positional embedding added to the tokens (bcos/models/vit.py:324-326). */
int bcos_add_rows_bcast(float* x, const float* pe, int64_t total, int64_t period, void* stream);

/* softmax(q k^T * scale) v per (batch, head), head dim 64.  qkv [B, T, 3*H*64] ordered (q | k | v) x (h d) like
 * vit.py:145-146; out [B, T, H*64]; stats (NULL or [B, H, T, 2]) = (row max, 1 / row sum) for the backward.
 * out_absmax (NULL or [B*T], ZERO-FILLED by the caller, ABI v5): row maxima of out (one atomic max per head and row).
 * T <= 288 (the operands of a head stay in LDS), otherwise BCOS_E_NOSUP.
 *
 * Two kernel families compute this and bcos_attention_bwd_v: the default on the f16 matrix pipe (attention_h2_kernel: scaled two-way
 * fp16 splits, base-2 online softmax) and, with BCOS_OPT_ATTENTION_F32 = 1, the fp32 matrix pipe (attention_mfma_kernel).  The option
 * alone selects the fp32 kernels; the contraction mode has no part in it.  `stats` means the same thing for both -- the NATURAL-log
 * row maximum of scale q k^T and the reciprocal of sum_k exp(s - max) -- so statistics of one family may feed the backward of the other.
 *
 * Accuracy, per element, both families (tests/attention_cases.py, tests/test_attention_gpu.py).  Against the same expressions in fp64
 * from the fp32 inputs (s = scale q k^T, m = rowmax s, l = sum_k exp(s - m), p = exp(s - m) / l, out = p v, gv = p^T gout), with
 * u = 2^-24 and delta[q] = scale ||q||_2 max_k ||k||_2, the Cauchy-Schwarz size of a score of row q:
 *     |out - out64|[q, d]     <=  7.2 u ( (2 delta[q] + 4) (p64 |v|)[q, d] + max_k |v[k, d]| )
 *     |gv - gv64|[k, d]       <=  8.0 u ( sum_q p64[q, k] (2 delta[q] + 4) |gout[q, d]| + max(1, sum_q p64[q, k]) max_q |gout[q, d]| )
 *     |stats[.., 0] - m64|    <= 22.8 u ( delta + |m64| )
 *     |stats[.., 1] l64 - 1|  <= 14.8 u ( 2 delta + 4 )
 * (gv from the statistics of the same family's forward).  2 delta is a score error carried through the softmax, + 4 the exponential
 * and the normalisation; the column-maximum term is the per-feature power of two of the value operand on the f16 pipe: an element
 * of v / gout is resolved relative to its column's maximum, not to itself.  Each constant is 4 x the worst use of its form by a
 * plain fp32 evaluation of the same expression over the test's case table (token counts 1 .. 288, token and feature magnitudes
 * spread over 3 / 8 decades, outliers, score maxima far beyond exp's fp32 range, all-negative scores next to zero padding). */
int bcos_attention_fwd(const float* qkv, float* out, float* stats, uint32_t* out_absmax, int B, int T, int H, int Dh, float scale,
                       void* stream);

/* Gradient w.r.t. v with q, k detached (vit.py:148-151, bcosattnpool.py:37-39): gv = attn^T gout, attn recomputed from
 * qkv and stats. gout, gv: [B, T, H*64]; gv_absmax as out_absmax of bcos_attention_fwd. */
int bcos_attention_bwd_v(const float* qkv, const float* stats, const float* gout, float* gv, uint32_t* gv_absmax, int B, int T,
                         int H, int Dh, float scale, void* stream);

/* -- training-mode backward of the token path (nothing detached; SURVEY.md section 8(f) N4 for the ViT family) ---------- */
/* (Accuracy, per element, of bcos_layernorm_bwd / _bwd_add, bcos_groupnorm_bwd and bcos_gelu_bwd: the `full gradients`, `xhat_out` and
 * `gx` lines of the paragraph at the head of the transformer section.) */
/* LayerNorm over the last dimension (centered_norms.py:187-245 outside explanation mode = F.layer_norm's gradient):
 * gx = rstd (h - mean(h) - x_hat mean(h x_hat)), h = gy * weight, x_hat = (x - mean) rstd; xhat_out (NULL or [rows, D])
 * receives x_hat for the weight gradient sum_rows gy x_hat (bcos_colsum). */
int bcos_layernorm_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xhat_out,
                       int64_t rows, int D, void* stream);
/* The same plus the gradient that reaches the LayerNorm's input by the residual connection around it: gx = (above) + addend
 * (addend [rows, D], may be NULL) -- one elementwise pass less per LayerNorm and training step.  (ABI v8) */
int bcos_layernorm_bwd_add(const float* gy, const float* x, const float* weight, const float* rstd, const float* addend, float* gx,
                           float* xhat_out, int64_t rows, int D, void* stream);
/* DetachableGroupNorm2d outside explanation mode (= F.group_norm's gradient, centered_norms.py:109-113): per (image, group)
 * gx = rstd (h - mean(h) - x_hat mean(h x_hat)), h = gy * weight; xhat_out (NULL or like x) for the affine gradients. */
int bcos_groupnorm_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xhat_out,
                       int N, int HW, int C, int G, void* stream);
/* MyGELU with the gate differentiated (bcosify_vit.py:27-32 with detach off): gx = gy (Phi(x) + x phi(x)). */
int bcos_gelu_bwd(const float* gy, const float* x, float* gx, int64_t n, void* stream);
/* Softmax attention with q, k, v all differentiated (vit.py:143-158 outside explanation mode): gqkv [B, T, 3*H*64] from qkv,
 * the forward's stats and output, and gout [B, T, H*64].  T <= 256.  Up to 207 tokens (16-byte aligned tensors) the five T x T x 64
 * products of a head run on the fp32 matrix pipe, one workgroup per (image, head), fixed summation order (round 5); longer sequences
 * on scalar FMA chains. */
int bcos_attention_bwd(const float* qkv, const float* stats, const float* out, const float* gout, float* gqkv,
                       int B, int T, int H, int Dh, float scale, void* stream);

/* End of the ViT explanation pass: gp [N, H/p, W/p, p, p, Cpad] (input gradient of the patch embedding, one row per
 * patch in the "(p1 p2 c)" order of vit.py:291) -> W(x) [N,6,H,W] (/ std) and contribution map [N,H,W].  Either output may be
 * NULL, H and W need not be equal; accuracy per element: the paragraph at the head of the transformer section. */
int bcos_finalize_explanation_patches(const float* gp, const float* x, const float* std6, float* weights_out,
                                      float* contrib_out, int N, int Cx, int H, int W, int patch, int Cpad,
                                      int add_inverse, void* stream);

/* Batched RGBA rendering of explanations on the device: gradient_to_image (bcos/common.py:387-436; duplicate in
 * interpretability/analyses/text_localisation.py:106-119) for N images at once.
 *   x [N,Cx,H,W] network input (Cx = 3 with add_inverse, else 6), weights [N,6,H,W] = W(x)  ->  rgba [N,H,W,4]:
 *   rgb = pair-normalised positive weight direction, alpha = ||W||_2 (1e-12 where the contribution is negative),
 *   box-smoothed (smooth x smooth, zero padded, count_include_pad; smooth odd, 0/1 = off) and divided by its
 *   q-quantile per image (torch.quantile linear interpolation: exact order statistics by radix select), clipped to [0,1].
 * scratch: 2*N*H*W floats; quantiles: NULL or [N] (the per-image divisor). */
int bcos_render_explanations(const float* x, const float* weights, float* rgba, float* scratch, float* quantiles,
                             int N, int Cx, int H, int W, int smooth, float q, int add_inverse, void* stream);

/* -- localisation (grid pointing game) harness, SURVEY.md section 8(f) N2 ----------------------------------------- */
/* out = avg_pool2d(in, k, stride 1, padding (k-1)/2) of N maps [N,H,W] (zero padded, divisor k*k; k odd): the
 * attribution smoothing of interpretability/analyses/localisation.py:313-317.  in != out. */
int bcos_box_filter(const float* in, float* out, int N, int H, int W, int k, void* stream);

/* Per-cell share of the positive attribution (localisation.py:319-321,387-401): attr [T,H,W] -> frac [T, cells]:
 * a = clamp(neg ? -attr : attr, 0); cell means over the (H/cell_h) x (W/cell_w) grid; mean / sum of means where that is
 * positive, else 0; cell order as the reference's permute(0,1,3,2).reshape: index = col * rows + row. */
int bcos_localisation_fractions(const float* attr, float* frac, int T, int H, int W, int cell_h, int cell_w, int neg,
                                void* stream);

/* -- training recipe: adaptive gradient clipping (ABI v10) ------------------------------------------------------------- */
/* One (parameter, gradient) pair of bcos_agc_clip: `units` contiguous units of `unit_len` floats each, p and g laid out alike. */
typedef struct bcos_agc_tensor {
    const float* p;
    float* g;
    int64_t units;
    int64_t unit_len;
} bcos_agc_tensor;

/* adaptive_clip_grad_ (bcos/training/agc.py:28-42, norm_type 2) of a whole parameter list, gradients rewritten in place.  Per unit u,
 * in fp32: pn = ||p_u||_2, gn = ||g_u||_2, max_norm = clamp(pn, min=eps) * clip_factor; unless gn < max_norm,
 * g_u <- g_u * (max_norm / clamp(gn, min=1e-6)) -- torch's clamp, which keeps a NaN, so a NaN norm clips the unit to NaN as the
 * reference's torch.where does; units that do not clip are not written.  The caller chooses the units (unitwise_norm, agc.py:12-25):
 * one unit for a tensor whose squeeze() has at most one dimension, one per output filter of an OIHW tensor, one per row of a matrix.
 * `tensors` is a HOST array read during the call: the descriptors travel by value in the kernel arguments, 64 tensors per launch, so
 * nothing is copied to the device, allocated or synchronised.  Fixed summation order, no atomics: two calls on the same data give the
 * same bits.  BCOS_E_INVAL (before anything is launched) for a NULL array or pointer, ntensors <= 0, units or unit_len <= 0, an
 * overflowing units * unit_len, or a clip_factor / eps that is not finite and positive. */
int bcos_agc_clip(const bcos_agc_tensor* tensors, int ntensors, float clip_factor, float eps, void* stream);

/* -- Occlusion baseline explainer (ABI v12) ------------------------------------------------------------------------------- */
/* An occlusion mask is a rectangle: four int32 (r0, r1, c0, c1), rows [r0, r1) x columns [c0, c1) with the half-open slice semantics of
 * interpretability/explanation_methods/explainers/occlusion.py:46-49, already clipped to the image.  A mask bank is a DEVICE array
 * [n, 4], 16-byte aligned. */

/* The prepared network input of n occluded copies of ONE image: what bcos_prep_input writes for `img * masks[i]` (occlusion.py:80, then
 * the 6-channel Normalize of bcosify.py:38-43), bit for bit, without the [n, 6, H, W] masked batch ever being stored.
 * x: [1,6,H,W] NCHW; rects: device [n,4] (the caller offsets the pointer into a larger bank); out: [n,H,W,Cpad], channels >= 6 zero;
 * inside rectangle i every channel of copy i is (0 - mean) / std: the mask multiplies the network input BEFORE Normalize.
 * absmax_out (NULL or [n*H*W]): per-pixel max |out| bit patterns, as bcos_prep_input.  One thread per output pixel, 16-byte stores for
 * Cpad == 8; the source image is re-read per copy (L2).  64-bit offsets.
 * BCOS_E_INVAL: a NULL pointer, n / H / W <= 0, Cpad < 6, Cx != 6 or add_inverse != 0 (masking before AddInverse is another operator),
 * H * W > 2^31 - 1, misaligned rects. */
int bcos_prep_input_occluded(const float* x, const int32_t* rects, float* out, const float* mean6, const float* std6,
                             uint32_t* absmax_out, int n, int Cx, int H, int W, int Cpad, int add_inverse, void* stream);

/* The attribution maps of occlusion.py:93-108 from logits that stayed on the device, without the [n_masks, classes, H, W] intermediate:
 *   out[t, h, w] = sum over m in ascending order of  [(h, w) in rect_m] * d(m, t) / n_part_m,
 *   d(m, t) = org[c_t] - pert[m, c_t] (clamped at 0 from below when only_positive; a NaN stays NaN), n_part_m = (r1 - r0) * (c1 - c0),
 *   c_t = targets[t] (device int32 [T]) or t when targets is NULL (then T must equal CL).
 * org [CL], pert [n, CL], rects device [n, 4], out [T, H, W]; pixels no mask covers get 0.  Everything is fp32: one subtraction, one
 * correctly rounded division and one addition per covering mask, the additions as ONE chain in ascending m for every element -- no
 * atomics; the bits do not depend on T, on the launch shape or on how pert was produced.  A target outside [0, CL) yields NaN for its
 * map (never an out-of-bounds read).  rects_host (NULL or a HOST copy of the bank) is what the call validates, since it never reads
 * device memory: BCOS_E_INVAL for a rectangle with an empty side (the reference divides 0 by 0 there) or one that leaves the image;
 * with NULL the caller vouches for the bank (an empty rectangle then contributes nothing).
 * BCOS_E_INVAL also: a NULL org / pert / rects / out, n / CL / T / H / W <= 0, targets == NULL with T != CL, misaligned rects. */
int bcos_occlusion_accumulate(const float* org, const float* pert, const int32_t* rects, const int32_t* rects_host,
                              const int32_t* targets, float* out, int n, int CL, int T, int H, int W, int only_positive, void* stream);

/* -- RISE baseline explainer (additive entry points of ABI v12) -------------------------------------------------------------- */
/* A RISE mask (interpretability/explanation_methods/explainers/rise.py:34-57 of the reference) is an s x s random 0/1 grid, upsampled
 * bilinearly to (s + 1) * cell pixels per side and cropped at a random shift.  It is fully described by four int32, so a mask bank is a
 * DEVICE array [n, 4], 16-byte aligned, of rows (bits_lo, bits_hi, shift_r, shift_c), and the mask VALUES are computed where they are
 * used.  THE MASK, stated here once (one __device__ function, csrc/bcos_rise_mask.h, serves the three kernels):
 *   grid     cell g[a, b] in {0, 1} (a: row) is bit a * s + b of the 64-bit word bits_hi:bits_lo; 2 <= s <= 8; bits at and above s * s
 *            are zero.
 *   sizes    cell_h = ceil(H / s), cell_w = ceil(W / s); 0 <= shift_r < cell_h, 0 <= shift_c < cell_w; U_h = (s + 1) * cell_h,
 *            U_w = (s + 1) * cell_w; 2 * U < 2^24 on both axes.
 *   axis     for pixel row r: p = r + shift_r, U = U_h (columns alike): num = (2 p + 1) * s - U (an integer); i0 = floor(num / (2 U)) by
 *            integer floor division (it can be -1); f = float(num - i0 * 2 U) / float(2 U), ONE fp32 division of two integers fp32
 *            holds exactly; the indices i0 and i0 + 1 are mirrored without repeating the edge: k -> |k|, then k >= s -> 2 (s - 1) - k.
 *   value    with row indices a0, a1 and weight fr, column indices b0, b1 and weight fc, in plain fp32 without contraction:
 *                top = g[a0,b0] + fc * (g[a0,b1] - g[a0,b0]);  bot = g[a1,b0] + fc * (g[a1,b1] - g[a1,b0]);  m = top + fr * (bot - top)
 *            Four equal corners give exactly 0 or 1.
 * This is `resize(grid, up_size, order=1, mode="reflect", anti_aliasing=False)[x : x + H, y : y + W]` of rise.py:53-55 with x = shift_r,
 * y = shift_c: the sample positions of scipy.ndimage.zoom(grid, U / s, order=1, mode="mirror", grid_mode=True), which current skimage
 * calls for these arguments. */

/* out[i, r, c] = m_{first + i}(r, c) for the bank rows [first, first + n): the dense masks, for tests and for callers without a fused
 * engine -- never on an engine's path.  bank: device [n_bank, 4]; out: [n, H, W].
 * BCOS_E_INVAL: a NULL pointer, s outside 2..8, H / W / n / n_bank <= 0, first < 0 or first + n > n_bank, H * W > 2^31 - 1, 2 U >= 2^24,
 * a misaligned bank. */
int bcos_rise_masks(const int32_t* bank, float* out, int n_bank, int first, int n, int s, int H, int W, void* stream);

/* The prepared network input of copies [first, first + n) of ONE image under the bank's masks: what bcos_prep_input writes for the
 * materialised `x * m_i` (one fp32 product per element, rise.py:79, then the 6-channel Normalize), bit for bit and absmax_out included,
 * without the masks or the [n, 6, H, W] batch ever being stored.  x: [1,6,H,W] NCHW; bank: device [n_bank, 4]; out: [n,H,W,Cpad],
 * channels >= 6 zero; absmax_out (NULL or [n*H*W]): per-pixel max |out| bit patterns, as bcos_prep_input.  One thread per output pixel,
 * 16-byte stores for Cpad == 8; a wavefront reads its copy's bank row through one uniform load (per lane only where a wavefront
 * straddles two copies); the source pixel is re-read per copy (L2).  64-bit offsets.
 * BCOS_E_INVAL: as bcos_rise_masks, and Cpad < 6, Cx != 6 or add_inverse != 0 (masking before AddInverse is another operator). */
int bcos_prep_input_rise(const float* x, const int32_t* bank, float* out, const float* mean6, const float* std6, uint32_t* absmax_out,
                         int n_bank, int first, int n, int s, int Cx, int H, int W, int Cpad, int add_inverse, void* stream);

/* The saliency maps of rise.py:93-95 from class scores that stayed on the device:
 *   out[t, r, c] = (sum_i scores[i, t] * m_i(r, c)) / float(n) / p1          scores [n, T], bank device [n, 4], out [T, H, W]
 * THE ORDER is fixed, all in fp32: the masks are taken in consecutive chunks of 64; a chunk's sum starts at 0 and adds, in ascending i,
 * the separately rounded products scores[i, t] * m_i (no fused multiply-add); the total starts at 0 and adds the chunk sums in ascending
 * chunk order; then two correctly rounded divisions.  No atomics: the bits of a map do not depend on T, on which other targets ride
 * along or on the launch shape.  NO TERM IS SKIPPED: the product is formed for every mask, also where m_i = 0, so a NaN score makes the
 * WHOLE map of its target NaN (0 * NaN), as does an infinite one wherever its mask is 0; other targets are not touched.
 * bank_host (NULL or a HOST copy of the bank) is what the call validates, since the library never reads device memory: BCOS_E_INVAL for
 * a shift outside its cell or grid bits at or above s * s; with NULL the caller vouches for the bank (a shift is then clamped into its
 * cell).  BCOS_E_INVAL also: a NULL scores / bank / out, n / T / H / W <= 0, s outside 2..8, p1 not positive and finite, the size limits
 * of bcos_rise_masks, a misaligned bank.  BCOS_E_NOSUP: ceil(H / s) + ceil(W / s) > 3546 (the per-axis tables live in LDS), H > 65535 * 8
 * or T > 65535 * 8. */
int bcos_rise_accumulate(const float* scores, const int32_t* bank, const int32_t* bank_host, float* out, int n, int T, int s, int H, int W,
                         float p1, void* stream);

/* -- block-boundary gradient fused with conv3's input gradient (additive entry point of ABI v12) ---------------------------- */
/* For an identity-shortcut bottleneck boundary (widths C1 = 64, C4 = 256; M = N * PQ rows) ONE launch computes what two bcos_tapconv_ops
 * launches compute -- the input gradient of the upper block's conv1 with mul / addend / out2 (BCOS_EPI_GATE2_FROM_MUL), then the input
 * gradient of the lower block's conv3 reading that launch's `out` -- without `out` ever reaching memory:
 *     v    = g1 W1^T + addend               [M,64] x [64,256]
 *     out2 = v [* mul2] gated by the low mantissa bit of t3     (mul2: the multiplier of the lower block's shortcut convolution, or NULL)
 *     G    = v * t3                         (kept on chip)
 *     g3   = (G W3^T) * t2                  [M,256] x [256,64];  t2 stored, or rebuilt from the kept activation as BCOS_EPI_MUL_FROM_ACT
 *                                           does when mul_norm is given (t2 then holds the activation; mul_csc / mul_csh NULL = 1 / 0)
 * on the f16x2 contraction, bit for bit what the two launches give: out2, g3, out2_absmax (NULL or [M]), g3_absmax (NULL or [M]) and the
 * per-image range g3_imgmax / g3_imgmin_c (both NULL or both [N], zero-filled by the caller, need g3_absmax; see bcos_epilogue).
 * w1_f16x2 / w3_f16x2: the images bcos_split_weights_f16x2 makes of the transposed conv1 weights [256][64] and of the transposed conv3
 * weights [64][256].  Nothing is allocated and no device memory is read by the host.
 * BCOS_E_INVAL: a NULL required pointer, N / PQ <= 0, one of the image-range arrays without the other or without g3_absmax, mul_csc /
 * mul_csh without mul_norm.  BCOS_E_NOSUP: anything but C1 = 64, C4 = 256, a 1 x 1 / stride-1 geometry (kh = kw = stride = 1), b = 2,
 * contraction BCOS_CONTRACT_F16X2 (or the default while the process-wide mode is f16x2) with both images and g1_absmax, tensors below
 * 2 GiB and 16-byte aligned pointers (4-byte for the maxima arrays and mul_norm). */
typedef struct bcos_boundary_conv3 {
    const float* g1;             /* [M,64]: g_lin of the upper block's conv1 */
    const uint32_t* g1_absmax;   /* [M]: its per-pixel maxima                 */
    const void* w1_f16x2;
    const float* addend;         /* [M,256]: the identity-shortcut gradient   */
    const float* t3;             /* [M,256]: stored multiplier of the lower block's conv3, gate in its low mantissa bit */
    const float* mul2;           /* NULL or [M,256] */
    float* out2;                 /* [M,256] */
    uint32_t* out2_absmax;
    const void* w3_f16x2;
    const float* t2;             /* [M,64] */
    const float* mul_norm;       /* NULL or [M] */
    const float* mul_csc;        /* NULL or [64] */
    const float* mul_csh;        /* NULL or [64] */
    float* g3;                   /* [M,64] */
    uint32_t* g3_absmax;
    uint32_t* g3_imgmax;
    uint32_t* g3_imgmin_c;
    int32_t N, PQ;               /* images, pixels per image */
    int32_t C1, C4;
    int32_t kh, kw, stride;      /* geometry of both convolutions */
    int32_t contraction;         /* BCOS_CONTRACT_* */
    float b;                     /* the B-cos exponent of the layers */
} bcos_boundary_conv3;
int bcos_boundary_conv3_grad(const bcos_boundary_conv3* args, void* stream);

/* -- downsample shortcut fused into conv3's forward launch (additive entry point of ABI v12) --------------------------------- */
/* For the first bottleneck of a stage (a 1 x 1 shortcut convolution beside the 1 x 1 conv3 whose epilogue adds it; M = N * P * Q output
 * pixels) ONE launch computes what two bcos_tapconv_ops forward launches compute -- the shortcut convolution (B-cos scale, channel affine,
 * no ReLU; optionally its multiplier), then conv3 with that launch's `out` as its addend, ReLU and optionally its multiplier -- without the
 * shortcut's output ever reaching memory:
 *     idn = csc_d (lin_d s_d) + csh_d           lin_d = x_sub Wd^T [M,Kd] x [Kd,C4], x_sub = pixels (p stride, q stride) of x [N,H,W,Kd],
 *     td  = s_d csc_d                           s = |lin| / sqrt(sum_k a_k^2 + 1e-6) of the row (BCOS_CONV_EPS, B = 2); td NULL or [M,C4]
 *     y   = csc_3 (lin_3 s_3) + csh_3 + idn     lin_3 = h W3^T [M,K3] x [K3,C4]
 *     out = relu(y);  t3 = s_3 csc_3 where y > 0, else 0 (NULL or [M,C4]); with BCOS_EPI_SCALE_GATE_LSB in `flags` an open gate also sets
 *                                               the low mantissa bit of t3
 * on the f16x2 contraction, bit for bit what the two launches give: out, t3, td and out_absmax (NULL or [M]).  P = ceil(H / stride),
 * Q = ceil(W / stride).  wd_f16x2 / w3_f16x2: the images bcos_split_weights_f16x2 makes of the shortcut weights [C4][Kd] and of the conv3
 * weights [C4][K3]; csc_* / csh_* (NULL = 1 / 0): the folded BatchNorm of the two layers, [C4] each.  Nothing is allocated and no device
 * memory is read by the host.
 * BCOS_E_INVAL: a NULL x / h / out, N / H / W <= 0, td without t3 or t3 without td, flag bits other than BCOS_EPI_SCALE_GATE_LSB.  BCOS_E_NOSUP: anything but
 * (K3, Kd, stride, C4) = (64, 64, 1, 256) or (128, 256, 2, 512), 1 x 1 kernels (kh = kw = 1), b = 2, max_out = 1, groups = 1, no bias, no
 * replayed gate tensor, contraction BCOS_CONTRACT_F16X2 (or the default while the process-wide mode is f16x2) with both images and both
 * operands' maxima, tensors below 2 GiB and 16-byte aligned pointers (4-byte for the maxima arrays). */
typedef struct bcos_shortcut_conv3 {
    const float* x;              /* [N,H,W,Kd]: the block input               */
    const uint32_t* x_absmax;    /* [N*H*W]: its per-pixel maxima             */
    const void* wd_f16x2;
    const float* csc_d;          /* NULL or [C4] */
    const float* csh_d;          /* NULL or [C4] */
    float* td;                   /* NULL or [M,C4] */
    const float* h;              /* [M,K3]: conv2's output                    */
    const uint32_t* h_absmax;    /* [M] */
    const void* w3_f16x2;
    const float* csc_3;          /* NULL or [C4] */
    const float* csh_3;          /* NULL or [C4] */
    float* out;                  /* [M,C4] */
    float* t3;                   /* NULL or [M,C4] */
    uint32_t* out_absmax;        /* NULL or [M] */
    const float* bias_d;         /* must be NULL (BCOS_E_NOSUP) */
    const float* bias_3;         /* must be NULL (BCOS_E_NOSUP) */
    const float* relu_gate;      /* must be NULL (BCOS_E_NOSUP): replayed gates keep the pair of launches */
    int32_t N, H, W;             /* the block input's extent */
    int32_t K3, Kd, C4;
    int32_t kh, kw, stride;      /* kernel of both convolutions, stride of the shortcut */
    int32_t max_out, groups;
    int32_t contraction;         /* BCOS_CONTRACT_* */
    int32_t flags;               /* 0 or BCOS_EPI_SCALE_GATE_LSB */
    float b;                     /* the B-cos exponent of the layers */
} bcos_shortcut_conv3;
int bcos_shortcut_conv3_fwd(const bcos_shortcut_conv3* args, void* stream);

/* -- the 7 x 7 / stride 2 stem convolution straight from the raw image (additive entry point of ABI v12) ---------------------------- */
/* ONE launch computes what bcos_prep_input (Cpad = 8, with its per-pixel maxima) followed by the forward bcos_tapconv_ops launch of a
 * ResNet's stem computes, without the prepared [N,H,W,8] copy of the image ever reaching memory:
 *     xn  = ([x, 1 - x] - mean6) / std6         x [N,Cx,H,W] raw NCHW pixels; Cx = 3 with add_inverse, Cx = 6 without; two zero channels added
 *     lin = conv(xn, W)                         7 x 7, stride 2, padding 3, 64 output channels: M = N * P * Q rows, P = (H - 1) / 2 + 1
 *     y   = csc (lin s) + csh                   s = |lin| / sqrt(sum_k a_k^2 + 1e-6) of the row (BCOS_CONV_EPS, B = 2); relu != 0: max(y, 0)
 *     t   = s csc (where y > 0 if relu, else 0) NULL or [M,64]; with BCOS_EPI_SCALE_GATE_LSB in `flags` an open gate also sets its low bit
 * on the f16x2 contraction, bit for bit what the two launches give: y, t, norm_out (NULL or [M]: the patch norms) and y_absmax (NULL or
 * [M]: per-pixel maxima of y).  w_f16x2: the image bcos_split_weights_f16x2_conv makes of the weights [64][49][8] (taps = 49, C = 8);
 * csc / csh (NULL = 1 / 0): the folded BatchNorm, [64] each.  x_imgmax / x_imgmin (both or neither, [N]): the per-image range of the
 * prepared input's per-pixel maxima in the form bcos_image_absrange leaves (bcos_stem_image_range computes it from the raw image) -- given
 * them, a row of an image whose nonzero pixel maxima lie within 2^16 of the image's maximum takes that maximum as the source of its operand
 * scale, as the tapconv launch does when it is handed bcos_operands.a_imgmax / a_imgmin; without them (or with option BCOS_OPT_PATCH = 0)
 * every row takes the maximum over its own 49 taps, as that launch does without them.  Nothing is allocated and no device memory is read
 * by the host.
 * BCOS_E_INVAL: a NULL x / mean6 / std6 / y, N / H / W <= 0, Cx other than 3 (add_inverse) or 6, one of x_imgmax / x_imgmin without the
 * other, flag bits other than BCOS_EPI_SCALE_GATE_LSB.  BCOS_E_NOSUP: anything but kh = kw = 7, stride 2, padding 3, Cout = 64, b = 2,
 * max_out = 1, groups = 1, no bias, no replayed gate tensor, relu 0 or 1, contraction BCOS_CONTRACT_F16X2 (or the default while the
 * process-wide mode is f16x2) with the weight image, tensors below 2 GiB, at most 65535 images, 16-byte aligned y / t / image and 4-byte
 * aligned arrays. */
typedef struct bcos_stem_conv {
    const float* x;              /* [N,Cx,H,W]: the raw image                 */
    const float* mean6;          /* [6] */
    const float* std6;           /* [6] */
    const void* w_f16x2;
    const float* csc;            /* NULL or [64] */
    const float* csh;            /* NULL or [64] */
    float* y;                    /* [M,64] */
    float* t;                    /* NULL or [M,64] */
    float* norm_out;             /* NULL or [M] */
    uint32_t* y_absmax;          /* NULL or [M] */
    const uint32_t* x_imgmax;    /* NULL or [N] */
    const uint32_t* x_imgmin;    /* NULL or [N] */
    const float* bias;           /* must be NULL (BCOS_E_NOSUP) */
    const float* relu_gate;      /* must be NULL (BCOS_E_NOSUP): replayed gates keep the pair of launches */
    int32_t N, Cx, H, W;         /* the image's extent */
    int32_t add_inverse;
    int32_t Cout, kh, kw, stride, padding;
    int32_t relu;                /* 0 none, 1 ReLU decided by the value */
    int32_t max_out, groups;
    int32_t contraction;         /* BCOS_CONTRACT_* */
    int32_t flags;               /* 0 or BCOS_EPI_SCALE_GATE_LSB */
    float b;                     /* the B-cos exponent of the layer */
} bcos_stem_conv;
int bcos_stem_conv_fwd(const bcos_stem_conv* args, void* stream);
/* out_max[n] / out_min[n]: the largest / the smallest nonzero per-pixel maximum of image n of the prepared input (0xffffffff as minimum
 * where every pixel is zero), computed from the raw image: what bcos_image_absrange gives on the maxima bcos_prep_input emits.
 * BCOS_E_INVAL: a NULL pointer, N / H / W <= 0, Cx other than 3 (add_inverse) or 6, Cx * H * W > 2^31 - 1. */
int bcos_stem_image_range(const float* x, const float* mean6, const float* std6, uint32_t* out_max, uint32_t* out_min, int N, int Cx,
                          int H, int W, int add_inverse, void* stream);

/* -- pixel perturbation (deletion curves; additive entry points of ABI v12) ------------------------------------------------- */
/* An image's HW = H * W pixels are ranked by a score s (fp32, one per pixel p = h * W + w) and the first k of the ranking are REMOVED:
 * all six channels of the [r,g,b,1-r,1-g,1-b] network input are set to 0 there, as inside an Occlusion rectangle.  THE RANKING, stated
 * here once:
 *   m(s)   = bits(s) ^ (bits(s) >> 31 ? 0xFFFFFFFF : 0x80000000)   the usual monotone map of fp32 onto uint32: -0.0 sorts below +0.0,
 *            -inf lowest, +inf above every finite value, and a NaN orders by its bit pattern (sign bit clear: above +inf; set: below
 *            -inf).  The library never reads device memory on the host, so it cannot refuse NaNs: they are ranked like this.
 *   key32  = m(s) for "least important first" (descending == 0), ~m(s) for "most important first" (descending != 0);
 *   key64  = (uint64)key32 << 32 | p: the HW keys of an image are distinct, ties of key32 break by ascending p in EITHER order;
 *   thr(k) = the k-th smallest key64 (0-based) for 0 <= k < HW, UINT64_MAX for k = HW;
 *   copy j of image b removes pixel p iff key64_b(p) < thr_b(k_j): exactly k_j pixels, the first k_j of a stable sort by key32. */
#define BCOS_PERTURB_MAX_COUNTS 64

/* Workspace of bcos_perturb_select in bytes.  BCOS_E_INVAL: bytes NULL, B outside [1, 65535], HW outside [1, 2^31 - 1], K outside [1, 64]. */
int bcos_perturb_select_ws_bytes(int B, int64_t HW, int K, int64_t* bytes);

/* thr_out[b, j] = thr_b(counts[j]) for B images and K removal counts in one call.  scores: device [B, HW]; counts_host: HOST int32 [K],
 * validated here and handed to the kernels by value in their arguments (as bcos_agc_clip hands over its descriptors); thr_out: device
 * uint64 [B, K]; ws: device workspace of at least bcos_perturb_select_ws_bytes, owned by the caller -- the call initialises what it
 * uses of it and never relies on what it held.  Counts may repeat and come in any order.
 * Method: a radix select on key32 -- four 8-bit passes from the top byte, the prefixes of all K targets resolved together from integer
 * histograms (LDS atomics per workgroup, integer global atomics between workgroups) -- then one scan per (image, target) over the pixels
 * in ascending p that takes the r-th pixel whose key32 equals the target's.  Integer counts only: the result is exact, identical from
 * call to call and independent of the launch shape.  Ten launches (five of them read the scores); nothing is allocated and no device
 * memory is read by the host.
 * BCOS_E_INVAL (before anything is launched): a NULL pointer, B / HW / K out of the ranges above, a count outside [0, HW], ws_bytes
 * too small, thr_out or ws not 8-byte aligned. */
int bcos_perturb_select(const float* scores, const int32_t* counts_host, int descending, uint64_t* thr_out, void* ws, int64_t ws_bytes,
                        int B, int64_t HW, int K, void* stream);

/* The prepared network input of copies c in [first, first + n) of the B * K perturbed copies (image-major: c = b * K + j), bit for bit
 * what bcos_prep_input writes for the materialised copy -- image b with the pixels p of key64_b(p) < thr[b, j] set to 0 in all six
 * channels -- without the [B * K, 6, H, W] batch ever being stored.  x: [B,6,H,W] NCHW; scores: [B, HW]; thr: device uint64 [B, K]
 * (bcos_perturb_select with the same `descending`); out: [n,H,W,Cpad], channels >= 6 zero; a removed pixel is (0 - mean) / std in every
 * channel: the removal acts on the network input BEFORE Normalize.  absmax_out (NULL or [n*H*W]): per-pixel max |out| bit patterns, as
 * bcos_prep_input.  One thread per output pixel, 16-byte stores for Cpad == 8; source pixel and score are re-read per copy (L2).
 * 64-bit offsets.
 * BCOS_E_INVAL: a NULL pointer, B / K / H / W <= 0, Cpad < 6, Cx != 6 or add_inverse != 0 (masking before AddInverse is another
 * operator), H * W > 2^31 - 1, first < 0, n <= 0 or first + n > B * K, thr not 8-byte aligned. */
int bcos_prep_input_perturbed(const float* x, const float* scores, const uint64_t* thr, int descending, float* out, const float* mean6,
                              const float* std6, uint32_t* absmax_out, int B, int K, int first, int n, int Cx, int H, int W, int Cpad,
                              int add_inverse, void* stream);

/* out[r] = score of class t = targets[r / group] in row r of logits [R, CL]; targets: device int32 [R / group] (R a multiple of group:
 * the `group` copies of an image share its class).  A target outside [0, CL) yields NaN, never an out-of-bounds read.  With x = the row,
 * u = 2^-24 and expf accurate to 1 ulp (relative error <= 2u; the device library's expf, not an approximate one) and the division
 * correctly rounded (relative error <= u) -- both hold for the build bcos_hip/lib.py makes, which passes neither -ffast-math nor
 * -fno-hip-fp32-correctly-rounded-divide-sqrt; a build with either voids the bounds below:
 *   mode 0  the logit x_t: an exact copy.
 *   mode 1  the sigmoid of BcosMixin.to_probabilities: 1 / (1 + expf(-x_t)) -- one expf, one addition, one correctly rounded division:
 *           |out - sigma(x_t)| <= 6 u sigma(x_t) + 2^-126   (2u + u + u to first order; the absolute term covers an overflowing expf,
 *           where the result is 0 and sigma(x_t) < 2^-126).
 *   mode 2  softmax over the row by one wavefront: M = max_c x_c; lane l adds e_c = expf(x_c - M) for c = l, l + 64, ... in ascending
 *           order as one fp32 chain; the 64 lane sums are combined by the butterfly xor 32, 16, 8, 4, 2, 1; out = expf(x_t - M) / sum.
 *           With p = softmax(x)_t and D = sum_c softmax(x)_c |x_c - M| (the weighted mean distance to the maximum):
 *           |out - p| <= (|x_t - M| + D + ceil(CL / 64) + 12) u p + 2^-126
 *           -- the rounded difference x_c - M perturbs e_c by |x_c - M| u relatively (numerator: |x_t - M| u; sum: D u), each expf adds
 *           2u to either, a lane's chain and the six butterfly levels add at most ceil(CL / 64) + 5 roundings of a sum of non-negative
 *           terms, the division one; 12 = 2 + 2 + 5 + 1 and 2 for the second-order terms.  The absolute term covers e_t underflowing.
 * BCOS_E_INVAL: a NULL pointer, R / CL / group <= 0, R not a multiple of group, mode outside 0..2. */
int bcos_class_scores(const float* logits, const int32_t* targets, int group, int mode, float* out, int64_t R, int CL, void* stream);

/* -- training recipe: the SigLIP distillation objective of the CLIP recipe (additive entry points of ABI v12) ------------------------- */
/* SigLipLoss (bcos/modules/losses.py:576-638: get_ground_truth :606-610, get_logits :612-624, _loss :626-638, the multi-rank sum of
 * forward :640-694) together with the two F.normalize of the training step that calls it (bcos/training/trainer.py:673-674, 699-707),
 * loss and every gradient in one call.
 *   s [L, N, D]  student features: L = 1 the pooled head, L = HW the attn_unpool layout [(HW), N, D];   t [M, D]  teacher features;
 *   scale, bias  one DEVICE float each (the recipe's learnable variant makes them parameters: model.logit_scale.exp(), model.logit_bias);
 *   pos_offset   column pos_offset + i is row i's positive (label y = +1), every other column y = -1; pos_offset < 0: no positives (the
 *                reference's negative_only).  M = W N with pos_offset = rank N is the whole multi-rank loss: the local term plus the
 *                negative_only terms against the other ranks' features, every term divided by N;
 *   p            0: z_ij = scale c_ij + bias (L must be 1);  p >= 1: z_ij = scale mean_l(c_lij |c_lij|^(p-1)) + bias (cos_scaling = p);
 *   flags        BCOS_SIGLIP_NORMALIZE: c is taken between u = x / max(||x||_2, 1e-12) of both operands (IEEE divisions, as F.normalize: a
 *                one-element row is exactly +-1) and the gradients go through the normalisation (a row below the clamp gets g / 1e-12, its norm held constant, as torch's autograd returns);
 *                BCOS_SIGLIP_DETACH_POW: the factor |c|^(p-1) is a constant in the gradient (the reference's self.detach).
 *   loss = -sum_ij logsigmoid(y_ij z_ij) / N, logsigmoid(x) = min(x, 0) - log1p(exp(-|x|));   G_ij = -y_ij sigmoid(-y_ij z_ij) / N;
 *   gbias = sum G;  gscale = sum G_ij q_ij with q the pooled cosine (z - bias) / scale, taken before the scaling, not by that division;
 *   gs [L, N, D], gt [M, D]: through the mean, the power and the normalisation.  gs, gt, gscale, gbias: NULL = not wanted.
 * Order of every sum, a function of (L, N, M, D) alone: a dot product over D as 64 lane chains d = lane, lane + 64, ... (FMA) combined
 * by the butterfly xor 32, 16, 8, 4, 2, 1; a row's sums over M likewise over j; the mean over l ascending; gs over j ascending; gt over
 * (l, i) with l outer; the three scalars over the rows' partial sums as lane chains and the butterfly.  No atomics: two calls on the
 * same data give the same bits.  Three launches; ws (bcos_siglip_loss_ws_floats floats, owned by the caller) is written before it is
 * read, nothing is allocated, copied or synchronised.
 * BCOS_E_INVAL (before anything is launched): NULL s / t / loss / scale / bias, a size <= 0 or L N M, L N D or M D above 2^38,
 * pos_offset + N > M, p outside [0, 64], L > 1 with p = 0, an unknown flag, ws NULL or ws_floats too small. */
#define BCOS_SIGLIP_NORMALIZE 1
#define BCOS_SIGLIP_DETACH_POW 2
int bcos_siglip_loss(const float* s, const float* t, const float* scale, const float* bias, float* loss, float* gs, float* gt,
                     float* gscale, float* gbias, float* ws, int64_t ws_floats, int L, int N, int M, int D, int pos_offset, int p,
                     int flags, void* stream);
/* floats = (L N + M) (D + 1) + 2 L N M + N M + 3 N.  BCOS_E_INVAL: floats NULL or sizes that bcos_siglip_loss refuses. */
int bcos_siglip_loss_ws_floats(int L, int N, int M, int D, int64_t* floats);

/* -- depthwise 7x7 B-cos convolution (csrc/bcos_dwconv.hip) ------------------------------------------------------------
 * The first layer of a ConvNeXt block (bcos/models/convnext.py: BcosConv2d(dim, dim, kernel_size=7, padding=3, groups=dim)): one
 * filter per channel, so there is nothing for the matrix pipe to contract -- a vector kernel, lanes along channels.
 *   x [N,H,W,C] NHWC fp32,  w [7,7,C] tap-major, channel-contiguous: the EFFECTIVE (already unit-normed) filter bank,
 *   stride 1, zero padding 3, dilation 1, C % 4 == 0.
 * Per output element (p, c), over the taps t = (r, s) in row-major ascending order, r outer (taps outside the image read x = 0, which
 * leaves both chains' bits as they were):
 *   lin = fma(w[t,c], x[p+t-3,c], lin)      ss = fma(x[p+t-3,c], x[p+t-3,c], ss)        (both start at 0)
 *   norm = sqrt(ss + 1e-6): with groups = C every channel has its own patch norm (bcosconv2d.py:196-231)
 *   scale = |lin| / norm (B = 2),  (|lin / norm| + 1e-6)^(B-1) otherwise;   y = scale * lin;   B = 1: y = lin
 * IEEE division and square root.  scale_out / norm_out ([N,H,W,C] each) may be NULL; with B = 1 scale_out must be NULL.
 * bcos_dwconv7_bwd is the explanation-mode input gradient (the scale is a constant):
 *   gx[p,c] = addend[p,c] + sum_t w[t,c] (mul gy)[p-t+3,c]
 * one FMA chain from 0 over the SOURCE pixels p-t+3 in row-major ascending order (t descending), then one addition of addend; mul
 * (the kept forward scale) and addend (the residual stream's gradient) may be NULL.  gx may alias addend, not gy or mul.
 * One thread owns an output element: no atomics, and the bits depend neither on N, nor on the image's position in the batch, nor on
 * the launch shape.  BCOS_E_INVAL, before any HIP call: a NULL x / w / y (gy / w / gx), a size <= 0, C % 4 != 0, a pointer that
 * is not 16-byte aligned, scale_out with B = 1, or more than 2^31 - 1 workgroups. */
int bcos_dwconv7_fwd(const float* x, const float* w, float* y, float* scale_out, float* norm_out, int N, int H, int W, int C, float b,
                     void* stream);
int bcos_dwconv7_bwd(const float* gy, const float* w, const float* mul, const float* addend, float* gx, int N, int H, int W, int C,
                     void* stream);

/* -- training-mode gradients of the depthwise 7x7 B-cos convolution (csrc/bcos_dwconv_train.hip) ---------------------------
 * The backward pass of bcos_dwconv7_fwd with the B-cos scale DIFFERENTIATED: what autograd derives from the reference's
 * bcos/modules/bcosconv2d.py:176-194 (the `self.b == 2` branch :186-187 with `self.detach` off, the patch norm of :196-231) on a layer
 * with groups = C.  B = 2 and B = 1 only; x, y, scale, norm are the forward's input and outputs, g = gy = dL/dy, all [N,H,W,C] fp32,
 * w [7,7,C] the effective filter bank as in bcos_dwconv7_fwd.
 *   glin = 2 (scale g)                    one rounded product, the doubling is exact     (dy/dlin = 2 |lin| / norm)
 *   r    = -(g y) / (norm norm)           two rounded products, one IEEE division        (dy/dnorm = -y / norm, dnorm/dx_q = x_q / norm)
 *   acc(q) = sum_t w_t glin(q - t + 3)    one FMA chain from 0 over the SOURCE pixels q - t + 3 in row-major ascending order
 *   box(q) = sum_t r(q - t + 3)           one chain of additions from 0 in the same order (pixels outside the image add an exact zero)
 *   gx(q)  = fma(x(q), box(q), acc(q)),   then one addition of addend(q) where addend != NULL
 *   B = 1:  glin = g, gx = acc [+ addend]; x, y, scale, norm are not read and may be NULL.
 * One launch; glin and r exist only in LDS.  One thread owns an output element: no atomics, the bits depend neither on N nor on the
 * image's position in the batch.  gx may alias addend, nothing else.
 * BCOS_E_INVAL, before any HIP call: B other than 1 or 2, a NULL gy / w / gx (B = 2: x / y / scale / norm too), a size <= 0,
 * C % 4 != 0, a pointer (the optional ones included) that is not 16-byte aligned, more than 2^31 - 1 workgroups. */
int bcos_dwconv7_train_bwd(const float* gy, const float* x, const float* y, const float* scale, const float* norm, const float* w,
                           const float* addend, float* gx, int N, int H, int W, int C, float b, void* stream);
/* Gradient of the EFFECTIVE (unit-norm) filter bank, gw [7,7,C] tap-major like w (the projection's own gradient stays
 * bcos_weight_rownorm_bwd's; the reference gets both from autograd of F.conv2d in bcosconv2d.py:172):
 *   glin = gain (mul gy) where mul != NULL (rounded as bcos_dwconv7_train_bwd rounds it), gain gy otherwise
 *   gw(t, c) = sum_{n,p} glin_c(n, p) x_c(n, p + t - 3)                                   (x = 0 outside the image)
 * Training passes mul = scale, gain = 2; mul = NULL, gain = 1 is the gradient with the scale held constant.
 * Order of every sum, a function of (N, H, W, C) alone.  The images are cut into tiles of 6 x 8 pixels; the P = N ceil(H / 6) ceil(W / 8)
 * (image, tile) pairs, image-major, tile rows before tile columns, are dealt in runs of L = ceil(P / 256) to G = ceil(P / L) workgroups
 * per slice of 64 channels.  A workgroup keeps, per (tap, channel), two partial sums: part 0 over tile rows 0-2, part 1 over tile rows
 * 3-5 of its pairs, each ONE FMA chain from 0 over pairs ascending, rows ascending, columns ascending (a pixel beyond the image adds an
 * exact zero).  Partial (2 g + part) of workgroup g goes to ws [2 G][49][C]; a second launch adds the 2 G partials in ascending index,
 * starting from partial 0.  No atomics: two calls on the same data give the same bits, whatever ws held before.
 * BCOS_E_INVAL, before any HIP call: a NULL gy / x / gw / ws, a size <= 0, C % 4 != 0, a pointer (mul included) that is not 16-byte
 * aligned, a gain that is not finite, ws_bytes < bcos_dwconv7_wgrad_workspace(N, H, W, C). */
int bcos_dwconv7_wgrad(const float* gy, const float* mul, float gain, const float* x, float* gw, void* ws, int64_t ws_bytes, int N, int H,
                       int W, int C, void* stream);
/* bytes = 4 * 49 * C * 2 * G with G as above (at most 100352 C).  Host only, no device needed.  BCOS_E_INVAL (negative): a size <= 0,
 * C % 4 != 0, or more than 2^31 - 1 bytes (C > 21396 at G = 256), which bcos_dwconv7_wgrad refuses as well. */
int bcos_dwconv7_wgrad_workspace(int N, int H, int W, int C);

/* -- uncentered position / group norms (csrc/bcos_norms.hip; additive, ABI v12) ---------------------------------------------
 * The norms of the B-cos v2 norm ablations whose variance is centred while the value that is divided is NOT: over a set S of n values
 * (a row of x [rows, D] = the channels of a pixel of the NHWC image; an (image, group) of x [N, HW, C])
 *     m = mean_S x,   var = mean_S (x - m)^2,   r = 1 / sqrt(var + eps),   y = weight x r + bias        (weight / bias may be NULL)
 *     explanation mode (var a constant):   gx = h r,   h = gy weight                      -- no mean is subtracted
 *     training mode:                       gx = r h - r^3 (x - m) (sum_S h x) / n
 *     weight / bias gradients:             sum gy (x r),  sum gy                          (column reductions: bcos_colsum)
 * Two-pass variance (the mean, then the centred squares); every reduction in one fixed order, no atomics, no workspace: a call repeated
 * gives the same bits, and no output depends on which optional outputs were requested.
 *
 * Accuracy, per element (tests/unorm_cases.py, tests/test_unorm_gpu.py).  Against the same expressions in fp64 from the fp32 inputs
 * (eps as the float passed; the gradients from the fp32 rstd they are GIVEN, not from an fp64 recomputation), with u = 2^-24,
 * A = max_S |x|, sd = sqrt(var + eps), q = A / sd -- `x - m` is exact only to u A, which is a relative u A / sd in sd -- and d = x - m:
 *     |y - y64|        <=  4.4 u ( |weight| |x / sd| (1 + q) + |y64| )
 *     |rstd sd - 1|    <=  4.4 u ( 1 + q )
 *     detached gradients, h = gy weight:
 *     |out - out64|    <=  5.2 u ( |h rstd| + |addend| + |out64| ),     out2: that form times |mul2|, plus |out2_64|
 *     full gradients, rs = rstd:
 *     |gx - gx64|      <= 10.0 u ( rs |h| + rs^3 (|d| + A) mean_S |h x| + |addend| + |gx64| )
 *     |xr_out - x rs|  <=  4.4 u |x rs|
 * No term takes credit for cancellation: a row whose mean is 1000 x its spread, or a constant row (sd = sqrt(eps)), is held to the q term
 * and no closer.  Each constant is 4 x the worst use of its form by a plain fp32 evaluation of the same expression (measured: y 1.015,
 * rstd 1.046, detached 1.222, full 2.391, xr 0.999 u, each rounded up to the next tenth that leaves 2 %) over the test's case
 * table (row widths 1 .. 1000 on both kernel forms, rows that leave wavefront groups partly empty, second passes of the grid-stride
 * loops, misaligned views, offset / constant / outlier rows and rows decades apart; groups of 1 .. 18816 values, G = 1 .. C).
 * BCOS_E_INVAL, before any HIP call: a NULL required pointer, a size <= 0; for the group form also C % G != 0. */

/* Row form, one wavefront per row; 16-byte accesses where D % 4 == 0, D <= 256 and every tensor is 16-byte aligned, a strided loop
 * otherwise.  Forward of PositionNormUncentered2d (bcos/modules/norms/uncentered_norms/posnorm_uncentered.py:39-58; the value does not
 * depend on explanation mode); rstd_out (NULL or [rows]) keeps r for the backward. */
int bcos_layernorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int64_t rows, int D,
                           float eps, void* stream);
/* ... its explanation-mode input gradient (posnorm_uncentered.py:45-50 with `detach`): out = gy weight rstd (+ addend),
 * out2 = out * mul2 (either output may be NULL, not both; mul2 NULL -> out2 = out): the contract of bcos_layernorm_bwd_detached
 * without the row maxima. */
int bcos_layernorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, const float* addend, const float* mul2,
                                    float* out, float* out2, int64_t rows, int D, void* stream);
/* ... its training-mode input gradient (autograd of posnorm_uncentered.py:45-58 with `detach` off):
 * gx = rs h - rs^3 (x - m) (sum h x) / D (+ addend); the mean is recomputed from the row; xr_out (NULL or [rows, D]) receives x rs for
 * the weight gradient sum_rows gy (x rs) (bcos_colsum). */
int bcos_layernorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, const float* addend, float* gx,
                           float* xr_out, int64_t rows, int D, void* stream);

/* Group form on NHWC tensors x [N, HW, C], one workgroup per (image, group): group g owns channels [g C/G, (g+1) C/G) of every pixel.
 * Forward of group_norm_uncentered / GroupNormUncentered2d (bcos/modules/norms/uncentered_norms/groupnorm_uncentered.py:21-61; G = C:
 * GNInstanceNormUncentered2d :82-89, G = 1: GNLayerNormUncentered2d :92-99); rstd_out (NULL or [N*G]).  Arguments as bcos_groupnorm_fwd. */
int bcos_groupnorm_unc_fwd(const float* x, const float* weight, const float* bias, float* y, float* rstd_out, int N, int HW, int C, int G,
                           float eps, void* stream);
/* ... explanation mode (groupnorm_uncentered.py:43-49 with `detach`): gx = gy weight rstd.  Arguments as bcos_groupnorm_bwd_detached. */
int bcos_groupnorm_unc_bwd_detached(const float* gy, const float* weight, const float* rstd, float* gx, int N, int HW, int C, int G,
                                    void* stream);
/* ... training mode (autograd of groupnorm_uncentered.py:43-61 with `detach` off): per (image, group) of n = HW C / G values
 * gx = rs h - rs^3 (x - m) (sum h x) / n; xr_out (NULL or like x) = x rs for the weight gradient.  Arguments as bcos_groupnorm_bwd, with
 * xr_out in place of xhat_out. */
int bcos_groupnorm_unc_bwd(const float* gy, const float* x, const float* weight, const float* rstd, float* gx, float* xr_out, int N,
                           int HW, int C, int G, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BCOS_HIP_H */
