// bcos_tapconv_dispatch.hip -- the host side of bcos_tapconv_ops: no kernel lives here.
//
// The dispatch runs in stages: validate -> (batch chunks: images_per_launch, chunk_of) -> resolve (select_operands,
// select_epilogue_kind) -> choose_route -> launch_route.  The two queries (bcos_tapconv_fuses_image_range, bcos_tapconv_route_query)
// run the same stages and stop ahead of the launch.  A route is a tile launcher of bcos_tapconv.hip, reached through the table
// ROUTES (one row per entry of BCOS_TC_ROUTES, bcos_tapconv_plan.h), or the narrow-output kernel of bcos_skinny.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "bcos_hip.h"
#include "bcos_internal.h"
#include "bcos_tapconv_plan.h"

namespace {

// process-wide DEFAULT for calls that do not choose (bcos_operands.contraction == 0): 0 = v_mfma_f32_32x32x2_f32,
// 1 = 6 x v_mfma_f32_32x32x16_bf16 on exact 3-way splits, 2 (default) = 3 x v_mfma_f32_32x32x16_f16 on scaled 2-way splits
// where the call provides what that needs (a_absmax + wt_f16x2), else 1
std::atomic<int> g_contraction_mode{2};

}  // namespace

extern "C" int bcos_set_contraction_mode(int mode) {
    if (mode < 0 || mode > 2)
        return bcos_set_error(BCOS_E_INVAL, "bcos_set_contraction_mode: 0 = fp32 MFMA, 1 = split-bf16 MFMA, 2 = split-f16 MFMA");
    g_contraction_mode = mode;
    return BCOS_OK;
}

extern "C" int bcos_get_contraction_mode(void) { return g_contraction_mode; }

extern "C" int bcos_tapconv(const float* a, const float* wt, const bcos_tapconv_geom* geom,
                            const bcos_epilogue* epi, void* stream) {
    bcos_operands o = {a, nullptr, wt, nullptr, nullptr, BCOS_CONTRACT_DEFAULT, nullptr, nullptr};
    return bcos_tapconv_ops(&o, geom, epi, stream);
}

extern "C" int bcos_tapconv_presplit(const float* a, const float* wt, const void* wt3, const bcos_tapconv_geom* geom,
                                     const bcos_epilogue* epi, void* stream) {
    bcos_operands o = {a, nullptr, wt, wt3, nullptr, BCOS_CONTRACT_DEFAULT, nullptr, nullptr};
    return bcos_tapconv_ops(&o, geom, epi, stream);
}

// ---- the stages --------------------------------------------------------------------------------------------------------------------------
namespace {
struct RouteEntry { const char* name; int fam, bm, bn; int (*launch)(const void*, int, hipStream_t); };
#define BCOS_TC_X_ROW(name, fam, bm, bn) {#name, fam, bm, bn, bcos_tc_##name},
const RouteEntry ROUTES[ROUTE_COUNT] = {BCOS_TC_ROUTES(BCOS_TC_X_ROW) {"skinny", -1, 0, 0, nullptr}};
struct Route { int id, ch_pass; };      // ROUTE_*; ch_pass: input channels per pass of ROUTE_skinny, 0 otherwise
struct Call { bcos_operands ops; bcos_tapconv_geom g; bcos_epilogue e; };

inline int contraction_mode(const bcos_operands& o) { return o.contraction == BCOS_CONTRACT_DEFAULT ? g_contraction_mode.load(std::memory_order_relaxed) : o.contraction - 1; }

// stage 1: the argument checks.  *gn receives the geometry with its default pitches filled in.
int validate(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi, bcos_tapconv_geom* gn) {
    if (!ops || !geom || !epi) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: NULL argument");
    if (!ops->a || !ops->wt) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: NULL operand");
    if (ops->contraction < 0 || ops->contraction > BCOS_CONTRACT_F16X2)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: bad contraction selector");
    const bcos_tapconv_geom& g = *geom;
    if (g.N <= 0 || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.P <= 0 || g.Q <= 0 || g.TH <= 0 || g.TW <= 0 ||
        g.Cout <= 0 || g.OH <= 0 || g.OW <= 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: non-positive dimension");
    if (g.C % 4 != 0) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: C must be a multiple of 4");
    if ((reinterpret_cast<uintptr_t>(ops->a) | reinterpret_cast<uintptr_t>(ops->wt)) & 15)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: operands must be 16-byte aligned");
    if ((int64_t)g.N * g.P * g.Q >= (int64_t)1 << 31) return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: more than 2^31 rows");
    if (!epi->out && !epi->out2 && !epi->scale_out) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: no output buffer");
    if (epi->max_out < 0) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: negative max_out");
    if ((epi->flags & BCOS_EPI_MUL_FROM_ACT) && (!epi->mul || !epi->mul_norm || (epi->flags & BCOS_EPI_GATE2_FROM_MUL)))
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: BCOS_EPI_MUL_FROM_ACT needs mul and mul_norm and excludes GATE2_FROM_MUL");
    if (epi->max_out > 1) {
        if ((epi->max_out != 2 && epi->max_out != 4) || g.Cout % 4 != 0)
            return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: fused MaxOut needs max_out in {2, 4} and Cout % 4 == 0");
        if (epi->addend || epi->mul || epi->mul2 || epi->gate2 || epi->relu_gate || epi->out2 || epi->ch_scale || epi->ch_shift ||
            epi->relu || epi->out_absmax || epi->out2_absmax || (epi->flags & ~(BCOS_EPI_FORCE_POW | BCOS_EPI_UNIT_NORM_W)))
            return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: fused MaxOut supports bias, the B-cos scale, out, scale_out and norm_out only");
        if ((reinterpret_cast<uintptr_t>(epi->scale_out) & 15))
            return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: scale_out must be 16-byte aligned");
    }
    if (epi->a_sumsq && epi->bcos_mode == BCOS_NONE)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: a_sumsq belongs to a B-cos launch (bcos_mode != BCOS_NONE)");
    if ((epi->row_scale || epi->a_sumsq) && (g.groups > 1 || g.out_cgroup != 0))
        return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: row_scale / a_sumsq exclude grouped and depth-to-space launches");
    if (epi->addend_sub < 0 || (epi->addend_sub > 1 && (!epi->addend || g.out_cgroup != 0 || g.groups > 1 || epi->bcos_mode != BCOS_NONE)))
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: addend_sub > 1 needs an addend and a plain gradient launch (bcos_mode BCOS_NONE, "
                                            "no out_cgroup, no groups)");
    // the last row/col written must be inside the output tensor
    if ((g.P - 1) * g.out_sh + g.out_h0 >= g.OH || (g.Q - 1) * g.out_sw + g.out_w0 >= g.OW || g.out_h0 < 0 || g.out_w0 < 0)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: output mapping outside [OH,OW]");
    const int G = g.groups > 1 ? g.groups : 1;
    if (g.groups < 0 || g.groups > 65535) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: bad group count");
    if (G > 1 && (g.out_cgroup != 0 || epi->max_out > 1 || epi->out_absmax || epi->out2_absmax))
        return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: grouped launches exclude out_cgroup, fused MaxOut and *_absmax");
    if (g.out_cgroup != 0) {     // depth to space: columns = (output parity class, channel)
        if (g.out_cgroup < 0 || g.out_cgroup % 4 != 0 || g.out_sh <= 0 || g.out_sw <= 0 || g.out_h0 != 0 || g.out_w0 != 0 ||
            g.Cout != g.out_sh * g.out_sw * g.out_cgroup || g.P * g.out_sh > g.OH || g.Q * g.out_sw > g.OW ||
            (g.out_pitch != 0 && g.out_pitch < g.out_cgroup))
            return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: out_cgroup needs Cout == out_sh * out_sw * out_cgroup, out_cgroup % 4 == 0, "
                                                "zero output offsets, P * out_sh <= OH, Q * out_sw <= OW and out_pitch >= out_cgroup");
        if (epi->max_out > 1 || epi->out_absmax || epi->out2_absmax || epi->norm_out || epi->bias || epi->ch_scale || epi->ch_shift ||
            (epi->flags & BCOS_EPI_MUL_FROM_ACT) || epi->bcos_mode != BCOS_NONE)
            return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: out_cgroup launches are plain gradient launches (addend / mul / mul2 / "
                                                "gate2 / out / out2 only)");
    }
    *gn = g;
    if (gn->a_pitch == 0) gn->a_pitch = G * g.C;
    if (gn->out_pitch == 0) gn->out_pitch = g.out_cgroup > 0 ? g.out_cgroup : G * g.Cout;
    if (gn->norm_pitch == 0) gn->norm_pitch = G;
    if (gn->a_pitch % 4 != 0 || gn->a_pitch < G * g.C) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: bad a_pitch");
    if (epi->max_out > 1 && g.out_pitch == 0) gn->out_pitch = g.Cout / epi->max_out;
    if (g.out_cgroup == 0 && gn->out_pitch < G * g.Cout / (epi->max_out > 1 ? epi->max_out : 1))
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: bad out_pitch");
    if (gn->norm_pitch < G) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: norm_pitch smaller than the group count");
    return BCOS_OK;
}

// How many images of a validated call go into one launch (g.N: all of them).  The split-bf16 path addresses its operands through
// 32-bit buffer offsets: keep each launch below 2 GiB of A by splitting the batch (every tensor of the call is per-image separable);
// a call that cannot be split falls back to fp32 MFMA in select_operands.
int images_per_launch(const bcos_operands& ops, const bcos_tapconv_geom& g) {
    const int G = g.groups > 1 ? g.groups : 1, Ktot = g.TH * g.TW * g.C;
    const int64_t img_bytes = (int64_t)g.H * g.W * g.a_pitch * 4, a_bytes = img_bytes * g.N, wt_bytes = (int64_t)G * g.Cout * Ktot * 4;
    // (BCOS_OPT_SPLIT_LIMIT: tests lower the chunking threshold to drive this path with small tensors)
    const int64_t chunk_lim = bcos_option(BCOS_OPT_SPLIT_LIMIT);
    const bool split = contraction_mode(ops) >= 1 && a_bytes >= chunk_lim && g.N > 1 && img_bytes < chunk_lim && wt_bytes < ((int64_t)1 << 31);
    return split ? (int)((chunk_lim - 1) / img_bytes) : g.N;
}

// images [n0, n0 + per) of a call (fewer in the last chunk) as a call of their own: every per-image pointer moved to image n0
Call chunk_of(const bcos_operands& ops, const bcos_tapconv_geom& g, const bcos_epilogue& epi, int n0, int per) {
    Call c = {ops, g, epi};
    bcos_epilogue& e2 = c.e;
    c.g.N = g.N - n0 < per ? g.N - n0 : per;
    const int64_t opix = (int64_t)n0 * g.OH * g.OW;
    const float** cin[] = {&e2.addend, &e2.mul, &e2.mul2, &e2.gate2, &e2.relu_gate, &e2.rowadd};      // indexed like out
    for (const float** q : cin) if (*q) *q += opix * g.out_pitch;
    if (const int sb = e2.addend_sub; e2.addend && sb > 1)      // subsampled addend: its own image size
        e2.addend = epi.addend + (int64_t)n0 * ((g.OH + sb - 1) / sb) * ((g.OW + sb - 1) / sb) * g.out_pitch;
    float** cout[] = {&e2.out, &e2.out2, &e2.scale_out};
    for (float** q : cout) if (*q) *q += opix * g.out_pitch;
    if (e2.norm_out) e2.norm_out += opix * g.norm_pitch;
    const float** cpx[] = {&e2.mul_norm, &e2.row_scale, &e2.a_sumsq, &e2.rowadd_scale};      // one value per output pixel
    for (const float** q : cpx) if (*q) *q += opix;
    if (e2.out_absmax) e2.out_absmax += opix;
    if (e2.out2_absmax) e2.out2_absmax += opix;
    if (e2.out_imgmax) e2.out_imgmax += n0;
    if (e2.out_imgmin_c) e2.out_imgmin_c += n0;
    bcos_operands& o2 = c.ops;
    o2.a = ops.a + (int64_t)n0 * g.H * g.W * g.a_pitch;
    if (o2.a_absmax) o2.a_absmax += (int64_t)n0 * g.H * g.W;
    if (o2.a_imgmax) o2.a_imgmax += n0;          // (per-image maxima are indexed by the chunk's local image index)
    if (o2.a_imgmin) o2.a_imgmin += n0;
    if (o2.a_imgmin_c) o2.a_imgmin_c += n0;
    return c;
}

// resolve, part 1: the contraction loop's operands -- x3, the pre-split weight image, the split-f16 decision (p.h2 and its side tensors) -- and the 2 GiB limits
void select_operands(const bcos_operands& ops, KArgs& p) {
    const bcos_tapconv_geom& g = p.g;
    const int mode = contraction_mode(ops), G = g.groups > 1 ? g.groups : 1;
    const int64_t a_bytes = (int64_t)g.H * g.W * g.a_pitch * 4 * g.N, wt_bytes = (int64_t)G * g.Cout * p.Ktot * 4;
    const int64_t lim = (int64_t)1 << 31;
    p.x3 = (mode >= 1 && a_bytes < lim && wt_bytes < lim) ? 1 : 0;
    p.a_bytes = (unsigned)(a_bytes < lim ? a_bytes : 0);
    p.wt_bytes = (unsigned)(wt_bytes < lim ? wt_bytes : 0);
    const int64_t w3b = split_bytes(G * g.Cout, p.Ktot);
    // (grouped launches index the image by global weight row: a group's rows must start on a 32-row fragment tile)
    const bool unit_w = (p.e.flags & BCOS_EPI_UNIT_NORM_W) != 0;     // norms come from the fp32 weight rows in the staging registers
    const void* wt3 = ops.wt_bf16x3;
    p.wt3 = (p.x3 && !unit_w && wt3 && w3b < lim && !(reinterpret_cast<uintptr_t>(wt3) & 15) && (G == 1 || g.Cout % 32 == 0)) ? wt3 : nullptr;
    p.wt3_bytes = (unsigned)(w3b < lim ? w3b : 0);
    p.h2 = 0;
    p.a_absmax = p.a_imgmax = p.a_imgmin = p.a_imgmin_c = nullptr;
    p.wt2 = nullptr, p.wt2_cinv = nullptr;
    p.absmax_bytes = p.wt2_bytes = 0;
    const int64_t w2b = h2_image_bytes(g.Cout, p.Ktot), pixb = (int64_t)g.N * g.H * g.W * 4;
    // below K = 256 a launch is HBM-bound and the bf16x3 loop (no operand maxima to produce) is as fast, unless the caller
    // insists on f16x2; at K = 256 the six bf16 products still occupy a third of the SIMD cycles (14^2 layers of ResNet-50:
    // -12 % per launch with three f16 products).  The stem's K is all taps over 8 channels: compute-bound at any K.
    const bool h2_pays = p.Ktot >= 256 || (g.C <= 16 && p.Ktot >= 128) || ops.contraction == BCOS_CONTRACT_F16X2;
    if (mode == 2 && G == 1 && h2_pays && !unit_w && p.x3 && ops.a_absmax && ops.wt_f16x2 && w2b < lim && pixb < lim &&
        !(reinterpret_cast<uintptr_t>(ops.wt_f16x2) & 15)) {
        p.h2 = 1;
        p.a_absmax = ops.a_absmax;
        // BCOS_OPT_PATCH = 0 (development / test switch): no per-image range, i.e. per-row scales everywhere -- the per-tap loops as they were
        if (bcos_option(BCOS_OPT_PATCH) != 0) {
            p.a_imgmax = ops.a_imgmax;
            p.a_imgmin = ops.a_imgmax ? ops.a_imgmin : nullptr;
            p.a_imgmin_c = (ops.a_imgmax && !ops.a_imgmin) ? ops.a_imgmin_c : nullptr;
        }
        p.absmax_bytes = (unsigned)pixb;
        p.wt2 = ops.wt_f16x2;
        p.wt2_bytes = (unsigned)w2b;
        p.wt2_cinv = reinterpret_cast<const float*>(static_cast<const char*>(ops.wt_f16x2) + w2b);
    }
}

// resolve, part 2: the specialised epilogue (tile_epilogue_fast) when the launch's feature set is one of the compiled kinds; sets p.epi_kind / p.out_bytes
void select_epilogue_kind(KArgs& p) {
    const bcos_tapconv_geom& g = p.g;
    const bcos_epilogue& e = p.e;
    p.epi_kind = 0, p.out_bytes = 0;
    const int64_t obytes = (int64_t)g.N * g.OH * g.OW * g.out_pitch * 4;
    const bool norm_l = e.bcos_mode != BCOS_NONE;
    const bool off = bcos_option(BCOS_OPT_EPI_GENERIC) != 0;                // development / test switch
    // (a row_scale rides in the inverse operand scale of the split-f16 loops; the other loops carry it through the general epilogue)
    bool ok = !off && p.vec_ok && g.Cout % 4 == 0 && obytes < ((int64_t)1 << 31) && e.max_out <= 1 && e.out != nullptr && !e.col_scale && !(e.flags & BCOS_EPI_UNIT_NORM_W) &&
              (!e.row_scale || p.h2) &&
              !e.gate2 && !e.relu_gate && !(e.flags & (BCOS_EPI_NORM_ONLY | BCOS_EPI_FORCE_POW)) &&
              ((reinterpret_cast<uintptr_t>(e.bias) | reinterpret_cast<uintptr_t>(e.ch_scale) | reinterpret_cast<uintptr_t>(e.ch_shift)) & 15) == 0;
    int ef = 0;
    if (norm_l) {
        ok = ok && e.b == 2.0f && e.relu >= 0 && e.relu <= 2 && !e.mul && !e.mul2 && !e.out2 && !e.out2_absmax &&
             !(e.flags & BCOS_EPI_MUL_FROM_ACT);
        ef = (e.addend ? EF_ADDEND : 0) | (e.relu == 1 ? EF_RELU : 0) | (e.relu == 2 ? EF_GELU : 0) | (e.scale_out ? EF_SCALE_OUT : 0);
    } else {
        ok = ok && e.relu == 0 && !e.ch_scale && !e.ch_shift && !e.scale_out && (!e.mul2 || e.out2) &&
             (!e.out2 || e.mul) && (!e.out2_absmax || e.out2);
        // out2 is either ungated or gated by the low bit of mul (BCOS_EPI_GATE2_FROM_MUL): both are what the kinds compute
        ef = (e.addend ? EF_ADDEND : 0) | (e.mul ? EF_MUL : 0) | (e.out2 ? EF_OUT2 : 0) | (e.mul2 ? EF_MUL2 : 0) |
             ((e.flags & BCOS_EPI_MUL_FROM_ACT) ? EF_MULACT : 0) | (e.rowadd ? (EF_ROWADD | EF_ADDEND) : 0);
        if (e.rowadd) ok = ok && e.rowadd_scale && e.addend_sub <= 1 && !(reinterpret_cast<uintptr_t>(e.rowadd) & 15) && g.out_cgroup == 0;
        if (e.flags & BCOS_EPI_MUL_FROM_ACT)
            ok = ok && ((reinterpret_cast<uintptr_t>(e.mul_csc) | reinterpret_cast<uintptr_t>(e.mul_csh)) & 15) == 0;
    }
    if (!ok) return;
    const int* kinds = norm_l ? EPI_KINDS_FWD : EPI_KINDS_BWD;
    for (int k = 0; k < N_EPI_KINDS; ++k)
        if (kinds[k] == ef) { p.epi_kind = k + 1; p.out_bytes = (unsigned)obytes; break; }
}

// stage 2: the launch descriptor of one validated call (a chunk of it).  *fuses: does the launch fold the per-image range of its
// out_absmax into out_imgmax / out_imgmin_c -- what bcos_tapconv_fuses_image_range answers, ahead of plan_launch's check of the pair.
int resolve(const Call& c, KArgs& p, bool* fuses) {
    const bcos_tapconv_geom& g = c.g;
    const bcos_epilogue& e = c.e;
    p.a = c.ops.a; p.wt = c.ops.wt; p.g = g; p.e = e;
    p.M = g.N * g.P * g.Q;
    p.PQ = g.P * g.Q;
    p.Ktot = g.TH * g.TW * g.C;
    p.cpt = g.C / 4;
    p.nchunks = p.Ktot / 4;
    p.nk = (p.nchunks + 7) / 8;
    p.tiles_n = p.n_big = p.n_small = p.rows_big = 0;
    p.uniform_tap = (g.C % BK == 0) ? 1 : 0;
    p.lvl_off = 0;
    p.lvl_on = bcos_option(BCOS_OPT_PATCH_LEVELS) != 0;
    p.t2_bw = p.t2_nbx = p.t2_nb = p.t2_rows = 0;
    select_operands(c.ops, p);
    uintptr_t bits = 0;
    const void* ptrs[] = {e.addend, e.mul, e.mul2, e.gate2, e.relu_gate, e.out, e.out2, e.scale_out};
    for (const void* q : ptrs) bits |= reinterpret_cast<uintptr_t>(q);
    p.vec_ok = ((bits & 15) == 0 && g.out_pitch % 4 == 0) ? 1 : 0;
    if (g.out_cgroup > 0 && !p.vec_ok)
        return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv: out_cgroup needs 16-byte addressable epilogue tensors");
    select_epilogue_kind(p);
    if (e.rowadd && (p.epi_kind == 0 || (e.bcos_mode != BCOS_NONE)))
        return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: rowadd / rowadd_scale belong to a plain gradient launch that takes a specialised epilogue "
                                            "(16-byte addressable tensors < 2 GiB, Cout % 4 == 0, no mul / out2 / addend_sub): use bcos_patch_norm_bwd_add");
    // per-image range of the emitted maxima (bcos_epilogue.out_imgmax / out_imgmin_c): folded into the specialised epilogues only, for
    // launches whose tiles span at most 16 images (256 rows at >= 19 rows per image), plain output mapping, one group
    *fuses = p.epi_kind > 0 && e.out_absmax && g.out_cgroup == 0 && g.groups <= 1 && (int64_t)g.P * g.Q >= 19;
    return BCOS_OK;
}

// stage 3: which launcher a resolved launch takes -- a function of the descriptor (geometry, epilogue, p.h2 / p.a_imgmax) and the
// option table; launches nothing
#define BCOS_TC_GO(name) Route{ROUTE_##name, 0}
Route choose_route(const KArgs& p) {
    const bcos_tapconv_geom& g = p.g;
    const bcos_epilogue& e = p.e;
    const int G = g.groups > 1 ? g.groups : 1;
    const int64_t M64 = p.M;
    const bool narrow = g.Cout <= 8 && G == 1 && !e.out_absmax && !e.out2_absmax && e.max_out <= 1 && e.addend_sub <= 1 && !e.row_scale && !e.a_sumsq && !e.rowadd;
    if (const int ch_pass = narrow ? bcos_skinny_ch_pass(g, e) : 0) return Route{ROUTE_skinny, ch_pass};
    if (p.h2) {
        // staging of the split-f16 loop: LDS-DMA (tile_body_d, default) or registers (tile_body_h2: BCOS_H2_LOOP=regs); same bits
        const bool dma = bcos_option(BCOS_OPT_H2_LOOP) == 0;
        {
            // multi-tap launches over an LDS-resident input patch (tile_body_p).  The choice depends on the layer's geometry alone,
            // never on the batch: the patch loop rounds differently from the per-tap loops (one operand scale per image), and an
            // image's bits must not depend on how many images share its launch.  (BCOS_OPT_PATCH = 0: select_operands passed no p.a_imgmax on.)
            const int ntaps = g.TH * g.TW;
            const bool geom_ok = ((ntaps == 9 && g.TH == 3) || (ntaps == 16 && g.TH == 4)) && g.C % X3_BK == 0 && g.in_sh == 1 && g.in_sw == 1 &&
                                 g.dstep_h == 1 && g.dstep_w == 1 && g.a_pitch >= g.C;
            if (dma && geom_ok && p.a_imgmax && !e.row_scale && !e.a_sumsq) {      // (the patch kernels compile those two out)
                if (ntaps == 16) {
                    if (g.Cout <= 32 && g.in_sh == 1) return BCOS_TC_GO(p2_256x32_t16);
                } else {
                if (g.Cout > 128 && g.Cout <= 256 && patch_fits(g, 128, 256, 256) && bcos_option(BCOS_OPT_PATCH_WIDE)) return BCOS_TC_GO(p_128x256_a);
                if (g.Cout > 64 && patch_fits(g, 128, 256, 256)) return BCOS_TC_GO(p_128x128_a);
                if (g.Cout > 64 && patch_fits(g, 128, 256, 448)) return BCOS_TC_GO(p_128x128_b);
                if (g.Cout > 64 && patch_fits(g, 128, 384, 320)) return BCOS_TC_GO(p_128x128_c);
                if (g.Cout > 32 && g.Cout <= 64 && patch_fits(g, 256, 640, 640)) return BCOS_TC_GO(p_256x64_a);
                // wider images (112^2: the 3 x 3 stem convolutions of the CLIP ResNets): 8 x 32 blocks.  (At 56^2 the linear tiles win,
                // 224 against 253 us: the blocks leave an eighth of the rows empty there.)
                if (g.Cout > 32 && g.Cout <= 64 && g.in_sh == 1 && g.Q > 64) return BCOS_TC_GO(p2_256x64_b32);
                if (g.Cout > 8 && g.Cout <= 32 && g.in_sh == 1 && g.Q > 64) return BCOS_TC_GO(p2_256x32_t9);
                }
            }
        }
        if (g.Cout > 64 && dma && bcos_option(BCOS_OPT_H2_TILE) == 0) {
            // FEW-ROW launches (M <= a few hundred rows: the pooled token of CLIP's attention pool at batch 256 -- 2 row tiles --, small
            // batches through every head): with 128- or 256-column tiles they occupy a handful of CUs and run at the latency of ONE
            // workgroup's K loop (256 x 2048 -> 1024: 8 workgroups, 111 us against 28 for the vendor's GEMM).  Narrower
            // column tiles multiply the workgroups -- 64 or 32 columns each, as many as it takes to put a workgroup on half the CUs -- at
            // no cost in bits (an output element's K order does not depend on its tile).
            const int64_t tm = (M64 + 127) / 128;
            const int64_t t128 = tm * ((g.Cout + 127) / 128);
            if (t128 < 64) {
                if (tm * ((g.Cout + 63) / 64) >= 96 || g.Cout <= 128) return BCOS_TC_GO(d_128x64);
                return BCOS_TC_GO(d_128x32);
            }
        }
        if (g.Cout > 64) {
            // 128 x 256 tiles stage half the A bytes per MFMA; they pay when they do not cost an extra round of tiles
            // (measured on the ResNet-50 shapes: M = 50176, N = 256: -3 %; M = 12544, N = 512: +17 % -> stays 128 x 128)
            const int64_t force = bcos_option(BCOS_OPT_H2_TILE);      // development switch: 1 = 128 x 128, 2 = 128 x 256
            const int64_t tm = (M64 + 127) / 128;
            const int64_t t1 = tm * ((g.Cout + 127) / 128), t2 = tm * ((g.Cout + 255) / 256);
            // (a finer cost model -- a wide tile = 1.75 narrow ones, which moves M = 200 704 with N = 256 / 512 and M = 50 176 with
            // N = 1024, K = 512 to wide tiles -- wins 11-18 % on those launches timed one by one and loses 0.1 ms on the step, where
            // consecutive launches overlap their tails: not adopted)
            // rounds of tiles, a wide tile priced at BCOS_OPT_H2_WIDE_COST / 4 narrow ones (8 = two, the model of rounds 2-3; the wide
            // tile shares the A operand's DMA and split between its halves, so 7 is nearer what the layers measure)
            const int64_t wc = bcos_option(BCOS_OPT_H2_WIDE_COST);
            const int64_t c1 = 4 * ((t1 + SLOTS - 1) / SLOTS), c2 = wc * ((t2 + SLOTS - 1) / SLOTS);
            bool wide = g.Cout > 128 && (c2 < c1 || (c2 == c1 && (wc < 8 || p.Ktot >= 1024)));
            if (force) wide = g.Cout > 128 && force == 2;
            // 129 ... 192 columns (the 192-wide linears of the SimpleViTs: to_out, linear2, their gradients): ONE tile of 192 columns
            // (six accumulator tiles per wave) instead of 128 + a half-empty second 128
            if (dma && g.Cout > 128 && g.Cout <= 192 && !force) return BCOS_TC_GO(d_128x192);
            // multiples of 192 that are not multiples of 256 (the 576-wide to_qkv of the SimpleViTs: 3 x 192 exactly, against 5 x 128 with
            // 64 empty columns or 3 x 256 with 192): whole 192-column tiles -- ViT-Ti batch 512 forward+explanation 18.26 -> 17.97 ms per step
            // in three same-node pairs (round 5); 768 = 4 x 192 against 3 x 256: no gain, stays on the 256-column tiles.  Bits unchanged.
            if (dma && g.Cout % 192 == 0 && g.Cout % 256 != 0 && g.Cout <= 1152 && !force) return BCOS_TC_GO(d_128x192);
            if (wide) return dma ? BCOS_TC_GO(d_128x256) : BCOS_TC_GO(h2_128x256);
            return dma ? BCOS_TC_GO(d_128x128) : BCOS_TC_GO(h2_128x128);
        }
        if (g.Cout > 32) {
            // 256 x 64 tiles (four waves of 64 x 64: the A operand's split, its LDS image and the per-tile prologue / epilogue
            // latencies are shared by twice the matrix instructions of a 128 x 64 tile) from two rounds of tiles on.  Same-node
            // A/B on the ResNet-50 step at batch 256 (M = 802 816): 3x3 64 -> 64 gradient 1.03 -> 0.90 ms, 256 -> 64 gradient
            // 1.21 -> 1.13 ms, stem forward 1.05 -> 1.01 ms, the forward launches -1 %.  Results are identical bit for bit (same
            // K walk, same product order per accumulator).
            const bool tall = bcos_option(BCOS_OPT_H2_TALL) != 0;       // development switch: 0 keeps the 128-row tiles
            const int64_t tall_min = bcos_option(BCOS_OPT_H2_TALL_MIN);     // default 2 * 256 * SLOTS (batch 128, M = 401 408: +0.4 % per step; M = 200 704: neutral)
            if (M64 >= tall_min && tall) return dma ? BCOS_TC_GO(d_256x64) : BCOS_TC_GO(h2_256x64);
            return dma ? BCOS_TC_GO(d_128x64) : BCOS_TC_GO(h2_128x64);
        }
        {   // 256 x 32 tiles likewise (the depth-to-space stem gradient, M = 3.2 M: 1.29-1.38 -> 1.17-1.20 ms in a same-node A/B)
            if (M64 >= 2 * 256 * SLOTS && bcos_option(BCOS_OPT_H2_TALL)) return dma ? BCOS_TC_GO(d_256x32) : BCOS_TC_GO(h2_256x32);
        }
        return dma ? BCOS_TC_GO(d_128x32) : BCOS_TC_GO(h2_128x32);
    }
    if (g.Cout > 64) {
        // few-row launches (see the split-f16 branch above): narrower column tiles put a workgroup on more CUs; same bits
        const int64_t tm = (M64 + 127) / 128;
        if (G == 1 && tm * ((g.Cout + 127) / 128) < 64 && bcos_option(BCOS_OPT_H2_TILE) == 0)
            return (tm * ((g.Cout + 63) / 64) >= 96 || g.Cout <= 128) ? BCOS_TC_GO(cfg_128x64) : BCOS_TC_GO(cfg_128x32);
        return BCOS_TC_GO(cfg_128x128);
    }
    if (g.Cout > 32) return BCOS_TC_GO(cfg_128x64);
    return BCOS_TC_GO(cfg_128x32);
}
#undef BCOS_TC_GO

// stage 4: the launcher of the route, or the narrow-output kernel
int launch_route(const Route& r, const KArgs& p, hipStream_t s) {
    if (r.id == ROUTE_skinny) return bcos_skinny_launch(p.a, p.wt, p.g, p.e, s);
    return ROUTES[r.id].launch(&p, p.e.bcos_mode != BCOS_NONE ? 1 : 0, s);
}

// resolve -> the check of the out_imgmax / out_imgmin_c pair -> choose_route: everything of one launch but the launch
int plan_launch(const Call& c, KArgs& p, Route* r) {
    bool fuses = false;
    const int rc = resolve(c, p, &fuses);
    if (rc != BCOS_OK) return rc;
    if ((c.e.out_imgmax || c.e.out_imgmin_c) && (!c.e.out_imgmax || !c.e.out_imgmin_c || !fuses))
        return bcos_set_error(BCOS_E_NOSUP, "bcos_tapconv: out_imgmax / out_imgmin_c come as a pair, with out_absmax, and only for launches "
                                            "bcos_tapconv_fuses_image_range() answers 1 for");
    *r = choose_route(p);
    return BCOS_OK;
}
}  // namespace

extern "C" int bcos_tapconv_ops(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi, void* stream) {
    bcos_tapconv_geom g;
    int rc = validate(ops, geom, epi, &g);
    if (rc != BCOS_OK) return rc;
    const int per = images_per_launch(*ops, g);
    for (int n0 = 0; n0 < g.N; n0 += per) {
        KArgs p; Route r;
        rc = plan_launch(chunk_of(*ops, g, *epi, n0, per), p, &r);
        if (rc == BCOS_OK) rc = launch_route(r, p, reinterpret_cast<hipStream_t>(stream));
        if (rc != BCOS_OK) return rc;
    }
    return BCOS_OK;
}

// 1: a bcos_tapconv_ops call with these arguments folds the per-image range of its out_absmax into bcos_epilogue.out_imgmax / out_imgmin_c
// itself; 0: it does not (general epilogue, depth-to-space or grouped launch, fewer than 19 rows per image, no out_absmax) and rejects
// the two fields; < 0: the arguments are invalid anyway.  Nothing is launched: validate and resolve, as the launch runs them.
extern "C" int bcos_tapconv_fuses_image_range(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi) {
    bcos_tapconv_geom g;
    int rc = validate(ops, geom, epi, &g);
    if (rc != BCOS_OK) return rc;
    const int per = images_per_launch(*ops, g);
    // (chunks differ in their image count alone, which decides the answer only through the 2 GiB limits: 1 if any chunk folds)
    for (int n0 = 0; n0 < g.N; n0 += per) {
        KArgs p; bool fuses = false;
        rc = resolve(chunk_of(*ops, g, *epi, n0, per), p, &fuses);
        if (rc != BCOS_OK) return rc;
        if (fuses) return 1;
    }
    return 0;
}

extern "C" int bcos_tapconv_route_query(const bcos_operands* ops, const bcos_tapconv_geom* geom, const bcos_epilogue* epi, bcos_tapconv_route* out) {
    if (!out) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv_route_query: NULL result");
    *out = bcos_tapconv_route{-1, 0, 0, 0, 0, 0, 0, 0};
    bcos_tapconv_geom g;
    int rc = validate(ops, geom, epi, &g);
    if (rc != BCOS_OK) return rc;
    const int per = images_per_launch(*ops, g);
    KArgs p; Route r;
    rc = plan_launch(chunk_of(*ops, g, *epi, 0, per), p, &r);      // (the first chunk's route)
    if (rc != BCOS_OK) return rc;
    const RouteEntry& row = ROUTES[r.id];
    const int chunks = (g.N + per - 1) / per;
    if (r.id == ROUTE_skinny) *out = bcos_tapconv_route{r.id, 0, 0, BCOS_LOOP_F32, 0, 0, chunks, r.ch_pass};      // (its own plain epilogue)
    else *out = bcos_tapconv_route{r.id, p.epi_kind, p.e.bcos_mode != BCOS_NONE ? 1 : 0, family_loop(row.fam, p), row.bm, row.bn, chunks, 0};
    return BCOS_OK;
}

extern "C" const char* bcos_tapconv_route_name(int route) { return route >= 0 && route < ROUTE_COUNT ? ROUTES[route].name : nullptr; }
extern "C" int bcos_tapconv_route_count(void) { return ROUTE_COUNT; }
extern "C" int bcos_tapconv_epilogue_kinds(void) { return N_EPI_KINDS; }

extern "C" int bcos_tapconv_group(const float* a, const float* const* wts, const bcos_tapconv_geom* geoms,
                                  const bcos_epilogue* epis, int count, void* stream) {
    if (!a || !wts || !geoms || !epis || count <= 0) return bcos_set_error(BCOS_E_INVAL, "bcos_tapconv_group: bad argument");
    const int fused = bcos_try_skinny_group(a, wts, geoms, epis, count, reinterpret_cast<hipStream_t>(stream));
    if (fused < 0) return fused;
    if (fused == 1) return BCOS_OK;
    for (int i = 0; i < count; ++i) {
        const int rc = bcos_tapconv(a, wts[i], &geoms[i], &epis[i], stream);
        if (rc != BCOS_OK) return rc;
    }
    return BCOS_OK;
}
