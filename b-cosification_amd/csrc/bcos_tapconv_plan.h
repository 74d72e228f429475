// bcos_tapconv_plan.h -- what the tile kernels (bcos_tapconv.hip), the host-side dispatcher (bcos_tapconv_dispatch.hip) and the
// weight-image kernels (bcos_weights.hip) share: the launch descriptor, the constants the planner prices tiles with, the epilogue
// kinds, the launcher seam and the sizes of the pre-split weight images.  The definitions sit in an anonymous namespace: every unit
// compiles its own copy, and KArgs keeps the internal-linkage name it has in every kernel's signature.
#ifndef BCOS_TAPCONV_PLAN_H
#define BCOS_TAPCONV_PLAN_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bcos_hip.h"

namespace {

constexpr int BK = 32;            // K floats per step
constexpr int NTHREADS = 256;

struct KArgs {
    const float* a;
    const float* wt;
    bcos_tapconv_geom g;
    bcos_epilogue e;
    int M;          // N*P*Q
    int PQ;
    int Ktot;       // taps*C
    int cpt;        // 16-byte chunks per tap = C/4
    int nchunks;    // Ktot/4
    int nk;         // K steps
    int tiles_n;            // column tiles
    int n_big, n_small;     // tiles of BM rows, then tiles of BM/2 rows (tail of the launch)
    int rows_big;           // rows covered by the BM-row tiles
    const void* wt3;              // optional pre-split weights in MFMA fragment order (bcos_split_weights), else NULL
    unsigned wt3_bytes;
    unsigned a_bytes, wt_bytes;   // operand sizes for the buffer descriptors of the split-bf16 path (< 2 GiB there)
    const unsigned* a_absmax;     // split-f16 path: per-pixel max |A| bit patterns (the operand scale source)
    unsigned absmax_bytes;
    const unsigned* a_imgmax;     // ... per-image maxima of those (input-patch loop, tile_body_p), else NULL
    const unsigned* a_imgmin;     // ... per-image minima over the NONZERO pixels of those (dynamic range inside an image), else NULL
    const unsigned* a_imgmin_c;   // ... or a LOWER BOUND of those minima, stored complemented (~v; 0 = no nonzero pixel), as the epilogue of the launch that
                                  //     produced A leaves it (bcos_epilogue.out_imgmin_c): decides only whether a tile runs the level bookkeeping, never a bit
    int lvl_on;                   // input-patch loop: 1 = one pass per operand-scale level present in a tile (BCOS_OPT_PATCH_LEVELS)
    int lvl_off;                  // input-patch loop: byte offset, inside the dynamic LDS, of the row-level table (beyond everything the epilogue uses)
    const void* wt2;              // split-f16 path: pre-split, pre-scaled weights in MFMA fragment order (bcos_split_weights_f16x2)
    unsigned wt2_bytes;
    const float* wt2_cinv;        // ... their inverse column scales [padded Cout]
    int h2;          // contraction on split-f16 MFMA (see tile_body_h2)
    int x3;          // contraction on split-bf16 MFMA (see tile_body_x3) instead of fp32 MFMA
    int uniform_tap; // C % 32 == 0: every K-step lies inside one tap
    int vec_ok;     // every per-element epilogue tensor is 16-byte addressable (pitch % 4 == 0, aligned bases)
    int epi_kind;   // 0 = general epilogue, k + 1 = specialisation k of EPI_KINDS_FWD (norm launches) / EPI_KINDS_BWD (tile_epilogue_fast)
    unsigned out_bytes;   // size of the [N*OH*OW][out_pitch] epilogue tensors (epi_kind > 0: < 2 GiB)
    // 2-D row tiles (input-patch loop on wide images, tile_body_p<..., T2D>): tile t = (image t / t2_nb, block t % t2_nb) and row r of a
    // tile is position (r / t2_bw, r % t2_bw) of that t2_bh x t2_bw block of the row grid; 0 = rows are m = n P Q + i Q + j
    int t2_bw, t2_nbx, t2_nb, t2_rows;
};

// feature bits of the specialised epilogues (bcos_tapconv.hip: "Specialised epilogues") and the feature sets compiled as kinds
enum : int { EF_ADDEND = 1, EF_RELU = 2, EF_SCALE_OUT = 4, EF_MUL = 8, EF_OUT2 = 16, EF_MUL2 = 32, EF_GELU = 64, EF_MULACT = 128, EF_ROWADD = 256, EF_NONE = -1 };
// forward kinds (NORM kernels): B = 2 scale, optional bias / channel affine;  backward kinds (no norm): gradient multipliers
// (the GELU kinds are the linear1 layers of the B-cosified ViTs: MyGELU with its gate folded into the stored multiplier)
constexpr int EPI_KINDS_FWD[] = {EF_RELU | EF_SCALE_OUT, EF_RELU | EF_SCALE_OUT | EF_ADDEND, EF_SCALE_OUT, EF_RELU, EF_RELU | EF_ADDEND, 0,
                                 EF_GELU | EF_SCALE_OUT, EF_GELU};
constexpr int EPI_KINDS_BWD[] = {EF_MUL, EF_MUL | EF_ADDEND | EF_OUT2, EF_MUL | EF_ADDEND | EF_OUT2 | EF_MUL2, 0, EF_ADDEND, EF_MUL | EF_OUT2,
                                 EF_MUL | EF_MULACT, EF_ADDEND | EF_ROWADD};       // MULACT: the multiplier is rebuilt from the kept activation (BCOS_EPI_MUL_FROM_ACT);
                                                                                   // ROWADD: out = acc + (rowadd_scale[pixel] rowadd + addend), the addend optional (bcos_epilogue.rowadd)
constexpr int N_EPI_KINDS = 8;

constexpr int X3_BK = 16;      // k per step = one MFMA k-block; two LDS buffers
constexpr int H2_MAX_TAPS = 16;    // channel-chunk-major K walk for up to this many taps (offset table: taps x BM x 4 bytes of LDS)
constexpr int SLOTS = 512;   // 256 CUs x 2 resident workgroups (LDS- and VGPR-limited)

// The launcher families (launch_cfg / launch_h2 / launch_d / launch_p) and the contraction loop a family's launch runs, numbered like BCOS_LOOP_* of
// include/bcos_hip.h: the one place that decides it, for launch_cfg (the LOOP template argument of its kernel) and for bcos_tapconv_route_query
enum : int { BCOS_FAM_CFG, BCOS_FAM_H2, BCOS_FAM_D, BCOS_FAM_P };
inline int family_loop(int fam, const KArgs& p) {
    if (fam == BCOS_FAM_CFG) return p.x3 ? (p.wt3 ? BCOS_LOOP_BF16X3_PRESPLIT : BCOS_LOOP_BF16X3) : BCOS_LOOP_F32;
    return fam == BCOS_FAM_H2 ? BCOS_LOOP_F16X2_REGS : fam == BCOS_FAM_D ? BCOS_LOOP_F16X2_DMA : BCOS_LOOP_F16X2_PATCH;
}
static_assert(BCOS_LOOP_F32 == 0 && BCOS_LOOP_BF16X3 == 1 && BCOS_LOOP_BF16X3_PRESPLIT == 2, "family_loop returns the kernel's LOOP argument");

// Does the input patch of every BM-row tile of the launch fit `px` pixels?  Upper bound over the tile positions: a tile touches
// at most R = (BM + Q - 2) / Q + 1 output rows, which cross at most ceil((R - 1) / P) image boundaries (TH - s extra virtual rows each)
inline bool patch_fits(const bcos_tapconv_geom& g, int BM, int items_px, int lds_px) {
    const int s = g.in_sh;
    const int R = (BM + g.Q - 2) / g.Q + 1;
    const int nb = (R - 1 + g.P - 1) / g.P;
    const int extra = g.TH > s ? g.TH - s : 0;
    const int64_t rows = (int64_t)(R - 1) * s + g.TH + (int64_t)nb * extra;
    const int pw = (g.Q - 1) * s + g.TW;
    int pitch = 1;
    while (pitch < pw) pitch <<= 1;                                  // (rows are stored with a power-of-two pitch, rotated: tile_body_p)
    return rows * pw <= items_px && rows * pitch <= lds_px && (int64_t)g.P * g.Q * 14 >= BM;      // (at most 16 images per tile)
}

// bytes of the pre-split weight images: bf16x3 (bcos_split_weights) and f16x2 without its inverse row scales (bcos_split_weights_f16x2)
inline int64_t split_bytes(int rows, int Ktot) {
    const int64_t tiles = (((int64_t)rows + 127) / 128) * 4, nk = ((int64_t)Ktot + 15) / 16;
    return tiles * nk * 3 * 1024;
}
__host__ __device__ inline int64_t h2_tiles(int rows) { return (((int64_t)rows + 127) / 128) * 4; }
__host__ __device__ inline int64_t h2_image_bytes(int rows, int Ktot) { return h2_tiles(rows) * (((int64_t)Ktot + 15) / 16) * 2 * 1024; }

}  // namespace

// The launchers cross units as plain functions taking the launch descriptor by address (every unit compiles the same KArgs).
#define BCOS_TC_LAUNCHER(name) __attribute__((visibility("hidden"))) int name(const void* kargs, int norm, hipStream_t s)
// every tile launcher, once: X(name, launcher family (BCOS_FAM_*: which loop it instantiates, family_loop), tile rows, tile columns).  The list declares the launchers, numbers them (the route ids of
// bcos_tapconv_route_query, the narrow-output kernel of bcos_skinny.hip last) and fills the table the dispatcher launches through;
// BCOS_TC_DEFINE refuses a launcher that is not in it, and one that is listed without a definition does not link
#define BCOS_TC_ROUTES(X) \
    X(cfg_128x128, BCOS_FAM_CFG, 128, 128) \
    X(cfg_128x64, BCOS_FAM_CFG, 128, 64) \
    X(cfg_128x32, BCOS_FAM_CFG, 128, 32) \
    X(h2_128x256, BCOS_FAM_H2, 128, 256) \
    X(h2_128x128, BCOS_FAM_H2, 128, 128) \
    X(h2_128x64, BCOS_FAM_H2, 128, 64) \
    X(h2_128x32, BCOS_FAM_H2, 128, 32) \
    X(h2_256x64, BCOS_FAM_H2, 256, 64) \
    X(h2_256x32, BCOS_FAM_H2, 256, 32) \
    X(d_128x256, BCOS_FAM_D, 128, 256) \
    X(d_128x128, BCOS_FAM_D, 128, 128) \
    X(d_128x192, BCOS_FAM_D, 128, 192) \
    X(d_128x64, BCOS_FAM_D, 128, 64) \
    X(d_128x32, BCOS_FAM_D, 128, 32) \
    X(d_256x64, BCOS_FAM_D, 256, 64) \
    X(d_256x32, BCOS_FAM_D, 256, 32) \
    X(p_128x256_a, BCOS_FAM_P, 128, 256) \
    X(p_128x128_a, BCOS_FAM_P, 128, 128) \
    X(p_128x128_b, BCOS_FAM_P, 128, 128) \
    X(p_128x128_c, BCOS_FAM_P, 128, 128) \
    X(p_256x64_a, BCOS_FAM_P, 256, 64) \
    X(p2_256x32_t16, BCOS_FAM_P, 256, 32) \
    X(p2_256x32_t9, BCOS_FAM_P, 256, 32) \
    X(p2_256x64_b32, BCOS_FAM_P, 256, 64)
#define BCOS_TC_X_DECL(name, fam, bm, bn) BCOS_TC_LAUNCHER(bcos_tc_##name);
BCOS_TC_ROUTES(BCOS_TC_X_DECL)
#define BCOS_TC_X_ID(name, fam, bm, bn) ROUTE_##name,
enum : int { BCOS_TC_ROUTES(BCOS_TC_X_ID) ROUTE_skinny, ROUTE_COUNT };

#endif
