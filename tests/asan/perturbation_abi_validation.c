/* Host-side argument validation of bcos_perturb_select_ws_bytes, bcos_perturb_select, bcos_prep_input_perturbed and bcos_class_scores
 * (additive entry points of ABI v12) under AddressSanitizer, beside occlusion_abi_validation.c: every call below must be REJECTED by the
 * library's own checks before anything is launched, so it runs without a GPU.  counts_host is the one array the library reads on the
 * host: it is allocated at exactly K entries, so a read past it is an ASan report.  Exit code 0 = every call returned BCOS_E_INVAL with
 * a message and ASan saw no bad access. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
#define EXPECT_INVAL(call, who)                                                                             \
    do {                                                                                                    \
        int rc_ = (call);                                                                                   \
        if (rc_ != BCOS_E_INVAL) { printf("FAIL %s -> %d (expected %d)\n", #call, rc_, BCOS_E_INVAL); ++failures; } \
        else if (strstr(bcos_last_error_string(), who) == NULL) {                                           \
            printf("FAIL %s: no error message\n", #call); ++failures; }                                     \
    } while (0)
#define SIZE(...) EXPECT_INVAL(bcos_perturb_select_ws_bytes(__VA_ARGS__), "bcos_perturb_select_ws_bytes")
#define SEL(...) EXPECT_INVAL(bcos_perturb_select(__VA_ARGS__), "bcos_perturb_select:")
#define PREP(...) EXPECT_INVAL(bcos_prep_input_perturbed(__VA_ARGS__), "bcos_prep_input_perturbed")
#define CLS(...) EXPECT_INVAL(bcos_class_scores(__VA_ARGS__), "bcos_class_scores")

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    uint32_t* am = (uint32_t*)aligned_alloc(64, 4096);
    uint64_t* thr = (uint64_t*)aligned_alloc(64, 4096);
    void* ws = aligned_alloc(64, 4096);
    enum { B = 3, H = 8, W = 12, HW = H * W, K = 5, CL = 10 };
    int32_t* counts = (int32_t*)malloc(K * sizeof(int32_t));      /* exactly K entries */
    const int32_t good[K] = {0, 1, HW, 7, 7};
    memcpy(counts, good, sizeof(good));
    int64_t need = -1;
    if (bcos_perturb_select_ws_bytes(B, HW, K, &need) != BCOS_OK || need <= 0) { printf("FAIL ws_bytes\n"); ++failures; }

    SIZE(B, HW, K, NULL);
    SIZE(0, HW, K, &need);
    SIZE(-1, HW, K, &need);
    SIZE(B, 0, K, &need);
    SIZE(B, (int64_t)1 << 31, K, &need);
    SIZE(B, HW, 0, &need);
    SIZE(B, HW, BCOS_PERTURB_MAX_COUNTS + 1, &need);
    if (bcos_perturb_select_ws_bytes(B, HW, K, &need) != BCOS_OK) { printf("FAIL ws_bytes\n"); ++failures; }

    SEL(NULL, counts, 0, thr, ws, need, B, HW, K, NULL);
    SEL(f, NULL, 0, thr, ws, need, B, HW, K, NULL);
    SEL(f, counts, 0, NULL, ws, need, B, HW, K, NULL);
    SEL(f, counts, 1, thr, NULL, need, B, HW, K, NULL);
    SEL(f, counts, 0, thr, ws, need, 0, HW, K, NULL);
    SEL(f, counts, 0, thr, ws, need, B, 0, K, NULL);
    SEL(f, counts, 0, thr, ws, need, B, (int64_t)1 << 31, K, NULL);
    SEL(f, counts, 0, thr, ws, need, B, HW, 0, NULL);
    SEL(f, counts, 0, thr, ws, need, B, HW, -2, NULL);
    SEL(f, counts, 0, thr, ws, need, B, HW, BCOS_PERTURB_MAX_COUNTS + 1, NULL);   /* refused before counts_host[K..] would be read */
    SEL(f, counts, 0, thr, ws, need - 1, B, HW, K, NULL);
    SEL(f, counts, 0, thr, ws, 0, B, HW, K, NULL);
    SEL(f, counts, 0, (uint64_t*)((char*)thr + 4), ws, need, B, HW, K, NULL);
    SEL(f, counts, 0, thr, (char*)ws + 4, need, B, HW, K, NULL);
    SEL(f, counts, 0, thr, ws, need, B, HW - 1, K, NULL);            /* the count HW leaves an image of HW - 1 pixels */
    /* one bad count -- at every position, the LAST included -- refuses the call, in either order */
    const int32_t bad[] = {-1, HW + 1, INT32_MIN, INT32_MAX};
    for (int pos = 0; pos < K; ++pos)
        for (int i = 0; i < 4; ++i) {
            memcpy(counts, good, sizeof(good));
            counts[pos] = bad[i];
            SEL(f, counts, 0, thr, ws, need, B, HW, K, NULL);
            SEL(f, counts, 1, thr, ws, need, B, HW, K, NULL);
        }

    PREP(NULL, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, NULL, thr, 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, f, NULL, 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, NULL, f, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, NULL, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 1, f, f, NULL, NULL, B, K, 0, B * K, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, 0, K, 0, 1, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, 0, 0, 1, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, 0, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, H, -1, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 5, 0, NULL);            /* Cpad < 6 */
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 3, H, W, 8, 1, NULL);            /* the AddInverse form: another operator */
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 3, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 8, 1, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K, 6, 1 << 16, 1 << 16, 8, 0, NULL); /* H * W past 2^31 - 1 */
    PREP(f, f, thr, 0, f, f, f, am, B, K, -1, 2, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, 0, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, -4, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, 0, B * K + 1, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, B * K, 1, 6, H, W, 8, 0, NULL);
    PREP(f, f, thr, 0, f, f, f, am, B, K, INT32_MAX, INT32_MAX, 6, H, W, 8, 0, NULL); /* first + n past int32 */
    PREP(f, f, (uint64_t*)((char*)thr + 4), 0, f, f, f, am, B, K, 0, B * K, 6, H, W, 8, 0, NULL);

    int32_t* tg = (int32_t*)am;
    CLS(NULL, tg, K, 0, f, B * K, CL, NULL);
    CLS(f, NULL, K, 0, f, B * K, CL, NULL);
    CLS(f, tg, K, 0, NULL, B * K, CL, NULL);
    CLS(f, tg, 0, 0, f, B * K, CL, NULL);
    CLS(f, tg, -1, 0, f, B * K, CL, NULL);
    CLS(f, tg, K - 1, 0, f, B * K, CL, NULL);                       /* R is no multiple of group */
    CLS(f, tg, K, 0, f, 0, CL, NULL);
    CLS(f, tg, K, 0, f, -5, CL, NULL);
    CLS(f, tg, K, 0, f, B * K, 0, NULL);
    CLS(f, tg, K, 3, f, B * K, CL, NULL);
    CLS(f, tg, K, -1, f, B * K, CL, NULL);
    CLS(f, tg, 1, 2, f, INT64_MAX / 2, CL, NULL);                   /* R * CL past int64 */

    free(counts);
    free(ws);
    free(thr);
    free(am);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_perturb_select, bcos_prep_input_perturbed, bcos_class_scores: all refusals ok\n");
    return 0;
}
