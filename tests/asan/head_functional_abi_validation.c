/* Host-side argument validation of bcos_head_rankm_grad and bcos_head_cotangent_grad (additive entry points of ABI v12) under
 * AddressSanitizer, beside occlusion_abi_validation.c: every call below must be REJECTED by the library's own checks before anything is
 * launched, so it runs without a GPU.  Exit code 0 = every call returned the expected code with a message and ASan saw no bad access. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
#define EXPECT_CODE(call, code, who)                                                                        \
    do {                                                                                                    \
        int rc_ = (call);                                                                                   \
        if (rc_ != (code)) { printf("FAIL %s -> %d (expected %d)\n", #call, rc_, (code)); ++failures; }     \
        else if (strstr(bcos_last_error_string(), who) == NULL) {                                           \
            printf("FAIL %s: no error message\n", #call); ++failures; }                                     \
    } while (0)
#define RANKM(...) EXPECT_CODE(bcos_head_rankm_grad(__VA_ARGS__), BCOS_E_INVAL, "bcos_head_rankm_grad")
#define COT(...) EXPECT_CODE(bcos_head_cotangent_grad(__VA_ARGS__), BCOS_E_INVAL, "bcos_head_cotangent_grad")

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    uint32_t* am = (uint32_t*)aligned_alloc(64, 4096);
    int64_t* cls = (int64_t*)aligned_alloc(64, 4096);
    enum { N = 2, R = 4, K = 10, D = 8, J = 2 };

    RANKM(NULL, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    RANKM(cls, NULL, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    RANKM(cls, f, J, NULL, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    RANKM(cls, f, J, f, NULL, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, NULL, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    RANKM(cls, f, 0, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);            /* J = 0 */
    RANKM(cls, f, -3, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);
    EXPECT_CODE(bcos_head_rankm_grad(cls, f, 9, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL), BCOS_E_NOSUP,
                "bcos_head_rankm_grad");                                                                       /* J = 9: the dense form */
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, 6, 1.0f, NULL);            /* D % 4 */
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, 0, R, K, D, 1.0f, NULL);
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, -1, K, D, 1.0f, NULL);
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, 0, D, 1.0f, NULL);
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, -8, 1.0f, NULL);
    RANKM(cls, f, J, f, f + 1, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);        /* misaligned w */
    RANKM(cls, f, J, f, f, NULL, f + 2, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);           /* misaligned mul */
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f + 3, NULL, am, NULL, N, R, K, D, 1.0f, NULL);        /* misaligned out */
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 0, f, f + 1, am, NULL, N, R, K, D, 1.0f, NULL);           /* misaligned out2 */
    RANKM((const int64_t*)(f + 1), f, J, f, f, NULL, NULL, NULL, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);     /* misaligned cls */
    RANKM(cls, f, J, f, f, NULL, f, f, NULL, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);                  /* mul2 without out2 */
    RANKM(cls, f, J, f, f, NULL, f, NULL, f, 0, f, NULL, am, NULL, N, R, K, D, 1.0f, NULL);                  /* gate2 without out2 */
    RANKM(cls, f, J, f, f, NULL, f, NULL, NULL, 0, f, NULL, am, am, N, R, K, D, 1.0f, NULL);                 /* out2_absmax without out2 */
    RANKM(cls, f, J, f, f, NULL, NULL, NULL, NULL, 1, f, f, am, am, N, R, K, D, 1.0f, NULL);                 /* gate from an absent mul */
    RANKM(cls, f, J, f, f, NULL, f, NULL, f, 1, f, f, am, am, N, R, K, D, 1.0f, NULL);                       /* both gates */

    COT(NULL, f, f, am, N, R, K, 1.0f, NULL);
    COT(f, NULL, f, am, N, R, K, 1.0f, NULL);
    COT(f, f, NULL, am, N, R, K, 1.0f, NULL);
    COT(f, f, f, am, 0, R, K, 1.0f, NULL);
    COT(f, f, f, am, N, 0, K, 1.0f, NULL);
    COT(f, f, f, am, N, R, -5, 1.0f, NULL);
    COT(f, f, f + 1, am, N, R, K, 1.0f, NULL);                    /* glin rows are written 16 bytes at a time */
    COT(f, f, f + 2, NULL, N, R, K, 1.0f, NULL);
    COT((const float*)((const char*)f + 2), f, f, am, N, R, K, 1.0f, NULL);
    COT(f, (const float*)((const char*)f + 1), f, am, N, R, K, 1.0f, NULL);
    COT(f, f, f, (uint32_t*)((char*)am + 2), N, R, K, 1.0f, NULL);
    COT(f, f, f, am, N, R, INT32_MAX, 1.0f, NULL);                /* K rounded up to 4 leaves int32 */

    free(f); free(am); free(cls);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("bcos_head_rankm_grad, bcos_head_cotangent_grad: all refusals ok\n");
    return 0;
}
