/* Host-side argument validation of bcos_prep_input_occluded and bcos_occlusion_accumulate (ABI v12) under AddressSanitizer, beside
 * abi_validation.c: every call below must be REJECTED by the library's own checks before anything is launched, so it runs without a
 * GPU.  Exit code 0 = every call returned BCOS_E_INVAL with a message and ASan saw no bad access. */
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
#define PREP(...) EXPECT_INVAL(bcos_prep_input_occluded(__VA_ARGS__), "bcos_prep_input_occluded")
#define ACC(...) EXPECT_INVAL(bcos_occlusion_accumulate(__VA_ARGS__), "bcos_occlusion_accumulate")

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    uint32_t* am = (uint32_t*)aligned_alloc(64, 4096);
    enum { N = 5, H = 8, W = 12, CL = 10 };
    int32_t* bank = (int32_t*)aligned_alloc(64, 128);             /* 16 * N = 80 bytes used: the host copy the accumulate call validates */
    for (int m = 0; m < N; ++m) { bank[4 * m] = 0; bank[4 * m + 1] = 4; bank[4 * m + 2] = m; bank[4 * m + 3] = m + 3; }
    int32_t* dev = bank;                                          /* stands in for the device bank */
    int32_t tg[3] = {1, 2, 3};

    PREP(NULL, dev, f, f, f, am, N, 6, H, W, 8, 0, NULL);
    PREP(f, NULL, f, f, f, am, N, 6, H, W, 8, 0, NULL);
    PREP(f, dev, NULL, f, f, am, N, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, NULL, f, am, N, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, NULL, NULL, N, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, 0, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, -2, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 6, 0, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 6, H, -1, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 6, H, W, 5, 0, NULL);            /* Cpad < 6 */
    PREP(f, dev, f, f, f, am, N, 3, H, W, 8, 1, NULL);            /* the AddInverse form: another operator */
    PREP(f, dev, f, f, f, am, N, 3, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 6, H, W, 8, 1, NULL);
    PREP(f, dev, f, f, f, am, N, 6, 1 << 16, 1 << 16, 8, 0, NULL);     /* H * W past 2^31 - 1 */
    PREP(f, dev + 1, f, f, f, am, N, 6, H, W, 8, 0, NULL);        /* a bank that is not 16-byte aligned */

    ACC(NULL, f, dev, bank, NULL, f, N, CL, CL, H, W, 0, NULL);
    ACC(f, NULL, dev, bank, NULL, f, N, CL, CL, H, W, 0, NULL);
    ACC(f, f, NULL, bank, NULL, f, N, CL, CL, H, W, 0, NULL);
    ACC(f, f, dev, bank, NULL, NULL, N, CL, CL, H, W, 0, NULL);
    ACC(f, f, dev, bank, NULL, f, 0, CL, CL, H, W, 0, NULL);
    ACC(f, f, dev, bank, NULL, f, -1, CL, CL, H, W, 0, NULL);
    ACC(f, f, dev, bank, NULL, f, N, 0, 0, H, W, 0, NULL);
    ACC(f, f, dev, bank, tg, f, N, CL, 0, H, W, 0, NULL);
    ACC(f, f, dev, bank, tg, f, N, CL, -3, H, W, 0, NULL);
    ACC(f, f, dev, bank, tg, f, N, CL, 3, 0, W, 0, NULL);
    ACC(f, f, dev, bank, tg, f, N, CL, 3, H, -4, 0, NULL);
    ACC(f, f, dev, bank, NULL, f, N, CL, 3, H, W, 0, NULL);       /* all classes asked for, T != CL */
    ACC(f, f, dev + 2, bank, tg, f, N, CL, 3, H, W, 0, NULL);     /* misaligned bank */
    ACC(f, f, dev, bank, tg, f, N, 1 << 30, 1 << 30, 1 << 20, 1 << 20, 0, NULL);      /* T * H * W past int64 */
    /* one bad rectangle -- the LAST of the bank -- refuses the call: empty rows, empty columns, reversed, outside the image */
    const int32_t bad[][4] = {{2, 2, 0, 3}, {0, 4, 5, 5}, {4, 0, 0, 3}, {0, 4, 7, 3}, {-1, 4, 0, 3}, {0, H + 1, 0, 3}, {0, 4, -2, 3}, {0, 4, 0, W + 1}};
    for (int i = 0; i < 8; ++i) {
        memcpy(bank + 4 * (N - 1), bad[i], 16);
        ACC(f, f, dev, bank, tg, f, N, CL, 3, H, W, 0, NULL);
        ACC(f, f, dev, bank, NULL, f, N, CL, CL, H, W, 1, NULL);
    }

    free(bank);
    free(am);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_prep_input_occluded, bcos_occlusion_accumulate: all refusals ok\n");
    return 0;
}
