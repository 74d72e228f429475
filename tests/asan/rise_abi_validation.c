/* Host-side argument validation of bcos_rise_masks, bcos_prep_input_rise and bcos_rise_accumulate (ABI v12) under AddressSanitizer,
 * beside occlusion_abi_validation.c: every call below must be REJECTED by the library's own checks before anything is launched, so it
 * runs without a GPU.  Exit code 0 = every call returned the expected code with a message and ASan saw no bad access. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
#define EXPECT_CODE(call, who, code)                                                                        \
    do {                                                                                                    \
        int rc_ = (call);                                                                                   \
        if (rc_ != (code)) { printf("FAIL %s -> %d (expected %d)\n", #call, rc_, (code)); ++failures; }     \
        else if (strstr(bcos_last_error_string(), who) == NULL) {                                           \
            printf("FAIL %s: no error message\n", #call); ++failures; }                                     \
    } while (0)
#define MASKS(...) EXPECT_CODE(bcos_rise_masks(__VA_ARGS__), "bcos_rise_masks", BCOS_E_INVAL)
#define PREP(...) EXPECT_CODE(bcos_prep_input_rise(__VA_ARGS__), "bcos_prep_input_rise", BCOS_E_INVAL)
#define ACC(...) EXPECT_CODE(bcos_rise_accumulate(__VA_ARGS__), "bcos_rise_accumulate", BCOS_E_INVAL)

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    uint32_t* am = (uint32_t*)aligned_alloc(64, 4096);
    enum { N = 5, H = 10, W = 12, S = 4, T = 3 };                 /* cells of 3 x 3, 16 grid bits */
    int32_t* bank = (int32_t*)aligned_alloc(64, 128);             /* 16 * N = 80 bytes used: the host copy the accumulate call validates */
    for (int m = 0; m < N; ++m) { bank[4 * m] = 0x8421 + m; bank[4 * m + 1] = 0; bank[4 * m + 2] = m % 3; bank[4 * m + 3] = (m + 1) % 3; }
    int32_t* dev = bank;                                          /* stands in for the device bank */

    MASKS(NULL, f, N, 0, N, S, H, W, NULL);
    MASKS(dev, NULL, N, 0, N, S, H, W, NULL);
    MASKS(dev, f, 0, 0, N, S, H, W, NULL);
    MASKS(dev, f, N, -1, 2, S, H, W, NULL);
    MASKS(dev, f, N, 0, 0, S, H, W, NULL);
    MASKS(dev, f, N, 0, -2, S, H, W, NULL);
    MASKS(dev, f, N, 3, 3, S, H, W, NULL);                        /* rows [3, 6) of a bank of 5 */
    MASKS(dev, f, N, N, 1, S, H, W, NULL);
    MASKS(dev, f, N, 0x7fffffff, 0x7fffffff, S, H, W, NULL);      /* first + n past int32 */
    MASKS(dev, f, N, 0, N, 1, H, W, NULL);
    MASKS(dev, f, N, 0, N, 9, H, W, NULL);
    MASKS(dev, f, N, 0, N, S, 0, W, NULL);
    MASKS(dev, f, N, 0, N, S, H, -3, NULL);
    MASKS(dev, f, N, 0, N, S, 1 << 16, 1 << 16, NULL);            /* H * W past 2^31 - 1 */
    MASKS(dev, f, N, 0, N, S, 1 << 24, 1, NULL);                  /* 2 U reaches 2^24 */
    MASKS(dev + 1, f, N, 0, N, S, H, W, NULL);                    /* a bank that is not 16-byte aligned */

    PREP(NULL, dev, f, f, f, am, N, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, NULL, f, f, f, am, N, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, NULL, f, f, am, N, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, NULL, f, am, N, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, NULL, NULL, N, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, 0, 0, N, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, -1, 1, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, 0, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 4, 2, S, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, 0, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, 9, 6, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, S, 6, 0, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, S, 6, H, -1, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, S, 6, H, W, 5, 0, NULL);             /* Cpad < 6 */
    PREP(f, dev, f, f, f, am, N, 0, N, S, 3, H, W, 8, 1, NULL);             /* the AddInverse form: another operator */
    PREP(f, dev, f, f, f, am, N, 0, N, S, 3, H, W, 8, 0, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, S, 6, H, W, 8, 1, NULL);
    PREP(f, dev, f, f, f, am, N, 0, N, S, 6, 1 << 16, 1 << 16, 8, 0, NULL);
    PREP(f, dev + 2, f, f, f, am, N, 0, N, S, 6, H, W, 8, 0, NULL);

    ACC(NULL, dev, bank, f, N, T, S, H, W, 0.1f, NULL);
    ACC(f, NULL, bank, f, N, T, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, NULL, N, T, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, 0, T, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, -1, T, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, 0, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, -2, S, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, T, 1, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, T, 9, H, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, T, S, 0, W, 0.1f, NULL);
    ACC(f, dev, bank, f, N, T, S, H, -4, 0.1f, NULL);
    ACC(f, dev, bank, f, N, T, S, H, W, 0.0f, NULL);
    ACC(f, dev, bank, f, N, T, S, H, W, -0.1f, NULL);
    ACC(f, dev, bank, f, N, T, S, H, W, NAN, NULL);
    ACC(f, dev, bank, f, N, T, S, H, W, INFINITY, NULL);
    ACC(f, dev + 3, bank, f, N, T, S, H, W, 0.1f, NULL);          /* misaligned bank */
    ACC(f, dev, bank, f, N, T, 3, H, W, 0.1f, NULL);              /* s = 3: the rows carry bits at and above 9 */
    ACC(f, dev, bank, f, N, T, S, 8, W, 0.1f, NULL);              /* cells of 2 rows: a shift of 2 leaves them */
    ACC(f, dev, bank, f, N, T, S, H, 8, 0.1f, NULL);
    /* one bad row -- the LAST of the bank -- refuses the call: bits past s * s in either word, a shift outside its cell */
    const int32_t bad[][4] = {{1 << 16, 0, 0, 0}, {0, 1, 0, 0}, {-1, -1, 0, 0}, {1, 0, 3, 0}, {1, 0, 0, 3}, {1, 0, -1, 0}, {1, 0, 0, -1}};
    for (int i = 0; i < 7; ++i) {
        memcpy(bank + 4 * (N - 1), bad[i], 16);
        ACC(f, dev, bank, f, N, T, S, H, W, 0.1f, NULL);
        ACC(f, dev, bank, f, N, 1, S, H, W, 0.5f, NULL);
    }
    /* the axis tables of a 32768-pixel side at s = 4 do not fit the LDS: not supported, and said so */
    EXPECT_CODE(bcos_rise_accumulate(f, dev, NULL, f, N, T, S, 1 << 15, 1 << 15, 0.1f, NULL), "bcos_rise_accumulate", BCOS_E_NOSUP);

    free(bank);
    free(am);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_rise_masks, bcos_prep_input_rise, bcos_rise_accumulate: all refusals ok\n");
    return 0;
}
