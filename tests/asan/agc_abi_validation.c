/* Host-side argument validation of bcos_agc_clip (ABI v10) under AddressSanitizer, beside abi_validation.c: every call below must be
 * REJECTED by the library's own checks before anything is launched, so it runs without a GPU.  Exit code 0 = every call returned
 * BCOS_E_INVAL with a message and ASan saw no bad access. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
#define EXPECT_INVAL(call)                                                                                  \
    do {                                                                                                    \
        int rc_ = (call);                                                                                   \
        if (rc_ != BCOS_E_INVAL) { printf("FAIL %s -> %d (expected %d)\n", #call, rc_, BCOS_E_INVAL); ++failures; } \
        else if (strstr(bcos_last_error_string(), "bcos_agc_clip") == NULL) {                               \
            printf("FAIL %s: no error message\n", #call); ++failures; }                                     \
    } while (0)

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* buf = (float*)aligned_alloc(64, 4096);
    enum { N = 130 };                           /* three chunks of at most 64 tensors */
    bcos_agc_tensor* d = (bcos_agc_tensor*)malloc(N * sizeof(bcos_agc_tensor));
    for (int t = 0; t < N; ++t) { d[t].p = buf; d[t].g = buf; d[t].units = 4; d[t].unit_len = 8; }

    EXPECT_INVAL(bcos_agc_clip(NULL, 1, 0.01f, 1e-3f, NULL));
    EXPECT_INVAL(bcos_agc_clip(d, 0, 0.01f, 1e-3f, NULL));
    EXPECT_INVAL(bcos_agc_clip(d, -3, 0.01f, 1e-3f, NULL));
    const float bad[] = {0.0f, -0.01f, INFINITY, -INFINITY, NAN};
    for (int i = 0; i < 5; ++i) {
        EXPECT_INVAL(bcos_agc_clip(d, N, bad[i], 1e-3f, NULL));
        EXPECT_INVAL(bcos_agc_clip(d, N, 0.01f, bad[i], NULL));
    }
    /* one malformed descriptor in the LAST chunk refuses the whole list */
    d[N - 1].p = NULL;
    EXPECT_INVAL(bcos_agc_clip(d, N, 0.01f, 1e-3f, NULL));
    d[N - 1].p = buf; d[N - 1].g = NULL;
    EXPECT_INVAL(bcos_agc_clip(d, N, 0.01f, 1e-3f, NULL));
    d[N - 1].g = buf;
    const int64_t bad_units[][2] = {{0, 8}, {-1, 8}, {4, 0}, {4, -8}, {INT64_MAX, 2}, {((int64_t)1 << 62), 4}};
    for (int i = 0; i < 6; ++i) {
        d[70].units = bad_units[i][0]; d[70].unit_len = bad_units[i][1];
        EXPECT_INVAL(bcos_agc_clip(d, N, 0.01f, 1e-3f, NULL));
    }
    d[70].units = 4; d[70].unit_len = 8;
    /* units of one chunk of 64 tensors past int64, each tensor valid on its own */
    d[64].units = (int64_t)1 << 62; d[64].unit_len = 1;
    d[65].units = (int64_t)1 << 62; d[65].unit_len = 1;
    EXPECT_INVAL(bcos_agc_clip(d, N, 0.01f, 1e-3f, NULL));

    free(d);
    free(buf);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_agc_clip: all refusals ok\n");
    return 0;
}
