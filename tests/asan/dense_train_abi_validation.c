/* Host-side argument validation of the training-mode dense-block entry points (bcos_slice_col_ws_floats, bcos_slice_batch_stats,
 * bcos_bn_reader_finish, bcos_slice_relu_bwd_colsums, bcos_slice_bn_bwd_acc; additive entry points of ABI v12) under AddressSanitizer,
 * beside dense_abi_validation.c: every call below must be REJECTED by the library's own checks before anything is launched, so it runs
 * without a GPU.  Exit code 0 = every call returned the documented code with a message and ASan saw no bad access. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
static void expect(int rc, int code, const char* fn, const char* what) {
    if (rc != code) { printf("FAIL %s: %s -> %d (expected %d)\n", fn, what, rc, code); ++failures; }
    else if (strstr(bcos_last_error_string(), fn) == NULL) { printf("FAIL %s: %s: no error message\n", fn, what); ++failures; }
}

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    float* odd = (float*)((char*)f + 2);
    int64_t n = 0;
    if (bcos_slice_col_ws_floats(4099, 32, &n) != BCOS_OK || n != 3 * 33 * 32) { printf("FAIL workspace of (4099, 32): %lld\n", (long long)n); ++failures; }
    if (bcos_slice_col_ws_floats(1, 4, &n) != BCOS_OK || n != 12) { printf("FAIL workspace of (1, 4): %lld\n", (long long)n); ++failures; }
    expect(bcos_slice_col_ws_floats(0, 32, &n), BCOS_E_INVAL, "bcos_slice_col_ws_floats", "rows = 0");
    expect(bcos_slice_col_ws_floats(4, 30, &n), BCOS_E_INVAL, "bcos_slice_col_ws_floats", "C % 4");
    expect(bcos_slice_col_ws_floats(4, 32, NULL), BCOS_E_INVAL, "bcos_slice_col_ws_floats", "NULL floats");
#define STATS(what, code, ...) expect(bcos_slice_batch_stats(__VA_ARGS__), code, "bcos_slice_batch_stats", what)
    STATS("NULL x", BCOS_E_INVAL, NULL, 64, f, f, f, 96, 4, 32, NULL);
    STATS("NULL mean", BCOS_E_INVAL, f, 64, NULL, f, f, 96, 4, 32, NULL);
    STATS("NULL var", BCOS_E_INVAL, f, 64, f, NULL, f, 96, 4, 32, NULL);
    STATS("NULL workspace", BCOS_E_INVAL, f, 64, f, f, NULL, 96, 4, 32, NULL);
    STATS("rows = 0", BCOS_E_INVAL, f, 64, f, f, f, 96, 0, 32, NULL);
    STATS("C % 4", BCOS_E_INVAL, f, 64, f, f, f, 96, 4, 30, NULL);
    STATS("pitch < C", BCOS_E_INVAL, f, 28, f, f, f, 96, 4, 32, NULL);
    STATS("pitch % 4", BCOS_E_INVAL, f, 34, f, f, f, 96, 4, 32, NULL);
    STATS("pitch < 0", BCOS_E_INVAL, f, -64, f, f, f, 96, 4, 32, NULL);
    STATS("misaligned x", BCOS_E_INVAL, f + 1, 64, f, f, f, 96, 4, 32, NULL);
    STATS("misaligned workspace", BCOS_E_INVAL, f, 64, f, f, f + 2, 96, 4, 32, NULL);
    STATS("misaligned mean", BCOS_E_INVAL, f, 64, odd, f, f, 96, 4, 32, NULL);
    STATS("small workspace", BCOS_E_INVAL, f, 64, f, f, f, 95, 4, 32, NULL);
#define FIN(what, code, ...) expect(bcos_bn_reader_finish(__VA_ARGS__), code, "bcos_bn_reader_finish", what)
    FIN("NULL var", BCOS_E_INVAL, NULL, f, f, f, f, 32, 1e-5f, 0.1f, NULL);
    FIN("NULL rstd", BCOS_E_INVAL, f, f, f, NULL, f, 32, 1e-5f, 0.1f, NULL);
    FIN("NULL g", BCOS_E_INVAL, f, f, f, f, NULL, 32, 1e-5f, 0.1f, NULL);
    FIN("C = 0", BCOS_E_INVAL, f, f, f, f, f, 0, 1e-5f, 0.1f, NULL);
    FIN("eps < 0", BCOS_E_INVAL, f, f, f, f, f, 32, -1.f, 0.1f, NULL);
    FIN("momentum > 1", BCOS_E_INVAL, f, f, f, f, f, 32, 1e-5f, 1.5f, NULL);
    FIN("misaligned running_var", BCOS_E_INVAL, f, f, odd, f, f, 32, 1e-5f, 0.1f, NULL);
#define SUMS(what, code, ...) expect(bcos_slice_relu_bwd_colsums(__VA_ARGS__), code, "bcos_slice_relu_bwd_colsums", what)
    SUMS("NULL d", BCOS_E_INVAL, NULL, f, 64, f, f, f, f, f, f, f, f, 64, 4, 32, NULL);
    SUMS("NULL x", BCOS_E_INVAL, f, NULL, 64, f, f, f, f, f, f, f, f, 64, 4, 32, NULL);
    SUMS("NULL gvec", BCOS_E_INVAL, f, f, 64, NULL, f, f, f, f, f, f, f, 64, 4, 32, NULL);
    SUMS("NULL sgx", BCOS_E_INVAL, f, f, 64, f, f, f, NULL, f, f, f, f, 64, 4, 32, NULL);
    SUMS("coef without rstd", BCOS_E_INVAL, f, f, 64, f, f, NULL, f, f, NULL, f, f, 64, 4, 32, NULL);
    SUMS("pitch < C", BCOS_E_INVAL, f, f, 28, f, f, f, f, f, f, f, f, 64, 4, 32, NULL);
    SUMS("misaligned shift", BCOS_E_INVAL, f, f, 64, f, f + 1, f, f, f, f, f, f, 64, 4, 32, NULL);
    SUMS("misaligned gw", BCOS_E_INVAL, f, f, 64, f, f, f, f, f, odd, f, f, 64, 4, 32, NULL);
    SUMS("small workspace", BCOS_E_INVAL, f, f, 64, f, f, f, f, f, f, f, f, 63, 4, 32, NULL);
    SUMS("rows < 0", BCOS_E_INVAL, f, f, 64, f, f, f, f, f, f, f, f, 64, -4, 32, NULL);
#define ACC(what, code, ...) expect(bcos_slice_bn_bwd_acc(__VA_ARGS__), code, "bcos_slice_bn_bwd_acc", what)
    ACC("NULL d", BCOS_E_INVAL, NULL, f, 64, f, f, f, f, f, 64, 4, 32, 1, NULL);
    ACC("NULL x", BCOS_E_INVAL, f, NULL, 64, f, f, f, f, f, 64, 4, 32, 1, NULL);
    ACC("NULL g", BCOS_E_INVAL, f, f, 64, f, f, f, f, NULL, 64, 4, 32, 1, NULL);
    ACC("mean without coef", BCOS_E_INVAL, f, f, 64, f, f, f, NULL, f, 64, 4, 32, 1, NULL);
    ACC("accumulate = 2", BCOS_E_INVAL, f, f, 64, f, f, f, f, f, 64, 4, 32, 2, NULL);
    ACC("g_pitch % 4", BCOS_E_INVAL, f, f, 64, f, f, f, f, f, 34, 4, 32, 1, NULL);
    ACC("misaligned mean", BCOS_E_INVAL, f, f, 64, f, f, f + 1, f, f, 64, 4, 32, 1, NULL);
    ACC("misaligned coef", BCOS_E_INVAL, f, f, 64, f, f, f, f + 1, f, 64, 4, 32, 1, NULL);
    ACC("C > 8192 on the looping form", BCOS_E_NOSUP, f, f, 0, f, f, f, f, f, 0, 4, 8196, 1, NULL);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("training-mode dense-block entry points: all refusals ok\n");
    return 0;
}
