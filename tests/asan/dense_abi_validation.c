/* Host-side argument validation of bcos_slice_affine_rows / bcos_slice_affine_bwd_acc (additive entry points of ABI v12) under
 * AddressSanitizer, beside abi_validation.c: every call below must be REJECTED by the library's own checks before anything is launched,
 * so it runs without a GPU.  Exit code 0 = every call returned the documented code with a message and ASan saw no bad access. */
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
    uint32_t* u = (uint32_t*)aligned_alloc(64, 4096);
#define ROWS(what, code, ...) expect(bcos_slice_affine_rows(__VA_ARGS__), code, "bcos_slice_affine_rows", what)
    ROWS("NULL x", BCOS_E_INVAL, NULL, 64, f, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("NULL y", BCOS_E_INVAL, f, 64, f, f, f, NULL, 64, u, 4, 32, 1, NULL);
    ROWS("rows = 0", BCOS_E_INVAL, f, 64, f, f, f, f, 64, u, 0, 32, 1, NULL);
    ROWS("rows < 0", BCOS_E_INVAL, f, 64, f, f, f, f, 64, u, -4, 32, 1, NULL);
    ROWS("C = 0", BCOS_E_INVAL, f, 64, f, f, f, f, 64, u, 4, 0, 1, NULL);
    ROWS("C % 4", BCOS_E_INVAL, f, 64, f, f, f, f, 64, u, 4, 30, 1, NULL);
    ROWS("relu = 2", BCOS_E_INVAL, f, 64, f, f, f, f, 64, u, 4, 32, 2, NULL);
    ROWS("x_pitch < C", BCOS_E_INVAL, f, 28, f, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("x_pitch % 4", BCOS_E_INVAL, f, 34, f, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("x_pitch < 0", BCOS_E_INVAL, f, -64, f, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("y_pitch < C", BCOS_E_INVAL, f, 64, f, f, f, f, 16, u, 4, 32, 1, NULL);
    ROWS("y_pitch % 4", BCOS_E_INVAL, f, 64, f, f, f, f, 66, u, 4, 32, 1, NULL);
    ROWS("misaligned x", BCOS_E_INVAL, f + 1, 64, f, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("misaligned scale", BCOS_E_INVAL, f, 64, f + 2, f, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("misaligned shift", BCOS_E_INVAL, f, 64, f, f + 3, f, f, 64, u, 4, 32, 1, NULL);
    ROWS("misaligned mul", BCOS_E_INVAL, f, 64, f, f, f + 1, f, 64, u, 4, 32, 1, NULL);
    ROWS("misaligned y", BCOS_E_INVAL, f, 64, f, f, f, f + 1, 64, u, 4, 32, 1, NULL);
    ROWS("misaligned maxima", BCOS_E_INVAL, f, 64, f, f, f, f, 64, (uint32_t*)((char*)u + 2), 4, 32, 1, NULL);
    ROWS("C > 8192 on the looping form", BCOS_E_NOSUP, f, 0, f, f, f, f, 0, u, 4, 8196, 1, NULL);
#define BWD(what, code, ...) expect(bcos_slice_affine_bwd_acc(__VA_ARGS__), code, "bcos_slice_affine_bwd_acc", what)
    BWD("NULL d", BCOS_E_INVAL, NULL, f, 64, f, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("NULL g", BCOS_E_INVAL, f, f, 64, f, f, NULL, 64, 4, 32, 1, 1, NULL);
    BWD("relu without x", BCOS_E_INVAL, f, NULL, 64, f, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("rows = 0", BCOS_E_INVAL, f, f, 64, f, f, f, 64, 0, 32, 1, 1, NULL);
    BWD("C % 4", BCOS_E_INVAL, f, f, 64, f, f, f, 64, 4, 6, 1, 1, NULL);
    BWD("relu = -1", BCOS_E_INVAL, f, f, 64, f, f, f, 64, 4, 32, -1, 1, NULL);
    BWD("accumulate = 2", BCOS_E_INVAL, f, f, 64, f, f, f, 64, 4, 32, 1, 2, NULL);
    BWD("x_pitch < C", BCOS_E_INVAL, f, f, 28, f, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("g_pitch % 4", BCOS_E_INVAL, f, f, 64, f, f, f, 34, 4, 32, 1, 1, NULL);
    BWD("misaligned d", BCOS_E_INVAL, f + 1, f, 64, f, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("misaligned x", BCOS_E_INVAL, f, f + 1, 64, f, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("misaligned g", BCOS_E_INVAL, f, f, 64, f, f, f + 2, 64, 4, 32, 1, 1, NULL);
    BWD("misaligned scale", BCOS_E_INVAL, f, f, 64, f + 1, f, f, 64, 4, 32, 1, 1, NULL);
    BWD("misaligned shift", BCOS_E_INVAL, f, f, 64, f, f + 1, f, 64, 4, 32, 1, 1, NULL);
    BWD("C > 8192 on the looping form", BCOS_E_NOSUP, f, f, 0, f, f, f, 0, 4, 8196, 1, 1, NULL);
    free(u);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_slice_affine_rows / bcos_slice_affine_bwd_acc: all refusals ok\n");
    return 0;
}
