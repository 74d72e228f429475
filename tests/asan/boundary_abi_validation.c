/* Host-side argument validation of bcos_boundary_conv3_grad (additive entry point of ABI v12) under AddressSanitizer, beside
 * abi_validation.c: every call below must be REJECTED by the library's own checks before anything is launched, so it runs without a
 * GPU.  Exit code 0 = every call returned the documented code with a message and ASan saw no bad access. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bcos_hip.h"

static int failures = 0;
static void expect(const bcos_boundary_conv3* a, int code, const char* what) {
    const int rc = bcos_boundary_conv3_grad(a, NULL);
    if (rc != code) { printf("FAIL %s -> %d (expected %d)\n", what, rc, code); ++failures; }
    else if (strstr(bcos_last_error_string(), "bcos_boundary_conv3_grad") == NULL) { printf("FAIL %s: no error message\n", what); ++failures; }
}

int main(void) {
    if (bcos_version() != BCOS_ABI_VERSION) { printf("ABI version mismatch\n"); return 2; }
    /* host buffers stand in for device pointers: validation never dereferences them */
    float* f = (float*)aligned_alloc(64, 4096);
    uint32_t* u = (uint32_t*)aligned_alloc(64, 4096);
    bcos_boundary_conv3 ok;
    memset(&ok, 0, sizeof ok);
    ok.g1 = f; ok.g1_absmax = u; ok.w1_f16x2 = f; ok.addend = f; ok.t3 = f; ok.out2 = f; ok.out2_absmax = u; ok.w3_f16x2 = f;
    ok.t2 = f; ok.g3 = f; ok.g3_absmax = u; ok.g3_imgmax = u; ok.g3_imgmin_c = u;
    ok.N = 2; ok.PQ = 25; ok.C1 = 64; ok.C4 = 256; ok.kh = ok.kw = ok.stride = 1; ok.contraction = BCOS_CONTRACT_F16X2; ok.b = 2.0f;
    bcos_boundary_conv3 a;

    expect(NULL, BCOS_E_INVAL, "NULL block");
#define BAD(code, what, stmt) do { a = ok; stmt; expect(&a, code, what); } while (0)
    BAD(BCOS_E_INVAL, "NULL g1", a.g1 = NULL);
    BAD(BCOS_E_INVAL, "NULL addend", a.addend = NULL);
    BAD(BCOS_E_INVAL, "NULL t3", a.t3 = NULL);
    BAD(BCOS_E_INVAL, "NULL out2", a.out2 = NULL);
    BAD(BCOS_E_INVAL, "NULL t2", a.t2 = NULL);
    BAD(BCOS_E_INVAL, "NULL g3", a.g3 = NULL);
    BAD(BCOS_E_INVAL, "N = 0", a.N = 0);
    BAD(BCOS_E_INVAL, "PQ < 0", a.PQ = -3);
    BAD(BCOS_E_INVAL, "imgmax without imgmin_c", a.g3_imgmin_c = NULL);
    BAD(BCOS_E_INVAL, "imgmin_c without imgmax", a.g3_imgmax = NULL);
    BAD(BCOS_E_INVAL, "image range without g3_absmax", a.g3_absmax = NULL);
    BAD(BCOS_E_INVAL, "mul_csc without mul_norm", a.mul_csc = f);
    BAD(BCOS_E_INVAL, "mul_csh without mul_norm", a.mul_csh = f);
    BAD(BCOS_E_NOSUP, "C1 = 128", a.C1 = 128);
    BAD(BCOS_E_NOSUP, "C4 = 512", a.C4 = 512);
    BAD(BCOS_E_NOSUP, "3 x 3", a.kh = a.kw = 3);
    BAD(BCOS_E_NOSUP, "stride 2", a.stride = 2);
    BAD(BCOS_E_NOSUP, "B = 1.5", a.b = 1.5f);
    BAD(BCOS_E_NOSUP, "bf16x3", a.contraction = BCOS_CONTRACT_BF16X3);
    BAD(BCOS_E_NOSUP, "f32", a.contraction = BCOS_CONTRACT_F32);
    BAD(BCOS_E_NOSUP, "no w1 image", a.w1_f16x2 = NULL);
    BAD(BCOS_E_NOSUP, "no w3 image", a.w3_f16x2 = NULL);
    BAD(BCOS_E_NOSUP, "no g1_absmax", a.g1_absmax = NULL);
    BAD(BCOS_E_NOSUP, "2 GiB", (a.N = 1 << 10, a.PQ = 1 << 11));
    BAD(BCOS_E_NOSUP, "N PQ past int32", (a.N = 1 << 20, a.PQ = 1 << 20));
    BAD(BCOS_E_NOSUP, "misaligned g1", a.g1 = f + 1);
    BAD(BCOS_E_NOSUP, "misaligned t3", a.t3 = f + 2);
    BAD(BCOS_E_NOSUP, "misaligned out2", a.out2 = f + 3);
    BAD(BCOS_E_NOSUP, "misaligned mul2", a.mul2 = f + 1);
    BAD(BCOS_E_NOSUP, "misaligned g3", a.g3 = f + 1);
    BAD(BCOS_E_NOSUP, "misaligned image", a.w3_f16x2 = (const char*)f + 8);
    BAD(BCOS_E_NOSUP, "misaligned maxima", a.g3_absmax = (uint32_t*)((char*)u + 2));
    BAD(BCOS_E_NOSUP, "misaligned mul_csc", (a.mul_norm = f, a.mul_csc = f + 1));
    /* the process-wide default decides a call that does not choose */
    bcos_set_contraction_mode(1);
    BAD(BCOS_E_NOSUP, "default mode bf16x3", a.contraction = BCOS_CONTRACT_DEFAULT);
    bcos_set_contraction_mode(2);

    free(u);
    free(f);
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("bcos_boundary_conv3_grad: all refusals ok\n");
    return 0;
}
