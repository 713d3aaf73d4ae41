/* ppdu_args.c -- a stand-alone driver of the argument checks of include/ofdm_mi355x_ppdu.h, for a sanitizer run of the
 * library's host code on a machine without a GPU.  Every call here must fail with OFDM_E_ARG and a message before anything
 * is launched, so no pointer is ever dereferenced and no context is needed.
 *
 * Build the library's host code instrumented (build_lib.build(out="variants/libofdm_hostsan.so", extra=["-Xarch_host",
 * "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]), as tools/sanitize.py does) and link this file
 * against it:
 *   hipcc -x c tests/host/ppdu_args.c -Iinclude -fsanitize=address,undefined -Lvariants -lofdm_hostsan
 *         -Wl,-rpath,$PWD/variants -o ppdu_args && ./ppdu_args
 * It prints the number of refusals and exits 0, or names the first call that did not behave. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "ofdm_mi355x_ppdu.h"

static int failures = 0;

static void expect(int rc, const char *want, const char *what) {
    const char *msg = ofdm_last_error();
    if (rc != OFDM_E_ARG || !msg || !strstr(msg, want)) {
        printf("FAIL %s: rc %d, message '%s', wanted '%s'\n", what, rc, msg ? msg : "(null)", want);
        ++failures;
    }
}

int main(void) {
    void *const p = (void *)(uintptr_t)0x1000; /* never dereferenced: every call fails first */
    void *const odd = (void *)(uintptr_t)0x1002, *const odd8 = (void *)(uintptr_t)0x1008, *const odd4 = (void *)(uintptr_t)0x1004;
    int n = 0;
    const int32_t bad_d[] = {1, 0, -1, 16, 1 << 30};
    for (size_t k = 0; k < sizeof bad_d / sizeof *bad_d; ++k, n += 2) {
        expect(ofdm_ppdu_encode(NULL, bad_d[k], NULL, NULL, NULL, NULL, -1, NULL, NULL), "n_data", "encode n_data");
        expect(ofdm_ppdu_decode(NULL, bad_d[k], NULL, NULL, NULL, -1, NULL, NULL, NULL), "n_data", "decode n_data");
    }
    expect(ofdm_ppdu_encode(NULL, 3, NULL, p, p, p, -1, p, p), "negative", "encode n"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, NULL, p, p, p, 4, p, p), "d_psdu is NULL", "encode d_psdu"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, NULL, p, p, 4, p, p), "d_len is NULL", "encode d_len"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, NULL, p, 4, p, p), "d_rate is NULL", "encode d_rate"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, NULL, 4, p, p), "d_seed is NULL", "encode d_seed"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 4, NULL, p), "d_info is NULL", "encode d_info"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 4, p, NULL), "d_words is NULL", "encode d_words"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, odd, p, p, p, 4, p, p), "d_psdu must", "encode d_psdu alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, odd, p, p, 4, p, p), "d_len must", "encode d_len alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, odd, p, 4, p, p), "d_rate must", "encode d_rate alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, odd, 4, p, p), "d_seed must", "encode d_seed alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 4, odd, p), "d_info must", "encode d_info alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 4, p, odd), "d_words must", "encode d_words alignment"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 4, p, p), "ctx is NULL", "encode ctx"), ++n;
    expect(ofdm_ppdu_encode(NULL, 15, p, p, p, p, INT64_MAX, p, p), "ctx is NULL", "encode ctx, huge n"), ++n;
    expect(ofdm_ppdu_encode(NULL, 3, p, p, p, p, 0, p, p), "ctx is NULL", "encode ctx, n = 0"), ++n;

    expect(ofdm_ppdu_decode(NULL, 3, NULL, NULL, NULL, -1, p, p, NULL), "negative", "decode n"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, NULL, NULL, NULL, 4, NULL, NULL, NULL), "d_eq is NULL", "decode d_eq"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, NULL, 4, NULL, p, NULL), "d_meta is NULL", "decode d_meta"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, NULL, 4, p, NULL, NULL), "d_psdu is NULL", "decode d_psdu"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, odd4, NULL, NULL, 4, p, p, NULL), "d_eq must be 8-byte", "decode d_eq alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, odd, NULL, 4, p, p, NULL), "d_csi must", "decode d_csi alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, odd4, 4, p, p, NULL), "d_count must", "decode d_count alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, NULL, 4, odd8, p, NULL), "d_meta must be 16-byte", "decode d_meta alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, NULL, 4, p, odd, NULL), "d_psdu must", "decode d_psdu alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, NULL, NULL, 4, p, p, odd), "d_path must", "decode d_path alignment"), ++n;
    expect(ofdm_ppdu_decode(NULL, 3, p, p, p, 4, p, p, p), "ctx is NULL", "decode ctx"), ++n;
    expect(ofdm_ppdu_decode(NULL, 2, p, p, p, INT64_MAX, p, p, p), "ctx is NULL", "decode ctx, huge n"), ++n;
    printf("%d refusals checked, %d failures\n", n, failures);
    return failures ? 1 : 0;
}
