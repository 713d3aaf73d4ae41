/*
 * stream_caller.c -- a C program decoding a recording through include/ofdm_mi355x.h and
 * include/ofdm_mi355x_stream.h only: Transmitter() and Transmission_Over_Air() build the
 * base stream zeros(700) | wave | zeros(1500) | wave[:3 frames] | zeros(400), ofdm_receive_stream finds and
 * decodes every packet in it.  Test infrastructure (tests/test_c_stream_caller.py): gcc compiles it against
 * the two headers, and on a GPU the packet list it prints equals Engine.receive_stream's on the stream it
 * wrote.  The three HIP runtime calls it needs for the device buffers are declared here, not included.
 *
 * usage: stream_caller OUT_DIR
 *   OUT_DIR/stream.bin    the recording (interleaved fp32)
 *   OUT_DIR/packets.txt   line 1: found written; then per packet: packet_pos flags packet_idx bit_err
 *                         post_axis_err evm_pre_sum evm_db_pre ber cfo_coarse_hz cfo_fine_hz bit words...
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ofdm_mi355x.h"
#include "ofdm_mi355x_stream.h"

_Static_assert(sizeof(ofdm_stream_packet) == 64, "ofdm_stream_packet is 64 bytes");
_Static_assert(offsetof(ofdm_stream_packet, r) == 16, "the record follows packet_pos and reserved");
_Static_assert(OFDM_STREAM_TILE == 256 * OFDM_STREAM_RUN && OFDM_STREAM_TILE % 32 == 0, "tile = 256 runs, whole words");

/* the HIP runtime (libamdhip64): device buffers for the recording and the results */
int hipMalloc(void **ptr, size_t size);
int hipFree(void *ptr);
int hipMemcpy(void *dst, const void *src, size_t size, int kind);
enum { H2D = 1, D2H = 2 };

#define WAVE_LEN 9800
#define PERIOD 980
#define N_SAMPLES (700 + WAVE_LEN + 1500 + 3 * PERIOD + 400)
#define MAX_PACKETS (N_SAMPLES / 301 + 1)

static int fail(const char *what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, ofdm_last_error());
    return 1;
}

int main(int argc, char **argv) {
    const char *out = argc > 1 ? argv[1] : ".";
    char path[4096];
    ofdm_ctx *ctx = NULL;
    int rc = ofdm_ctx_create(0, &ctx);
    if (rc) return fail("ofdm_ctx_create", rc);
    static float tx[2 * WAVE_LEN], ota[2 * WAVE_LEN], rec[2 * N_SAMPLES];
    int32_t len = 0, nd = 0;
    if ((rc = ofdm_transmitter(ctx, OFDM_CONV_C, OFDM_PAYLOAD_MESSAGE, 1, tx, WAVE_LEN, &len))) return fail("ofdm_transmitter", rc);
    if (len != WAVE_LEN) return fail("waveform length", len);
    if ((rc = ofdm_payload_frames(ctx, OFDM_PAYLOAD_MESSAGE, &nd))) return fail("ofdm_payload_frames", rc);
    if ((rc = ofdm_transmission_over_air(ctx, tx, ota, len, 14.0, 0x80211A, 0, 0))) return fail("ofdm_transmission_over_air", rc);
    memcpy(rec + 2 * 700, ota, sizeof(float) * 2 * WAVE_LEN);
    memcpy(rec + 2 * (700 + WAVE_LEN + 1500), ota, sizeof(float) * 2 * 3 * PERIOD);
    snprintf(path, sizeof path, "%s/stream.bin", out);
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(rec, sizeof(float), 2 * N_SAMPLES, f) != 2 * N_SAMPLES) { perror(path); return 1; }
    fclose(f);

    void *d_x = NULL, *d_pk = NULL, *d_cnt = NULL, *d_bits = NULL;
    const size_t bits_bytes = sizeof(uint32_t) * MAX_PACKETS * 3 * (size_t)nd;
    if (hipMalloc(&d_x, sizeof rec) || hipMalloc(&d_pk, sizeof(ofdm_stream_packet) * MAX_PACKETS) ||
        hipMalloc(&d_cnt, 2 * sizeof(int64_t)) || hipMalloc(&d_bits, bits_bytes) || hipMemcpy(d_x, rec, sizeof rec, H2D)) {
        fprintf(stderr, "device buffers failed\n");
        return 1;
    }
    const ofdm_rx_opts opts = {0, 1, 0, 1, -1, 0, {0, 0}};
    /* the argument checks come first */
    if (ofdm_receive_stream(ctx, d_x, -1, &opts, OFDM_PAYLOAD_MESSAGE, MAX_PACKETS, d_pk, d_cnt, NULL, NULL, NULL, NULL, NULL) != OFDM_E_ARG ||
        ofdm_receive_stream(ctx, d_x, N_SAMPLES, &opts, OFDM_PAYLOAD_RANDOM, MAX_PACKETS, d_pk, d_cnt, NULL, NULL, NULL, NULL, NULL) != OFDM_E_ARG ||
        ofdm_receive_stream(ctx, d_x, N_SAMPLES, &opts, OFDM_PAYLOAD_MESSAGE, MAX_PACKETS, d_pk, NULL, NULL, NULL, NULL, NULL, NULL) != OFDM_E_ARG) {
        fprintf(stderr, "a bad argument was accepted\n");
        return 1;
    }
    if ((rc = ofdm_receive_stream(ctx, d_x, N_SAMPLES, &opts, OFDM_PAYLOAD_MESSAGE, MAX_PACKETS, d_pk, d_cnt, d_bits, NULL, NULL,
                                  NULL, NULL)))
        return fail("ofdm_receive_stream", rc);
    if ((rc = ofdm_ctx_synchronize(ctx))) return fail("ofdm_ctx_synchronize", rc);
    int64_t cnt[2] = {-1, -1};
    static ofdm_stream_packet pk[MAX_PACKETS];
    static uint32_t words[MAX_PACKETS * 3 * 15];                  /* at most 15 data symbols per packet */
    if (hipMemcpy(cnt, d_cnt, sizeof cnt, D2H) || cnt[1] < 0 || cnt[1] > MAX_PACKETS ||
        hipMemcpy(pk, d_pk, sizeof(ofdm_stream_packet) * (size_t)cnt[1], D2H) || hipMemcpy(words, d_bits, bits_bytes, D2H)) {
        fprintf(stderr, "read-back failed\n");
        return 1;
    }
    snprintf(path, sizeof path, "%s/packets.txt", out);
    f = fopen(path, "w");
    if (!f) { perror(path); return 1; }
    fprintf(f, "%lld %lld\n", (long long)cnt[0], (long long)cnt[1]);
    for (int64_t k = 0; k < cnt[1]; ++k) {
        const ofdm_capture_result *r = &pk[k].r;
        fprintf(f, "%lld %d %d %d %d %.9g %.9g %.9g %.9g %.9g", (long long)pk[k].packet_pos, r->flags, r->packet_idx, r->bit_err,
                r->post_axis_err, r->evm_pre_sum, r->evm_db_pre, r->ber, r->cfo_coarse_hz, r->cfo_fine_hz);
        for (int w = 0; w < 3 * nd; ++w) fprintf(f, " %u", words[k * 3 * nd + w]);
        fputc('\n', f);
    }
    fclose(f);
    /* the bitmap and the front slots are scratch of the context */
    int64_t held = 0, released = -1;
    if ((rc = ofdm_ctx_scratch_bytes(ctx, &held))) return fail("ofdm_ctx_scratch_bytes", rc);
    if ((rc = ofdm_ctx_trim(ctx, &released))) return fail("ofdm_ctx_trim", rc);
    if (held < (N_SAMPLES - 47) / 8 || released != held) {
        fprintf(stderr, "scratch: held %lld, released %lld\n", (long long)held, (long long)released);
        return 1;
    }
    hipFree(d_x); hipFree(d_pk); hipFree(d_cnt); hipFree(d_bits);
    if ((rc = ofdm_ctx_destroy(ctx))) return fail("ofdm_ctx_destroy", rc);
    return nd == 2 && cnt[0] >= 1 ? 0 : 1;
}
