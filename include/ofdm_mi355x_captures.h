/*
 * ofdm_mi355x_captures.h -- extension of the C ABI (ofdm_mi355x.h): the reference's Receiver()
 * (OFDM.c:941-1165) over a device-resident batch of caller-supplied captures.
 *
 * ofdm_frame_sweep draws its captures inside the kernel (real-only AWGN over the clean waveform) and
 * ofdm_receiver takes one host capture per call.  ofdm_receive_captures decodes n arbitrary complex
 * captures that already sit in device memory -- recorded ones, or ones impaired by a carrier frequency
 * offset, multipath or complex noise -- one wavefront per capture, and writes one record per capture,
 * the two CFO estimates (Coarse_CFO_Estimation / Fine_CFO_Estimation, OFDM.c:773-828) included.
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes
 * this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_CAPTURES_H
#define OFDM_MI355X_CAPTURES_H
#include "ofdm_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_CAPTURE_MAX_LEN 9400     /* longest capture (15 data symbols: 9,394 samples) */
#define OFDM_CAPTURE_SYNC_FAIL 1      /* ofdm_capture_result.flags bit 0 */
#define OFDM_CAPTURE_OOB 2            /* ofdm_capture_result.flags bit 1 */

typedef struct {            /* 48 bytes, one per capture */
    int32_t packet_idx;     /* Packet_Selection result, 0 on failure (OFDM.c:752) */
    int32_t flags;          /* bit 0 sync_fail, bit 1 oob (down-sampler ran past the capture) */
    int32_t bit_err;        /* vs the context's payload (MESSAGE or TESTER), of 96 D bits */
    int32_t post_axis_err;  /* slicer axis errors (OFDM_C_EVM_POST_AXIS semantics) */
    float   evm_pre_sum;    /* sum |z - d|^2 over the 48 D equalised data subcarriers */
    float   evm_db_pre;     /* res[0] of Receiver(), OFDM.c:1126 */
    float   evm_db_post;    /* res[1], -inf when post_axis_err == 0 */
    float   ber;            /* res[2] */
    float   cfo_coarse_hz;  /* Coarse_CFO_Estimation, OFDM.c:773-804 */
    float   cfo_fine_hz;    /* Fine_CFO_Estimation, OFDM.c:806-828 */
    int32_t reserved[2];    /* written as 0 */
} ofdm_capture_result;

/* Receiver() on n captures in device memory.  Capture i is cap_len interleaved fp32 complex samples
 * starting at complex sample i * pitch of d_captures (pitch >= cap_len); the kernel only reads them.
 * cap_len = opts->cap_len, or int(0.307 x waveform length) of the payload's frame when 0 (OFDM.c:945),
 * at most OFDM_CAPTURE_MAX_LEN.  opts->float_cfo means what it means in ofdm_receiver.  matlab_slicer and
 * float_taps are accepted and change nothing, here as in ofdm_receiver: the GPU receivers filter with the fp32
 * taps (OFDM.c:32) and apply the C slicer, where a zero or NaN component decides "-" (Z > 0 fails,
 * OFDM.c:858-866); the MATLAB rule differs only for an exactly zero component, which the Tester's known answer
 * never produces.  fixed_start is ignored; word_stats != 0 is OFDM_E_ARG.  payload is MESSAGE or TESTER.
 *   d_results   ofdm_capture_result[n]            (device, required)
 *   d_bits      uint32 [n][3 D], MSB-first        (device, optional)
 *   d_eq        float2 [n][48 D]                  (device, optional)
 *   d_counters  int64 [OFDM_NCOUNTERS], one row   (device, optional, ADDED to)
 * D = ofdm_payload_frames(payload).  Samples the receiver needs past a capture's end read as zero and
 * set the oob flag; the frame still counts.  A data symbol d that lies wholly past the end
 * (packet_idx + 2 (336 + 80 d) - 20 >= cap_len) is then 64 exact zeros: its subcarriers are 0, its bits
 * (1, 0) for every pair, and bit_err, post_axis_err, evm_db_post, ber and the counters count it by that
 * same rule, as Receiver() does.  When the long training symbols themselves lie past the end
 * (packet_idx + 364 >= cap_len) the channel estimate is 0 in every bin and Z = 0 / 0: d_eq is NaN, the bits
 * are (1, 0) throughout, evm_pre_sum and evm_db_pre are NaN (Receiver()'s own answer), evm_db_post is finite.
 * Samples must be finite: the detection metric slides its sums in fp32, so one NaN or infinity stays in a
 * lane's sums for the rest of its run of positions, where Receiver() recomputes every window.  Amplitude: the
 * metric compares 0.75 p^2 with |c|^2 in fp32, p the sum of 32 |sample|^2, so p^2 must stay inside the fp32
 * range -- sample magnitudes between about 1e-8 and 1e8.  A batch scaled by 2^-12 or 2^12 from
 * Transmitter()'s own level decodes bit for bit as the unscaled one (tests/test_gpu_oob.py).
 * Each capture adds to the counters row: FRAMES 1, SYMBOLS D, BITS 96 D, EVM_TERMS 48 D, BIT_ERR
 * bit_err, FRAME_ERR (bit_err > 0), SYNC_FAIL flags & 1, OOB flags >> 1 & 1, EVM_POST_AXIS
 * post_axis_err, only when evm_pre_sum is finite EVM_PRE_Q llrint(evm_pre_sum 2^20) and EVMDB_PRE_Q
 * llrint(evm_db_pre 2^20) and, only when evm_db_post is finite, EVMDB_POST_Q llrint(evm_db_post 2^20) and
 * EVMDB_POST_FINITE 1: a non-finite term is left out of the row, never converted to an integer.  The
 * fixed-point terms are taken from the fp32 values stored in the record, so the row is exactly the
 * host-side reduction of the records whatever the launch shape.  The OFDM_C_WL_* slots are untouched.
 * The work is enqueued on the context's stream; the call does not synchronise.  n == 0 returns OFDM_OK
 * and touches nothing. */
int ofdm_receive_captures(ofdm_ctx *ctx, const void *d_captures, int64_t n, int64_t pitch,
                          const ofdm_rx_opts *opts, int payload,
                          void *d_results, void *d_bits, void *d_eq, void *d_counters);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_CAPTURES_H */
