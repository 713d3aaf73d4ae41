/*
 * ofdm_mi355x_stream.h -- extension of the C ABI (ofdm_mi355x.h, ofdm_mi355x_captures.h): the reference's
 * packet detection and receiver (OFDM.c:659-771, 941-1165) over ONE device-resident recording of any
 * length, decoding every packet it holds.
 *
 * ofdm_receive_captures keeps the shape of the reference's Monte-Carlo trial: windows of exactly cap_len
 * samples, at most one packet per window.  ofdm_receive_stream takes the recording as it is -- an unknown
 * number of packets at unknown positions, idle gaps, a truncated packet at either end -- applies the
 * reference's detection rule once over the whole of it and decodes every packet found.
 *
 * The rule (n samples r[0..n), Lc = n - 47 positions; n < 48: no positions, no packets):
 *   metric     M[i] = |sum_{k<32} r[i+k] r[i+k+16]|^2 / (sum_{k<32} |r[i+k+16]|^2)^2, 0 <= i < Lc -- no
 *              conjugate, exactly as OFDM.c:659-683.
 *   crossing   M[i] > 0.75, decided without a division as 0.75 p p - |c|^2 < 0; zero power is no crossing
 *              (an all-zero idle gap has none).
 *   front      a crossing i whose previous crossing b (b = -1 when there is none) has i - b > 300.  A
 *              stream that begins inside a plateau has no front there (OFDM.c:716-741).
 *   confirmed  a front with i + 230 < Lc and a crossing at i + 230 (OFDM.c:745-760).
 *   packets    every confirmed front, in ascending position, packet_pos = i + 11 (len_RRC_rx + 1,
 *              OFDM.c:758).  The reference never takes the last front of its capture (its loop bound); a
 *              stream reports that packet too and marks it OFDM_STREAM_LAST_FRONT when its front is the
 *              largest front of the stream, confirmed or not.  Dropping the flagged packets and taking the
 *              first one left is therefore Packet_Selection on that array.
 *   decode     the receiver chain of ofdm_receive_captures from the matched filter on, at p = packet_pos,
 *              with the stream as the capture: the 21-tap RRC filter at p + 2 ii for the instants the
 *              receiver uses, coarse and fine CFO (float_cfo), one combined rotation, 64-point FFTs, LS
 *              estimate, ZF equaliser, slicer, demap, EVM and BER against the context's payload.
 *   bounds     samples outside [0, n) read as zero; OFDM_CAPTURE_OOB is set when
 *              p + 2 (nfr - 1) >= n + 20, nfr = 320 + 80 D: the recording's last packet, cut off, comes back
 *              with flags 2 | 4.  Its record follows ofdm_receive_captures' rule with n for cap_len: a data
 *              symbol wholly past the end (p + 2 (336 + 80 d) - 20 >= n) has subcarriers 0 and bits (1, 0),
 *              and the error counts say the same; a stream that ends before the long training symbols
 *              (p + 364 >= n; the front is still confirmed when n > front + 277) has S = 0 in every bin, NaN
 *              subcarriers, bits (1, 0) throughout, NaN evm_pre_sum and evm_db_pre and a finite evm_db_post,
 *              which is Receiver()'s own answer (tests/test_gpu_oob.py).
 *   input      samples must be finite: the metric slides its sums in fp32, so one NaN or infinity stays in a
 *              lane's sums for the rest of its run, where Receiver() recomputes every window.  0.75 p^2 and
 *              |c|^2 are fp32, p the sum of 32 |sample|^2: p^2 must stay inside the fp32 range, sample
 *              magnitudes between about 1e-8 and 1e8.  A recording scaled by 2^-12 or 2^12 from
 *              Transmitter()'s own level decodes bit for bit as the unscaled one.
 * Fronts are at least 301 positions apart, so a stream holds at most n / 301 + 1 of them: one slot per 301
 * positions holds at most one front (the bound to size max_packets with).
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes this
 * file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_STREAM_H
#define OFDM_MI355X_STREAM_H
#include "ofdm_mi355x_captures.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_STREAM_LAST_FRONT 4      /* ofdm_capture_result.flags bit 2: the packet of the stream's last front */
/* detection positions per block of the detection kernel.  A block stages OFDM_STREAM_TILE + 47 samples; a
 * lane owns runs of OFDM_STREAM_RUN contiguous positions whose boundaries are fixed in stream coordinates
 * (run j is [j RUN, (j + 1) RUN)), so M[i] and every crossing do not depend on the launch shape. */
#define OFDM_STREAM_RUN 31
#define OFDM_STREAM_TILE 7936         /* 256 lanes x 31 positions = 248 bitmap words */

/* kernel ids for ofdm_timing_query, after the base header's 0..3 */
#define OFDM_K_STREAM_DETECT 4
#define OFDM_K_STREAM_SELECT 5
#define OFDM_K_STREAM_DECODE 6

typedef struct {                 /* 64 bytes, one per packet */
    int64_t packet_pos;          /* front + 11, stream coordinates */
    int64_t reserved;            /* written as 0 */
    ofdm_capture_result r;       /* packet_idx = (int32) packet_pos if it fits, else -1; flags: OFDM_CAPTURE_OOB,
                                    OFDM_STREAM_LAST_FRONT; never OFDM_CAPTURE_SYNC_FAIL */
} ofdm_stream_packet;

/* Detects and decodes every packet of the n_samples interleaved fp32 complex samples at d_samples (device,
 * 8-byte aligned, only read).  opts->float_cfo means what it means in ofdm_receive_captures; matlab_slicer
 * and float_taps change nothing, as there (fp32 taps, the C slicer: zero and NaN decide "-"); cap_len and
 * fixed_start are ignored; word_stats != 0 is OFDM_E_ARG.  payload is MESSAGE or TESTER and fixes the data
 * symbols per packet, D = ofdm_payload_frames(payload).
 *   d_packets   ofdm_stream_packet[max_packets]          (device, required) ascending packet_pos
 *   d_count     int64[2]: packets found in the stream, records written = min(found, max_packets)
 *                                                        (device, required)
 *   d_bits      uint32 [max_packets][3 D], MSB-first     (device, optional)
 *   d_eq        float2 [max_packets][48 D]               (device, optional)
 *   d_counters  int64 [OFDM_NCOUNTERS], one row          (device, optional, ADDED to: exactly the reduction
 *               of the written records by the rule of ofdm_receive_captures; a non-finite evm_pre_sum is
 *               left out of EVM_PRE_Q and EVMDB_PRE_Q, as a -inf evm_db_post is out of EVMDB_POST_Q)
 *   d_metric    float  [n_samples - 47], M[i]            (device, optional; NaN where the power is zero)
 *   d_cross     uint32 [ceil((n_samples - 47) / 32)], crossing i is bit i & 31 of word i >> 5
 *                                                        (device, optional)
 * Only the first d_count[1] rows of d_packets, d_bits and d_eq are written.  When more packets are found
 * than max_packets, the first max_packets by position are decoded and the call still returns OFDM_OK.
 * n_samples < 48 writes d_count = {0, 0} and nothing else.
 * Everything is enqueued on the context's stream; the call does not synchronise, so the packet count is
 * not known on the host: the decode launch is sized from max_packets and the device and loops over
 * d_count.  The crossing bitmap and the front slots (about n_samples / 32 bytes) live in the context's
 * scratch (ofdm_ctx_scratch_bytes, ofdm_ctx_trim).  All positions are 64-bit.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: a NULL ctx, opts, d_samples (with
 * n_samples > 0), d_packets (with max_packets > 0) or d_count; n_samples < 0; max_packets < 0;
 * word_stats != 0; a payload that is not MESSAGE or TESTER; d_samples not 8-byte aligned. */
int ofdm_receive_stream(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples,
                        const ofdm_rx_opts *opts, int payload, int64_t max_packets,
                        void *d_packets, void *d_count, void *d_bits, void *d_eq,
                        void *d_counters, void *d_metric, void *d_cross);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_STREAM_H */
