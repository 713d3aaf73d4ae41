/*
 * ofdm_mi355x_detect.h -- extension of the C ABI (ofdm_mi355x.h, ofdm_mi355x_stream.h): an optional detector and
 * a threshold for the stream receiver.
 *
 * ofdm_receive_stream applies the reference's detection metric, |sum r[i+k] r[i+k+16]|^2 / p^2 -- a product without
 * a conjugate.  It reaches its plateau only while r^2 keeps a constant phase over the window: a complex multi-tap
 * channel destroys that, and a carrier offset moves the front (2 samples at -90 kHz, no front at all at 200 kHz).
 * ofdm_receive_stream_ex is ofdm_receive_stream with two options: the detector, and the threshold of either
 * detector.  OFDM_DETECT_CONJUGATE is the delay-and-correlate metric with the conjugate at the short training
 * field's true period, 32 samples at the recording's 40 MS/s; |c| is then blind to the channel's phase and to any
 * carrier offset.
 *
 * The conjugate rule (n samples r[0..n), Lc = n - 63 positions; n < 64: no positions, no packets):
 *   metric     c[i] = sum_{k<32} r[i+k] conj(r[i+k+32]),  p[i] = sum_{k<32} |r[i+k+32]|^2,
 *              M[i] = |c[i]|^2 / p[i]^2,  0 <= i < Lc.
 *   crossing   M[i] > thr, decided without a division as thr p p - |c|^2 < 0; zero power is no crossing: a power
 *              window without a non-zero sample has c = p = 0 exactly, so an all-zero idle gap has none and its
 *              M is NaN.  c and p of a position are fp32 sums of that position's own 32 terms (partial sums
 *              inside runs of OFDM_STREAM_RUN positions whose boundaries are fixed in stream coordinates), never a
 *              running difference: M[i] and every crossing are independent of the launch shape, and nothing of
 *              samples that have left the window stays in them.
 *   front, confirmed, packets, decode, bounds, input
 *              exactly ofdm_mi355x_stream.h's, with this Lc: a front is a crossing whose previous crossing is
 *              more than 300 back, confirmed by a crossing at front + 230 < Lc; packet_pos = front + 11; the
 *              OFDM_STREAM_LAST_FRONT flag, the ascending order, max_packets, OFDM_CAPTURE_OOB and the whole
 *              decode chain are unchanged.  On an unfaded noise-free stream the conjugate fronts are the
 *              reference's own (packet offset 16), so front + 11 and the + 230 confirmation carry over; the
 *              plateau is 265 positions long against the reference's 281.
 * OFDM_DETECT_REFERENCE keeps ofdm_mi355x_stream.h's metric and Lc = n - 47.
 * threshold applies to both detectors, 0 < thr < 1; the plateau of either metric sits near (snr / (1 + snr))^2,
 * 0.83 at 10 dB.  The arithmetic is fp32: h = thr * p, then fma(h, p, -|c|^2) < 0, so for one detector the
 * crossings at a larger threshold are a subset of those at a smaller one, bit for bit.
 *
 * The base header's function list, OFDM_ABI_VERSION and ofdm_mi355x_stream.h are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_DETECT_H
#define OFDM_MI355X_DETECT_H
#include "ofdm_mi355x_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_DETECT_REFERENCE 0       /* ofdm_mi355x_stream.h's metric: lag 16, no conjugate, Lc = n - 47 */
#define OFDM_DETECT_CONJUGATE 1       /* lag 32 with the conjugate, Lc = n - 63 */
#define OFDM_DETECT_THRESHOLD 0.75f   /* the default of both detectors (OFDM.c:701) */

/* ofdm_timing_query id of the conjugate detection kernel, after OFDM_K_DRAW_TAPS = 11.  The reference detector at
 * another threshold is timed under OFDM_K_STREAM_DETECT; selection and decode keep their ids. */
#define OFDM_K_STREAM_DETECT_CONJ 12

typedef struct {                 /* 32 bytes */
    int32_t detector;            /* OFDM_DETECT_* */
    float threshold;             /* 0 < threshold < 1 */
    int32_t reserved[6];         /* must be 0 */
} ofdm_stream_opts;

/* Lc, the detection positions of a stream of n_samples under `detector`: n_samples - 47 or n_samples - 63, 0 when
 * there are none (n_samples below 48 or 64, or negative).  OFDM_E_ARG (-1) for an unknown detector. */
int64_t ofdm_stream_positions(int64_t n_samples, int detector);

/* ofdm_receive_stream with a detector and a threshold.  Every argument and every output is ofdm_receive_stream's;
 * d_metric (float [Lc]) and d_cross (uint32 [ceil(Lc / 32)]) are sized by the detector's
 * Lc = ofdm_stream_positions(n_samples, sopts->detector), and a stream without positions writes d_count = {0, 0}
 * and nothing else.  sopts == NULL means {OFDM_DETECT_REFERENCE, 0.75}; with NULL or exactly those values the call
 * enqueues what ofdm_receive_stream enqueues -- the same kernels, byte-identical outputs.  Any other combination
 * replaces the detection launch alone: the selection and decode launches are ofdm_receive_stream's.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: an unknown detector; a threshold that is NaN or
 * outside (0, 1); a non-zero reserved word; and everything ofdm_receive_stream refuses. */
int ofdm_receive_stream_ex(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples,
                           const ofdm_rx_opts *opts, const ofdm_stream_opts *sopts, int payload,
                           int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq,
                           void *d_counters, void *d_metric, void *d_cross);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_DETECT_H */
