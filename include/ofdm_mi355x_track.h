/*
 * ofdm_mi355x_track.h -- extension of the C ABI (ofdm_mi355x.h, ofdm_mi355x_stream.h, ofdm_mi355x_detect.h,
 * ofdm_mi355x_timing.h): pilot phase tracking in the stream receiver's decode.
 *
 * Every receiver of this library follows Receiver() (OFDM.c:1059-1068) in discarding the four pilots after
 * equalisation: the phase is corrected once, from the long training pair, and extrapolated over the packet.  The error
 * of the fine CFO estimate is a phase error across a lag of 64 samples; at data symbol d it has grown by
 * (112 + 80 d) / 64, about 2 at the first symbol and about 19 at the fifteenth, so on 15-symbol packets the late symbols
 * turn past the QPSK decision boundary long before noise alone would make them fail.  ofdm_receive_stream_tracked is
 * ofdm_receive_stream_timed with one more option: with OFDM_TRACK_PILOTS every data symbol is turned back by the
 * common phase its four pilots measure before anything is decided.
 *
 * The rule (stream.track_pilots is its executable specification, fp64), per packet, after the existing chain up to and
 * including the 64-point transforms, with H[k] the LS estimate and Y_d[k] the spectrum of data symbol d in the
 * reference's bin order, pilots p = {+1, +1, +1, -1} at bins {11, 25, 39, 53}:
 *   pilot sum  P_d = sum_pilots p_k Y_d[k] conj(H[k]): a maximal-ratio sum without a division, so a faded pilot bin
 *              weighs little.  On the device sum p_k L_k Y conj(S) with the training spectrum S = F(LTF1 + LTF2) and
 *              the training sign L_k: H = L S / 2, and a positive scale does not matter.
 *   phasor     u_d = P_d / |P_d|; u_d = 1 when |P_d| is 0 or P_d is not finite (a symbol wholly past the recording's
 *              end, or S = 0).  P_d is scaled by the power of two of its larger component before it is squared, so a
 *              recording scaled by 2^12 or 2^-12 gives byte-identical bits and phases, as ofdm_mi355x_stream.h
 *              promises for the untracked chain.
 *   correction z'_d[j] = (Y_d[k_j] / H[k_j]) conj(u_d) for the 48 data bins.
 *   downstream everything that used z uses z': d_eq, the slicer (the C slicer: "-" for zero or NaN), demap and d_bits,
 *              bit_err, ber, post_axis_err, evm_pre_sum = sum |z' - ref|^2 and both EVM dB fields, and the counter
 *              terms (a non-finite term is left out, as before).
 *   unchanged  detection, selection, timing, positions, flags, cfo_coarse_hz, cfo_fine_hz, max_packets and d_count.
 *   past the end  a data symbol wholly past the end has Y = 0, so u = 1 and z' = 0: bits (1, 0), counts the payload's
 *              own; its share of the record equals the untracked record's.
 *   order      all sums are in a fixed order (per lane ascending, then an xor butterfly): a packet's record does not
 *              depend on the launch shape, on max_packets or on the recording's alignment.
 *
 * When it pays.  Four pilots are a noisier phase reference than two training symbols while the extrapolation is still
 * short: tracking is for long packets and costs a little BER on 2-symbol packets.  Measured on an MI355X with
 * `ofdm_pkg.py link --packets 65536 --noise complex`, unfaded, bit errors over the bits of the matched packets without
 * -> with tracking (the matched, missed and false-alarm counts do not change; DESIGN.md K14 has the faded tables):
 *   15 data symbols   10 dB 5.2e-2 -> 3.8e-3    14 dB 5.2e-3 -> 5.6e-6 (489,346 -> 524 errors)    18 dB 6.7e-5 -> 0
 *    2 data symbols   10 dB 2.3e-3 -> 2.7e-3    14 dB 4.0e-6 -> 4.6e-6 (50 -> 58 errors)          18 dB 0 -> 0
 * On this library's own chain on the CPU (the oracle's decode at the true position, real noise at 10 dB, 64 packets):
 * 15 data symbols 3,446 -> 4 bit errors of 92,160 bits; 2 data symbols 0 -> 0 of 12,288.
 * On an MI355X the phase differs from the fp64 rule's by at most 7.3e-7 rad over the streams of
 * tests/test_gpu_track.py (614 symbols whose |P_d| is at least a quarter of its noise-free value), and the corrected
 * subcarriers by at most 7.5e-7 of the packet's largest.
 *
 * Out of scope: ofdm_receive_captures and the frame-mode sweeps (they keep discarding the pilots), and any smoothing of
 * the phase across symbols (every symbol is corrected by its own four pilots alone).
 *
 * The base header's function list, OFDM_ABI_VERSION and the older extension headers are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_TRACK_H
#define OFDM_MI355X_TRACK_H
#include "ofdm_mi355x_timing.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_TRACK_NONE 0             /* the pilots are discarded, as ofdm_receive_stream_timed */
#define OFDM_TRACK_PILOTS 1           /* every data symbol is turned back by its four pilots' common phase */

/* ofdm_timing_query id of the tracking decode kernel, after OFDM_K_STREAM_TIMING = 13 */
#define OFDM_K_STREAM_DECODE_TRACK 14

/* ofdm_receive_stream_timed with a tracking option.  Every other argument and output is ofdm_receive_stream_timed's.
 * tracking OFDM_TRACK_NONE: the call is ofdm_receive_stream_timed itself, the same launches and byte-identical
 *          outputs; d_phase must then be NULL.  OFDM_TRACK_PILOTS: the decode launch is stream_decode_track_kernel,
 *          under the timing id OFDM_K_STREAM_DECODE_TRACK, in place of the one under OFDM_K_STREAM_DECODE; every launch
 *          before it is unchanged.
 * d_phase  optional, float [max_packets][D] on the device (D: the payload's data symbols); the first d_count[1] rows
 *          are written: atan2 of P_d per data symbol, in radians, 0 where u_d = 1 by the fallback.  Allowed with
 *          OFDM_TRACK_PILOTS.
 * The call does not synchronise and allocates nothing beyond what ofdm_receive_stream_timed does.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: an unknown tracking; d_phase with OFDM_TRACK_NONE; and
 * everything ofdm_receive_stream_timed refuses. */
int ofdm_receive_stream_tracked(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples,
                                const ofdm_rx_opts *opts, const ofdm_stream_opts *sopts, int timing, int tracking,
                                int payload, int64_t max_packets, void *d_packets, void *d_count, void *d_bits,
                                void *d_eq, void *d_counters, void *d_metric, void *d_cross, void *d_timing,
                                void *d_phase);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_TRACK_H */
