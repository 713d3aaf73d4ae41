/*
 * ofdm_mi355x_timing.h -- extension of the C ABI (ofdm_mi355x.h, ofdm_mi355x_stream.h, ofdm_mi355x_detect.h): fine
 * timing for the stream receiver by cross-correlation against the known long training field.
 *
 * ofdm_receive_stream and ofdm_receive_stream_ex decode every packet at packet_pos = front + 11, and the front is the
 * first position at which a sliding metric crosses its threshold: it moves with the noise and with the channel.  The
 * decode chain reads frame sample k at packet_pos + 2 k with a margin of 4 samples, so a late packet_pos pulls the
 * next symbol into the transform's window.  ofdm_receive_stream_timed is ofdm_receive_stream_ex with one more
 * option: with OFDM_TIMING_LTF every coarse packet_pos is refined against the long training field before the decode.
 *
 * The rule (n samples x[0..n), coarse position p = front + 11; stream.refine_timing is its executable specification):
 *   template   P[k] = w[394 + k], k < 128, of one period w of Transmitter()'s 40 MS/s waveform: the first long
 *              training symbol (394 = 2 * 192 + 10), cyclic on both sides, independent of the payload and of the
 *              number of data symbols; t[k] = P[k mod 128], k < 256.  The context builds it once from its own
 *              Transmitter() waveform and keeps it.
 *   candidates j = 0 .. 63 is the shift j - OFDM_TIMING_BACK: 256 samples from q = p + 322 + j (322 = 394 - 16 - 56:
 *              at the nominal offset a packet's first sample is p - 16).
 *   metric     L[j] = sum_{s<8} | sum_{k<32} x[q + 32 s + k] conj(t[32 s + k]) |^2: non-coherent over 8 segments of
 *              32 samples, so that a carrier offset of 200 kHz costs under 10 % of the peak.  Every inner sum is an
 *              fp32 chain of fused multiply-adds in ascending k, the outer one ascending in s: L does not depend on
 *              the launch shape, on max_packets or on the alignment of the recording.
 *   choice     packet_pos = p - 56 + argmax_j L[j]; the smallest j wins a tie.
 *   bounds     a packet is refined only when its whole search window lies inside the stream, p + 640 < n, and some
 *              L[j] is above 0; otherwise packet_pos = p, shift 0, quality 0 (a cut training field would drag the
 *              position).
 *   quality    L[j*] / sum_s (sum_k |t[32 s + k]|^2 sum_k |x[q* + 32 s + k]|^2), in [0, 1] by Cauchy-Schwarz per
 *              segment, invariant to the scale of the recording and of the template.
 *   unchanged  fronts are at least 301 apart and |shift| <= 56, so the records stay ascending; flags
 *              (OFDM_STREAM_LAST_FRONT from the front, OFDM_CAPTURE_OOB from the refined position by the existing
 *              rule), max_packets, d_count, ofdm_stream_packet.reserved = 0 and the whole decode chain, which runs at
 *              the refined position: packet_idx is the refined position.
 *
 * The recording's transform convention chooses the template, and the caller has to say which: ofdm_rx_opts carries no
 * convention (mode "c" decodes recordings of either one).  OFDM_TIMING_LTF takes w from Transmitter() under
 * OFDM_CONV_C and is for C-convention recordings.  OFDM_TIMING_LTF_MATLAB is the same rule word for word with w from
 * Transmitter() under OFDM_CONV_MATLAB, for recordings of that convention (ofdm_transmit_packets with
 * OFDM_CONV_MATLAB, the MATLAB tester's waveform).  The two long training symbols are each other's rotation by half
 * a period, w_matlab[394 + k] == w_c[394 + ((k + 64) mod 128)] exactly; the short training field and everything
 * before sample 320 are the same to rounding, so detection does not see the convention.  The wrong template still finds a peak,
 * a weak one in the wrong place.  stream.refine_timing in fp64 on MATLAB-convention streams of the oracle's
 * Transmitter(), C template against MATLAB template:
 *   noise-free, 0 Hz, 2 or 15 data symbols   every packet at first sample + 20 (coarse: + 16), quality 0.27 .. 0.30,
 *                                            against + 16 and 0.986 .. 1.000
 *   noise-free, +200 kHz                     positions - 38 .. + 20, 339 bit errors of 18 packets (2 symbols) and
 *                                            1,193 of 7 (15 symbols) where the coarse positions give 0, against + 16,
 *                                            quality 0.90 .. 0.91 and 0 errors
 *   14 and 25 dB, +-40 / -90 kHz             + 20 always -- the decode's 4 samples of margin all spent -- quality
 *                                            0.26 .. 0.30, against + 16 always and 0.93 .. 0.99
 * On an MI355X OFDM_TIMING_LTF_MATLAB gives the fp64 rule's position on all 84 packets of six such noisy and faded
 * streams (quality within 2.9e-7 of fp64) and decodes the noise-free 200 kHz streams at + 16 without a bit error, where
 * OFDM_TIMING_LTF makes 51 (2 symbols) and 394 (15 symbols).
 *
 * The base header's function list, OFDM_ABI_VERSION, ofdm_mi355x_stream.h and ofdm_mi355x_detect.h are unchanged; a
 * caller that never includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_TIMING_H
#define OFDM_MI355X_TIMING_H
#include "ofdm_mi355x_detect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_TIMING_NONE 0            /* packet_pos = front + 11, as ofdm_receive_stream_ex */
#define OFDM_TIMING_LTF 1             /* refined against the long training field of a C-convention recording */
#define OFDM_TIMING_LTF_MATLAB 2      /* the same rule, template of OFDM_CONV_MATLAB: for MATLAB-convention recordings */
#define OFDM_TIMING_BACK 56           /* the search reaches this many samples back from the coarse position ... */
#define OFDM_TIMING_FWD 8             /* ... and up to this many forward, exclusive: shifts -56 .. +7 */

/* ofdm_timing_query id of the timing kernel, after OFDM_K_STREAM_DETECT_CONJ = 12 */
#define OFDM_K_STREAM_TIMING 13

typedef struct {                 /* 16 bytes, one per record */
    int64_t coarse_pos;          /* front + 11, what packet_pos would be without timing */
    float quality;               /* [0, 1]; 0 when the packet was not refined */
    int32_t shift;               /* packet_pos - coarse_pos, -56 .. +7 */
} ofdm_stream_timing;

/* ofdm_receive_stream_ex with a timing option.  Every other argument and output is ofdm_receive_stream_ex's.
 * timing   OFDM_TIMING_NONE: the call is ofdm_receive_stream_ex itself, the same launches and byte-identical
 *          outputs; d_timing must then be NULL.  OFDM_TIMING_LTF: one more launch between the selection and the
 *          decode, under the timing id OFDM_K_STREAM_TIMING, rewrites packet_pos of the first d_count[1] records
 *          by the rule above.  OFDM_TIMING_LTF_MATLAB: the same kernel launched under the same id with the
 *          MATLAB convention's template.
 * d_timing optional, ofdm_stream_timing [max_packets] on the device; the first d_count[1] rows are written.  Allowed
 *          with OFDM_TIMING_LTF and OFDM_TIMING_LTF_MATLAB.
 * The call does not synchronise and allocates nothing, except that a context's first call with OFDM_TIMING_LTF and
 * its first with OFDM_TIMING_LTF_MATLAB each build their template (Transmitter() once, and a wait for it); the context
 * keeps both, and neither disturbs the other.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: an unknown timing; d_timing with OFDM_TIMING_NONE;
 * and everything ofdm_receive_stream_ex refuses. */
int ofdm_receive_stream_timed(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples,
                              const ofdm_rx_opts *opts, const ofdm_stream_opts *sopts, int timing, int payload,
                              int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq,
                              void *d_counters, void *d_metric, void *d_cross, void *d_timing);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_TIMING_H */
