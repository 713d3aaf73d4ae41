/*
 * ofdm_mi355x_channel.h -- extension of the C ABI (ofdm_mi355x.h and its other extension headers): the channel
 * between ofdm_transmit_packets and ofdm_receive_stream, and the scoring of what was received against what was
 * sent, both over device-resident buffers and both enqueued without a host round trip.
 *
 * ofdm_impair_stream is Transmission_Over_Air() (OFDM.c:635-655) for a recording of any length, with a multipath
 * FIR and a carrier frequency offset in front of the noise, and with noise that is a pure function of (seed,
 * trial, snr_index, absolute sample index): the oracle, another rank or a second call on a sub-range reproduce it.
 * ofdm_score_packets matches the records of ofdm_receive_stream to the transmitted packets by position and counts
 * the bit errors of each matched packet against its own payload words.
 *
 * ofdm_impair_stream, for u[i] = in[lead + i] (i >= -lead; u = 0 before that) and the absolute index
 * k = index0 + i of output sample i, 0 <= i < n:
 *   filter    y[i] = sum_{j < n_taps} h[j] u[i - j], accumulated from zero in ascending j with fp32 fused
 *             multiply-adds in this order:
 *                 re = fma(hr, ur, re); re = fma(-hi, ui, re); im = fma(hr, ui, im); im = fma(hi, ur, im)
 *             n_taps == 0: y = u bit for bit.  With lead = n_taps - 1 samples of history in front of every chunk
 *             but the first, a recording filtered chunk by chunk equals the recording filtered whole.
 *   rotation  cfo_hz != 0: y[i] is multiplied by exp(j 2 pi cfo_hz k 25e-9), built as ofdm_transmit_packets
 *             builds a packet's carrier offset: fp64 revolutions rev = cfo_hz k 25e-9, rev - rint(rev), cast to
 *             fp32, then the fp32 sine and cosine of pi times twice that.  The phasor is a function of k alone,
 *             never a running product, so it does not depend on where a call or a block starts.  cfo_hz == 0: no
 *             multiplication.
 *   noise     sigma = (float) sqrt(power / 10^(snr_db / 10)) for OFDM_NOISE_REAL, sigma_c =
 *             (float) sqrt(0.5 power / 10^(snr_db / 10)) per axis for OFDM_NOISE_COMPLEX (the base header's
 *             OFDM_NOISE_* values).  Philox4x32-10 with key `seed` and counter (trial low word, trial high word, b,
 *             0x5A000000 | snr_index), four Gaussians per block by the library's Box-Muller; each noisy component
 *             is one fma(radius, cosine or sine, y).
 *             REAL     sample k takes Gaussian k & 3 of block b = k >> 2, added to the real part.  For
 *                      index0 = 0 this is the stream and the arithmetic of ofdm_transmission_over_air, whose
 *                      result it equals bit for bit when `power` is that routine's mean |x|^2.
 *             COMPLEX  sample k takes Gaussians 2 (k & 1) and 2 (k & 1) + 1 of block b = k >> 1, for the real and
 *                      the imaginary part.
 *             b must fit counter word 2: index0 + n <= 2^34 (REAL), <= 2^33 (COMPLEX); no limit with
 *             OFDM_NOISE_NONE.
 *   order     filter, then rotation, then noise.
 * One kernel launch on the context's stream; the call does not synchronise.  n == 0 launches nothing.  Samples of
 * d_out outside [0, n) are never written.
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes this file
 * sees the library exactly as before.
 */
#ifndef OFDM_MI355X_CHANNEL_H
#define OFDM_MI355X_CHANNEL_H
#include "ofdm_mi355x_tx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_CHANNEL_MAX_TAPS 32
/* output samples per block and grid-stride step of the channel kernel: 256 lanes x the four samples of one
 * real-noise Philox block.  Tile boundaries sit at multiples of 4 in the absolute index k. */
#define OFDM_CHANNEL_TILE 1024
#define OFDM_K_CHANNEL 8           /* ofdm_timing_query ids after OFDM_K_TRANSMIT = 7 */
#define OFDM_K_SCORE   9

typedef struct {                   /* 64 bytes */
    double   power;                /* reference signal power P (mean |x|^2 of what the SNR refers to), >= 0 */
    double   snr_db;
    double   cfo_hz;               /* 0: no rotation, and no multiplication */
    uint64_t seed;                 /* Philox key, as everywhere else */
    uint64_t trial;                /* noise stream: counter words 0, 1 */
    int64_t  index0;               /* stream index of output sample 0 (>= 0) */
    int32_t  noise;                /* OFDM_NOISE_REAL, OFDM_NOISE_COMPLEX or OFDM_NOISE_NONE (ofdm_mi355x.h) */
    int32_t  snr_index;            /* q, 0 .. 2^24 - 1: counter word 3 = 0x5A000000 | q */
    int32_t  n_taps;               /* 0 .. OFDM_CHANNEL_MAX_TAPS; 0: no filter */
    int32_t  lead;                 /* history samples in front of d_in's first output sample, >= 0 */
} ofdm_channel_opts;

/*   taps   interleaved fp32 complex [n_taps], HOST memory (copied into the launch; required when n_taps > 0)
 *   d_in   interleaved fp32 complex [lead + n]   (device, 8-byte aligned, only read)
 *   d_out  interleaved fp32 complex [n]          (device, 8-byte aligned)
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: a NULL ctx or opts; NULL buffers with n > 0; NULL
 * taps with n_taps > 0; n < 0, lead < 0 or index0 < 0; n_taps, noise or snr_index out of range; a non-finite power,
 * snr_db or cfo_hz, or power < 0; buffers not 8-byte aligned; the noise index limits above; d_out overlapping
 * [d_in, d_in + lead + n) -- except d_out == d_in with lead == 0 and n_taps <= 1, the in-place case, which is
 * allowed. */
int ofdm_impair_stream(ofdm_ctx *ctx, const ofdm_channel_opts *opts, const float *taps,
                       const void *d_in, void *d_out, int64_t n);

typedef struct { int32_t rx_index; int32_t bit_err; } ofdm_score;     /* 8 bytes per transmitted packet */
#define OFDM_NSCORE 8   /* totals: 0 transmitted, 1 matched, 2 received (records written), 3 bits compared,
                           4 bit errors, 5 matched packets with >= 1 bit error, 6 and 7 unused (nothing is added) */

/* Scores the records of one ofdm_receive_stream call against the n_tx packets that were transmitted.
 *   d_tx_words  uint32 [n_tx][3 D], the payload words given to ofdm_transmit_packets   (device, required when n_tx > 0)
 *   d_tx_pos    int64 [n_tx], ascending: the stream index of packet k's first sample   (device, optional)
 *               NULL: pos_k = pos0 + k stride
 *   d_packets, d_count, d_bits   ofdm_receive_stream's outputs (device, required); d_count[1] records are read
 *   d_scores    ofdm_score [n_tx]                                                      (device, optional)
 *   d_totals    int64 [OFDM_NSCORE], ADDED to                                          (device, required)
 * Transmitted packet k matches the received record j with the smallest j among the d_count[1] written records
 * for which off_lo <= packet_pos_j - pos_k <= off_hi (a binary search: the records are ascending).  Then
 * rx_index = j and bit_err = the number of differing bits among the 96 D; with no match rx_index = -1 and
 * bit_err = 0.  0 <= off_lo <= off_hi and off_hi - off_lo <= 300 are required: fronts are at least 301 apart, so a
 * window holds at most one record.  The caller keeps the transmitted positions further apart than the window, so
 * that no record serves two packets; this is not checked.  False alarms are received - matched.
 * One kernel launch on the context's stream; the call does not synchronise.  n_tx == 0 still adds `received`.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: a NULL ctx, d_packets, d_count, d_bits or
 * d_totals; a NULL d_tx_words with n_tx > 0; n_tx < 0; n_data outside 1..15; a window that breaks the rule above. */
int ofdm_score_packets(ofdm_ctx *ctx, int32_t n_data,
                       const void *d_tx_words, int64_t n_tx,
                       const void *d_tx_pos, int64_t pos0, int64_t stride,
                       const void *d_packets, const void *d_count, const void *d_bits,
                       int32_t off_lo, int32_t off_hi,
                       void *d_scores, void *d_totals);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_CHANNEL_H */
