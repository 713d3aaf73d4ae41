/*
 * ofdm_mi355x_fading.h -- extension of the C ABI (ofdm_mi355x.h and its other extension headers): a channel of its
 * own for every packet of ofdm_transmit_packets, and Rayleigh taps drawn on the device to feed it.
 *
 * ofdm_impair_stream filters a whole recording with ONE FIR, so every packet of a link sweep sees the same
 * channel realisation.  A fading link gives every packet its own: ofdm_transmit_faded is ofdm_transmit_packets
 * with a per-packet FIR of up to 32 taps between the packet and its gain and carrier offset -- each transmitter
 * reaches the receiver through its own path, and collisions compose in accumulate mode.  ofdm_draw_taps fills the
 * tap table with independent complex Gaussians of a caller-given power delay profile.
 *
 * Packet k of D data symbols and n_taps taps h_k is n_taps - 1 samples longer than ofdm_transmit_packets':
 *     v_k[m] = sum_{l < n_taps} h_k[l] w_k[m - l],   0 <= m < P + n_taps - 1,   P = 2 (320 + 80 D) + 20,
 * where w_k is the packet ofdm_transmit_packets builds from the same words (ofdm_mi355x_tx.h) and is zero outside
 * [0, P).  Every v_k[m] accumulates from zero over all n_taps taps in ascending l with the four fp32 fused
 * multiply-adds per tap in the order ofdm_mi355x_channel.h writes down,
 *     re = fma(hr, wr, re); re = fma(-hi, wi, re); im = fma(hr, wi, im); im = fma(hi, wr, im),
 * so v_k equals, bit for bit, what ofdm_impair_stream (OFDM_NOISE_NONE, cfo_hz 0, taps h_k, lead 0, index0 0) makes
 * of [w_k | n_taps - 1 zeros].  Gain and carrier offset then apply to v_k[m] exactly as ofdm_transmit_packets applies
 * them to w_k[m]: sample m is g_k exp(j 2 pi f_k m 25e-9) v_k[m], the phase counted from the packet's first sample
 * and m running to P + n_taps - 2.
 *
 * The taps are spaced by the recording's 25 ns, so OFDM_FADE_MAX_TAPS = 32 spans 775 ns, inside the 800 ns cyclic
 * prefix.
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes this file
 * sees the library exactly as before.
 */
#ifndef OFDM_MI355X_FADING_H
#define OFDM_MI355X_FADING_H
#include "ofdm_mi355x_channel.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_FADE_MAX_TAPS 32
#define OFDM_K_FADE      10       /* ofdm_timing_query ids after OFDM_K_SCORE = 9 */
#define OFDM_K_DRAW_TAPS 11

/* *len = P + n_taps - 1 with P = 2 (320 + 80 n_data) + 20, the samples of one faded packet.  OFDM_E_ARG for n_data
 * outside 1..15, n_taps outside 1..OFDM_FADE_MAX_TAPS or a NULL len. */
int ofdm_faded_len(int32_t n_data, int32_t n_taps, int32_t *len);

/* Rayleigh taps for n packets.
 *   pdp      float [n_taps], HOST memory: the power of each tap, finite and >= 0.  The library does not normalise it.
 *   d_taps   float2 [n][n_taps]                                                  (device, 8-byte aligned)
 * Tap l of packet k is h = a_l (z[2 (l & 1)], z[2 (l & 1) + 1]) with a_l = (float) sqrt(pdp[l] / 2), computed on the
 * host in double, and z the four Gaussians (the library's Box-Muller) of the Philox4x32-10 block with key `seed` and
 * counter (low word of index0 + k, high word of index0 + k, l >> 1, 0xC4A00000); each component is one fp32
 * multiply.  A tap is a function of (seed, index0 + k, l) alone: a sub-range, another rank or a second call
 * reproduce it.  For n_taps = 4 and pdp = 1/4 each these are the taps of symbol mode's OFDM_CHAN_RAYLEIGH4 channel
 * for frame index0 + k -- the same constant, blocks and order (no entry point dumps those, so this holds by
 * construction, not by a test).
 * One kernel launch on the context's stream; the call does not synchronise.  n == 0 launches nothing.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: a NULL ctx or pdp; a NULL d_taps with n > 0;
 * n < 0; n_taps outside 1..OFDM_FADE_MAX_TAPS; a pdp entry that is negative or not finite; d_taps not 8-byte
 * aligned. */
int ofdm_draw_taps(ofdm_ctx *ctx, uint64_t seed, uint64_t index0, int64_t n, int32_t n_taps,
                   const float *pdp, void *d_taps);

/* ofdm_transmit_packets through a FIR per packet.  opts, d_words, n, d_pos, pos0, stride, d_gain, d_cfo_hz, d_out
 * and n_out mean what they mean there, on packets of P + n_taps - 1 samples:
 *   d_taps   float2 [n][n_taps], packet k's taps h_k                             (device, 8-byte aligned, required)
 *   n_taps   1 .. OFDM_FADE_MAX_TAPS
 * Store mode, accumulate mode (OFDM_TX_ACCUMULATE), the dropping of samples outside [0, n_out), the caller's
 * no-overlap rule in store mode (the n_taps - 1 tail samples are stored too) and the reproducibility statement for
 * the atomic adds are those of ofdm_transmit_packets.
 * Everything is enqueued on the context's stream (one kernel launch); the call does not synchronise.  n == 0 or
 * n_out == 0 launches nothing.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: every case of ofdm_transmit_packets; a NULL
 * d_taps with n > 0; n_taps out of range; d_taps not 8-byte aligned. */
int ofdm_transmit_faded(ofdm_ctx *ctx, const ofdm_tx_opts *opts,
                        const void *d_words, int64_t n,
                        const void *d_pos, int64_t pos0, int64_t stride,
                        const void *d_gain, const void *d_cfo_hz,
                        const void *d_taps, int32_t n_taps,
                        void *d_out, int64_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_FADING_H */
