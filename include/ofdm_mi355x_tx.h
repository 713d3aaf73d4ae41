/*
 * ofdm_mi355x_tx.h -- extension of the C ABI (ofdm_mi355x.h and its other extension headers): the reference's
 * Transmitter() (OFDM.c:467-618) over a device-resident batch of per-packet payloads, written straight into a
 * device-resident recording at per-packet positions.
 *
 * ofdm_transmitter builds one waveform for the one message the context holds and returns it to the host.
 * ofdm_transmit_packets is its batched counterpart and the stream receiver's other half: every packet carries
 * its own payload and may arrive with its own complex gain and carrier offset, which is what a recording of
 * several transmitters looks like to ofdm_receive_stream.
 *
 * A packet of D data symbols is ONE period of Transmitter() for its bits: the frame
 * [STF 160 | LTF 160 | D x (16-sample cyclic prefix + 64)] of nfr = 320 + 80 D samples (QPSK map, pilots,
 * 64-point IFFT), zero-stuffed by 2 and convolved in full with the 21-tap RRC filter,
 *     w[m] = sum_j h[j] u[m - j],  u[2 i] = frame[i], u[2 i + 1] = 0,  0 <= m < P = 2 nfr + 20,
 * accumulated tap by tap in ascending j with fp32 fused multiply-adds -- the arithmetic of ofdm_transmitter,
 * whose output is ten such periods.  The payload words have the layout of ofdm_receive_stream's and
 * ofdm_receive_captures' d_bits, so received bits can be transmitted again without leaving the device.
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes this file
 * sees the library exactly as before.
 */
#ifndef OFDM_MI355X_TX_H
#define OFDM_MI355X_TX_H
#include "ofdm_mi355x_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_TX_ACCUMULATE 1      /* ofdm_tx_opts.flags bit 0: add to d_out instead of storing */
#define OFDM_K_TRANSMIT    7      /* ofdm_timing_query id, after the stream receiver's 4..6 */

typedef struct {                  /* 16 bytes */
    int32_t conv;                 /* OFDM_CONV_C / OFDM_CONV_MATLAB, as ofdm_transmitter */
    int32_t float_taps;           /* as ofdm_transmitter: the taps are fp32 on the GPU either way */
    int32_t n_data;               /* D data symbols per packet, 1..15 */
    int32_t flags;                /* OFDM_TX_ACCUMULATE or 0 */
} ofdm_tx_opts;

/* *len = P = 2 (320 + 80 n_data) + 20, the samples of one packet.  OFDM_E_ARG for n_data outside 1..15 or a
 * NULL len. */
int ofdm_transmit_len(int32_t n_data, int32_t *len);

/* Builds n packets and writes them into the recording d_out.
 *   d_words    uint32 [n][3 D], three MSB-first words per data symbol           (device, required when n > 0)
 *   d_pos      int64 [n]: the stream index of packet k's first sample           (device, optional)
 *              NULL: pos_k = pos0 + k stride.  Positions may be negative or reach past n_out: samples outside
 *              [0, n_out) are dropped (the truncated packet at either end of a recording), and a packet that
 *              lies outside altogether writes nothing.
 *   d_gain     float2 [n], complex gain g_k                                     (device, optional: 1)
 *   d_cfo_hz   float [n], carrier offset f_k in Hz                              (device, optional: 0)
 *              Sample m of packet k is g_k exp(j 2 pi f_k m 25e-9) w_k[m]; the phase counts from the packet's
 *              own first sample, in fp64 revolutions reduced to [-1/2, 1/2] before the fp32 sine and cosine.
 *              The product g_k exp(..) is rounded to fp32 once and then multiplies w_k[m].  With both
 *              pointers NULL the samples are w_k[m] itself, with no multiplication.
 *   d_out      interleaved fp32 complex [n_out]                                 (device, 8-byte aligned)
 * Without OFDM_TX_ACCUMULATE the packet samples are stored and everything else in d_out is left untouched.
 * The caller guarantees that packets do not overlap; where they do, one of the packets wins per sample (each
 * sample is stored whole, and every store is in bounds).
 * With OFDM_TX_ACCUMULATE each sample is added to what d_out holds with fp32 atomic adds, so overlapping
 * packets (collisions) and a noise floor that is already there compose.  Floating-point addition is not
 * associative: a sample that receives one addend on any base, or two addends on a zero base, has one result;
 * a sample that receives three or more addends (two packets on a non-zero base) depends on their arrival
 * order and is NOT bit-reproducible from run to run.
 * Everything is enqueued on the context's stream (one kernel launch); the call does not synchronise.  n == 0 or
 * n_out == 0 launches nothing.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: a NULL ctx or opts; a NULL d_words with
 * n > 0; a NULL d_out with n_out > 0; n < 0 or n_out < 0; n_data outside 1..15; an unknown conv; unknown flag
 * bits; d_out not 8-byte aligned. */
int ofdm_transmit_packets(ofdm_ctx *ctx, const ofdm_tx_opts *opts,
                          const void *d_words, int64_t n,
                          const void *d_pos, int64_t pos0, int64_t stride,
                          const void *d_gain, const void *d_cfo_hz,
                          void *d_out, int64_t n_out);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_TX_H */
