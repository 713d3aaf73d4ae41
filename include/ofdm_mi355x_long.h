/*
 * ofdm_mi355x_long.h -- extension of the C ABI (ofdm_mi355x.h) for long messages: frames of up to 15
 * data symbols, such as the reference's second, 171-character message (OFDM.c:21: 15 data symbols, a
 * 30,600-sample waveform, 9,394-sample captures).
 *
 * The base header's function list and OFDM_ABI_VERSION are unchanged; a caller that never includes
 * this file sees the library exactly as before (ofdm_set_message still stops at 96 characters).
 *
 * The cap.  A frame carries at most OFDM_LONG_MAX_DATA_SYMBOLS = 15 data symbols
 * (OFDM_LONG_MSG_MAX_CHARS = 180 characters).  It is the largest frame whose matched-filter window
 * -- capture samples [p + 140, p + 2 (nfr - 1) + 10] for a frame of nfr = 320 + 80 D samples found
 * at p, 2 nfr - 131 samples -- still fits the sync kernel's per-wave capture ring: 2,909 samples for
 * 15 symbols against the 2,973 the ring keeps (16 symbols would need 3,069).  With 15 symbols the
 * sync -> symbol hand-off is exactly 16 windows per item (the LTF sum and 15 data windows).
 *
 * Long messages are a frame-mode feature: ofdm_payload_frames, ofdm_transmitter, ofdm_receiver and
 * ofdm_frame_sweep work for 9..15 symbols as they do for 1..8 (captures up to 9,400 samples).  The
 * symbol-mode entry points (ofdm_tx_frames, ofdm_rx_frames*, ofdm_txrx_frames, ofdm_set_next_tx,
 * ofdm_symbol_sweep) return OFDM_E_ARG for OFDM_PAYLOAD_MESSAGE while a message of more than 8
 * symbols is set.
 */
#ifndef OFDM_MI355X_LONG_H
#define OFDM_MI355X_LONG_H
#include "ofdm_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_LONG_MSG_MAX_CHARS 180
#define OFDM_LONG_MAX_DATA_SYMBOLS 15

/* MESSAGE payload = `msg`, 1 <= len <= OFDM_LONG_MSG_MAX_CHARS, framed as ceil(8 len / 96) data
 * symbols (Data_Generator, OFDM.c:435-465).  For len <= 96 the call is ofdm_set_message itself: the
 * same context state, kernels and results.  A later ofdm_set_message replaces a long message.
 * `frames` (optional) receives the data symbols per frame. */
int ofdm_set_long_message(ofdm_ctx *ctx, const char *msg, int32_t len, int32_t *frames);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_LONG_H */
