/*
 * ofdm_mi355x_ppdu.h -- extension of the C ABI (ofdm_mi355x.h and the extension headers up to the punctured rates'
 * header, ofdm_mi355x_punct.h): self-describing coded packets.  A PPDU (802.11a's name for a physical-layer packet) carries
 * a header symbol in the robust rate that names the rate and the length of the rest, 802.11a's scrambler with a seed per
 * packet that the receiver recovers from the SERVICE field, and a CRC-32 frame check sequence (FCS).  One recording can
 * then mix the three rates and one decode call sorts them out per packet on the device; and the receiver can tell whether
 * a packet came out right without knowing what was sent.  Everything around the two calls stays: the transmitters, the
 * receivers, d_eq, the gains call, the scoring, the rate-taking encoder and decoder.  No existing kernel or entry point
 * changes.
 *
 * The rules (stream.ppdu_header, stream.ppdu_header_check, stream.scramble_sequence, stream.fcs32, stream.crc8,
 * stream.ppdu_encode and stream.ppdu_decode are their executable specification, exact, bit for bit):
 *   bit order  all bit strings are MSB first in uint32 words, the coded link's layout: bit 0 of a string is bit 31 of
 *              word 0, and a byte's first bit is its top bit.  This deliberately differs from 802.11's LSB-first octets.
 *   packet     D symbols, 2 <= D <= 15: one header symbol and D - 1 data symbols.  Airtime stays fixed per call.
 *   header     rate 1/2, 48 steps: 42 header bits and six zero tail bits, exactly a one-symbol rate-1/2 packet of the coded
 *              link.  The header so terminates its own trellis, and the data part starts in state 0.
 *                bits 0..3    RATE = 5 + the rate's code: 0101 and 0111 are 802.11a's QPSK 1/2 and 3/4; 0110, unused in
 *                             802.11a, stands for 2/3
 *                bit 4        reserved, 0
 *                bits 5..16   LENGTH, 12 bits: the PSDU's bytes, the 4 FCS bytes among them
 *                bit 17       even parity over bits 0..16
 *                bits 18..25  CRC-8 of bits 0..17: an 8-bit register c starts at 0xFF; per bit b in order f = b ^ (c >> 7),
 *                             c = ((c << 1) & 0xFF) ^ (f ? 0x07 : 0); the field is ~c
 *                bits 26..41  zero
 *              A header is valid only if RATE is 5, 6 or 7, bit 4 is 0, the parity and the CRC-8 are right, bits 26..41
 *              are zero and 4 <= LENGTH <= cap(D, rate).  No flip of 1, 2 or 3 of the 42 bits leaves a valid header; 21 of
 *              the 447,720 four-bit flips do.  Known answer: rate 3/4, LENGTH 123 gives word 0 = 0x703DF9C0, word 1 = 0.
 *   data       a (D - 1)-symbol packet of the punctured rates' header at the header's rate: K = S (D - 1) - 6 information
 *              bits and the six tail bits, S = 48, 64 or 72.  Before scrambling the K bits are 16 SERVICE bits (all zero),
 *              the 8 LENGTH PSDU bits and zero pad up to K.  All K bits are XORed with the scrambler sequence of the
 *              packet's seed from its first bit.  The tail is not scrambled and stays at the very end, where the decoder
 *              rule's traceback from state 0 wants it: this differs from 802.11a's tail-before-pad order.
 *              cap(D, rate) = (K - 16) div 8: 3 / 5 / 6 bytes at D = 2 (rate 1/2 holds no LENGTH there and is refused),
 *              9 / 13 / 15 at D = 3, 81 / 109 / 123 at D = 15.
 *   scrambler  802.11a's x^7 + x^4 + 1.  The state is seven bits, the seed 1..127; an output bit is x7 ^ x4 and is shifted
 *              in.  Seed 1111111 gives the standard's 127-bit sequence 00001110 11110010 11001001 ..; it repeats.  The
 *              receiver takes the first seven decoded data bits as the register's state and goes on from there: for any
 *              seed the sequence from bit 7 on is the sequence of the seed that equals output bits 0..6.  Seven zero bits
 *              are no state: "bad service", seed 0, nothing descrambled.  Descrambled SERVICE bits 7..15 must be zero,
 *              else "bad service".
 *   FCS        the PSDU's last four bytes are zlib's crc32 of the LENGTH - 4 before them, big-endian (reflected polynomial
 *              0xEDB88320, start 0xFFFFFFFF, complemented; "123456789" gives 0xCBF43926).
 *   payload    the 3 D payload words of a packet are the rate-taking encoder's 3 words of the header followed by its
 *              3 (D - 1) words of the scrambled data at the packet's rate.  The receiver's soft values and Viterbi rule are
 *              those of the punctured rates' header on d_eq's columns [0, 48) and [48, 48 D); the packet's 48 gains serve
 *              both parts.
 *
 * The device code (csrc/ofdm_ppdu.hip).  The encoder is two launches: one thread per packet writes d_info (header bits,
 * FCS by a byte table in LDS, scrambling, padding), then one thread per output word encodes, at rate 1/2 for symbol 0 and
 * at the rate the packet's header names for the others.  The decoder is one fused kernel, one wave per row with lane =
 * trellis state in the layout of the punctured rates' decode kernel.  The rate is not known at launch, so a wave's LDS
 * region is sized for the worst one: 72 (D - 1) decision words of 8 bytes and the data symbols' 96 (D - 1) soft values,
 * 8,064 + 5,376 = 13,440 bytes at D = 15; two waves per block are 26,880 bytes, six blocks and twelve waves per CU.  The
 * header costs no LDS of its own: its 48 decision words and 96 soft values lie at the head of the decision area and are
 * dead before the data part's first decision is written (kept apart they would make 14,208 and 28,416 bytes, five blocks).
 * The wave stages all soft values, runs the header's 48
 * steps, traces them back and checks the header with wave-uniform scalar code; an invalid header ends the row there.
 * Otherwise the metrics restart (state 0 = 0, the rest -inf), the S (D - 1) steps run in the branch of the packet's rate --
 * uniform within the wave, so nothing diverges; the two waves of a block may finish at different times -- and the
 * traceback leaves information word l in lane l.  The lanes find the seven state bits in the 127-bit sequence by one
 * ballot, which gives the seed and each lane's 32 sequence bits; the PSDU words are the descrambled words moved up by the
 * 16 SERVICE bits, and the FCS runs as wave-uniform code over a 256-entry table that the wave holds in four registers per
 * lane and reads with readlane.
 *
 * Timing.  The context's kernel ids are not extended: both launches of the encoder are timed under id 18 and the decoder
 * under id 20, the ids of the coded link's encoder and decoder.
 *
 * Out of scope: variable airtime (the stream receiver cuts 48 D subcarriers per record before anything is decoded),
 * ofdm_receive_captures and the frame-mode sweeps.
 *
 * The base header's function list, OFDM_ABI_VERSION and the older extension headers are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_PPDU_H
#define OFDM_MI355X_PPDU_H
#include "ofdm_mi355x_punct.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_PPDU_MIN_SYMBOLS 2
#define OFDM_PPDU_PSDU_WORDS 31      /* 124 bytes >= cap(15, 3/4) */
#define OFDM_PPDU_INFO_WORDS 36      /* 2 header words and room for 34 more; W_i(14, 3/4) = 32 are the most in use */
#define OFDM_PPDU_SERVICE_BITS 16
#define OFDM_PPDU_MIN_LENGTH 4
/* status bits */
#define OFDM_PPDU_BAD_HEADER 1
#define OFDM_PPDU_BAD_SERVICE 2
#define OFDM_PPDU_BAD_FCS 4

/* Both calls enqueue on the context's stream, do not synchronise and allocate nothing.  Their argument checks come in the
 * order of the rate-taking encoder's and decoder's, give OFDM_E_ARG with an ofdm_last_error text and come before any
 * launch: n_data (2 .. 15), n, NULL pointers, alignments, ctx. */

/* Encode n packets of n_data symbols.  d_psdu: uint32 [n][31]; d_len, d_rate (the rate's code), d_seed: int32 [n]; all on
 * the device.  d_info: uint32 [n][36], written: the 2 header words, then the data part's scrambled information words,
 * zeros behind them.  d_words: uint32 [n][3 n_data], written: the payload words for the transmitters.  The FCS is computed
 * over the first LENGTH - 4 bytes of the packet's d_psdu row and replaces whatever sits in the next four; bytes past
 * LENGTH are ignored.  Per-packet values cannot be checked on the host without a synchronisation: a packet whose rate is
 * outside 0 .. 2, whose LENGTH is outside [4, cap(n_data, rate)] or whose seed is outside [1, 127] is sent as LENGTH = 0
 * under a RATE field of 0 -- a header that fails every receiver's check -- with an all-zero data part at rate 1/2.
 * n = 0 writes nothing. */
int ofdm_ppdu_encode(ofdm_ctx *ctx, int32_t n_data, const void *d_psdu, const void *d_len, const void *d_rate,
                     const void *d_seed, int64_t n, void *d_info, void *d_words);

/* Decode rows of equalised subcarriers.  d_eq: float2 [n][48 n_data]; d_csi: optional, float [n][48]; d_count: optional,
 * int64 [2] on the device: rows = min(n, d_count[1]), else rows = n; rows past that are not written.  d_meta: int32 [n][4],
 * written: status (the OFDM_PPDU_BAD_* bits, 0 for a packet whose FCS passed), the rate's code, LENGTH, seed.  d_psdu:
 * uint32 [n][31], written: the LENGTH PSDU bytes, the FCS among them, zeros behind.  d_path: optional, float [n][2]: the
 * header's and the data part's path metric.  A row whose header is invalid gets status 1, rate -1, length 0, seed 0, a
 * zero PSDU and a data path metric of 0.  n = 0 launches nothing. */
int ofdm_ppdu_decode(ofdm_ctx *ctx, int32_t n_data, const void *d_eq, const void *d_csi, const void *d_count, int64_t n,
                     void *d_meta, void *d_psdu, void *d_path);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_PPDU_H */
