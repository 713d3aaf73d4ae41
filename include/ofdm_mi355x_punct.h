/*
 * ofdm_mi355x_punct.h -- extension of the C ABI (ofdm_mi355x.h and the extension headers up to the coded link's header,
 * ofdm_mi355x_code.h): 802.11a's punctured rates 2/3 and 3/4 of the K = 7 mother code.  The coded link's header gives
 * the rate-1/2 code, its interleaver, precoding, soft values and Viterbi rule; this header changes none of them.  It adds
 * an encoder and a decoder that take a rate, so that a link sweep can ask what each rate costs in SNR.  Everything around
 * them stays: the transmitters, the receivers, d_eq, the gains call and the scoring.  No existing kernel or entry point
 * changes.
 *
 * The rules (stream.conv_encode_rate, stream.conv_soft_rate and stream.viterbi_decode_rate are their executable
 * specification, exact, bit for bit):
 *   rates      "1/2", "2/3" and "3/4" have the codes 0, 1 and 2 (OFDM_PUNCT_RATE_*).
 *   steps      a data symbol carries 96 sent bits, which is S = 48, 64 or 72 trellis steps (OFDM_PUNCT_STEPS).
 *   packet     D data symbols (1 <= D <= 15) carry S D steps: K_info = S D - 6 information bits followed by six zero tail
 *              bits.  W_i = ceil(K_info / 32) words of uint32, MSB first, the layout of the coded link's header: the
 *              unused low bits of the last word are ignored on input and written as 0 on output.  K_info is 58, 122, 954
 *              (W_i 2, 4, 30) for D = 1, 2, 15 at rate 2/3 and 66, 138, 1074 (W_i 3, 5, 34) at rate 3/4.
 *   puncturing 802.11a's patterns.  64 is a multiple of 2 and 72 a multiple of 3, so the pattern restarts at every data
 *              symbol.  With tau the step inside the symbol, rate 2/3 sends A_tau always and B_tau for even tau only
 *              (sent order A0 B0 A1 A2 B2 A3 ..); rate 3/4 sends A_tau for tau mod 3 != 2 and B_tau for tau mod 3 != 1
 *              (sent order A0 B0 A1 B2 A3 B3 A4 B5 ..).  Sent bit k (0 .. 95) of the symbol then goes through the
 *              interleaver j = 6 (k mod 16) + k / 16 and the precoding of the coded link's header.  Rate 1/2 sends
 *              every bit: that header's rule.  The free distances are 10, 6 and 5, the published values for the
 *              punctured 133/171 code.
 *   soft value a sent position's value is exactly that header's: one fp32 product with the gain, a non-finite value
 *              becomes 0, the clamp is 2^100.  The values are de-interleaved and belong at their (step, A/B) place in a
 *              row of 2 S D values; a stolen place holds +0.0f.
 *   decoder    that header's Viterbi rule over S D steps, unchanged: the state numbering, the roundings, the sign flips,
 *              the tie rule, the traceback and the path metric.  An erased value takes part as +0.0f.  No metric of the
 *              rule is ever -0.0f (the start is +0.0f or -inf, and a sum is -0.0f only if both terms are), so adding
 *              a zero of either sign leaves a candidate as it is: the kernel leaves those additions out and its bits and
 *              path metric still equal the rule.
 *
 * The device code (csrc/ofdm_punct.hip).  The encoder runs one thread per output word.  A symbol sees S + 6 = 70 or 78
 * information bits, u_SD-6 .. u_SD+S-1: more than one 64-bit register, and up to four input words; the thread holds them
 * in a 128-bit pair, forms every A and B by five shifts and XORs each and picks its 32 bits -- no serial chain over the
 * steps.  The decoder runs one wave per row with lane = state, in the layout of the coded link's decode kernel (ballot
 * decision words in LDS, ds_bpermute for the predecessors' metrics, readlane traceback).  Its LDS region per wave holds
 * the S D decision words of 8 bytes and only the 96 D sent soft values in sent order; a step reads the one or two values
 * it has and takes the stolen ones as constants.  At rate 3/4 and D = 15 that is 8,640 + 5,760 = 14,400 bytes per wave
 * (the depunctured row would take 17,280).  A block is two waves, 28,800 bytes of dynamic LDS at the most, under the
 * 64 KiB that need no function attribute: five blocks, ten waves, fit a CU's 160 KiB at rate 3/4, D = 15, where blocks of
 * four waves (57,600 bytes) would fit twice, eight waves.  W_i reaches 34, under the 64 lanes that write the words.
 *
 * Timing.  The context's kernel ids are not extended: the encoder is timed under id 18 and the decoder under id 20, the
 * ids of the coded link's encoder and decoder, whose launches they count with.
 *
 * What the rates cost.  The CPU model of the coded link's header (numpy at subcarrier level: four taps of profile 1, 0.5,
 * 0.25, 0.125, complex noise, an LS estimate from two training symbols, zero-forcing, soft values x |H|^2), 3,000
 * two-symbol packets, information bit error rates for rates 1/2 / 2/3 / 3/4 against the uncoded payload's:
 * 12 dB 8.8e-3 / 3.1e-2 / 6.0e-2 against 5.6e-2; 16 dB 7.5e-4 / 4.3e-3 / 1.3e-2 against 2.4e-2; 20 dB 6.3e-5 / 9.1e-4 /
 * 1.7e-3 against 1.0e-2 (tests/test_punct_host.py).  On a selective channel with zero-forcing a stolen bit next to a
 * faded one costs much: below 12 dB rate 3/4 decodes worse than no code at all.  The SNR axis stays per sample.
 * Figures measured on an MI355X are in DESIGN.md (K21).
 *
 * Out of scope: what the coded link's header leaves out, but for puncturing.
 *
 * The base header's function list, OFDM_ABI_VERSION and the older extension headers are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_PUNCT_H
#define OFDM_MI355X_PUNCT_H
#include "ofdm_mi355x_code.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_PUNCT_RATE_1_2 0
#define OFDM_PUNCT_RATE_2_3 1
#define OFDM_PUNCT_RATE_3_4 2
#define OFDM_PUNCT_RATES 3
#define OFDM_PUNCT_TAIL_BITS 6
/* S, K_info and W_i of rate code r and d data symbols */
#define OFDM_PUNCT_STEPS(r) ((r) == OFDM_PUNCT_RATE_1_2 ? 48 : (r) == OFDM_PUNCT_RATE_2_3 ? 64 : 72)
#define OFDM_PUNCT_INFO_BITS(d, r) (OFDM_PUNCT_STEPS(r) * (d) - OFDM_PUNCT_TAIL_BITS)
#define OFDM_PUNCT_INFO_WORDS(d, r) ((OFDM_PUNCT_INFO_BITS(d, r) + 31) / 32)

/* Both calls enqueue on the context's stream, do not synchronise and allocate nothing.  Their argument checks are those
 * of the coded link's encoder and decoder, in the same order, and in addition a rate outside 0 .. 2 gives OFDM_E_ARG,
 * with an ofdm_last_error text and before any launch.  With rate 0 they write exactly what those calls write. */

/* Encode n packets at a rate.  d_info: uint32 [n][W_i(n_data, rate)] on the device; d_words: uint32 [n][3 n_data],
 * written.  One thread per output word; an output word is a function of at most four input words.  n = 0 writes
 * nothing. */
int ofdm_punct_encode(ofdm_ctx *ctx, int32_t rate, int32_t n_data, const void *d_info, int64_t n, void *d_words);

/* Decode rows of equalised subcarriers at a rate.  d_eq: float2 [n][48 n_data]; d_csi: optional, float [n][48]; d_count:
 * optional, int64 [2] on the device: rows = min(n, d_count[1]), else rows = n; rows past that are not written.  d_info:
 * uint32 [n][W_i(n_data, rate)], written; d_path: optional, float [n], the path metric.  n = 0 launches nothing. */
int ofdm_punct_decode(ofdm_ctx *ctx, int32_t rate, int32_t n_data, const void *d_eq, const void *d_csi, const void *d_count,
                      int64_t n, void *d_info, void *d_path);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_PUNCT_H */
