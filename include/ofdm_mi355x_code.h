/*
 * ofdm_mi355x_code.h -- extension of the C ABI (ofdm_mi355x.h and the stream receiver's extension headers up to
 * ofdm_mi355x_diversity.h): the coded link.  802.11a's mother code -- K = 7, rate 1/2, generators 133 and 171 (octal)
 * -- as a layer over what the library already exchanges: payload words go in (ofdm_transmit_packets' d_words,
 * [n][3 D] uint32, MSB first) and equalised subcarriers come out (the stream receivers' d_eq, [rows][48 D] float2).
 * Under Rayleigh fading what the stream receiver's options leave of the loss is the fade itself; diversity
 * (ofdm_mi355x_diversity.h) is one lever against it and this code the other.  No existing kernel or entry point changes.
 *
 * The rules (stream.conv_encode, stream.conv_soft, stream.viterbi_decode and stream.channel_gain are their executable
 * specification; the first three are exact, bit for bit):
 *   packet     D data symbols (1 <= D <= 15) carry 48 D trellis steps: K_info = 48 D - 6 information bits followed by
 *              six zero tail bits, so the trellis starts and ends in state 0.  Information bits travel in words of
 *              uint32, MSB first, W_i = ceil(K_info / 32) words per packet (2, 3 and 23 for D = 1, 2 and 15); the unused
 *              low bits of the last word are ignored on input and written as 0 on output.
 *   encoder    A_t = u_t ^ u_t-2 ^ u_t-3 ^ u_t-5 ^ u_t-6,  B_t = u_t ^ u_t-1 ^ u_t-2 ^ u_t-3 ^ u_t-6,  u_t = 0 for t < 0;
 *              the coded sequence is c[2 t] = A_t, c[2 t + 1] = B_t.
 *   interleaver per data symbol, 802.11a's first permutation for N_CBPS = 96 (the second is the identity for QPSK):
 *              coded bit k of the symbol goes to position j = 6 (k mod 16) + k / 16.
 *   precoding  the reference's QPSK map has re > 0 iff b0 == b1 and im > 0 iff b0 == 0 -- not a Gray map: b1 depends on
 *              both axes.  With g the interleaved bits, subcarrier m gets the payload bits b[2 m] = g[2 m] and
 *              b[2 m + 1] = g[2 m] ^ g[2 m + 1], so that im > 0 iff g[2 m] = 0 and re > 0 iff g[2 m + 1] = 0: one coded
 *              bit per axis.  The transmitters and their map are untouched.
 *   soft value for record i, data symbol d, position j and subcarrier m = j >> 1: z = eq[i][48 d + m]; w = csi[i][m], or
 *              1 without gains; v = Im z for even j and Re z for odd j; lam = w v as one fp32 product; a non-finite lam
 *              becomes 0; |lam| is clamped to 2^100, so that 1,440 of them cannot overflow; positive means bit 0.  The
 *              gains matter: zero-forcing makes a faded bin's value large and wrong, and an unweighted soft decoder is
 *              then worse than a hard one.
 *   decoder    a Viterbi decoder over the 64 states with a correlation metric that is maximised.  State
 *              s = u_t-1 << 5 | u_t-2 << 4 | .. | u_t-6; the new state s' = u_t << 5 | s >> 1 has the predecessors
 *              p0 = (2 s') & 63 and p1 = p0 | 1.  Initial metrics 0 for state 0 and -inf for the others.  Per step and
 *              new state the two candidates c_p = M[p] + ((+-lam[2 t]) + (+-lam[2 t + 1])), "-" where the branch's coded
 *              bit is 1; the inner sum is rounded to fp32 first, then the outer one; the signs are sign flips, so no
 *              product and no FMA occurs.  p1 wins iff c_p1 > c_p0; a tie takes p0.  Traceback starts from state 0
 *              after the last step; the final metric of state 0 is the path metric.  Every rounding and the tie are
 *              fixed, so the kernel's bits and path metric equal the fp32 rule exactly.
 *   gains      csi[i][m] = sum_b |H_b[bin(m)]|^2 over the branches, H_b = L S_b / 2 and S_b = F(LTF1 + LTF2)_b exactly as
 *              ofdm_mi355x_diversity.h defines them (G[k] there), in d_eq's data-subcarrier order.  Each branch is staged
 *              and matched-filtered as the decode does, over the frame instants 192 .. 319 only, and rotated by
 *              fc + ff read from the record -- (double) cfo_coarse_hz + (double) cfo_fine_hz; nothing is re-estimated.
 *              Samples outside [0, n_samples) read as zero; an all-zero training field gives 0.
 *
 * What it is worth.  A CPU model (numpy at subcarrier level, not the waveform chain): complex noise, an LS estimate from
 * two training symbols, zero-forcing, four taps of profile 1, 0.5, 0.25, 0.125 at 40 MS/s, 6,000 two-symbol packets, bit
 * error rates on the 90 information bits, uncoded / soft unweighted / hard decisions / soft x |H|^2: 14 dB 2.9e-2 /
 * 2.7e-2 / 1.9e-2 / 4.7e-3; 20 dB 7.3e-3 / 3.8e-3 / 1.5e-3 / 2.3e-4; 26 dB 1.9e-3 / 7.4e-4 / 1.6e-4 / 0 of 540,000.
 * Without the precoding the code loses a factor of 15 at 6 dB AWGN (3.1e-3 against 2.1e-4).  The SNR axis stays per
 * sample: at equal SNR a coded packet carries (48 D - 6) / 96 D of the bits.  Figures measured on an MI355X are in
 * DESIGN.md (K18 to K20).
 *
 * Out of scope: the scrambler, puncturing (rates 2/3 and 3/4), the SIGNAL field, interleaving across packets,
 * ofdm_receive_captures and the frame-mode sweeps, and hard-decision input.
 *
 * The base header's function list, OFDM_ABI_VERSION and the older extension headers are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_CODE_H
#define OFDM_MI355X_CODE_H
#include "ofdm_mi355x_diversity.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_CODE_TAIL_BITS 6
#define OFDM_CODE_MAX_DATA_SYMBOLS 15 /* the stream receiver's longest packet (ofdm_mi355x_long.h) */
/* K_info and W_i of a packet of d data symbols */
#define OFDM_CODE_INFO_BITS(d) (48 * (d) - OFDM_CODE_TAIL_BITS)
#define OFDM_CODE_INFO_WORDS(d) ((OFDM_CODE_INFO_BITS(d) + 31) / 32)

/* ofdm_timing_query ids of the three kernels, after 17, the last of ofdm_mi355x_diversity.h */
#define OFDM_K_CODE_ENCODE 18
#define OFDM_K_STREAM_CSI 19
#define OFDM_K_CODE_DECODE 20

/* All three calls enqueue on the context's stream, do not synchronise and allocate nothing.  OFDM_E_ARG, with an
 * ofdm_last_error text and before any launch: ctx or a required pointer NULL, a negative count, n_data outside [1, 15],
 * a pointer that is not aligned to its element (4 bytes; 8 for d_eq, d_count, d_packets and the branches), n_branches
 * outside [1, 4]. */

/* Encode n packets.  d_info: uint32 [n][W_i] on the device; d_words: uint32 [n][3 n_data], written.  One thread per
 * output word; an output word is a function of at most three input words.  n = 0 writes nothing. */
int ofdm_code_encode(ofdm_ctx *ctx, int32_t n_data, const void *d_info, int64_t n, void *d_words);

/* The gains of the first min(d_count[1], max_packets) records of a finished receive call over the same recordings.
 * d_branches, n_branches, n_samples: as the diversity receive call's of ofdm_mi355x_diversity.h: a host array of
 * n_branches device pointers, each to n_samples complex float samples (one branch: the recording of any of the
 * single-branch calls).  d_packets, d_count: what that call wrote, read on the device.  d_csi: float [max_packets][48],
 * the first min(d_count[1], max_packets) rows are written.  max_packets = 0 launches nothing. */
int ofdm_stream_csi(ofdm_ctx *ctx, const void *const *d_branches, int32_t n_branches, int64_t n_samples,
                    const void *d_packets, const void *d_count, int64_t max_packets, void *d_csi);

/* Decode rows of equalised subcarriers.  d_eq: float2 [n][48 n_data]; d_csi: optional, float [n][48]; d_count: optional,
 * int64 [2] on the device: rows = min(n, d_count[1]), else rows = n; rows past that are not written.  d_info: uint32
 * [n][W_i], written; d_path: optional, float [n], the path metric.  n = 0 launches nothing. */
int ofdm_code_decode(ofdm_ctx *ctx, int32_t n_data, const void *d_eq, const void *d_csi, const void *d_count, int64_t n,
                     void *d_info, void *d_path);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_CODE_H */
