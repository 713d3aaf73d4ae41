/*
 * ofdm_mi355x_diversity.h -- extension of the C ABI (ofdm_mi355x.h, ofdm_mi355x_stream.h, ofdm_mi355x_detect.h,
 * ofdm_mi355x_timing.h, ofdm_mi355x_track.h): receive diversity for the stream receiver.
 *
 * Under Rayleigh fading what is left of a single-antenna link's loss is the fade itself: a packet whose channel is
 * deep in a fade is missed or decoded wrong whatever the receiver does.  ofdm_receive_stream_diversity takes B = 1..4
 * recordings of the same n_samples -- one per antenna, on a common sample clock and a common oscillator -- and
 * combines them at every step where the single-branch receiver uses one: detection, fine timing, the carrier offset
 * estimates and the equaliser (maximal-ratio combining).  It returns what ofdm_receive_stream_tracked returns: one
 * record per packet, positions ascending.
 *
 * The rules for B >= 2 (stream.diversity_metric, stream.refine_timing_branches and stream.combine_branches are their
 * executable specification, fp64).  r_b is branch b's recording; every sum over branches runs b = 0, 1, .. in that
 * order, and every other sum in an order fixed by stream coordinates, so no output depends on the launch shape, on
 * max_packets or on the branches' alignments.
 *   detection  c[i] = sum_b c_b[i], p[i] = sum_b p_b[i] with c_b and p_b the sums of ofdm_mi355x_detect.h's conjugate
 *              rule on branch b; M[i] = |c[i]|^2 / p[i]^2 over Lc = n - 63 positions, crossing
 *              fma(thr p, p, -|c|^2) < 0 in fp32; zero power is no crossing and M is NaN.  A position sums only terms
 *              of its own window (no running difference).  c_b does not see the phase of branch b's channel, so the
 *              branches add coherently; that is why B >= 2 needs OFDM_DETECT_CONJUGATE: the reference's metric has no
 *              conjugate, carries twice the channel's phase, and its branch sums would cancel.  Fronts, the + 230
 *              confirmation, packet_pos = front + 11, OFDM_STREAM_LAST_FRONT, d_metric, d_cross and the selection are
 *              ofdm_mi355x_detect.h's.
 *   timing     L[j] = sum_b L_b[j] over the 64 candidates of ofdm_mi355x_timing.h, the largest L with the smallest j
 *              wins; quality = L[j*] / sum_b sum_s te_s xe_{b,s}.  The window rule and the ofdm_stream_timing rows are
 *              unchanged; OFDM_TIMING_LTF and OFDM_TIMING_LTF_MATLAB are both supported.
 *   decode     every branch is staged and matched-filtered as the single-branch chain does.  One coarse and one fine
 *              carrier offset per packet from the branch-summed correlations (the formulas of the single-branch
 *              chain with pp = sum_b sum_k ...), one rotation by their sum on every branch.  With S_b = F(LTF1 + LTF2)_b,
 *              H_b = L S_b / 2 and Y_{b,d} the spectrum of data symbol d:
 *                N_d[k] = sum_b Y_{b,d}[k] conj(H_b[k]),  G[k] = sum_b |H_b[k]|^2,  z_d[k] = N_d[k] / G[k]
 *              over the 48 data bins.  G = 0 gives 0 / 0 and the slicer decides "-", as it does for one branch.
 *              OFDM_TRACK_PILOTS: P_d = sum_pilots p_k N_d[k]; from there u_d, the fallback u_d = 1, the power-of-two
 *              scaling, z' = z conj(u_d) and d_phase are exactly ofdm_mi355x_track.h's.
 *              gain[b] = sum over the 52 used bins of |H_b[k]|^2 / 52 (d_gain).
 *              The record, d_bits, d_eq, the counters, OFDM_CAPTURE_OOB, the zero-symbol rule past the recording's end
 *              and the invariance to scaling every branch by 2^12 or 2^-12 are those of the tracked decode applied to
 *              z (OFDM_TRACK_NONE) or z'; cfo_coarse_hz and cfo_fine_hz carry the common estimates.
 * Maximal-ratio weights assume the same noise power on every branch: a caller whose antennas have unequal noise floors
 * scales its recordings to a common noise power first.
 *
 * When it pays.  Measured on an MI355X with `ofdm_pkg.py link --packets 65536 --pdp 1,0.5,0.25,0.125 --noise complex
 * --detector conjugate --timing ltf --branches B`, 2 data symbols, missed packets and BER over the matched ones for
 * B = 1 / 2 / 4: 10 dB 27,198 / 20,751 / 13,373 and 1.6e-2 / 1.2e-3 / 1.1e-5; 20 dB 422 / 8 / 0 and 3.6e-3 / 4.1e-5 / 0.
 * On the CPU in fp64, 300 flat-Rayleigh 2-symbol packets at 10 dB: 2,376 / 192 / 3 bit errors of 57,600.  The kernels
 * differ from the fp64 rules by at most 1.3e-6 in M (relative to max(M, 0.075)), 2.4e-7 in the timing quality, 4.8e-7 rad
 * in the phase, 2.3e-7 (relative) in the gain and 6.1e-7 of the packet's largest in the combined subcarriers, over the
 * streams of tests/test_gpu_diversity.py.  A two-branch call takes 0.89 x two single-branch calls on 2-symbol packets and
 * 1.39 x on 15-symbol ones.
 *
 * Out of scope: ofdm_receive_captures and the frame-mode sweeps, selection or equal-gain combining, per-branch noise
 * estimation and transmit diversity.
 *
 * The base header's function list, OFDM_ABI_VERSION and the older extension headers are unchanged; a caller that never
 * includes this file sees the library exactly as before.
 */
#ifndef OFDM_MI355X_DIVERSITY_H
#define OFDM_MI355X_DIVERSITY_H
#include "ofdm_mi355x_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_DIVERSITY_MAX_BRANCHES 4

/* ofdm_timing_query ids of the three kernels of the B >= 2 path, after OFDM_K_STREAM_DECODE_TRACK = 14 */
#define OFDM_K_STREAM_DETECT_DIV 15
#define OFDM_K_STREAM_TIMING_DIV 16
#define OFDM_K_STREAM_DECODE_DIV 17

/* ofdm_receive_stream_tracked over n_branches recordings.  Every argument and output but d_branches, n_branches and
 * d_gain is ofdm_receive_stream_tracked's.
 * d_branches  a host array of n_branches device pointers, each to n_samples complex float samples, 8-byte aligned; the
 *             branches may sit at different 16-byte alignments.  Read during the call only.
 * n_branches  1: the call is ofdm_receive_stream_tracked itself on d_branches[0] -- the same launches, byte-identical
 *             outputs; d_gain must then be NULL.  2..4: the rules above, with the detection, timing and decode launches
 *             under OFDM_K_STREAM_DETECT_DIV, OFDM_K_STREAM_TIMING_DIV (with a timing option) and
 *             OFDM_K_STREAM_DECODE_DIV; the selection launches are unchanged.
 * d_gain      optional, float [max_packets][n_branches] on the device; the first d_count[1] rows are written.
 * The call does not synchronise and allocates nothing beyond what ofdm_receive_stream_tracked does.
 * OFDM_E_ARG, with an ofdm_last_error text and before any launch: n_branches outside [1, 4]; d_branches NULL, or an
 * entry NULL or not 8-byte aligned when n_samples > 0; n_branches >= 2 without OFDM_DETECT_CONJUGATE (sopts == NULL
 * included); d_gain with n_branches == 1; a packet whose n_branches filtered frames do not fit the LDS of a block; and
 * everything ofdm_receive_stream_tracked refuses. */
int ofdm_receive_stream_diversity(ofdm_ctx *ctx, const void *const *d_branches, int32_t n_branches, int64_t n_samples,
                                  const ofdm_rx_opts *opts, const ofdm_stream_opts *sopts, int timing, int tracking,
                                  int payload, int64_t max_packets, void *d_packets, void *d_count, void *d_bits,
                                  void *d_eq, void *d_counters, void *d_metric, void *d_cross, void *d_timing,
                                  void *d_phase, void *d_gain);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_DIVERSITY_H */
