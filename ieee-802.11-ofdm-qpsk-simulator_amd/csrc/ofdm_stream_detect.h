// ofdm_stream_detect.h -- what ofdm_stream.hip (ofdm_receive_stream), ofdm_stream_conj.hip (ofdm_receive_stream_ex),
// ofdm_stream_timing.hip (ofdm_receive_stream_timed), ofdm_stream_track.hip (ofdm_receive_stream_tracked) and
// ofdm_stream_div.hip (ofdm_receive_stream_diversity, which fills all three hooks) share: the
// detection kernels' argument block, the hook through which the extended entry point replaces the detection launch
// alone, the hook through which the timed one adds a launch between the selection and the decode, and the hook through
// which the tracked one replaces the decode launch.  The selection and decode kernels stay in ofdm_stream.hip and are
// launched from there (stream_receive); the decode kernels' chain itself is ofdm_stream_decode.h and ofdm_rxchain.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ofdm_mi355x_detect.h"

namespace ofdm {

struct Ctx;

struct DetArgs {
    const float2 *x;
    int64_t n, lc, tiles, words;   // samples, positions, tiles, bitmap words
    uint32_t *bitmap;              // scratch, padded to whole 16-byte groups
    uint32_t *cross;               // the caller's copy (optional)
    float *metric;                 // optional
};

// A detector other than ofdm_receive_stream's own: positions are [0, n - halo), the launch writes the crossing bitmap
// (and the caller's copy and metric) of a.tiles tiles of OFDM_STREAM_TILE positions exactly as stream_detect_kernel
// does, under the timing id `kernel`.
struct StreamDetector {
    int halo;                      // samples a position reads past itself: 47 for the reference's metric, 63 for lag 32
    int kernel;                    // ofdm_timing_query id of the launch
    float threshold;
    void (*launch)(const StreamDetector *det, dim3 grid, hipStream_t stream, const DetArgs &a);
    const char *name;              // for the launch error's text
    const void *user;              // the hook's own (ofdm_stream_div.hip: the branch table), nullptr for the existing ones
};

// What a refiner's launch works on: the recording, and the records stream_select_kernel<2> has just written.
struct RefineArgs {
    const float2 *x;
    int64_t n;
    const int64_t *count;          // d_count: [1] records written
    ofdm_stream_packet *pk;
    int64_t max_packets;
};

// A launch between the selection and the decode (ofdm_stream_timing.hip: the fine timing of ofdm_receive_stream_timed)
// that may rewrite packet_pos of the first d_count[1] records, under the timing id `kernel`; the decode kernel then
// runs on what it left.  Not launched when max_packets is 0 or the stream has no positions.
struct StreamRefiner {
    int kernel;                    // ofdm_timing_query id of the launch
    int (*prepare)(const StreamRefiner *ref, Ctx *c);   // after every argument check, before the first launch; an OFDM_E_* code
    void (*launch)(const StreamRefiner *ref, Ctx *c, hipStream_t stream, const RefineArgs &a);
    const char *name;              // for the launch error's text
    void *out;                     // the refiner's own output (optional)
    const void *user;              // as StreamDetector's
};

// Another decode kernel in place of stream_decode_kernel (ofdm_stream_track.hip: the pilot-tracking decode of
// ofdm_receive_stream_tracked), under the timing id `kernel`: the launch gets the grid, the block, the dynamic LDS and
// the argument block stream_receive has prepared for stream_decode_kernel (DecArgs, ofdm_stream_decode.h), and the
// payload as plain MSB-first words, three per data symbol.
struct DecArgs;
struct StreamDecoder {
    int kernel;                    // ofdm_timing_query id of the launch
    void (*launch)(const StreamDecoder *dec, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const DecArgs &a,
                   const uint32_t *payload);
    const char *name;              // for the launch error's text
    void *out;                     // the decoder's own output (optional)
    const void *user;              // as StreamDetector's
};

// ofdm_receive_stream's body; det == nullptr is the reference's rule with stream_detect_kernel, ref == nullptr no
// launch between the selection and the decode, and dec == nullptr stream_decode_kernel: with all three, bit for bit what
// the entry point enqueued before the hooks existed.
int stream_receive(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts, int payload,
                   int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq, void *d_counters,
                   void *d_metric, void *d_cross, const StreamDetector *det, const StreamRefiner *ref = nullptr,
                   const StreamDecoder *dec = nullptr);

// ofdm_receive_stream_ex's body (ofdm_stream_conj.hip): sopts checked and turned into a detector, then stream_receive
int stream_receive_ex(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                      const ofdm_stream_opts *sopts, int payload, int64_t max_packets, void *d_packets, void *d_count,
                      void *d_bits, void *d_eq, void *d_counters, void *d_metric, void *d_cross, const StreamRefiner *ref,
                      const StreamDecoder *dec = nullptr);

// ofdm_receive_stream_timed's body (ofdm_stream_timing.hip): timing checked and turned into a refiner, then
// stream_receive_ex
int stream_receive_timed(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                         const ofdm_stream_opts *sopts, int timing, int payload, int64_t max_packets, void *d_packets,
                         void *d_count, void *d_bits, void *d_eq, void *d_counters, void *d_metric, void *d_cross,
                         void *d_timing, const StreamDecoder *dec);

}  // namespace ofdm
