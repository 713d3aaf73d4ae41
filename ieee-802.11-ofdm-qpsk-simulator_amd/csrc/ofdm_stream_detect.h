// ofdm_stream_detect.h -- what ofdm_stream.hip (ofdm_receive_stream) and ofdm_stream_conj.hip (ofdm_receive_stream_ex)
// share: the detection kernels' argument block and the hook through which the extended entry point replaces the
// detection launch alone.  The selection and decode kernels stay in ofdm_stream.hip
// and are launched from there (stream_receive), so their certified builds do not move and nothing of them is restated.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ofdm_mi355x_stream.h"

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
};

// ofdm_receive_stream's body; det == nullptr is the reference's rule with stream_detect_kernel, bit for bit what the
// entry point enqueued before the hook existed.
int stream_receive(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts, int payload,
                   int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq, void *d_counters,
                   void *d_metric, void *d_cross, const StreamDetector *det);

}  // namespace ofdm
