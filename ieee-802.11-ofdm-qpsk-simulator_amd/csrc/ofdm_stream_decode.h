// ofdm_stream_decode.h -- what the stream receiver's two decode kernels share: stream_decode_kernel (ofdm_stream.hip) and
// stream_decode_track_kernel (ofdm_stream_track.hip, the pilot-tracking decode of include/ofdm_mi355x_track.h).  The
// decode's constants, its argument block and the small inlined device helpers of the chain up to the transforms, lifted
// out of ofdm_stream.hip word for word: the kernels of that file build to the same instructions as before.
#pragma once
#include <cmath>
#include "ofdm_mi355x_stream.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"
#include "ofdm_stream_detect.h"

namespace ofdm {

constexpr int SDEC_MAX_DATA = LONG_MAX_FRAMES;
constexpr int SDEC_BLOCK_WAVES = 8;                   // both kernels' launch bound; ofdm_stream.hip sizes the block (SDEC_MAX_WAVES)
constexpr size_t SDEC_LDS_PER_CU = 160 * 1024;
constexpr int SDEC_ACC_WORDS = OFDM_NCOUNTERS;
constexpr double SDEC_TS = 1.0 / 20e6;                // OFDM.c:16-17
constexpr int SDEC_SPEC_PITCH = 130;                  // floats per parked spectrum (as capture_rx_kernel)
constexpr int SDEC_LOADS = 8;                         // 16-byte loads a lane keeps in flight while staging (all of a 2-symbol packet's)
constexpr uint64_t sdec_ltf_neg() {
    uint64_t v = 0;
    for (int b = 0; b < 64; ++b) v |= (uint64_t)(ltf_sign(b) < 0) << b;
    return v;
}
constexpr uint64_t SDEC_LTF_NEG = sdec_ltf_neg();

struct DecArgs {
    const float2 *x;
    int64_t n;
    const int64_t *count;    // d_count: [1] records to decode
    ofdm_stream_packet *pk;
    uint32_t *bits;
    float2 *eq;
    unsigned long long *counters;
    int32_t n_data, float_cfo;
    int32_t plane;           // floats per plane (2 nfr + 19 rounded up to 4)
    int32_t wave_floats;     // floats per wave: two planes and fr[]
    float taps[21];
    uint32_t dtable[4 * SDEC_MAX_DATA];
    uint32_t ztable[SDEC_MAX_DATA];   // per data symbol, were it all zeros: bit errors | slicer axis errors << 16 (stream_zero_errors)
};

// LDS ordering between the lanes of one wave (the block's other waves run other packets)
__device__ __forceinline__ void sdec_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float sdec_sum_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// rotate by exp(-j 2 pi f Ts i): the phase in revolutions in fp64, range-reduced, then v_sin / v_cos (OFDM.c:802,825)
__device__ __forceinline__ float2 sdec_rot(float2 v, double f_ts, int i) {
    const double rev = -f_ts * (double)i;
    const float fr = (float)(rev - rint(rev));
    const float s = __builtin_amdgcn_sinf(fr), c = __builtin_amdgcn_cosf(fr);
    return make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
}
// frame sample ii is one the receiver uses: STF tail [80, 112), LTF pair [192, 320), data symbols past their prefixes
__device__ __forceinline__ bool sdec_needed(int ii) {
    if (ii < 192) return ii >= 80 && ii < 112;
    if (ii < 320) return true;
    const int r = (ii - 320) % 80;
    return r >= 16;
}

}  // namespace ofdm
