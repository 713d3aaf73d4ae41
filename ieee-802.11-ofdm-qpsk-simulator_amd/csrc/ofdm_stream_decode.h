// ofdm_stream_decode.h -- what only the stream receiver's decode kernels share: stream_decode_kernel (ofdm_stream.hip),
// stream_decode_track_kernel (ofdm_stream_track.hip, the pilot-tracking decode of include/ofdm_mi355x_track.h) and
// stream_decode_div_kernel (ofdm_stream_div.hip, the diversity decode of include/ofdm_mi355x_diversity.h).  The argument
// block stream_receive prepares, and the part of a packet's chain that comes before ofdm_rxchain.h's stages: reading
// the packet's record, staging its samples, the matched filter on the staged planes and the sync half of the record;
// and the pilots' bins and signs for the pilot step of the two tracking decodes.
#pragma once
#include <cmath>
#include "ofdm_mi355x_stream.h"
#include "ofdm_ctx.h"
#include "ofdm_rxchain.h"
#include "ofdm_stream_detect.h"

namespace ofdm {

constexpr int SDEC_LOADS = 8;                         // 16-byte loads a lane keeps in flight while staging (all of a 2-symbol packet's)

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
    uint32_t dtable[4 * RXC_MAX_DATA];
    uint32_t ztable[RXC_MAX_DATA];    // per data symbol, were it all zeros: bit errors | slicer axis errors << 16 (zero_errors)
};

// the record stream_select_kernel<2> (or a refiner) left: packet_pos and the LAST_FRONT flag, wave-uniform, made scalar
__device__ __forceinline__ void sdec_packet(const ofdm_stream_packet *pkt, int64_t &p, int &last_front) {
    const int64_t pv = pkt->packet_pos;
    p = ((int64_t)__builtin_amdgcn_readfirstlane((int)(pv >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)pv);
    last_front = __builtin_amdgcn_readfirstlane(pkt->r.flags) & OFDM_STREAM_LAST_FRONT;
}

// ---- stage [p - 20, p + 2 nfr - 2] (len = 2 nfr + 19 samples): the wave holds only the samples the filter reads, sample
// s of the stream at plane index s - (p - 20), aligned 16-byte loads inside the stream, zero outside.  q: sample s is
// 16-byte aligned when s + q is even ----
__device__ __forceinline__ void sdec_stage(const float2 *x, int64_t n, int64_t p, int q, int len, int lane, float *re, float *im) {
    const int64_t s0 = p - 20, e0 = s0 - ((s0 + q) & 1);
    for (int kb = lane; 2 * kb < len + 1; kb += 64 * SDEC_LOADS) {     // SDEC_LOADS loads in flight, then their writes
        f4v t[SDEC_LOADS];
#pragma unroll
        for (int j = 0; j < SDEC_LOADS; ++j) {
            const int k = kb + 64 * j;
            const int64_t s = e0 + 2 * k;
            t[j] = f4v{0.f, 0.f, 0.f, 0.f};
            if (2 * k >= len + 1) continue;
            if (s >= 0 && s + 1 < n) {
                t[j] = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(x + s));
            } else {
                if (s >= 0 && s < n) { const float2 u = x[s]; t[j].x = u.x; t[j].y = u.y; }
                if (s + 1 >= 0 && s + 1 < n) { const float2 u = x[s + 1]; t[j].z = u.x; t[j].w = u.y; }
            }
        }
#pragma unroll
        for (int j = 0; j < SDEC_LOADS; ++j) {
            const int k = kb + 64 * j;
            const int m = 2 * k - (int)(s0 - e0);                  // -1 for the pair's first sample when e0 < s0
            if (2 * k >= len + 1) continue;
            if (m >= 0 && m < len) { re[m] = t[j].x; im[m] = t[j].y; }
            if (m + 1 < len) { re[m + 1] = t[j].z; im[m + 1] = t[j].w; }
        }
    }
}

// ---- RRC matched filter at the down-sampled instants: stream sample p + 2 ii - tt is plane index 20 + 2 ii - tt, so
// the filter needs no bounds test (capture_rx_kernel's tap order) ----
__device__ __forceinline__ void sdec_filter(const float *re, const float *im, const float *taps, int nfr, int lane,
                                            float *fre, float *fim) {
    for (int ii = lane; ii < nfr; ii += 64) {
        if (!rxc_needed(ii)) continue;
        const int n = 20 + 2 * ii;
        float vx = 0.f, vy = 0.f;
#pragma unroll
        for (int tt = 0; tt < 21; ++tt) {
            vx = fmaf(re[n - tt], taps[tt], vx);
            vy = fmaf(im[n - tt], taps[tt], vy);
        }
        fre[ii] = vx;
        fim[ii] = vy;
    }
}

// the pilots' bins (pilot_at, ofdm_device.h) and p_k L_k, for the pilot step of the tracking decodes
// (ofdm_stream_track.hip, ofdm_stream_div.hip)
__device__ __forceinline__ int track_pilot_bin(int i) { return 11 + 14 * i; }
static_assert(pilot_at(11) == 1.f && pilot_at(25) == 1.f && pilot_at(39) == 1.f && pilot_at(53) == -1.f, "pilots {1,1,1,-1} at 11, 25, 39, 53");
constexpr uint32_t track_pilot_neg() {
    uint32_t v = 0;
    for (int i = 0; i < 4; ++i) v |= (uint32_t)(pilot_at(11 + 14 * i) * (float)ltf_sign(11 + 14 * i) < 0.f) << i;
    return v;
}
constexpr uint32_t TRACK_PILOT_NEG = track_pilot_neg();

// the sync half of the record and its counter term leave ahead of the transforms, so nothing of it stays live over them
__device__ __forceinline__ void sdec_sync_record(ofdm_capture_result *r, unsigned long long *acc, bool counters, int lane,
                                                 int64_t p, int last_front, bool oob, double fc, double ff) {
    if (lane == 0) {
        r->packet_idx = p <= 0x7fffffffll ? (int32_t)p : -1;
        r->flags = last_front | (oob ? OFDM_CAPTURE_OOB : 0);
        r->cfo_coarse_hz = (float)fc;
        r->cfo_fine_hz = (float)ff;
        r->reserved[0] = 0;
        r->reserved[1] = 0;
        if (counters) atomicAdd(&acc[OFDM_C_OOB], (unsigned long long)oob);
    }
}

}  // namespace ofdm
