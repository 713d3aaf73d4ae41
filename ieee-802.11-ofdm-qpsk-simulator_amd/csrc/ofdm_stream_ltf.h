// ofdm_stream_ltf.h -- what the fine timing kernels share (ofdm_stream_timing.hip: stream_timing_kernel;
// ofdm_stream_div.hip: stream_timing_div_kernel): the search window's geometry, the kernels' argument block and the
// context's cached long-training templates (built and filled in ofdm_stream_timing.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "ofdm_mi355x_timing.h"
#include "ofdm_ctx.h"
#include "ofdm_stream_detect.h"

namespace ofdm {

constexpr int TM_CAND = OFDM_TIMING_BACK + OFDM_TIMING_FWD;   // 64: one candidate per lane
constexpr int TM_LTF = 394;                                   // 2 * 192 + 10: the first long training symbol in the waveform
constexpr int TM_FIRST = TM_LTF - 16 - OFDM_TIMING_BACK;      // 322: candidate 0 reads from p + 322
constexpr int TM_LEN = 256, TM_SEG = 32, TM_NSEG = TM_LEN / TM_SEG, TM_PERIOD = 128;
constexpr int TM_WINDOW = TM_CAND - 1 + TM_LEN;               // 319 samples staged per packet
constexpr int TM_PLANE = 320;
constexpr int TM_LOADS = (TM_WINDOW + 63) / 64;
static_assert(TM_CAND == 64, "lane = candidate");
static_assert(TM_FIRST == 322 && TM_FIRST + TM_WINDOW - 1 == 640, "the search window is [p + 322, p + 640]");
static_assert(TM_WINDOW <= TM_PLANE && (TM_CAND - 1) + (TM_LEN - 1) < TM_WINDOW, "every lane's last sample is staged");
static_assert(sizeof(ofdm_stream_timing) == 16, "ofdm_stream_timing is 16 bytes");

struct TimArgs {
    const float2 *x;
    int64_t n;
    const int64_t *count;          // d_count: [1] records to refine
    ofdm_stream_packet *pk;
    ofdm_stream_timing *out;       // optional
    float te[TM_NSEG];             // sum_k |t[32 s + k]|^2
    float2 t[TM_PERIOD];           // the template's period: t[k] = P[k mod 128]
};

// LDS ordering between the lanes of one wave (the block's other waves run other packets)
__device__ __forceinline__ void tm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// w[394 .. 522) of the context's own Transmitter() waveform under the convention conv (OFDM_CONV_C or
// OFDM_CONV_MATLAB), once per context and convention: the two templates are cached side by side.  An OFDM_E_* code.
int timing_template(Ctx *c, int conv);
// the template of `conv` (after timing_template) and its segment energies into a.t and a.te
void timing_fill(const Ctx *c, int conv, TimArgs &a);

}  // namespace ofdm
