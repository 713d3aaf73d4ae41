// ofdm_stream_timing.hip -- fine timing for the stream receiver (include/ofdm_mi355x_timing.h:
// ofdm_receive_stream_timed).  A translation unit of its own: ofdm_stream.hip and ofdm_stream_conj.hip keep their
// kernels as they are; this file adds one kernel and hands it to stream_receive as a refiner (ofdm_stream_detect.h),
// which launches it between stream_select_kernel<2> and stream_decode_kernel.
//
//   stream_timing_kernel : one wave per packet, TM_WAVES waves per block, looping over d_count; lane j is candidate j
//     (shift j - 56).  The wave stages the 319 samples [p + 322, p + 640] of the search window as real and imaginary
//     planes in LDS, so lane j reads its 256 samples at plane index j + m: stride 1 across the lanes, no bank
//     conflict.  The template is a kernel argument, wave-uniform: its operands come through the scalar cache into
//     SGPRs, never through a per-lane load.  Per lane and packet: 8 segments of 32 complex multiply-adds
//     x conj(t) -- four fused multiply-adds each, ascending k -- then L += |segment|^2, ascending s.  The order is fixed
//     per packet, so L, the choice and the quality depend on nothing but the packet's own samples.
//     The largest L with the smallest j is found by a 64-lane butterfly on (L, j); lanes 0..7 then sum the chosen
//     window's power per segment for the quality, lane 0 writes packet_pos and the timing row.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ofdm_mi355x_timing.h"
#include "ofdm_ctx.h"
#include "ofdm_stream_detect.h"
#include "ofdm_stream_ltf.h"

namespace ofdm {

constexpr int TM_WAVES = 4;                                   // packets per block and sweep
constexpr int TM_BLOCKS_PER_CU = 8;                           // the grid's cap: the waves loop past it
static_assert(OFDM_K_STREAM_TIMING == Ctx::K_STREAM_TIMING && Ctx::K_STREAM_TIMING < Ctx::NK, "the timing kernel's id is one of the context's");

__global__ __launch_bounds__(64 * TM_WAVES) void stream_timing_kernel(TimArgs a) {
    __shared__ float planes[TM_WAVES][2][TM_PLANE];
    __shared__ float power[TM_WAVES][TM_NSEG];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    float *re = planes[wave][0], *im = planes[wave][1];
    const int64_t cnt = a.count[1];
    for (int64_t i = (int64_t)blockIdx.x * TM_WAVES + wave; i < cnt; i += (int64_t)gridDim.x * TM_WAVES) {
        ofdm_stream_packet *pkt = a.pk + i;
        const int64_t pv = pkt->packet_pos;
        const int64_t p = ((int64_t)__builtin_amdgcn_readfirstlane((int)(pv >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)pv);
        int shift = 0;
        float quality = 0.f;
        // the whole search window inside the stream, or the packet keeps its position (wave-uniform)
        if (p + TM_FIRST >= 0 && p + TM_FIRST + TM_WINDOW - 1 < a.n) {
            const float2 *row = a.x + (p + TM_FIRST);
            float2 v[TM_LOADS];
#pragma unroll
            for (int r = 0; r < TM_LOADS; ++r) {
                const int m = lane + 64 * r;
                v[r] = m < TM_WINDOW ? row[m] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int r = 0; r < TM_LOADS; ++r) {
                const int m = lane + 64 * r;
                if (m < TM_PLANE) { re[m] = v[r].x; im[m] = v[r].y; }
            }
            tm_wave_sync();
            // ---- L[lane]: 8 segments of 32 terms x conj(t) ----
            float lam = 0.f;
#pragma unroll 1
            for (int s = 0; s < TM_NSEG; ++s) {
                const float *xr = re + lane + TM_SEG * s, *xi = im + lane + TM_SEG * s;
                const float2 *t = a.t + ((TM_SEG * s) & (TM_PERIOD - 1));
                float cx = 0.f, cy = 0.f;
#pragma unroll
                for (int k = 0; k < TM_SEG; ++k) {
                    const float ur = xr[k], ui = xi[k], tr = t[k].x, ti = t[k].y;
                    cx = fmaf(ur, tr, cx); cx = fmaf(ui, ti, cx);
                    cy = fmaf(ui, tr, cy); cy = fmaf(-ur, ti, cy);
                }
                lam = fmaf(cx, cx, lam);
                lam = fmaf(cy, cy, lam);
            }
            // ---- the largest L, the smallest candidate among equals ----
            float best = lam;
            int bj = lane;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oj = __shfl_xor(bj, o, 64);
                if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
            }
            bj = __builtin_amdgcn_readfirstlane(bj);
            const float lbest = __shfl(lam, bj, 64);
            if (lbest > 0.f) {                                          // wave-uniform
                // ---- the chosen window's power per segment, then the quality ----
                if (lane < TM_NSEG) {
                    const float *xr = re + bj + TM_SEG * lane, *xi = im + bj + TM_SEG * lane;
                    float e = 0.f;
#pragma unroll 8
                    for (int k = 0; k < TM_SEG; ++k) { e = fmaf(xr[k], xr[k], e); e = fmaf(xi[k], xi[k], e); }
                    power[wave][lane] = e;
                }
                tm_wave_sync();
                float den = 0.f;
#pragma unroll
                for (int s = 0; s < TM_NSEG; ++s) den = fmaf(a.te[s], power[wave][s], den);
                quality = lbest / den;
                shift = bj - OFDM_TIMING_BACK;
            }
            tm_wave_sync();                                             // the next packet overwrites the planes
        }
        if (lane == 0) {
            if (shift) pkt->packet_pos = p + shift;
            if (a.out) {
                ofdm_stream_timing *o = a.out + i;
                o->coarse_pos = p;
                o->quality = quality;
                o->shift = shift;
            }
        }
    }
}

// ofdm_stream_ltf.h: the template from the context's own Transmitter() waveform (frame_wave_kernel through
// ofdm_transmitter)
int timing_template(Ctx *c, int conv) {
    if (c->ltf_ready[conv]) return OFDM_OK;
    std::vector<float2> w(10 * (2 * (320 + 80 * LONG_MAX_FRAMES) + 20));
    int32_t len = 0;
    int rc = ofdm_transmitter(reinterpret_cast<ofdm_ctx *>(c), conv, OFDM_PAYLOAD_MESSAGE, 1,
                              reinterpret_cast<float *>(w.data()), (int32_t)w.size(), &len);
    if (rc) return rc;
    if (len < TM_LTF + TM_PERIOD) return set_error(OFDM_E_HIP, "Transmitter() gave %d samples, the template needs %d", len, TM_LTF + TM_PERIOD);
    std::copy(w.begin() + TM_LTF, w.begin() + TM_LTF + TM_PERIOD, c->ltf_template[conv]);
    c->ltf_ready[conv] = true;
    return OFDM_OK;
}

void timing_fill(const Ctx *c, int conv, TimArgs &a) {
    std::copy(c->ltf_template[conv], c->ltf_template[conv] + TM_PERIOD, a.t);
    for (int s = 0; s < TM_NSEG; ++s) {
        double e = 0.0;
        for (int k = 0; k < TM_SEG; ++k) {
            const float2 v = a.t[(TM_SEG * s + k) & (TM_PERIOD - 1)];
            e += (double)v.x * v.x + (double)v.y * v.y;
        }
        a.te[s] = (float)e;
    }
}

template <int CONV>
static int timing_prepare(const StreamRefiner *, Ctx *c) {
    static_assert(CONV == OFDM_CONV_C || CONV == OFDM_CONV_MATLAB, "one cached template per convention");
    return timing_template(c, CONV);
}

template <int CONV>
static void timing_launch(const StreamRefiner *ref, Ctx *c, hipStream_t stream, const RefineArgs &r) {
    TimArgs a{};
    a.x = r.x;
    a.n = r.n;
    a.count = r.count;
    a.pk = r.pk;
    a.out = (ofdm_stream_timing *)ref->out;
    timing_fill(c, CONV, a);
    // the packet count stays on the device: enough blocks for max_packets, at most TM_BLOCKS_PER_CU per CU; the waves loop
    const int64_t blocks = (r.max_packets + TM_WAVES - 1) / TM_WAVES;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, TM_BLOCKS_PER_CU * (int64_t)c->cus));
    hipLaunchKernelGGL(stream_timing_kernel, grid, dim3(64 * TM_WAVES), 0, stream, a);
}

// ofdm_receive_stream_timed's body; dec (ofdm_stream_detect.h) is handed on to stream_receive
int stream_receive_timed(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                         const ofdm_stream_opts *sopts, int timing, int payload, int64_t max_packets, void *d_packets,
                         void *d_count, void *d_bits, void *d_eq, void *d_counters, void *d_metric, void *d_cross,
                         void *d_timing, const StreamDecoder *dec) {
    if (timing != OFDM_TIMING_NONE && timing != OFDM_TIMING_LTF && timing != OFDM_TIMING_LTF_MATLAB)
        return set_error(OFDM_E_ARG, "timing must be OFDM_TIMING_NONE (0), OFDM_TIMING_LTF (1) or OFDM_TIMING_LTF_MATLAB (2), got %d", timing);
    if (timing == OFDM_TIMING_NONE && d_timing)
        return set_error(OFDM_E_ARG, "d_timing needs OFDM_TIMING_LTF or OFDM_TIMING_LTF_MATLAB: timing is OFDM_TIMING_NONE");
    // no timing is ofdm_receive_stream_ex itself: the same launches, byte-identical outputs
    if (timing == OFDM_TIMING_NONE)
        return stream_receive_ex(c, d_samples, n_samples, opts, sopts, payload, max_packets, d_packets, d_count, d_bits, d_eq,
                                 d_counters, d_metric, d_cross, nullptr, dec);
    StreamRefiner ref{};
    ref.kernel = OFDM_K_STREAM_TIMING;
    // the same kernel under the same id; the recording's convention only chooses the template
    const bool matlab = timing == OFDM_TIMING_LTF_MATLAB;
    ref.prepare = matlab ? timing_prepare<OFDM_CONV_MATLAB> : timing_prepare<OFDM_CONV_C>;
    ref.launch = matlab ? timing_launch<OFDM_CONV_MATLAB> : timing_launch<OFDM_CONV_C>;
    ref.name = "stream_timing_kernel";
    ref.out = d_timing;
    return stream_receive_ex(c, d_samples, n_samples, opts, sopts, payload, max_packets, d_packets, d_count, d_bits, d_eq,
                             d_counters, d_metric, d_cross, &ref, dec);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_receive_stream_timed(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                                         const ofdm_stream_opts *sopts, int timing, int payload, int64_t max_packets,
                                         void *d_packets, void *d_count, void *d_bits, void *d_eq, void *d_counters,
                                         void *d_metric, void *d_cross, void *d_timing) {
    return stream_receive_timed(reinterpret_cast<Ctx *>(ctx), d_samples, n_samples, opts, sopts, timing, payload, max_packets,
                                d_packets, d_count, d_bits, d_eq, d_counters, d_metric, d_cross, d_timing, nullptr);
}
