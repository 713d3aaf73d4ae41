// ofdm_stream_track.hip -- pilot phase tracking in the stream receiver's decode (include/ofdm_mi355x_track.h:
// ofdm_receive_stream_tracked).  A translation unit of its own: ofdm_stream.hip, ofdm_stream_conj.hip and
// ofdm_stream_timing.hip keep their kernels as they are; this file adds one kernel and hands it to stream_receive as a
// decoder (ofdm_stream_detect.h), which launches it in place of stream_decode_kernel with the same argument block, grid
// and dynamic LDS.
//
//   stream_decode_track_kernel : one wave per packet, W waves per block, looping over d_count, as stream_decode_kernel.
//     Through the transforms' first stage the chain is that kernel's, from the same inlined stages (ofdm_stream_decode.h:
//     staging, the matched filter at the used instants, the sync record; ofdm_rxchain.h: coarse and fine CFO, the
//     combined rotation, quads {LTF1 + LTF2, D_3q, D_3q+1, D_3q+2}, the window load), and so is the record's decode
//     half and the counter terms from the packet's totals.  In between:
//       1  every lane parks its finished spectrum in the wave's LDS region (row pitch 130 floats: the 64 lanes' 8-byte
//          writes of one bin fall on distinct bank pairs) -- nothing is demapped inside the transform, since the pilot
//          bins 11 and 39 finish in sub-transform 3 and 25 and 53 in sub-transform 1, after most data bins;
//       2  lane 4 d + i forms term i of P_d = sum_pilots p_k L_k Y_d[k] conj(S[k]), a 4-lane xor butterfly adds them,
//          and every lane of the four normalises: P_d is scaled by the power of two of its larger component before it
//          is squared, so u_d = P_d / |P_d| and the phase do not see the scale of the recording;
//       3  one lane per subcarrier and step over 48 D subcarriers: Z = 2 L Y conj(S) / |S|^2 as stream_decode_kernel's
//          output pass forms it, Z' = Z conj(u_d) with u_d fetched from lane 4 d, the coalesced d_eq store, the C slicer
//          ("-" for zero and NaN), the bit word by a 16-lane OR, bit errors by popcount against the plain payload word,
//          axis errors and |Z' - ref|^2 from the payload bits (re > 0 iff b0 == b1, im > 0 iff b0 == 0, D10); per lane
//          ascending, then the 64-lane xor butterfly;
//       4  d_phase (optional) = atan2f of the scaled P_d, 0 where u_d = 1 by the fallback.
//     A data symbol wholly past the stream's end has Y = 0, so P = 0, u = 1 and Z' = 0: its bits are (1, 0) and its
//     counts the payload's own, with no table.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_track.h"
#include "ofdm_stream_decode.h"

namespace ofdm {

static_assert(OFDM_K_STREAM_DECODE_TRACK == Ctx::K_STREAM_DECODE_TRACK && Ctx::K_STREAM_DECODE_TRACK < Ctx::NK,
              "the tracking decode's id is one of the context's");
static_assert(4 * RXC_MAX_DATA <= 64, "the pilot step is one step: lane 4 d + i");

struct TrackArgs {
    const float2 *x;
    int64_t n;
    const int64_t *count;    // d_count: [1] records to decode
    ofdm_stream_packet *pk;
    uint32_t *bits;
    float2 *eq;
    float *phase;            // optional, [max_packets][D]
    unsigned long long *counters;
    int32_t n_data, float_cfo;
    int32_t plane;           // floats per plane (2 nfr + 19 rounded up to 4)
    int32_t wave_floats;     // floats per wave: two planes and fr[]
    float taps[21];
    uint32_t words[3 * RXC_MAX_DATA];   // the payload, MSB first, three words per data symbol
};

__global__ __launch_bounds__(64 * RXC_MAX_WAVES) void stream_decode_track_kernel(TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long strk_smem[];
    unsigned long long *acc = strk_smem;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int nd = a.n_data, nfr = 320 + 80 * nd, plane = a.plane, len = 2 * nfr + 19;
    float *re = reinterpret_cast<float *>(strk_smem + RXC_ACC_WORDS) + (size_t)wave * a.wave_floats;
    float *im = re + plane;
    float *fre = re + 2 * plane, *fim = fre + nfr;
    if (threadIdx.x < RXC_ACC_WORDS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t cnt = a.count[1];
    const int q = (int)((reinterpret_cast<uintptr_t>(a.x) >> 3) & 1u);     // sample s is 16-byte aligned when s + q is even
    for (int64_t i = (int64_t)blockIdx.x * W + wave; i < cnt; i += (int64_t)gridDim.x * W) {
        ofdm_stream_packet *pkt = a.pk + i;
        int64_t p;
        int last_front;
        sdec_packet(pkt, p, last_front);
        sdec_stage(a.x, a.n, p, q, len, lane, re, im);
        rxc_wave_sync();
        const bool oob = p + 2 * (int64_t)(nfr - 1) >= a.n + 20;       // the reference reads past its buffer
        sdec_filter(re, im, a.taps, nfr, lane, fre, fim);
        rxc_wave_sync();
        double fc, ff;
        rxc_cfo(fre, fim, lane, a.float_cfo, fc, ff);
        sdec_sync_record(&pkt->r, acc, a.counters != nullptr, lane, p, last_front, oob, fc, ff);
        rxc_rotate(fre, fim, lane, nd, fc, ff);
        rxc_wave_sync();
        // ---- the quads' transforms: nothing is demapped inside them, every lane parks its finished spectrum ----
        {
            float2 x[64];
            rxc_window(fre, fim, rxc_quad(lane, nd).k0, x);
            float2 *spec_row = rxc_spec_row(re, lane, nd);
            rxc_wave_sync();
            static_for<0, 4>([&](auto rc) {
                constexpr int R = decltype(rc)::value;
                dif_sub16<false, R>(x);
                rxc_park<R>(x, spec_row);
                sched_fence();
            });
        }
        rxc_wave_sync();
        // ---- the pilot step: lane 4 d + i is term i of P_d; every lane of the four ends with u_d ----
        float ux = 1.f, uy = 0.f;
        {
            const int d = lane >> 2, pi = lane & 3;
            const bool on = d < nd;
            const int dd = on ? d : 0, bin = track_pilot_bin(pi);
            const int l0 = 4 * (dd / 3), ln = l0 + 1 + dd % 3;
            const float2 Y = reinterpret_cast<const float2 *>(re + ln * RXC_SPEC_PITCH)[bin];
            const float2 S = reinterpret_cast<const float2 *>(re + l0 * RXC_SPEC_PITCH)[bin];
            float2 t = cmulc(Y, S);
            if ((TRACK_PILOT_NEG >> pi) & 1u) t = make_float2(-t.x, -t.y);
            t.x += __shfl_xor(t.x, 1, 64);
            t.y += __shfl_xor(t.y, 1, 64);
            t.x += __shfl_xor(t.x, 2, 64);
            t.y += __shfl_xor(t.y, 2, 64);
            // the larger component's power of two leaves P before it is squared: a recording scaled by 2^k gives the
            // same mantissas here, hence the same u and the same phase
            const float big = fmaxf(fabsf(t.x), fabsf(t.y));
            const bool good = on && fabsf(t.x) < INFINITY && fabsf(t.y) < INFINITY && big > 0.f;
            float ph = 0.f;
            if (good) {
                const int e = __builtin_amdgcn_frexp_expf(big);
                const float sx = __builtin_amdgcn_ldexpf(t.x, -e), sy = __builtin_amdgcn_ldexpf(t.y, -e);
                const float rn = __builtin_amdgcn_rsqf(fmaf(sx, sx, sy * sy));
                ux = sx * rn;
                uy = sy * rn;
                if (a.phase) ph = atan2f(sy, sx);
            }
            if (a.phase && on && pi == 0) a.phase[i * nd + d] = ph;
        }
        // ---- the subcarrier pass: Z = Y / H = 2 Lf Y conj(S) / |S|^2 (OFDM.c:1044-1052), Z' = Z conj(u_d), the decided
        // bits (OFDM.c:852-908) and the metrics, one subcarrier per lane and step ----
        float fev = 0.f;
        uint32_t bev = 0u, axv = 0u;
        {
            const int nsc = 48 * nd;
            for (int j0 = 0; j0 < nsc; j0 += 64) {
                const int j = j0 + lane;
                const bool ok = j < nsc;
                const int jj = ok ? j : 0, d = jj / 48, m = jj - 48 * d, bin = data_bin(m);
                const float cx = __shfl(ux, 4 * d, 64), cy = __shfl(uy, 4 * d, 64);
                const float2 z0 = rxc_equalised(re, d, bin);
                // u = 1 (the fallback) leaves Z as it is, a NaN or a signed zero included
                const bool unit = cx == 1.f && cy == 0.f;
                const float2 z = unit ? z0 : make_float2(fmaf(z0.x, cx, z0.y * cy), fmaf(z0.y, cx, -(z0.x * cy)));
                if (a.eq && ok) a.eq[i * nsc + j] = z;
                const uint32_t pr = z.x > 0.f, pi = z.y > 0.f;
                const int sh = 30 - 2 * (lane & 15);
                uint32_t wv = ok ? (((pi ^ 1u) << 1) | (pr ^ pi)) << sh : 0u;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) wv |= (uint32_t)__shfl_xor((int)wv, o, 64);
                const bool lead = ok && (lane & 15) == 0;
                if (a.bits && lead) a.bits[i * (3 * nd) + (j >> 4)] = wv;
                // the truth from the plain payload word of these 16 subcarriers
                const uint32_t tw = a.words[jj >> 4];
                if (lead) bev += (uint32_t)__popc(wv ^ tw);
                const uint32_t b0 = (tw >> (sh + 1)) & 1u, b1 = (tw >> sh) & 1u;
                const bool tr = b0 == b1, ti = b0 == 0u;
                const float ex = z.x - (tr ? INV_SQRT2 : -INV_SQRT2), ey = z.y - (ti ? INV_SQRT2 : -INV_SQRT2);
                if (ok) {
                    axv += (uint32_t)((pr != 0u) != tr) + (uint32_t)((pi != 0u) != ti);
                    fev += fmaf(ex, ex, ey * ey);
                }
            }
        }
        // ---- the packet's totals, its record and its counter terms ----
        const float fe = rxc_sum_f(fev);
        uint32_t ferr = bev, fax = axv;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ferr += (uint32_t)__shfl_xor((int)ferr, o, 64);
            fax += (uint32_t)__shfl_xor((int)fax, o, 64);
        }
        rxc_record(&pkt->r, acc, a.counters != nullptr, lane, nd, fe, ferr, fax);
        rxc_wave_sync();                                             // the next packet overwrites the planes
    }
    rxc_flush(acc, a.counters);
}

static void track_launch(const StreamDecoder *dec, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const DecArgs &d,
                         const uint32_t *payload) {
    TrackArgs a{};
    a.x = d.x;
    a.n = d.n;
    a.count = d.count;
    a.pk = d.pk;
    a.bits = d.bits;
    a.eq = d.eq;
    a.phase = (float *)dec->out;
    a.counters = d.counters;
    a.n_data = d.n_data;
    a.float_cfo = d.float_cfo;
    a.plane = d.plane;
    a.wave_floats = d.wave_floats;
    std::copy(d.taps, d.taps + 21, a.taps);
    std::copy(payload, payload + 3 * d.n_data, a.words);
    hipLaunchKernelGGL(stream_decode_track_kernel, grid, block, lds, stream, a);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_receive_stream_tracked(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                                           const ofdm_stream_opts *sopts, int timing, int tracking, int payload,
                                           int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq,
                                           void *d_counters, void *d_metric, void *d_cross, void *d_timing, void *d_phase) {
    if (tracking != OFDM_TRACK_NONE && tracking != OFDM_TRACK_PILOTS)
        return set_error(OFDM_E_ARG, "tracking must be OFDM_TRACK_NONE (0) or OFDM_TRACK_PILOTS (1), got %d", tracking);
    if (tracking == OFDM_TRACK_NONE && d_phase)
        return set_error(OFDM_E_ARG, "d_phase needs OFDM_TRACK_PILOTS: tracking is OFDM_TRACK_NONE");
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    // no tracking is ofdm_receive_stream_timed itself: the same launches, byte-identical outputs
    if (tracking == OFDM_TRACK_NONE)
        return stream_receive_timed(c, d_samples, n_samples, opts, sopts, timing, payload, max_packets, d_packets, d_count,
                                    d_bits, d_eq, d_counters, d_metric, d_cross, d_timing, nullptr);
    StreamDecoder dec{};
    dec.kernel = OFDM_K_STREAM_DECODE_TRACK;
    dec.launch = track_launch;
    dec.name = "stream_decode_track_kernel";
    dec.out = d_phase;
    return stream_receive_timed(c, d_samples, n_samples, opts, sopts, timing, payload, max_packets, d_packets, d_count,
                                d_bits, d_eq, d_counters, d_metric, d_cross, d_timing, &dec);
}
