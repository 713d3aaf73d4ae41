// ofdm_captures.hip -- Receiver() (OFDM.c:941-1165) over a device-resident batch of caller-supplied complex
// captures (include/ofdm_mi355x_captures.h: ofdm_receive_captures), in a translation unit of its own: the kernels of
// ofdm_frame.hip / ofdm_frame_xl.hip draw their captures themselves (real-only noise, imaginary parts from a table of
// the clean waveform) and are certified by build id, so nothing of theirs moves.  This kernel shares the inlined
// device helpers (FFT, equaliser, demap, atan2) with them, and the chain after packet selection (ofdm_rxchain.h) with
// the stream receiver's decode kernels.
//
//   capture_rx_kernel : one WAVE per capture, W waves per block.  A wave stages its capture in dynamic LDS as separate
//   real and imaginary planes (8 cap_len bytes) and runs the whole chain on it:
//     Packet_Detection (OFDM.c:659-683) on the unfiltered capture -- delay 16, window 32, no conjugate, cap_len - 47
//       positions: a lane owns `run` contiguous positions (run odd, so the lanes' strides fall on distinct banks),
//       opens with a direct 32-term sum and slides; threshold crossings go into a bitmap of the wave;
//     Packet_Selection (OFDM.c:685-771): 0.75, fronts more than 300 apart, the +230 check, front + 11;
//     the 21-tap RRC matched filter (OFDM.c:962-992) only at the down-sampled instants packet_idx + 2 i that the
//       receiver uses (STF tail, LTF pair, the data symbols past their prefixes), written into the part of the planes
//       the filter does not read;
//     then ofdm_rxchain.h's stages: Coarse_CFO_Estimation and Fine_CFO_Estimation (OFDM.c:773-828), one combined
//       rotation; per symbol a lane holds one 64-point window in registers (lane 0 of a quad the LTF pair's sum, lanes
//       1..3 three data symbols), FFT, LS estimate, ZF, slicer, demap, EVM and BER (OFDM.c:830-1165) with the helpers
//       of ofdm_rxcommon.h.
//   One record per capture; the counters row is reduced per block in LDS and added with 64-bit vector atomics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "ofdm_mi355x_captures.h"
#include "ofdm_ctx.h"
#include "ofdm_rxchain.h"

namespace ofdm {

struct CapArgs {
    const float2 *cap;
    int64_t n, pitch;
    ofdm_capture_result *res;
    uint32_t *bits;
    float2 *eq;
    unsigned long long *counters;
    int32_t cap_len, n_data, float_cfo;
    int32_t run;             // detection positions per lane (odd)
    int32_t plane;           // floats per plane (cap_len rounded up to 4)
    int32_t wave_floats;     // floats per wave: two planes, the separate fr[] when fr_sep, the crossing bitmap
    int32_t cross_words;     // bitmap words (32 positions each)
    int32_t fr_sep;          // 1: fr[] has an area of its own (captures too short to hold it beside the filter's reads)
    float taps[21];
    uint32_t dtable[4 * RXC_MAX_DATA];     // demap words of the payload (ofdm_rxcommon.h demap_words)
    uint32_t ztable[RXC_MAX_DATA];         // per data symbol, were it all zeros: bit errors | slicer axis errors << 16 (zero_errors)
};

__device__ __forceinline__ int caprx_min_i(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int caprx_max_i(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}


template <bool OUT>   // OUT: d_bits and / or d_eq are written; without them the records and counters alone
__global__ __launch_bounds__(64 * RXC_MAX_WAVES) void capture_rx_kernel(CapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long caprx_smem[];
    unsigned long long *acc = caprx_smem;
    // wave-uniform values are made scalar (readfirstlane): the capture index, the LDS bases and packet_idx stay out of the VGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int L = a.cap_len, Lc = L - 47, nd = a.n_data, nfr = 320 + 80 * nd, plane = a.plane;
    float *re = reinterpret_cast<float *>(caprx_smem + RXC_ACC_WORDS) + (size_t)wave * a.wave_floats;
    float *im = re + plane;
    uint32_t *cross = reinterpret_cast<uint32_t *>(re + a.wave_floats - a.cross_words);
    if (threadIdx.x < RXC_ACC_WORDS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * W + wave; i < a.n; i += (int64_t)gridDim.x * W) {
        // ---- stage the capture: 16-byte loads of two complex samples, planes in LDS; the tail and the bitmap zeroed ----
        {
            const float2 *row = a.cap + i * a.pitch;
            const int head = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1u);     // 1: row starts 8 bytes off a 16-byte line
            if (head && lane == 0) { const float2 v = row[0]; re[0] = v.x; im[0] = v.y; }
            const f4v *r4 = reinterpret_cast<const f4v *>(row + head);
            const int np = (L - head) >> 1;
            for (int k = lane; k < np; k += 64) {
                const f4v v = __builtin_nontemporal_load(r4 + k);
                const int m = head + 2 * k;
                re[m] = v.x; im[m] = v.y; re[m + 1] = v.z; im[m + 1] = v.w;
            }
            if (((L - head) & 1) && lane == 0) { const float2 v = row[L - 1]; re[L - 1] = v.x; im[L - 1] = v.y; }
            for (int k = L + lane; k < plane; k += 64) { re[k] = 0.f; im[k] = 0.f; }
            for (int k = lane; k < a.cross_words; k += 64) cross[k] = 0u;
        }
        rxc_wave_sync();
        // ---- Packet_Detection: this lane's positions [n0, n0 + cnt) ----
        int first = -1, last = -1;
        {
            const int n0 = lane * a.run, cnt = min(a.run, Lc - n0);
            if (cnt > 0) {
                float sx = 0.f, sy = 0.f, pw = 0.f;
#pragma unroll 8
                for (int k = 0; k < 32; ++k) {
                    const float ux = re[n0 + k], uy = im[n0 + k], vx = re[n0 + k + 16], vy = im[n0 + k + 16];
                    sx = fmaf(ux, vx, sx); sx = fmaf(-uy, vy, sx);
                    sy = fmaf(ux, vy, sy); sy = fmaf(uy, vx, sy);
                    pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
                }
                for (int j = 0; j < cnt; ++j) {
                    const int n = n0 + j;
                    const float num = fmaf(sx, sx, sy * sy), h = 0.75f * pw;
                    if (fmaf(h, pw, -num) < 0.f) {                 // |c|^2 / p^2 > 0.75
                        atomicOr(&cross[n >> 5], 1u << (n & 31));
                        first = first < 0 ? n : first;
                        last = n;
                    }
                    if (j + 1 < cnt) {                             // n + 48 <= cap_len - 1
                        const float o0x = re[n], o0y = im[n], o1x = re[n + 16], o1y = im[n + 16];
                        const float i0x = re[n + 32], i0y = im[n + 32], i1x = re[n + 48], i1y = im[n + 48];
                        sx = fmaf(i0x, i1x, sx); sx = fmaf(-i0y, i1y, sx);
                        sx = fmaf(-o0x, o1x, sx); sx = fmaf(o0y, o1y, sx);
                        sy = fmaf(i0x, i1y, sy); sy = fmaf(i0y, i1x, sy);
                        sy = fmaf(-o0x, o1y, sy); sy = fmaf(-o0y, o1x, sy);
                        pw = fmaf(i1x, i1x, pw); pw = fmaf(i1y, i1y, pw);
                        pw = fmaf(-o1x, o1x, pw); pw = fmaf(-o1y, o1y, pw);
                    }
                }
            }
        }
        rxc_wave_sync();
        // ---- Packet_Selection: a lane's run is shorter than 300, so only its first crossing can be a front ----
        int p;
        bool sync_fail;
        {
            int pm = last;                                           // inclusive prefix max of the last crossings
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(pm, o, 64);
                pm = lane >= o ? max(pm, t) : pm;
            }
            int prev = __shfl_up(pm, 1, 64);
            prev = lane == 0 ? -1 : prev;
            const int front = (first >= 0 && first - prev > 300) ? first : -1;
            const int pos = front + 230;
            const bool in = front >= 0 && pos < Lc;
            const uint32_t wbits = cross[in ? pos >> 5 : 0];
            const bool valid = in && ((wbits >> (pos & 31)) & 1u);
            // the first front with a crossing at + 230 that is not the last front (OFDM.c:745-760)
            const int cmin = caprx_min_i(valid ? front : 0x7fffffff), cmax = caprx_max_i(front);
            sync_fail = __builtin_amdgcn_readfirstlane((int)!(cmin < cmax)) != 0;
            p = __builtin_amdgcn_readfirstlane(sync_fail ? 0 : cmin + 10 + 1);                      // len_RRC_rx + 1 (OFDM.c:758)
        }
        // ---- RRC matched filter at the down-sampled instants; fr[] beside the samples it reads ----
        float *fre, *fim;
        {
            const int lo = max(p - 20, 0), hi = min(p + 2 * nfr - 2, L - 1);
            if (a.fr_sep) { fre = re + 2 * plane; fim = fre + nfr; }
            else if (lo >= nfr) { fre = re; fim = im; }
            else { fre = re + hi + 1; fim = im + hi + 1; }           // hi + 1 + nfr <= plane (host: cap_len >= 4 nfr + 20)
        }
        const bool oob = p + 2 * (nfr - 1) >= L + 20;                // the reference reads past its buffer
        // the first data symbol wholly past the end: the least d >= 0 with p + 2 (336 + 80 d) >= L + 20; D when none
        const int zfirst = min(max((L - 652 - p + 159) / 160, 0), nd);
        for (int ii = lane; ii < nfr; ii += 64) {
            if (!rxc_needed(ii)) continue;
            const int n = p + 2 * ii;
            float vx = 0.f, vy = 0.f;
            if (n >= 20 && n < L) {
#pragma unroll
                for (int tt = 0; tt < 21; ++tt) {
                    vx = fmaf(re[n - tt], a.taps[tt], vx);
                    vy = fmaf(im[n - tt], a.taps[tt], vy);
                }
            } else if (n < L + 20) {
#pragma unroll
                for (int tt = 0; tt < 21; ++tt) {
                    const int m = n - tt;
                    const bool in = m >= 0 && m < L;
                    const int mc = in ? m : 0;
                    vx = fmaf(in ? re[mc] : 0.f, a.taps[tt], vx);
                    vy = fmaf(in ? im[mc] : 0.f, a.taps[tt], vy);
                }
            }
            fre[ii] = vx;
            fim[ii] = vy;
        }
        rxc_wave_sync();
        double fc, ff;
        rxc_cfo(fre, fim, lane, a.float_cfo, fc, ff);
        // the sync half of the record and its counter terms leave here, so nothing of it stays live over the transforms
        if (lane == 0) {
            ofdm_capture_result *r = a.res + i;
            r->packet_idx = p;
            r->flags = (sync_fail ? OFDM_CAPTURE_SYNC_FAIL : 0) | (oob ? OFDM_CAPTURE_OOB : 0);
            r->cfo_coarse_hz = (float)fc;
            r->cfo_fine_hz = (float)ff;
            r->reserved[0] = 0;
            r->reserved[1] = 0;
            if (a.counters) {
                atomicAdd(&acc[OFDM_C_SYNC_FAIL], (unsigned long long)sync_fail);
                atomicAdd(&acc[OFDM_C_OOB], (unsigned long long)oob);
            }
        }
        rxc_rotate(fre, fim, lane, nd, fc, ff);
        rxc_wave_sync();
        const RxcQuad qd = rxc_quad(lane, nd);
        float2 x[64];
        rxc_window(fre, fim, qd.k0, x);
        SymState st;
        rxc_demap<OUT>(x, a.dtable, qd.dsc, re, lane, nd, st);
        if constexpr (OUT) rxc_outputs(re, lane, nd, i, a.eq, a.bits);
        float fe;
        uint32_t ferr, fax;
        rxc_totals(st, qd.dlane, nd, zfirst, a.ztable, fe, ferr, fax);
        rxc_record(a.res + i, acc, a.counters != nullptr, lane, nd, fe, ferr, fax);
        rxc_wave_sync();                                             // the next capture overwrites the planes
    }
    rxc_flush(acc, a.counters);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_receive_captures(ofdm_ctx *ctx, const void *d_captures, int64_t n, int64_t pitch,
                                     const ofdm_rx_opts *opts, int payload, void *d_results, void *d_bits, void *d_eq,
                                     void *d_counters) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (!opts) return set_error(OFDM_E_ARG, "opts is NULL");
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (payload != OFDM_PAYLOAD_MESSAGE && payload != OFDM_PAYLOAD_TESTER)
        return set_error(OFDM_E_ARG, "captures are decoded against a fixed payload (MESSAGE or TESTER), got %d", payload);
    if (opts->word_stats) return set_error(OFDM_E_ARG, "word_stats is not available for caller-supplied captures");
    if (n == 0) return OFDM_OK;
    if (!d_captures || !d_results) return set_error(OFDM_E_ARG, "d_captures and d_results are required");
    CapArgs a{};
    uint32_t table[3 * LONG_MAX_FRAMES];
    a.n_data = payload_table_long(payload, c->message, table);
    for (int d = 0; d < a.n_data; ++d) {
        demap_words(table + 3 * d, a.dtable + 4 * d);
        a.ztable[d] = zero_errors(table + 3 * d);
    }
    const int nfr = 320 + 80 * a.n_data;
    const int L = opts->cap_len ? opts->cap_len : (int)(10 * (2 * nfr + 20) * 0.307);     // OFDM.c:945
    if (L < 400 || L > OFDM_CAPTURE_MAX_LEN)
        return set_error(OFDM_E_ARG, "cap_len %d must be in [400, %d]", L, OFDM_CAPTURE_MAX_LEN);
    if (pitch < L) return set_error(OFDM_E_ARG, "pitch %lld is below cap_len %d", (long long)pitch, L);
    if (reinterpret_cast<uintptr_t>(d_captures) & 7u) return set_error(OFDM_E_ARG, "d_captures must be 8-byte aligned");
    a.cap = (const float2 *)d_captures;
    a.n = n;
    a.pitch = pitch;
    a.res = (ofdm_capture_result *)d_results;
    a.bits = (uint32_t *)d_bits;
    a.eq = (float2 *)d_eq;
    a.counters = (unsigned long long *)d_counters;
    a.cap_len = L;
    a.float_cfo = opts->float_cfo;
    a.run = ((L - 47 + 63) / 64) | 1;
    a.plane = (L + 3) & ~3;
    a.cross_words = ((L - 47 + 31) / 32 + 3) & ~3;
    a.fr_sep = L < 4 * nfr + 20;
    // the region also parks the spectra of the quads in use for the output pass (4 ceil(D / 3) rows and one for the idle lanes)
    a.wave_floats = ((std::max(2 * a.plane + (a.fr_sep ? 2 * nfr : 0), rxc_spec_floats(a.n_data)) + 3) & ~3) + a.cross_words;
    rrc_design(a.taps);
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    // waves per block from the capture's LDS; the request is checked before the launch
    WaveBlock wb;
    if (wave_block(c, RXC_ACC_WORDS * sizeof(unsigned long long), (size_t)a.wave_floats * sizeof(float), RXC_MAX_WAVES, n, &wb))
        return OFDM_E_HIP;
    if (!wb.W) return set_error(OFDM_E_ARG, "a %d-sample capture needs %zu bytes of LDS, above the %zu available", L, wb.lds, wb.limit);
    const int W = wb.W;
    const size_t lds = wb.lds;
    const int64_t blocks = (n + W - 1) / W;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 2 * (int64_t)c->cus));
    if (a.bits || a.eq) hipLaunchKernelGGL(capture_rx_kernel<true>, grid, dim3(64 * W), lds, c->stream, a);
    else hipLaunchKernelGGL(capture_rx_kernel<false>, grid, dim3(64 * W), lds, c->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "capture_rx_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
