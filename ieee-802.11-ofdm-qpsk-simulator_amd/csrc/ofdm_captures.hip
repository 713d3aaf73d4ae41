// ofdm_captures.hip -- Receiver() (OFDM.c:941-1165) over a device-resident batch of caller-supplied complex
// captures (include/ofdm_mi355x_captures.h: ofdm_receive_captures), in a translation unit of its own: the kernels of
// ofdm_frame.hip / ofdm_frame_xl.hip draw their captures themselves (real-only noise, imaginary parts from a table of
// the clean waveform) and are certified by build id, so nothing of theirs moves.  This kernel shares only the inlined
// device helpers (FFT, equaliser, demap, atan2) with them.
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
//     Coarse_CFO_Estimation and Fine_CFO_Estimation (OFDM.c:773-828), one combined rotation;
//     per symbol: a lane holds one 64-point window in registers (lane 0 of a quad the LTF pair's sum, lanes 1..3
//       three data symbols), FFT, LS estimate, ZF, slicer, demap, EVM and BER (OFDM.c:830-1165) with the helpers of
//       ofdm_rxcommon.h.
//   One record per capture; the counters row is reduced per block in LDS and added with 64-bit vector atomics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "ofdm_mi355x_captures.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"

namespace ofdm {

constexpr int CAPRX_MAX_DATA = LONG_MAX_FRAMES;
constexpr int CAPRX_MAX_WAVES = 8;                    // 512 threads: two waves per SIMD, 256 VGPRs each
constexpr size_t CAPRX_LDS_PER_CU = 160 * 1024;
constexpr int CAPRX_ACC_WORDS = OFDM_NCOUNTERS;       // the block's counter row (64-bit words) ahead of the waves' regions
constexpr double CAPRX_TS = 1.0 / 20e6;               // OFDM.c:16-17
constexpr int CAPRX_SPEC_PITCH = 130;                 // floats per parked spectrum (64 float2 + one: 8-byte accesses, 2 banks apart)
// long training tones with L_k = -1 (ofdm_device.h ltf_sign), bit k
constexpr uint64_t caprx_ltf_neg() {
    uint64_t v = 0;
    for (int b = 0; b < 64; ++b) v |= (uint64_t)(ltf_sign(b) < 0) << b;
    return v;
}
constexpr uint64_t CAPRX_LTF_NEG = caprx_ltf_neg();
static_assert(sizeof(ofdm_capture_result) == 48, "ofdm_capture_result is 48 bytes");

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
    uint32_t dtable[4 * CAPRX_MAX_DATA];   // demap words of the payload (ofdm_rxcommon.h demap_words)
    uint32_t ztable[CAPRX_MAX_DATA];       // per data symbol, were it all zeros: bit errors | slicer axis errors << 16 (caprx_zero_errors)
};

// The errors of a data symbol that arrives as 64 exact zeros (its window lies wholly past the capture's end): the
// reference's slicer decides "-" on both axes for a zero (Z > 0 fails, OFDM.c:858-866), the demapper then (1, 0) for
// every pair (OFDM.c:873-908), so the counts depend on the payload alone.  w: the symbol's 96 payload bits, MSB first.
// An axis is wrong where the truth is "+": re > 0 iff b0 == b1, im > 0 iff b0 == 0 (D10).
static uint32_t caprx_zero_errors(const uint32_t w[3]) {
    uint32_t be = 0u, ax = 0u;
    for (int k = 0; k < 3; ++k) be += (uint32_t)__builtin_popcount(w[k] ^ 0xAAAAAAAAu);
    for (int m = 0; m < 48; ++m) {
        const uint32_t b0 = (w[(2 * m) >> 5] >> (31 - ((2 * m) & 31))) & 1u;
        const uint32_t b1 = (w[(2 * m + 1) >> 5] >> (31 - ((2 * m + 1) & 31))) & 1u;
        ax += (uint32_t)(b0 == b1) + (uint32_t)(b0 == 0u);
    }
    return be | (ax << 16);
}

// LDS ordering between the lanes of one wave (the block's other waves run other captures)
__device__ __forceinline__ void caprx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float caprx_sum_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
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
// rotate by exp(-j 2 pi f Ts i): the phase in revolutions in fp64, range-reduced, then v_sin / v_cos (OFDM.c:802,825)
__device__ __forceinline__ float2 caprx_rot(float2 v, double f_ts, int i) {
    const double rev = -f_ts * (double)i;
    const float fr = (float)(rev - rint(rev));
    const float s = __builtin_amdgcn_sinf(fr), c = __builtin_amdgcn_cosf(fr);
    return make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
}
// frame sample ii is one the receiver uses: STF tail [80, 112), LTF pair [192, 320), data symbols past their prefixes
__device__ __forceinline__ bool caprx_needed(int ii) {
    if (ii < 192) return ii >= 80 && ii < 112;
    if (ii < 320) return true;
    const int r = (ii - 320) % 80;
    return r >= 16;
}

template <bool OUT>   // OUT: d_bits and / or d_eq are written; without them the records and counters alone
__global__ __launch_bounds__(64 * CAPRX_MAX_WAVES) void capture_rx_kernel(CapArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long caprx_smem[];
    unsigned long long *acc = caprx_smem;
    // wave-uniform values are made scalar (readfirstlane): the capture index, the LDS bases and packet_idx stay out of the VGPRs
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int L = a.cap_len, Lc = L - 47, nd = a.n_data, nfr = 320 + 80 * nd, plane = a.plane;
    float *re = reinterpret_cast<float *>(caprx_smem + CAPRX_ACC_WORDS) + (size_t)wave * a.wave_floats;
    float *im = re + plane;
    uint32_t *cross = reinterpret_cast<uint32_t *>(re + a.wave_floats - a.cross_words);
    if (threadIdx.x < CAPRX_ACC_WORDS) acc[threadIdx.x] = 0ull;
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
        caprx_wave_sync();
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
        caprx_wave_sync();
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
            if (!caprx_needed(ii)) continue;
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
        caprx_wave_sync();
        // ---- Coarse_CFO_Estimation, Fine_CFO_Estimation (OFDM.c:773-828) ----
        double fc, ff;
        {
            const int k = lane & 15;
            const float2 cu = make_float2(fre[80 + k], fim[80 + k]), cw = make_float2(fre[96 + k], fim[96 + k]);
            float2 pp = lane < 16 ? cmulc(cu, cw) : make_float2(0.f, 0.f);
            pp.x = caprx_sum_f(pp.x);
            pp.y = caprx_sum_f(pp.y);
            fc = (-1.0 / (2.0 * M_PI * 16.0 * CAPRX_TS)) * (double)atan2_cfo(pp.y, pp.x);
            if (a.float_cfo) fc = (double)(float)fc;
            const float2 u = caprx_rot(make_float2(fre[192 + lane], fim[192 + lane]), fc * CAPRX_TS, 192 + lane);
            const float2 w = caprx_rot(make_float2(fre[256 + lane], fim[256 + lane]), fc * CAPRX_TS, 256 + lane);
            pp = cmulc(u, w);
            pp.x = caprx_sum_f(pp.x);
            pp.y = caprx_sum_f(pp.y);
            ff = (-1.0 / (2.0 * M_PI * 64.0 * CAPRX_TS)) * (double)atan2_cfo(pp.y, pp.x);
            if (a.float_cfo) ff = (double)(float)ff;
        }
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
        // ---- the combined rotation in place, 64 samples per step: the LTF pair's sum over LTF1 (H = 0.5 (F1 + F2) conj(Lf) and
        // fft() is linear), then the data windows ----
        {
            const double fcf_ts = (fc + ff) * CAPRX_TS;
            const int k = 192 + lane;
            const float2 u = caprx_rot(make_float2(fre[k], fim[k]), fcf_ts, k);
            const float2 w = caprx_rot(make_float2(fre[k + 64], fim[k + 64]), fcf_ts, k + 64);
            fre[k] = u.x + w.x;
            fim[k] = u.y + w.y;
            for (int d = 0; d < nd; ++d) {
                const int kd = 336 + 80 * d + lane;
                const float2 v = caprx_rot(make_float2(fre[kd], fim[kd]), fcf_ts, kd);
                fre[kd] = v.x;
                fim[kd] = v.y;
            }
        }
        caprx_wave_sync();
        // ---- symbols: quad {LTF1 + LTF2, D_3q, D_3q+1, D_3q+2}; fft() = DFT(x (-1)^n) ----
        const int role = lane & 3, dsym = 3 * (lane >> 2) + max(role - 1, 0), dsc = min(dsym, nd - 1);
        const bool dlane = role >= 1 && dsym < nd;
        const int k0 = role == 0 ? 192 : 336 + 80 * dsc;
        float2 x[64];
        static_for<0, 64>([&](auto nc) {
            constexpr int n = decltype(nc)::value;
            const float vx = fre[k0 + n], vy = fim[k0 + n];
            x[n] = (n & 1) ? make_float2(-vx, -vy) : make_float2(vx, vy);
        });
        static_for<0, 16>([&](auto jc) { dif_stage1<false, decltype(jc)::value>(x); });
        const uint32_t wd[4] = {a.dtable[4 * dsc], a.dtable[4 * dsc + 1], a.dtable[4 * dsc + 2], a.dtable[4 * dsc + 3]};
        SymState st;
        sym_init(st);
        auto Hof = [&](float2 Y, auto binc) { return ls_equalise<decltype(binc)::value>(Y); };
        // OUT: every window is in registers by now, so the wave's region is free: the quads in use park their finished
        // spectra there, sub-block by sub-block (row pitch CAPRX_SPEC_PITCH floats: the lanes' 8-byte writes fall on
        // distinct banks), for the output pass below
        // (no branch around the writes -- control flow inside the transform costs 60 spilled VGPRs: the idle lanes
        // share one more row that nobody reads)
        [[maybe_unused]] float2 *spec_row = reinterpret_cast<float2 *>(re + min(lane, 4 * ((nd + 2) / 3)) * CAPRX_SPEC_PITCH);
        if constexpr (OUT) caprx_wave_sync();
        static_for<0, 4>([&](auto rc) {
            constexpr int R = decltype(rc)::value;
            dif_sub16<false, R>(x);
            demap_sub<false, R, 2>(x, wd[R], Hof, nullptr, st);
            sched_fence();
            if constexpr (OUT) {
                static_for<0, 16>([&](auto kc) {
                    constexpr int bin = 4 * decltype(kc)::value + R;
                    spec_row[bin] = x[digit_rev4(bin)];
                });
                sched_fence();
            }
        });
        // OUT: the equalised subcarriers Z = Y / H = 2 Lf Y conj(S) / |S|^2 and the decided bits (OFDM.c:1044-1052,
        // 852-908), one subcarrier per lane and step: coalesced stores, a 16-lane OR per word of 32 bits.  (Taken from
        // the lanes' registers inside the metrics pass they cost 113 spilled VGPRs.)
        if constexpr (OUT) {
            caprx_wave_sync();
            const int nsc = 48 * nd;
            for (int j0 = 0; j0 < nsc; j0 += 64) {
                const int j = j0 + lane;
                const bool ok = j < nsc;
                const int jj = ok ? j : 0, d = jj / 48, m = jj - 48 * d, bin = data_bin(m);
                const int l0 = 4 * (d / 3), ln = l0 + 1 + d % 3;
                const float2 Y = reinterpret_cast<const float2 *>(re + ln * CAPRX_SPEC_PITCH)[bin];
                const float2 S = reinterpret_cast<const float2 *>(re + l0 * CAPRX_SPEC_PITCH)[bin];
                const float r = __builtin_amdgcn_rcpf(fmaf(S.x, S.x, S.y * S.y));
                const float g = ((CAPRX_LTF_NEG >> bin) & 1ull) ? -2.0f * r : 2.0f * r;
                const float2 u = cmulc(Y, S);
                const float2 z = make_float2(u.x * g, u.y * g);
                if (a.eq && ok) a.eq[i * nsc + j] = z;
                const uint32_t pr = z.x > 0.f, pi = z.y > 0.f;
                uint32_t wv = ok ? (((pi ^ 1u) << 1) | (pr ^ pi)) << (30 - 2 * (lane & 15)) : 0u;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) wv |= (uint32_t)__shfl_xor((int)wv, o, 64);
                if (a.bits && ok && (lane & 15) == 0) a.bits[i * (3 * nd) + (j >> 4)] = wv;
            }
        }
        // ---- the capture's totals in symbol order, its record and its counter terms ----
        // A data symbol whose window lies wholly past the capture's end (sample p + 2 (336 + 80 d) and all after it are
        // at L + 20 or beyond) reached the demapper as 64 exact zeros: Y = +-0 and u = +-0, and the sign bit of u, which
        // demap_sub counts, is then an accident of S.  The reference decides "-" on both axes for a zero, as the output
        // pass above does, so that symbol's counts are the payload's own (ztable).  Those symbols are zfirst .. D - 1
        // (none unless oob); the branch is wave-uniform and rare, and it stands here, after the transforms (a branch
        // inside them costs 60 spilled VGPRs).  Its EVM term needs nothing: u' = +-0 gives |0 - d|^2 either way.
        const float fev = dlane ? finish_evm<2>(st) : 0.f;
        const uint32_t bev = dlane ? st.be : 0u, axv = dlane ? st.ax : 0u;
        float fe = 0.f;
        uint32_t ferr = 0u, fax = 0u;
        for (int d = 0; d < nd; ++d) {
            const int src = 4 * (d / 3) + 1 + d % 3;
            fe += __shfl(fev, src, 64);
            ferr += (uint32_t)__shfl((int)bev, src, 64);
            fax += (uint32_t)__shfl((int)axv, src, 64);
        }
        if (zfirst < nd) {
            for (int d = zfirst; d < nd; ++d) {
                const int src = 4 * (d / 3) + 1 + d % 3;
                const uint32_t z = a.ztable[d];
                ferr += (z & 0xffffu) - (uint32_t)__shfl((int)bev, src, 64);
                fax += (z >> 16) - (uint32_t)__shfl((int)axv, src, 64);
            }
        }
        if (lane == 0) {
            const float N = 48.0f * (float)nd;
            // a NaN sum (the long training symbols themselves past the end: S = 0, Z = 0 / 0) stays NaN, as the reference's
            const float db = fe > 0.f ? fmaxf(3.01029995663981195214f * __builtin_amdgcn_logf(fe / N), -400.f)
                                      : (fe == fe ? -400.f : fe);
            const float dbp = fax > 0u ? 3.01029995663981195214f * __builtin_amdgcn_logf(2.0f * (float)fax / N) : -INFINITY;
            ofdm_capture_result *r = a.res + i;
            r->bit_err = (int32_t)ferr;
            r->post_axis_err = (int32_t)fax;
            r->evm_pre_sum = fe;
            r->evm_db_pre = db;
            r->evm_db_post = dbp;
            r->ber = (float)ferr / (96.0f * (float)nd);
            if (a.counters) {
                const float Q = (float)OFDM_EVM_Q_SCALE;             // x 2^20 is exact in fp32
                atomicAdd(&acc[OFDM_C_FRAMES], 1ull);
                atomicAdd(&acc[OFDM_C_SYMBOLS], (unsigned long long)nd);
                atomicAdd(&acc[OFDM_C_BITS], 96ull * nd);
                atomicAdd(&acc[OFDM_C_EVM_TERMS], 48ull * nd);
                atomicAdd(&acc[OFDM_C_BIT_ERR], (unsigned long long)ferr);
                atomicAdd(&acc[OFDM_C_FRAME_ERR], (unsigned long long)(ferr > 0u));
                atomicAdd(&acc[OFDM_C_EVM_POST_AXIS], (unsigned long long)fax);
                if (fabsf(fe) < INFINITY) {                          // a non-finite term is left out, never converted
                    atomicAdd(&acc[OFDM_C_EVM_PRE_Q], (unsigned long long)__float2ll_rn(fe * Q));
                    atomicAdd(&acc[OFDM_C_EVMDB_PRE_Q], (unsigned long long)__float2ll_rn(db * Q));
                }
                if (fax > 0u) {
                    atomicAdd(&acc[OFDM_C_EVMDB_POST_Q], (unsigned long long)__float2ll_rn(dbp * Q));
                    atomicAdd(&acc[OFDM_C_EVMDB_POST_FINITE], 1ull);
                }
            }
        }
        caprx_wave_sync();                                           // the next capture overwrites the planes
    }
    __syncthreads();
    if (a.counters && threadIdx.x < CAPRX_ACC_WORDS && acc[threadIdx.x]) atomicAdd(&a.counters[threadIdx.x], acc[threadIdx.x]);
}

// rcosdesign(0.5, 10, 2, 'sqrt') (Tester.m:112; OFDM.c:32 holds the same values as floats)
static void caprx_taps(float out[21]) {
    const double beta = 0.5, sps = 2.0, pi = M_PI;
    double h[21], e = 0.0;
    for (int i = 0; i < 21; ++i) {
        const double t = (i - 10) / sps, q = 4 * beta * t;
        double b;
        if (t == 0.0) b = -1.0 / (pi * sps) * (pi * (beta - 1) - 4 * beta);
        else if (std::fabs(std::fabs(q) - 1.0) < 1e-12)
            b = 1.0 / (2 * pi * sps) * (pi * (beta + 1) * std::sin(pi * (beta + 1) / (4 * beta)) -
                                        4 * beta * std::sin(pi * (beta - 1) / (4 * beta)) +
                                        pi * (beta - 1) * std::cos(pi * (beta - 1) / (4 * beta)));
        else
            b = -4 * beta / sps * (std::cos((1 + beta) * pi * t) + std::sin((1 - beta) * pi * t) / q) / (pi * (q * q - 1));
        h[i] = b;
        e += b * b;
    }
    for (int i = 0; i < 21; ++i) out[i] = (float)(h[i] / std::sqrt(e));
    for (int i = 0; i < 10; ++i) out[20 - i] = out[i];
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
        a.ztable[d] = caprx_zero_errors(table + 3 * d);
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
    const int spec_floats = (4 * ((a.n_data + 2) / 3) + 1) * CAPRX_SPEC_PITCH;
    a.wave_floats = ((std::max(2 * a.plane + (a.fr_sep ? 2 * nfr : 0), spec_floats) + 3) & ~3) + a.cross_words;
    caprx_taps(a.taps);
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    // waves per block from the capture's LDS against the CU's 160 KiB; the request is checked before the launch
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess || lds_max <= 0)
        return set_error(OFDM_E_HIP, "cannot query the device's LDS size");
    const size_t limit = std::min<size_t>((size_t)lds_max, CAPRX_LDS_PER_CU);
    const size_t head = CAPRX_ACC_WORDS * sizeof(unsigned long long), per_wave = (size_t)a.wave_floats * sizeof(float);
    if (head + per_wave > limit)
        return set_error(OFDM_E_ARG, "a %d-sample capture needs %zu bytes of LDS, above the %zu available", L, head + per_wave, limit);
    const int W = (int)std::min<int64_t>(std::min<int64_t>(CAPRX_MAX_WAVES, (int64_t)((limit - head) / per_wave)), n);
    const size_t lds = head + (size_t)W * per_wave;
    if (lds > limit) return set_error(OFDM_E_ARG, "dynamic LDS request %zu above the limit %zu", lds, limit);
    const int64_t blocks = (n + W - 1) / W;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 2 * (int64_t)c->cus));
    if (a.bits || a.eq) hipLaunchKernelGGL(capture_rx_kernel<true>, grid, dim3(64 * W), lds, c->stream, a);
    else hipLaunchKernelGGL(capture_rx_kernel<false>, grid, dim3(64 * W), lds, c->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "capture_rx_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
