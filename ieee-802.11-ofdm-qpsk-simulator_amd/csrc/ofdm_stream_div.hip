// ofdm_stream_div.hip -- receive diversity for the stream receiver (include/ofdm_mi355x_diversity.h:
// ofdm_receive_stream_diversity).  A translation unit of its own: ofdm_stream.hip, ofdm_stream_conj.hip,
// ofdm_stream_timing.hip and ofdm_stream_track.hip keep their kernels as they are; this file adds three kernels and
// hands them to stream_receive through its three hooks (ofdm_stream_detect.h), whose `user` pointer carries the branch
// table.  The selection kernels run unchanged on the combined bitmap.  Every sum over branches runs b = 0, 1, .. in
// that order.
//
//   stream_detect_div_kernel<METRIC> : stream_detect_conj_kernel's shape (ofdm_stream_tile.h: 256 lanes, a tile of
//     OFDM_STREAM_TILE positions, runs of OFDM_STREAM_RUN positions with boundaries fixed in stream coordinates), the
//     branches staged in turn into the same two planes, each with its own alignment parity.  A lane keeps one total
//     (c, p) per position of its run -- the 3 x RUN registers conj_run holds -- and adds each branch's tails (the
//     descending pass over the run's first 32 terms) and heads (the ascending pass over the next) straight into them:
//     every total only ever grows by terms of its own window.  The decisions follow the last branch.
//   stream_timing_div_kernel : stream_timing_kernel's shape (ofdm_stream_ltf.h: one wave per packet, lane = candidate,
//     the template wave-uniform in SGPRs); the wave stages every branch's search window into planes of its own, sums
//     L_b[j] over the branches (each L_b as that kernel forms it), and lanes 8 b + s sum branch b's power in segment s
//     of the chosen window for the quality.
//   stream_decode_div_kernel : one wave per packet, W waves per block, looping over d_count, as
//     stream_decode_track_kernel.  Every branch is staged and matched-filtered by ofdm_stream_decode.h's stages into a
//     filtered frame of its own in the wave's LDS region; the coarse and fine carrier offsets come from the
//     branch-summed correlations (rxc_cfo's formulas).  Then per branch: ofdm_rxchain.h's rotation, window load,
//     transforms and parking, and with one bin per lane N_d[k] += Y_d[k] conj(S[k]), G[k] += |S[k]|^2 into an LDS area
//     of the wave's own before the next branch overwrites the rows (H = L S / 2, so z = N / G is
//     2 L sum Y conj(S) / sum |S|^2: for one branch, what rxc_equalised forms).  After the last branch: the pilot step
//     on N_d (lane 4 d + i, as stream_decode_track_kernel; skipped without tracking, u = 1) and that kernel's
//     subcarrier pass on z = N / G.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_diversity.h"
#include "ofdm_stream_decode.h"
#include "ofdm_stream_ltf.h"
#include "ofdm_stream_tile.h"

namespace ofdm {

constexpr int DV_MAX = OFDM_DIVERSITY_MAX_BRANCHES;
constexpr int DVT_WAVES = 4;                                  // stream_timing_div_kernel: packets per block and sweep
constexpr int DVT_BLOCKS_PER_CU = 8;                          // its grid's cap: the waves loop past it
static_assert(OFDM_K_STREAM_DETECT_DIV == Ctx::K_STREAM_DETECT_DIV && OFDM_K_STREAM_TIMING_DIV == Ctx::K_STREAM_TIMING_DIV &&
              OFDM_K_STREAM_DECODE_DIV == Ctx::K_STREAM_DECODE_DIV && Ctx::K_STREAM_DECODE_DIV < Ctx::NK,
              "the diversity kernels' ids are the context's");
static_assert(4 * RXC_MAX_DATA <= 64, "the pilot step is one step: lane 4 d + i");
static_assert(DV_MAX * TM_NSEG <= 64, "the quality's powers are one step: lane 8 b + s");

// the recordings, one per branch (a kernel argument: wave-uniform, read through the scalar cache)
struct DivBranches {
    const float2 *x[DV_MAX];
    int32_t nb;
};

// 1: the branch starts 8 bytes off a 16-byte line
__device__ __forceinline__ int div_parity(const float2 *x) { return (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1u); }

// ---- detection ----
// one branch's share of the run's totals: conj_run's two passes (ofdm_stream_conj.hip), added instead of assigned.  The
// run's positions are n0 + [0, RUN); term m is r[m] conj(r[m+32]) with the power |r[m+32]|^2.
__device__ __forceinline__ void div_run_add(int n0, const float *re, const float *im, float (&tx)[CD_RUN],
                                            float (&ty)[CD_RUN], float (&tp)[CD_RUN]) {
    {
        float sx = 0.f, sy = 0.f, pw = 0.f;
#pragma unroll
        for (int k = 31; k >= 0; --k) {                                // n0 + k + 32 <= n0 + 63, inside the planes
            const float ux = re[n0 + k], uy = im[n0 + k], vx = re[n0 + k + 32], vy = im[n0 + k + 32];
            sx = fmaf(ux, vx, sx); sx = fmaf(uy, vy, sx);              // u conj(v)
            sy = fmaf(uy, vx, sy); sy = fmaf(-ux, vy, sy);
            pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
            if (k < CD_RUN) { tx[k] += sx; ty[k] += sy; tp[k] += pw; }
            if ((k & 7) == 0) sched_fence();                           // the LDS reads stay 8 terms ahead, not 32: 93 totals are live
        }
    }
    float hx = 0.f, hy = 0.f, hp = 0.f;
#pragma unroll
    for (int j = 0; j + 1 < CD_RUN; ++j) {                             // n0 + j + 64 <= 255 RUN + 93 < TILE + 63
        const int m = n0 + 32 + j;
        const float ux = re[m], uy = im[m], vx = re[m + 32], vy = im[m + 32];
        hx = fmaf(ux, vx, hx); hx = fmaf(uy, vy, hx);
        hy = fmaf(uy, vx, hy); hy = fmaf(-ux, vy, hy);
        hp = fmaf(vx, vx, hp); hp = fmaf(vy, vy, hp);
        tx[j + 1] += hx; ty[j + 1] += hy; tp[j + 1] += hp;
        if ((j & 7) == 7) sched_fence();
    }
}
static_assert((CD_THREADS - 1) * CD_RUN + CD_RUN - 2 + 64 < DetShape<true>::SAMPLES, "the last lane's last term is staged");

template <bool METRIC>
__global__ __launch_bounds__(CD_THREADS, 2) void stream_detect_div_kernel(DetArgs a, float thr, DivBranches br) {
    using S = DetShape<true>;
    __shared__ __attribute__((aligned(16))) float re[S::PLANE];
    __shared__ __attribute__((aligned(16))) float im[S::PLANE];
    __shared__ __attribute__((aligned(16))) uint32_t bm[CD_WORDS];
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int64_t t0 = t * CD_TILE;
        // this lane's run: positions t0 + [n0, n0 + cnt)
        const int n0 = tid * CD_RUN;
        const int cnt = (int)std::min<int64_t>(CD_RUN, a.lc - (t0 + n0));
        float tx[CD_RUN], ty[CD_RUN], tp[CD_RUN];
#pragma unroll
        for (int j = 0; j < CD_RUN; ++j) { tx[j] = 0.f; ty[j] = 0.f; tp[j] = 0.f; }
#pragma unroll 1
        for (int b = 0; b < br.nb; ++b) {
            DetArgs ab = a;
            ab.x = br.x[b];
            det_stage<S>(ab, t0, div_parity(ab.x), re, im, bm);       // tiles start at even samples: one parity per branch
            __syncthreads();
            if (cnt > 0) div_run_add(n0, re, im, tx, ty, tp);
            __syncthreads();                                           // the next branch overwrites the planes
        }
        if (cnt > 0) {
#pragma unroll
            for (int j = 0; j < CD_RUN; ++j) {
                if (j >= cnt) break;
                det_decide<METRIC>(a, t0, n0 + j, tx[j], ty[j], tp[j], thr, bm);
            }
        }
        __syncthreads();
        det_store(a, t0, bm);
        __syncthreads();                                               // the next tile's staging clears the bitmap
    }
}

// ---- fine timing ----
__global__ __launch_bounds__(64 * DVT_WAVES) void stream_timing_div_kernel(TimArgs a, DivBranches br) {
    __shared__ float planes[DVT_WAVES][DV_MAX][2][TM_PLANE];
    __shared__ float power[DVT_WAVES][DV_MAX][TM_NSEG];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nb = br.nb;
    const int64_t cnt = a.count[1];
    for (int64_t i = (int64_t)blockIdx.x * DVT_WAVES + wave; i < cnt; i += (int64_t)gridDim.x * DVT_WAVES) {
        ofdm_stream_packet *pkt = a.pk + i;
        const int64_t pv = pkt->packet_pos;
        const int64_t p = ((int64_t)__builtin_amdgcn_readfirstlane((int)(pv >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)pv);
        int shift = 0;
        float quality = 0.f;
        // the whole search window inside the stream, or the packet keeps its position (wave-uniform)
        if (p + TM_FIRST >= 0 && p + TM_FIRST + TM_WINDOW - 1 < a.n) {
#pragma unroll 1
            for (int b = 0; b < nb; ++b) {
                const float2 *row = br.x[b] + (p + TM_FIRST);
                float *re = planes[wave][b][0], *im = planes[wave][b][1];
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
            }
            tm_wave_sync();
            // ---- L[lane] = sum_b L_b[lane], each L_b 8 segments of 32 terms x conj(t) ----
            float lam = 0.f;
#pragma unroll 1
            for (int b = 0; b < nb; ++b) {
                float lb = 0.f;
#pragma unroll 1
                for (int s = 0; s < TM_NSEG; ++s) {
                    const float *xr = planes[wave][b][0] + lane + TM_SEG * s, *xi = planes[wave][b][1] + lane + TM_SEG * s;
                    const float2 *t = a.t + ((TM_SEG * s) & (TM_PERIOD - 1));
                    float cx = 0.f, cy = 0.f;
#pragma unroll
                    for (int k = 0; k < TM_SEG; ++k) {
                        const float ur = xr[k], ui = xi[k], tr = t[k].x, ti = t[k].y;
                        cx = fmaf(ur, tr, cx); cx = fmaf(ui, ti, cx);
                        cy = fmaf(ui, tr, cy); cy = fmaf(-ur, ti, cy);
                    }
                    lb = fmaf(cx, cx, lb);
                    lb = fmaf(cy, cy, lb);
                }
                lam += lb;
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
                // ---- the chosen window's power per branch and segment, then the quality ----
                if (lane < TM_NSEG * nb) {
                    const int b = lane >> 3, s = lane & (TM_NSEG - 1);
                    const float *xr = planes[wave][b][0] + bj + TM_SEG * s, *xi = planes[wave][b][1] + bj + TM_SEG * s;
                    float e = 0.f;
#pragma unroll 8
                    for (int k = 0; k < TM_SEG; ++k) { e = fmaf(xr[k], xr[k], e); e = fmaf(xi[k], xi[k], e); }
                    power[wave][b][s] = e;
                }
                tm_wave_sync();
                float den = 0.f;
                for (int b = 0; b < nb; ++b)
#pragma unroll
                    for (int s = 0; s < TM_NSEG; ++s) den = fmaf(a.te[s], power[wave][b][s], den);
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

// ---- decode ----
struct DivArgs {
    DivBranches br;
    int64_t n;
    const int64_t *count;    // d_count: [1] records to decode
    ofdm_stream_packet *pk;
    uint32_t *bits;
    float2 *eq;
    float *phase;            // optional, [max_packets][D]
    float *gain;             // optional, [max_packets][B]
    unsigned long long *counters;
    int32_t n_data, float_cfo, track;
    int32_t plane;           // floats per staging plane (2 nfr + 19 rounded up to 4)
    int32_t work_floats;     // floats of the wave's working area: the two staging planes, later the parked spectra
    int32_t wave_floats;     // floats per wave: the working area, B filtered frames, N [D][64] and G [64]
    float taps[21];
    uint32_t words[3 * RXC_MAX_DATA];   // the payload, MSB first, three words per data symbol
};

// a wave's LDS need in floats (the host's check and the kernel's layout)
constexpr int div_work_floats(int plane, int nd) { return (std::max(2 * plane, rxc_spec_floats(nd)) + 3) & ~3; }
constexpr int div_wave_floats(int plane, int nd, int nb) {
    return div_work_floats(plane, nd) + nb * 2 * (320 + 80 * nd) + 128 * nd + 64;
}

// rxc_cfo over the branches: the correlations summed over b before the 64-lane sum (ofdm_rxchain.h, OFDM.c:773-828)
__device__ __forceinline__ void div_cfo(const float *fr, int nfr, int nb, int lane, int float_cfo, double &fc, double &ff) {
    const int k = lane & 15;
    float2 pp = make_float2(0.f, 0.f);
    for (int b = 0; b < nb; ++b) {
        const float *fre = fr + (size_t)b * 2 * nfr, *fim = fre + nfr;
        const float2 cu = make_float2(fre[80 + k], fim[80 + k]), cw = make_float2(fre[96 + k], fim[96 + k]);
        const float2 t = lane < 16 ? cmulc(cu, cw) : make_float2(0.f, 0.f);
        pp.x += t.x;
        pp.y += t.y;
    }
    pp.x = rxc_sum_f(pp.x);
    pp.y = rxc_sum_f(pp.y);
    fc = (-1.0 / (2.0 * M_PI * 16.0 * RXC_TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (float_cfo) fc = (double)(float)fc;
    pp = make_float2(0.f, 0.f);
    for (int b = 0; b < nb; ++b) {
        const float *fre = fr + (size_t)b * 2 * nfr, *fim = fre + nfr;
        const float2 u = rxc_rot(make_float2(fre[192 + lane], fim[192 + lane]), fc * RXC_TS, 192 + lane);
        const float2 w = rxc_rot(make_float2(fre[256 + lane], fim[256 + lane]), fc * RXC_TS, 256 + lane);
        const float2 t = cmulc(u, w);
        pp.x += t.x;
        pp.y += t.y;
    }
    pp.x = rxc_sum_f(pp.x);
    pp.y = rxc_sum_f(pp.y);
    ff = (-1.0 / (2.0 * M_PI * 64.0 * RXC_TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (float_cfo) ff = (double)(float)ff;
}

__global__ __launch_bounds__(64 * RXC_MAX_WAVES) void stream_decode_div_kernel(DivArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sdiv_smem[];
    unsigned long long *acc = sdiv_smem;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int nd = a.n_data, nfr = 320 + 80 * nd, plane = a.plane, len = 2 * nfr + 19, nb = a.br.nb;
    float *re = reinterpret_cast<float *>(sdiv_smem + RXC_ACC_WORDS) + (size_t)wave * a.wave_floats;
    float *im = re + plane;
    float *fr = re + a.work_floats;                                    // branch b: fre = fr + 2 nfr b, fim = fre + nfr
    float2 *N = reinterpret_cast<float2 *>(fr + (size_t)nb * 2 * nfr); // [D][64], sum_b Y_d conj(S)
    float *G = reinterpret_cast<float *>(N + 64 * nd);                 // [64], sum_b |S|^2
    if (threadIdx.x < RXC_ACC_WORDS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t cnt = a.count[1];
    for (int64_t i = (int64_t)blockIdx.x * W + wave; i < cnt; i += (int64_t)gridDim.x * W) {
        ofdm_stream_packet *pkt = a.pk + i;
        int64_t p;
        int last_front;
        sdec_packet(pkt, p, last_front);
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            const float2 *x = a.br.x[b];
            sdec_stage(x, a.n, p, div_parity(x), len, lane, re, im);
            rxc_wave_sync();
            sdec_filter(re, im, a.taps, nfr, lane, fr + (size_t)b * 2 * nfr, fr + (size_t)b * 2 * nfr + nfr);
            rxc_wave_sync();                                           // the next branch overwrites the planes
        }
        const bool oob = p + 2 * (int64_t)(nfr - 1) >= a.n + 20;       // the reference reads past its buffer
        double fc, ff;
        div_cfo(fr, nfr, nb, lane, a.float_cfo, fc, ff);
        sdec_sync_record(&pkt->r, acc, a.counters != nullptr, lane, p, last_front, oob, fc, ff);
        for (int d = 0; d < nd; ++d) N[64 * d + lane] = make_float2(0.f, 0.f);
        G[lane] = 0.f;
        // ---- per branch: rotate, the quads' transforms, park, then one bin per lane into N and G ----
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            float *fre = fr + (size_t)b * 2 * nfr, *fim = fre + nfr;
            rxc_rotate(fre, fim, lane, nd, fc, ff);
            rxc_wave_sync();
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
            const float2 S0 = reinterpret_cast<const float2 *>(re)[lane];
            const float g2 = fmaf(S0.x, S0.x, S0.y * S0.y);
            G[lane] += g2;
            // gain[b] = sum over the 52 used bins of |H|^2 / 52, H = L S / 2
            const bool used = lane >= 6 && lane <= 58 && lane != 32;
            const float gs = rxc_sum_f(used ? g2 : 0.f);
            if (a.gain && lane == 0) a.gain[i * nb + b] = gs * (1.0f / 208.0f);
            for (int d = 0; d < nd; ++d) {
                const int l0 = 4 * (d / 3), ln = l0 + 1 + d % 3;
                const float2 Y = reinterpret_cast<const float2 *>(re + ln * RXC_SPEC_PITCH)[lane];
                const float2 S = reinterpret_cast<const float2 *>(re + l0 * RXC_SPEC_PITCH)[lane];
                const float2 t = cmulc(Y, S);
                float2 acc2 = N[64 * d + lane];
                acc2.x += t.x;
                acc2.y += t.y;
                N[64 * d + lane] = acc2;
            }
            rxc_wave_sync();                                           // the next branch overwrites the rows
        }
        // ---- the pilot step on N: lane 4 d + i is term i of P_d; every lane of the four ends with u_d.  This step and
        // the subcarrier pass below are stream_decode_track_kernel's text, not a shared function: lifted into
        // ofdm_stream_decode.h they compile that kernel to other bytes (the same 214 VGPRs), and its bytes are pinned ----
        float ux = 1.f, uy = 0.f;
        if (a.track) {
            const int d = lane >> 2, pi = lane & 3;
            const bool on = d < nd;
            const int dd = on ? d : 0, bin = track_pilot_bin(pi);
            float2 t = N[64 * dd + bin];
            if ((TRACK_PILOT_NEG >> pi) & 1u) t = make_float2(-t.x, -t.y);
            t.x += __shfl_xor(t.x, 1, 64);
            t.y += __shfl_xor(t.y, 1, 64);
            t.x += __shfl_xor(t.x, 2, 64);
            t.y += __shfl_xor(t.y, 2, 64);
            // the larger component's power of two leaves P before it is squared: recordings scaled by 2^k give the
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
        // ---- the subcarrier pass of stream_decode_track_kernel on z = N / G = 2 L sum Y conj(S) / sum |S|^2 ----
        float fev = 0.f;
        uint32_t bev = 0u, axv = 0u;
        {
            const int nsc = 48 * nd;
            for (int j0 = 0; j0 < nsc; j0 += 64) {
                const int j = j0 + lane;
                const bool ok = j < nsc;
                const int jj = ok ? j : 0, d = jj / 48, m = jj - 48 * d, bin = data_bin(m);
                const float cx = __shfl(ux, 4 * d, 64), cy = __shfl(uy, 4 * d, 64);
                const float2 nv = N[64 * d + bin];
                const float r = __builtin_amdgcn_rcpf(G[bin]);
                const float g = ((RXC_LTF_NEG >> bin) & 1ull) ? -2.0f * r : 2.0f * r;
                const float2 z0 = make_float2(nv.x * g, nv.y * g);
                // u = 1 (no tracking, or the fallback) leaves z as it is, a NaN or a signed zero included
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
        rxc_wave_sync();                                             // the next packet overwrites the wave's region
    }
    rxc_flush(acc, a.counters);
}

// ---- the hooks ----
// what the three launches need beyond stream_receive's own argument blocks
struct DivUser {
    DivBranches br;
    int conv;                // the fine timing template's convention
    int track;
    float *gain;
    int64_t max_packets;
    int cus;
    int W;                   // the decode block's waves and dynamic LDS, sized for B filtered frames
    size_t lds;
    int32_t work_floats, wave_floats;
};

static void div_detect_launch(const StreamDetector *det, dim3 grid, hipStream_t stream, const DetArgs &a) {
    const DivUser *u = (const DivUser *)det->user;
    if (a.metric) hipLaunchKernelGGL(stream_detect_div_kernel<true>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold, u->br);
    else hipLaunchKernelGGL(stream_detect_div_kernel<false>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold, u->br);
}

static int div_timing_prepare(const StreamRefiner *ref, Ctx *c) {
    return timing_template(c, ((const DivUser *)ref->user)->conv);
}

static void div_timing_launch(const StreamRefiner *ref, Ctx *c, hipStream_t stream, const RefineArgs &r) {
    const DivUser *u = (const DivUser *)ref->user;
    TimArgs a{};
    a.x = r.x;
    a.n = r.n;
    a.count = r.count;
    a.pk = r.pk;
    a.out = (ofdm_stream_timing *)ref->out;
    timing_fill(c, u->conv, a);
    // as stream_timing_kernel's grid: enough blocks for max_packets, at most DVT_BLOCKS_PER_CU per CU; the waves loop
    const int64_t blocks = (r.max_packets + DVT_WAVES - 1) / DVT_WAVES;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, DVT_BLOCKS_PER_CU * (int64_t)c->cus));
    hipLaunchKernelGGL(stream_timing_div_kernel, grid, dim3(64 * DVT_WAVES), 0, stream, a, u->br);
}

// stream_receive sized its block for one branch's frame: the grid, the block and the LDS here are the hook's own
static void div_decode_launch(const StreamDecoder *dec, dim3, dim3, size_t, hipStream_t stream, const DecArgs &d,
                              const uint32_t *payload) {
    const DivUser *u = (const DivUser *)dec->user;
    DivArgs a{};
    a.br = u->br;
    a.n = d.n;
    a.count = d.count;
    a.pk = d.pk;
    a.bits = d.bits;
    a.eq = d.eq;
    a.phase = (float *)dec->out;
    a.gain = u->gain;
    a.counters = d.counters;
    a.n_data = d.n_data;
    a.float_cfo = d.float_cfo;
    a.track = u->track;
    a.plane = d.plane;
    a.work_floats = u->work_floats;
    a.wave_floats = u->wave_floats;
    std::copy(d.taps, d.taps + 21, a.taps);
    std::copy(payload, payload + 3 * d.n_data, a.words);
    // as stream_receive: enough blocks for max_packets, at most two per CU; the waves loop over d_count
    const int64_t blocks = (u->max_packets + u->W - 1) / u->W;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 2 * (int64_t)u->cus));
    hipLaunchKernelGGL(stream_decode_div_kernel, grid, dim3(64 * u->W), u->lds, stream, a);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_receive_stream_diversity(ofdm_ctx *ctx, const void *const *d_branches, int32_t n_branches,
                                             int64_t n_samples, const ofdm_rx_opts *opts, const ofdm_stream_opts *sopts,
                                             int timing, int tracking, int payload, int64_t max_packets, void *d_packets,
                                             void *d_count, void *d_bits, void *d_eq, void *d_counters, void *d_metric,
                                             void *d_cross, void *d_timing, void *d_phase, void *d_gain) {
    if (n_branches < 1 || n_branches > DV_MAX)
        return set_error(OFDM_E_ARG, "n_branches must be in [1, %d], got %d", DV_MAX, (int)n_branches);
    if (!d_branches) return set_error(OFDM_E_ARG, "d_branches is NULL");
    if (n_samples > 0)
        for (int b = 0; b < n_branches; ++b) {
            if (!d_branches[b]) return set_error(OFDM_E_ARG, "d_branches[%d] is NULL", b);
            if (reinterpret_cast<uintptr_t>(d_branches[b]) & 7u)
                return set_error(OFDM_E_ARG, "d_branches[%d] must be 8-byte aligned", b);
        }
    // one branch is ofdm_receive_stream_tracked itself: the same launches, byte-identical outputs
    if (n_branches == 1) {
        if (d_gain) return set_error(OFDM_E_ARG, "d_gain needs n_branches >= 2: n_branches is 1");
        return ofdm_receive_stream_tracked(ctx, d_branches[0], n_samples, opts, sopts, timing, tracking, payload, max_packets,
                                           d_packets, d_count, d_bits, d_eq, d_counters, d_metric, d_cross, d_timing, d_phase);
    }
    // what ofdm_receive_stream_tracked, _timed and _ex check before they reach stream_receive, in their order
    if (tracking != OFDM_TRACK_NONE && tracking != OFDM_TRACK_PILOTS)
        return set_error(OFDM_E_ARG, "tracking must be OFDM_TRACK_NONE (0) or OFDM_TRACK_PILOTS (1), got %d", tracking);
    if (tracking == OFDM_TRACK_NONE && d_phase)
        return set_error(OFDM_E_ARG, "d_phase needs OFDM_TRACK_PILOTS: tracking is OFDM_TRACK_NONE");
    if (timing != OFDM_TIMING_NONE && timing != OFDM_TIMING_LTF && timing != OFDM_TIMING_LTF_MATLAB)
        return set_error(OFDM_E_ARG, "timing must be OFDM_TIMING_NONE (0), OFDM_TIMING_LTF (1) or OFDM_TIMING_LTF_MATLAB (2), got %d", timing);
    if (timing == OFDM_TIMING_NONE && d_timing)
        return set_error(OFDM_E_ARG, "d_timing needs OFDM_TIMING_LTF or OFDM_TIMING_LTF_MATLAB: timing is OFDM_TIMING_NONE");
    if (!sopts || sopts->detector == OFDM_DETECT_REFERENCE)
        return set_error(OFDM_E_ARG, "%d branches need the detector OFDM_DETECT_CONJUGATE (1): the reference's metric carries the "
                         "channel's phase and its branch sums would cancel", (int)n_branches);
    if (sopts->detector != OFDM_DETECT_CONJUGATE)
        return set_error(OFDM_E_ARG, "detector must be OFDM_DETECT_REFERENCE (0) or OFDM_DETECT_CONJUGATE (1), got %d", sopts->detector);
    if (!(sopts->threshold > 0.f && sopts->threshold < 1.f))
        return set_error(OFDM_E_ARG, "threshold must be inside (0, 1), got %g", (double)sopts->threshold);
    for (int k = 0; k < 6; ++k)
        if (sopts->reserved[k]) return set_error(OFDM_E_ARG, "ofdm_stream_opts.reserved[%d] must be 0", k);
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (payload != OFDM_PAYLOAD_MESSAGE && payload != OFDM_PAYLOAD_TESTER)
        return set_error(OFDM_E_ARG, "a stream is decoded against a fixed payload (MESSAGE or TESTER), got %d", payload);

    DivUser u{};
    u.br.nb = n_branches;
    for (int b = 0; b < n_branches; ++b) u.br.x[b] = (const float2 *)d_branches[b];
    u.conv = timing == OFDM_TIMING_LTF_MATLAB ? OFDM_CONV_MATLAB : OFDM_CONV_C;
    u.track = tracking == OFDM_TRACK_PILOTS;
    u.gain = (float *)d_gain;
    u.max_packets = std::max<int64_t>(max_packets, 1);
    u.cus = c->cus;
    // the decode block's LDS with B filtered frames per wave, checked before anything is launched
    uint32_t table[3 * LONG_MAX_FRAMES];
    const int nd = payload_table_long(payload, c->message, table);
    const int plane = (2 * (320 + 80 * nd) + 19 + 3) & ~3;
    u.work_floats = div_work_floats(plane, nd);
    u.wave_floats = (div_wave_floats(plane, nd, n_branches) + 3) & ~3;
    WaveBlock wb;
    if (wave_block(c, RXC_ACC_WORDS * sizeof(unsigned long long), (size_t)u.wave_floats * sizeof(float), RXC_MAX_WAVES,
                   u.max_packets, &wb))
        return OFDM_E_HIP;
    if (!wb.W)
        return set_error(OFDM_E_ARG, "a %d-symbol packet on %d branches needs %zu bytes of LDS, above the %zu available", nd,
                         (int)n_branches, wb.lds, wb.limit);
    u.W = wb.W;
    u.lds = wb.lds;

    StreamDetector det{};
    det.halo = DetShape<true>::HALO;
    det.kernel = OFDM_K_STREAM_DETECT_DIV;
    det.threshold = sopts->threshold;
    det.launch = div_detect_launch;
    det.name = "stream_detect_div_kernel";
    det.user = &u;
    StreamRefiner ref{};
    ref.kernel = OFDM_K_STREAM_TIMING_DIV;
    ref.prepare = div_timing_prepare;
    ref.launch = div_timing_launch;
    ref.name = "stream_timing_div_kernel";
    ref.out = d_timing;
    ref.user = &u;
    StreamDecoder dec{};
    dec.kernel = OFDM_K_STREAM_DECODE_DIV;
    dec.launch = div_decode_launch;
    dec.name = "stream_decode_div_kernel";
    dec.out = d_phase;
    dec.user = &u;
    return stream_receive(c, d_branches[0], n_samples, opts, payload, max_packets, d_packets, d_count, d_bits, d_eq,
                          d_counters, d_metric, d_cross, &det, timing == OFDM_TIMING_NONE ? nullptr : &ref, &dec);
}
