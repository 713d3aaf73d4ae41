// ofdm_stream_conj.hip -- the optional detectors of the stream receiver (include/ofdm_mi355x_detect.h:
// ofdm_receive_stream_ex, ofdm_stream_positions).  A translation unit of its own: ofdm_stream.hip is certified as it
// is, so its kernels do not move; this file adds detection kernels only and hands them to ofdm_stream.hip's
// stream_receive (ofdm_stream_detect.h), which launches the selection and decode kernels it already has.
//
//   stream_detect_conj_kernel<METRIC> : the delay-and-correlate metric with the conjugate at lag 32,
//     c[i] = sum_{k<32} r[i+k] conj(r[i+k+32]), p[i] = sum_{k<32} |r[i+k+32]|^2, crossing thr p p - |c|^2 < 0, in
//     stream_detect_kernel's shape: 256 lanes, a tile of OFDM_STREAM_TILE positions, TILE + 63 samples staged once
//     (two planes of 8,000 floats and 248 bitmap words: 64,992 B of static LDS, two blocks per CU), every 16-byte load
//     of a lane in flight before the first LDS write, the 8-byte head misalignment path, runs of OFDM_STREAM_RUN
//     positions with boundaries fixed in stream coordinates -- M[i] and every crossing are independent of the launch
//     shape.  A run opens with the direct 32-term sum; its further positions are composed from partial sums of their
//     own terms in fp32 instead of a running difference (conj_run says why): 2 samples, 4 LDS words per position
//     against stream_detect_kernel's 8.
//   stream_detect_thr_kernel<METRIC> : the reference's metric (lag 16, no conjugate, TILE + 47 samples), term for term
//     and in the order of stream_detect_kernel, with the threshold as an argument.  Its sums are bit-identical to that
//     kernel's, so the crossings at any threshold nest with those of the default.
// Both share one body, stream_detect_body<CONJ, METRIC>, with a run function each; the threshold is a kernel argument.
// The tile's geometry, staging, decision and store are ofdm_stream_tile.h's, shared with ofdm_stream_div.hip.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_detect.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"
#include "ofdm_stream_detect.h"
#include "ofdm_stream_tile.h"

namespace ofdm {

static_assert(sizeof(ofdm_stream_opts) == 32, "ofdm_stream_opts is 32 bytes");
static_assert(OFDM_K_STREAM_DETECT_CONJ == Ctx::K_STREAM_DETECT_CONJ && Ctx::K_STREAM_DETECT_CONJ < Ctx::NK, "the timing id of ofdm_mi355x_detect.h");

// ---- the conjugate metric over one run, positions n0 + [0, cnt), without a running difference ----
// Term m of the run is g[m] = r[m] conj(r[m+32]) with the power q[m] = |r[m+32]|^2; position n0 + j sums the 32 terms
// m = n0 + j .. n0 + j + 31, that is the tail of the run's first 32 terms from j on plus the head of the next 32 up to
// j - 1.  The tails are one descending pass (its last value, j = 0, is the direct 32-term sum that opens the run) kept
// in registers, the heads one ascending pass: every sum only ever grows by terms of its own window, none is taken
// back.  A sum that slides -- add the incoming term, subtract the outgoing one -- keeps the rounding of terms long
// gone: where the power window leaves a packet for a gap 25 dB down it measured a deviation of 4.7e-4 of M from the
// fp64 metric on an MI355X, four times the bound of 1e-3 allows.  Here c and p carry the rounding of at most 64 fused
// multiply-adds of their own terms, so p is relatively exact and an all-zero power window gives c = p = 0 exactly:
// the non-zero-sample count with which stream_detect_kernel resets its sliding sums has nothing to reset.
// The ascending pass reads r[m] and r[m+32] of one new term per position: 2 samples, 4 LDS words (the descending pass
// is the 32-term opening sum, 128 words per run, as before).
template <bool METRIC>
__device__ __forceinline__ void conj_run(const DetArgs &a, int64_t t0, int n0, int cnt, float thr, const float *re,
                                         const float *im, uint32_t *bm) {
    float tx[CD_RUN], ty[CD_RUN], tp[CD_RUN];
    {
        float sx = 0.f, sy = 0.f, pw = 0.f;
#pragma unroll
        for (int k = 31; k >= 0; --k) {                                // n0 + k + 32 <= n0 + 63, inside the planes
            const float ux = re[n0 + k], uy = im[n0 + k], vx = re[n0 + k + 32], vy = im[n0 + k + 32];
            sx = fmaf(ux, vx, sx); sx = fmaf(uy, vy, sx);              // u conj(v)
            sy = fmaf(uy, vx, sy); sy = fmaf(-ux, vy, sy);
            pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
            if (k < CD_RUN) { tx[k] = sx; ty[k] = sy; tp[k] = pw; }
        }
    }
    float hx = 0.f, hy = 0.f, hp = 0.f;
#pragma unroll
    for (int j = 0; j < CD_RUN; ++j) {
        if (j >= cnt) break;
        det_decide<METRIC>(a, t0, n0 + j, tx[j] + hx, ty[j] + hy, tp[j] + hp, thr, bm);
        if (j + 1 < CD_RUN) {                                          // n0 + j + 64 <= 255 RUN + 93 < TILE + 63
            const int m = n0 + 32 + j;
            const float ux = re[m], uy = im[m], vx = re[m + 32], vy = im[m + 32];
            hx = fmaf(ux, vx, hx); hx = fmaf(uy, vy, hx);
            hy = fmaf(uy, vx, hy); hy = fmaf(-ux, vy, hy);
            hp = fmaf(vx, vx, hp); hp = fmaf(vy, vy, hp);
        }
    }
}
static_assert((CD_THREADS - 1) * CD_RUN + CD_RUN - 2 + 64 < DetShape<true>::SAMPLES, "the last lane's last term is staged");

// ---- the reference's metric over one run: stream_detect_kernel's sums, term for term and in its order ----
template <bool METRIC>
__device__ __forceinline__ void ref_run(const DetArgs &a, int64_t t0, int n0, int cnt, float thr, const float *re,
                                        const float *im, uint32_t *bm) {
    float sx = 0.f, sy = 0.f, pw = 0.f;
    int nz = 0;                                                        // samples of the power window that are not zero
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
        const float ux = re[n0 + k], uy = im[n0 + k], vx = re[n0 + k + 16], vy = im[n0 + k + 16];
        sx = fmaf(ux, vx, sx); sx = fmaf(-uy, vy, sx);
        sy = fmaf(ux, vy, sy); sy = fmaf(uy, vx, sy);
        pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
        nz += (vx != 0.f) | (vy != 0.f);
    }
    for (int j = 0; j < cnt; ++j) {
        const int n = n0 + j;
        // an all-zero power window has c = p = 0 exactly: what the slide left behind is rounding residue of the samples
        // that have gone, and must not decide a crossing (idle gaps have none)
        if (nz == 0) { sx = 0.f; sy = 0.f; pw = 0.f; }
        det_decide<METRIC>(a, t0, n, sx, sy, pw, thr, bm);
        if (j + 1 < cnt) {                                             // n + 48 <= t0 + n0 + cnt + 46 < the stream's end
            const float o0x = re[n], o0y = im[n], o1x = re[n + 16], o1y = im[n + 16];
            const float i0x = re[n + 32], i0y = im[n + 32], i1x = re[n + 48], i1y = im[n + 48];
            sx = fmaf(i0x, i1x, sx); sx = fmaf(-i0y, i1y, sx);
            sx = fmaf(-o0x, o1x, sx); sx = fmaf(o0y, o1y, sx);
            sy = fmaf(i0x, i1y, sy); sy = fmaf(i0y, i1x, sy);
            sy = fmaf(-o0x, o1y, sy); sy = fmaf(-o0y, o1x, sy);
            pw = fmaf(i1x, i1x, pw); pw = fmaf(i1y, i1y, pw);
            pw = fmaf(-o1x, o1x, pw); pw = fmaf(-o1y, o1y, pw);
            nz += (int)((i1x != 0.f) | (i1y != 0.f)) - (int)((o1x != 0.f) | (o1y != 0.f));
        }
    }
}

template <bool CONJ, bool METRIC>
__device__ __forceinline__ void stream_detect_body(const DetArgs &a, const float thr) {
    using S = DetShape<CONJ>;
    __shared__ __attribute__((aligned(16))) float re[S::PLANE];
    __shared__ __attribute__((aligned(16))) float im[S::PLANE];
    __shared__ __attribute__((aligned(16))) uint32_t bm[CD_WORDS];
    const int tid = threadIdx.x;
    // 1: the stream starts 8 bytes off a 16-byte line; tiles start at even samples, so every tile shares it
    const int head = (int)((reinterpret_cast<uintptr_t>(a.x) >> 3) & 1u);
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int64_t t0 = t * CD_TILE;
        det_stage<S>(a, t0, head, re, im, bm);
        __syncthreads();
        // this lane's run: positions t0 + [n0, n0 + cnt)
        const int n0 = tid * CD_RUN;
        const int cnt = (int)std::min<int64_t>(CD_RUN, a.lc - (t0 + n0));
        if (cnt > 0) {
            if constexpr (CONJ) conj_run<METRIC>(a, t0, n0, cnt, thr, re, im, bm);
            else ref_run<METRIC>(a, t0, n0, cnt, thr, re, im, bm);
        }
        __syncthreads();
        det_store(a, t0, bm);
        __syncthreads();                                               // the next tile overwrites the planes
    }
}

template <bool METRIC>
__global__ __launch_bounds__(CD_THREADS) void stream_detect_conj_kernel(DetArgs a, float thr) {
    stream_detect_body<true, METRIC>(a, thr);
}

template <bool METRIC>
__global__ __launch_bounds__(CD_THREADS) void stream_detect_thr_kernel(DetArgs a, float thr) {
    stream_detect_body<false, METRIC>(a, thr);
}

static void launch_conj(const StreamDetector *det, dim3 grid, hipStream_t stream, const DetArgs &a) {
    if (a.metric) hipLaunchKernelGGL(stream_detect_conj_kernel<true>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold);
    else hipLaunchKernelGGL(stream_detect_conj_kernel<false>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold);
}

static void launch_thr(const StreamDetector *det, dim3 grid, hipStream_t stream, const DetArgs &a) {
    if (a.metric) hipLaunchKernelGGL(stream_detect_thr_kernel<true>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold);
    else hipLaunchKernelGGL(stream_detect_thr_kernel<false>, grid, dim3(CD_THREADS), 0, stream, a, det->threshold);
}

// ofdm_receive_stream_ex's body; ref and dec (ofdm_stream_detect.h) are handed on to stream_receive
int stream_receive_ex(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                      const ofdm_stream_opts *sopts, int payload, int64_t max_packets, void *d_packets, void *d_count,
                      void *d_bits, void *d_eq, void *d_counters, void *d_metric, void *d_cross, const StreamRefiner *ref,
                      const StreamDecoder *dec) {
    int detector = OFDM_DETECT_REFERENCE;
    float thr = OFDM_DETECT_THRESHOLD;
    if (sopts) {
        detector = sopts->detector;
        thr = sopts->threshold;
        if (detector != OFDM_DETECT_REFERENCE && detector != OFDM_DETECT_CONJUGATE)
            return set_error(OFDM_E_ARG, "detector must be OFDM_DETECT_REFERENCE (0) or OFDM_DETECT_CONJUGATE (1), got %d", detector);
        if (!(thr > 0.f && thr < 1.f)) return set_error(OFDM_E_ARG, "threshold must be inside (0, 1), got %g", (double)thr);
        for (int k = 0; k < 6; ++k)
            if (sopts->reserved[k]) return set_error(OFDM_E_ARG, "ofdm_stream_opts.reserved[%d] must be 0", k);
    }
    // the defaults are ofdm_receive_stream itself: the same instantiations, byte-identical outputs
    if (detector == OFDM_DETECT_REFERENCE && thr == OFDM_DETECT_THRESHOLD)
        return stream_receive(c, d_samples, n_samples, opts, payload, max_packets, d_packets, d_count, d_bits, d_eq,
                              d_counters, d_metric, d_cross, nullptr, ref, dec);
    StreamDetector det{};
    det.threshold = thr;
    if (detector == OFDM_DETECT_CONJUGATE) {
        det.halo = DetShape<true>::HALO;
        det.kernel = OFDM_K_STREAM_DETECT_CONJ;
        det.launch = launch_conj;
        det.name = "stream_detect_conj_kernel";
    } else {
        det.halo = DetShape<false>::HALO;
        det.kernel = OFDM_K_STREAM_DETECT;
        det.launch = launch_thr;
        det.name = "stream_detect_thr_kernel";
    }
    return stream_receive(c, d_samples, n_samples, opts, payload, max_packets, d_packets, d_count, d_bits, d_eq,
                          d_counters, d_metric, d_cross, &det, ref, dec);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int64_t ofdm_stream_positions(int64_t n_samples, int detector) {
    if (detector != OFDM_DETECT_REFERENCE && detector != OFDM_DETECT_CONJUGATE)
        return set_error(OFDM_E_ARG, "detector must be OFDM_DETECT_REFERENCE (0) or OFDM_DETECT_CONJUGATE (1), got %d", detector);
    const int halo = detector == OFDM_DETECT_CONJUGATE ? DetShape<true>::HALO : DetShape<false>::HALO;
    return std::max<int64_t>(n_samples - halo, 0);
}

extern "C" int ofdm_receive_stream_ex(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                                      const ofdm_stream_opts *sopts, int payload, int64_t max_packets, void *d_packets,
                                      void *d_count, void *d_bits, void *d_eq, void *d_counters, void *d_metric,
                                      void *d_cross) {
    return stream_receive_ex(reinterpret_cast<Ctx *>(ctx), d_samples, n_samples, opts, sopts, payload, max_packets, d_packets,
                             d_count, d_bits, d_eq, d_counters, d_metric, d_cross, nullptr);
}
