// ofdm_channel.hip -- K8, K9: the device channel and the per-packet scoring (include/ofdm_mi355x_channel.h).
//
//   K8 channel_kernel<HAS_FIR, HAS_CFO, NOISE> : multipath FIR, carrier rotation and Philox noise over a
//                        device-resident recording, in one pass: 8 bytes read and 8 written per sample.  A stage that
//                        is off is not compiled in.
//   K9 score_kernel    : ofdm_receive_stream's records against the transmitted packets: a binary search by position
//                        and the popcount of the payload words' differences, one lane per transmitted packet.
//
// K8's work is cut in ABSOLUTE index k = index0 + i: a lane owns the four samples 4 Q .. 4 Q + 3 of quad Q = k >> 2,
// which are the four Gaussians of one real-noise Philox block (and of two complex-noise blocks), and a block owns the
// OFDM_CHANNEL_TILE samples of 256 consecutive quads.  Tile boundaries therefore sit at multiples of 4 in k, never
// at the buffer's start, and a sample's value does not depend on where a call, a block or a lane starts: the head
// and the tail of a call are quads with some samples outside [0, n), which are neither read nor written.
//   load     without the filter a lane's quad is two 16-byte loads when its address is 16-byte aligned -- a
//            property of the call -- and guarded 8-byte loads when not or at the call's head and tail.
//   filter   the tile and its n_taps - 1 samples of history are staged in LDS (zeros in front of the history the
//            caller gave); a lane keeps a window of four samples in registers and reads one more LDS sample per
//            tap, accumulating in ascending tap order with the header's fma order.  The taps arrive by value in the
//            kernel arguments and are read with scalar loads.
//   rotate   carrier_phasor(cfo_hz, k) per sample (ofdm_phasor.h, the transmitter's construction).
//   noise    noise4_of / noise_k (ofdm_device.h), one fma per noisy component: ota_kernel's arithmetic.
//   store    as the load.
#include "ofdm_internal.h"
#include "ofdm_ctx.h"
#include "ofdm_phasor.h"
#include "ofdm_mi355x_channel.h"
#include <algorithm>
#include <cmath>

namespace ofdm {

constexpr int CH_THREADS = 256;
constexpr int CH_TILE = 4 * CH_THREADS;
constexpr int CH_MAX_GRID = 2048;
static_assert(CH_TILE == OFDM_CHANNEL_TILE, "the header documents the tile");

struct ChanArgs {
    const float2 *in;            // u[-lead]: [lead + n]
    float2 *out;                 // [n]
    int64_t n, index0, lead;
    int64_t q0, tiles;           // first quad index0 >> 2; tiles of 256 quads
    double cfo_hz;
    float sigma;                 // per noisy axis
    uint32_t t_lo, t_hi, c3, k0, k1;
    int32_t n_taps;
    int32_t vec_in, vec_out;     // quads are 16-byte aligned in d_in / d_out
    float2 taps[OFDM_CHANNEL_MAX_TAPS];
};

template <bool HAS_FIR, bool HAS_CFO, int NOISE>
__global__ __launch_bounds__(CH_THREADS) void channel_kernel(ChanArgs a) {
    __shared__ float2 lds[HAS_FIR ? CH_TILE + OFDM_CHANNEL_MAX_TAPS : 1];
    const int tid = threadIdx.x;
    const float K = noise_k(a.sigma);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t Q = a.q0 + tile * CH_THREADS + tid;          // this lane's quad
        const int64_t i0 = 4 * Q - a.index0;                       // its first sample: -3 <= i0
        const bool full = i0 >= 0 && i0 + 3 < a.n, any = i0 + 3 >= 0 && i0 < a.n;
        float2 y[4];
        if constexpr (HAS_FIR) {
            const int H = a.n_taps - 1;
            const int64_t t0 = 4 * (a.q0 + tile * CH_THREADS) - a.index0 - H;    // the sample at lds[0]
            for (int p = tid; p < CH_TILE + H; p += CH_THREADS) {
                const int64_t i = t0 + p;
                lds[p] = (i >= -a.lead && i < a.n) ? a.in[a.lead + i] : make_float2(0.f, 0.f);
            }
            __syncthreads();
            if (any) {
                const int base = H + 4 * tid;
                float2 w[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    w[s] = lds[base + s];
                    y[s] = make_float2(0.f, 0.f);
                }
                for (int j = 0; j < a.n_taps; ++j) {
                    const float hr = a.taps[j].x, hi = a.taps[j].y;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        y[s].x = fmaf(hr, w[s].x, y[s].x);
                        y[s].x = fmaf(-hi, w[s].y, y[s].x);
                        y[s].y = fmaf(hr, w[s].y, y[s].y);
                        y[s].y = fmaf(hi, w[s].x, y[s].y);
                    }
                    w[3] = w[2]; w[2] = w[1]; w[1] = w[0];
                    if (j + 1 < a.n_taps) w[0] = lds[base - (j + 1)];           // j + 1 <= H: never below lds[0]
                }
            }
            __syncthreads();                                       // the next tile overwrites the staging
        } else if (any) {
            const float2 *src = a.in + (a.lead + i0);
            if (full && a.vec_in) {
                const float4 v0 = *reinterpret_cast<const float4 *>(src), v1 = *reinterpret_cast<const float4 *>(src + 2);
                y[0] = make_float2(v0.x, v0.y); y[1] = make_float2(v0.z, v0.w);
                y[2] = make_float2(v1.x, v1.y); y[3] = make_float2(v1.z, v1.w);
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    y[s] = (i0 + s >= 0 && i0 + s < a.n) ? src[s] : make_float2(0.f, 0.f);
            }
        }
        if (!any) continue;
        if constexpr (HAS_CFO) {
#pragma unroll
            for (int s = 0; s < 4; ++s) y[s] = cmul(carrier_phasor(a.cfo_hz, (double)(4 * Q + s)), y[s]);
        }
        if constexpr (NOISE == OFDM_NOISE_REAL) {
            // Gaussian s of block Q on the real part of sample 4 Q + s: ota_kernel
            const Noise4 nz = noise4_of(philox10(a.t_lo, a.t_hi, (uint32_t)Q, a.c3, a.k0, a.k1), K);
            y[0].x = fmaf(nz.r0, nz.c0, y[0].x);
            y[1].x = fmaf(nz.r0, nz.s0, y[1].x);
            y[2].x = fmaf(nz.r1, nz.c1, y[2].x);
            y[3].x = fmaf(nz.r1, nz.s1, y[3].x);
        } else if constexpr (NOISE == OFDM_NOISE_COMPLEX) {
            // sample k: Gaussians 2 (k & 1), 2 (k & 1) + 1 of block k >> 1
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const Noise4 nz = noise4_of(philox10(a.t_lo, a.t_hi, (uint32_t)(2 * Q + h), a.c3, a.k0, a.k1), K);
                y[2 * h].x = fmaf(nz.r0, nz.c0, y[2 * h].x);
                y[2 * h].y = fmaf(nz.r0, nz.s0, y[2 * h].y);
                y[2 * h + 1].x = fmaf(nz.r1, nz.c1, y[2 * h + 1].x);
                y[2 * h + 1].y = fmaf(nz.r1, nz.s1, y[2 * h + 1].y);
            }
        }
        float2 *dst = a.out + i0;
        if (full && a.vec_out) {
            *reinterpret_cast<float4 *>(dst) = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
            *reinterpret_cast<float4 *>(dst + 2) = make_float4(y[2].x, y[2].y, y[3].x, y[3].y);
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (i0 + s >= 0 && i0 + s < a.n) dst[s] = y[s];
        }
    }
}

template <bool HAS_FIR, bool HAS_CFO>
static void launch_channel_noise(hipStream_t st, const ChanArgs &a, int noise, unsigned grid) {
    const dim3 g(grid), b(CH_THREADS);
    if (noise == OFDM_NOISE_REAL) hipLaunchKernelGGL((channel_kernel<HAS_FIR, HAS_CFO, OFDM_NOISE_REAL>), g, b, 0, st, a);
    else if (noise == OFDM_NOISE_COMPLEX) hipLaunchKernelGGL((channel_kernel<HAS_FIR, HAS_CFO, OFDM_NOISE_COMPLEX>), g, b, 0, st, a);
    else hipLaunchKernelGGL((channel_kernel<HAS_FIR, HAS_CFO, OFDM_NOISE_NONE>), g, b, 0, st, a);
}

static void launch_channel(hipStream_t st, const ChanArgs &a, bool fir, bool cfo, int noise, unsigned grid) {
    if (fir) {
        if (cfo) launch_channel_noise<true, true>(st, a, noise, grid);
        else launch_channel_noise<true, false>(st, a, noise, grid);
    } else {
        if (cfo) launch_channel_noise<false, true>(st, a, noise, grid);
        else launch_channel_noise<false, false>(st, a, noise, grid);
    }
}

// ======================================================================== K9: scoring
constexpr int SC_THREADS = 256;

struct ScoreArgs {
    const uint32_t *tx_words;    // [n_tx][3 D]
    const int64_t *tx_pos;       // [n_tx] or null
    const ofdm_stream_packet *packets;
    const int64_t *count;        // [2]: found, written
    const uint32_t *rx_words;    // [written][3 D]
    ofdm_score *scores;          // [n_tx] or null
    unsigned long long *totals;  // [OFDM_NSCORE]
    int64_t n_tx, pos0, stride;
    int32_t words;               // 3 D
    int32_t off_lo, off_hi;
};

__global__ __launch_bounds__(SC_THREADS) void score_kernel(ScoreArgs a) {
    __shared__ unsigned long long acc[OFDM_NSCORE];
    const int tid = threadIdx.x;
    if (tid < OFDM_NSCORE) acc[tid] = 0ull;
    __syncthreads();
    const int64_t written = a.count[1];
    const int64_t k = (int64_t)blockIdx.x * SC_THREADS + tid;
    if (k < a.n_tx) {
        const int64_t pos = a.tx_pos ? a.tx_pos[k] : (int64_t)((uint64_t)a.pos0 + (uint64_t)k * (uint64_t)a.stride);
        // the first record at or behind pos + off_lo
        int64_t lo = 0, hi = written;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.packets[mid].packet_pos - pos < (int64_t)a.off_lo) lo = mid + 1;
            else hi = mid;
        }
        const bool hit = lo < written && a.packets[lo].packet_pos - pos <= (int64_t)a.off_hi;
        int32_t err = 0;
        if (hit) {
            const uint32_t *t = a.tx_words + k * a.words, *r = a.rx_words + lo * a.words;
            for (int w = 0; w < a.words; ++w) err += __popc(t[w] ^ r[w]);
            atomicAdd(&acc[1], 1ull);
            atomicAdd(&acc[3], 32ull * (unsigned long long)a.words);
            atomicAdd(&acc[4], (unsigned long long)err);
            atomicAdd(&acc[5], (unsigned long long)(err > 0));
        }
        if (a.scores) {
            ofdm_score s;
            s.rx_index = hit ? (int32_t)lo : -1;
            s.bit_err = err;
            a.scores[k] = s;
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        atomicAdd(&acc[0], (unsigned long long)a.n_tx);
        atomicAdd(&acc[2], (unsigned long long)written);
    }
    __syncthreads();
    if (tid < OFDM_NSCORE && acc[tid]) atomicAdd(&a.totals[tid], acc[tid]);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_impair_stream(ofdm_ctx *ctx, const ofdm_channel_opts *opts, const float *taps, const void *d_in,
                                  void *d_out, int64_t n) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (!opts) return set_error(OFDM_E_ARG, "opts is NULL");
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (opts->lead < 0) return set_error(OFDM_E_ARG, "lead %d is negative", opts->lead);
    if (opts->index0 < 0) return set_error(OFDM_E_ARG, "index0 %lld is negative", (long long)opts->index0);
    if (opts->n_taps < 0 || opts->n_taps > OFDM_CHANNEL_MAX_TAPS)
        return set_error(OFDM_E_ARG, "n_taps %d outside [0, %d]", opts->n_taps, OFDM_CHANNEL_MAX_TAPS);
    if (opts->noise != OFDM_NOISE_REAL && opts->noise != OFDM_NOISE_COMPLEX && opts->noise != OFDM_NOISE_NONE)
        return set_error(OFDM_E_ARG, "bad noise %d", opts->noise);
    if (opts->snr_index < 0 || opts->snr_index >= (1 << 24))
        return set_error(OFDM_E_ARG, "snr_index %d outside [0, 2^24)", opts->snr_index);
    if (!std::isfinite(opts->power) || opts->power < 0.0) return set_error(OFDM_E_ARG, "power %g is not a finite value >= 0", opts->power);
    if (!std::isfinite(opts->snr_db)) return set_error(OFDM_E_ARG, "snr_db %g is not finite", opts->snr_db);
    if (!std::isfinite(opts->cfo_hz)) return set_error(OFDM_E_ARG, "cfo_hz %g is not finite", opts->cfo_hz);
    if (opts->n_taps > 0 && !taps) return set_error(OFDM_E_ARG, "taps is required with n_taps %d", opts->n_taps);
    if (n > 0 && (!d_in || !d_out)) return set_error(OFDM_E_ARG, "d_in and d_out are required");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(d_in), po = reinterpret_cast<uintptr_t>(d_out);
    if ((pi | po) & 7u) return set_error(OFDM_E_ARG, "d_in and d_out must be 8-byte aligned");
    if (opts->noise != OFDM_NOISE_NONE) {
        const int64_t lim = int64_t(1) << (opts->noise == OFDM_NOISE_REAL ? 34 : 33);
        if (opts->index0 > lim || n > lim - opts->index0)
            return set_error(OFDM_E_ARG, "index0 + n = %lld + %lld exceeds the noise stream's %lld samples",
                             (long long)opts->index0, (long long)n, (long long)lim);
    }
    if (n > (INT64_MAX >> 4) || opts->index0 > (INT64_MAX >> 4)) return set_error(OFDM_E_ARG, "n or index0 too large");
    if (n > 0) {
        const uintptr_t in_end = pi + 8u * (uintptr_t)(opts->lead + n), out_end = po + 8u * (uintptr_t)n;
        const bool in_place = po == pi && opts->lead == 0 && opts->n_taps <= 1;
        if (po < in_end && pi < out_end && !in_place)
            return set_error(OFDM_E_ARG, "d_out overlaps d_in (in place needs d_out == d_in, lead 0 and at most one tap)");
    }
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);

    ChanArgs a{};
    a.in = (const float2 *)d_in;
    a.out = (float2 *)d_out;
    a.n = n;
    a.index0 = opts->index0;
    a.lead = opts->lead;
    a.q0 = opts->index0 >> 2;
    const int64_t quads = ((opts->index0 + n - 1) >> 2) - a.q0 + 1;
    a.tiles = (quads + CH_THREADS - 1) / CH_THREADS;
    a.cfo_hz = opts->cfo_hz;
    const double lin = std::pow(10.0, opts->snr_db / 10.0);
    a.sigma = opts->noise == OFDM_NOISE_COMPLEX ? (float)std::sqrt(0.5 * opts->power / lin)
                                                : (float)std::sqrt(opts->power / lin);
    a.t_lo = (uint32_t)opts->trial;
    a.t_hi = (uint32_t)(opts->trial >> 32);
    a.c3 = STREAM_NOISE | (uint32_t)opts->snr_index;
    a.k0 = (uint32_t)opts->seed;
    a.k1 = (uint32_t)(opts->seed >> 32);
    a.n_taps = opts->n_taps;
    for (int j = 0; j < opts->n_taps; ++j) a.taps[j] = make_float2(taps[2 * j], taps[2 * j + 1]);
    // a quad starts at sample 4 Q - index0 (+ lead in d_in): 16-byte aligned when that sample's address is
    a.vec_in = (((pi >> 3) + (uintptr_t)opts->lead - (uintptr_t)opts->index0) & 1u) == 0;
    a.vec_out = (((po >> 3) - (uintptr_t)opts->index0) & 1u) == 0;
    const unsigned grid = (unsigned)std::min<int64_t>(a.tiles, CH_MAX_GRID);
    c->tic(OFDM_K_CHANNEL);
    launch_channel(c->stream, a, opts->n_taps > 0, opts->cfo_hz != 0.0, opts->noise, grid);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "channel_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_score_packets(ofdm_ctx *ctx, int32_t n_data, const void *d_tx_words, int64_t n_tx,
                                  const void *d_tx_pos, int64_t pos0, int64_t stride, const void *d_packets,
                                  const void *d_count, const void *d_bits, int32_t off_lo, int32_t off_hi,
                                  void *d_scores, void *d_totals) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n_tx < 0) return set_error(OFDM_E_ARG, "n_tx %lld is negative", (long long)n_tx);
    if (n_data < 1 || n_data > LONG_MAX_FRAMES)
        return set_error(OFDM_E_ARG, "n_data %d outside [1, %d]", n_data, LONG_MAX_FRAMES);
    if (off_lo < 0 || off_hi < off_lo || off_hi - off_lo > 300)
        return set_error(OFDM_E_ARG, "window [%d, %d]: 0 <= off_lo <= off_hi and off_hi - off_lo <= 300 are required",
                         off_lo, off_hi);
    if (!d_tx_words && n_tx > 0) return set_error(OFDM_E_ARG, "d_tx_words is required");
    if (!d_packets || !d_count || !d_bits) return set_error(OFDM_E_ARG, "d_packets, d_count and d_bits are required");
    if (!d_totals) return set_error(OFDM_E_ARG, "d_totals is required");
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);

    ScoreArgs a{};
    a.tx_words = (const uint32_t *)d_tx_words;
    a.tx_pos = (const int64_t *)d_tx_pos;
    a.packets = (const ofdm_stream_packet *)d_packets;
    a.count = (const int64_t *)d_count;
    a.rx_words = (const uint32_t *)d_bits;
    a.scores = (ofdm_score *)d_scores;
    a.totals = (unsigned long long *)d_totals;
    a.n_tx = n_tx;
    a.pos0 = pos0;
    a.stride = stride;
    a.words = 3 * n_data;
    a.off_lo = off_lo;
    a.off_hi = off_hi;
    const int64_t blocks = std::max<int64_t>((n_tx + SC_THREADS - 1) / SC_THREADS, 1);
    if (blocks > 0x7fffffff) return set_error(OFDM_E_ARG, "n_tx %lld is too large", (long long)n_tx);
    c->tic(OFDM_K_SCORE);
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)blocks), dim3(SC_THREADS), 0, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "score_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
