// ofdm_transmit.hip -- K7: the batched packet transmitter (include/ofdm_mi355x_tx.h).
//
//   K7 transmit_kernel : Transmitter() (OFDM.c:467-618) for a batch of per-packet payloads, one period per packet,
//                        written into one device-resident recording at per-packet positions, with an optional
//                        complex gain and carrier offset per packet.
//
// A block of four waves takes groups of TXP_GROUP_SYMS / D packets.  Per group:
//   IFFT     the (packet, symbol) pairs of the group are flattened over the lanes of wave 0: 62 register-resident
//            64-point inverse transforms at once (ofdm_device.h fft64<true>), the arithmetic of frame_wave_kernel.
//            The time symbols go to LDS rows of 65 complex samples (the odd pitch keeps the 64 lanes' stores of one
//            sample index on different banks).  In a block's first group lanes 62 and 63 build the short and the
//            long training symbol, which all threads then lay out as the 320 preamble samples every packet shares.
//   filter   all 256 lanes.  The zero-stuffed input makes the 21-tap RRC filter polyphase: outputs 2q and 2q + 1
//            both read frame samples q - 10 .. q, the even one through the 11 even taps and the odd one through
//            the 10 odd taps.  A lane owns one such pair (16 bytes of output), reads its 11 frame samples from LDS
//            once and accumulates in ascending tap order with fmaf, as frame_wave_kernel does, so the samples are
//            those of ofdm_transmitter bit for bit.  The frame is never laid out whole: index n maps to the shared
//            preamble (with ten zeros in front), to a symbol row (cyclic prefix = the row's last 16 samples) or to
//            ten zeros behind the frame, and a window of 11 crosses at most one seam of that map (seams are 16 or
//            64 samples apart), so a lane resolves two addresses and selects per tap.
//   store    a lane's pair is one 16-byte store, consecutive lanes consecutive pairs (1 KiB per wave-instruction),
//            when the pair's address is 16-byte aligned -- a property of the packet -- and two 8-byte stores when
//            not or when the pair straddles an end of the recording.
//   add      OFDM_TX_ACCUMULATE: the wave's 128 samples are 256 floats; they are re-dealt with lane shuffles so
//            that each of four atomic wave-instructions adds 64 consecutive floats (256 contiguous bytes), the shape
//            the memory side takes float atomics at full rate in.
#include "ofdm_internal.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"
#include "ofdm_phasor.h"
#include "ofdm_mi355x_tx.h"
#include <algorithm>
#include <cmath>

namespace ofdm {

constexpr int TXP_THREADS = 256;
constexpr int TXP_GROUP_SYMS = 62;           // data symbols per group: lanes 0..61 of wave 0; 62, 63: STF, LTF
constexpr int TXP_ROW = 65;                  // LDS pitch of a time symbol (complex samples)
constexpr int TXP_PAD = 10;                  // (taps - 1) / 2: zeros in front of and behind the frame
constexpr int TXP_PRE = 0;                   // [10 zeros | 320 preamble samples]
constexpr int TXP_ZERO = TXP_PRE + TXP_PAD + 320;
constexpr int TXP_ROWS = TXP_ZERO + TXP_PAD;
constexpr int TXP_LDS = TXP_ROWS + 64 * TXP_ROW;     // 4,500 complex samples = 36,000 B: four blocks per CU
constexpr int TXP_BLOCKS_PER_CU = 2;         // resident blocks the launch is sized for (200-210 VGPRs: 2 waves per SIMD)

// short training tones S_k at bins 6..58 (OFDM.c:483-490), as ofdm_frame.hip
__host__ __device__ constexpr int txp_stf_sign(int bin) {
    constexpr int8_t S[53] = {0, 0, 1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 0,
                              0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0};
    return (bin >= 6 && bin <= 58) ? S[bin - 6] : 0;
}

struct TxPkArgs {
    const uint32_t *words;       // [n][3 D]
    const int64_t *pos;          // [n] or null
    const float2 *gain;          // [n] or null
    const float *cfo;            // [n] or null
    float2 *out;                 // [n_out]
    int64_t n, n_out, pos0, stride, groups;
    int32_t n_data, per_group;   // D; packets per group = TXP_GROUP_SYMS / D
    float stf_scale;             // sqrt(13/6) as the float of OFDM.c:479
    float taps[21];
};

// g exp(j 2 pi f m Ts): revolutions in fp64, reduced to [-1/2, 1/2], then the fp32 sine and cosine
__device__ __forceinline__ float2 txp_phasor(bool has_gain, float2 g, bool has_cfo, double f, int m) {
    const float2 e = has_cfo ? carrier_phasor(f, (double)m) : make_float2(1.0f, 0.0f);
    return has_gain ? cmul(g, e) : e;
}

template <int CONV, bool IMPAIR, bool ACC>
__global__ __launch_bounds__(TXP_THREADS) void transmit_kernel(TxPkArgs a) {
    __shared__ float2 lds[TXP_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int D = a.n_data, nfr = 320 + 80 * D, half = nfr + TXP_PAD, P = 2 * half;
    float2 *const T = lds + TXP_ROWS;
    if (tid < TXP_PAD) {
        lds[TXP_PRE + tid] = make_float2(0.f, 0.f);
        lds[TXP_ZERO + tid] = make_float2(0.f, 0.f);
    }
    bool first = true;
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t g0 = grp * a.per_group;
        const int np = (int)min((int64_t)a.per_group, a.n - g0);
        // ---------------------------------------------------------------- the group's time symbols
        if (tid < 64) {
            const bool is_data = tid < np * D, is_pre = first && tid >= TXP_GROUP_SYMS;
            if (is_data || is_pre) {
                uint32_t w[3] = {0u, 0u, 0u};
                if (is_data) {
                    const uint32_t *p = a.words + (g0 * D + tid) * 3;
                    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
                }
                float2 X[64];
                static_for<0, 64>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    constexpr float sgn = (CONV == OFDM_CONV_C && (i & 1)) ? -1.0f : 1.0f;   // D5
                    const float2 data = tx_bin<CONV, i>(w);
                    const float s = sgn * a.stf_scale * (float)txp_stf_sign(i);
                    X[i] = is_data ? data
                         : tid == TXP_GROUP_SYMS ? make_float2(s, s)                          // (1+j) S_k scale
                         : make_float2(sgn * (float)ltf_sign(i), 0.f);                        // L_k
                });
                fft64<true>(X);
                static_for<0, 64>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    T[tid * TXP_ROW + n] = cscale(X[digit_rev4(n)], (n & 1) ? -1.0f / 64.0f : 1.0f / 64.0f);
                });
            }
        }
        __syncthreads();
        if (first) {
            // short = first 16 samples x10, long = [T(32:64) T T] (Preamble_Generator, OFDM.c:392-398)
            for (int n = tid; n < 320; n += TXP_THREADS)
                lds[TXP_PRE + TXP_PAD + n] = n < 160 ? T[TXP_GROUP_SYMS * TXP_ROW + (n & 15)]
                                                     : T[(TXP_GROUP_SYMS + 1) * TXP_ROW + ((n - 160 + 32) & 63)];
            __syncthreads();
            first = false;
        }
        // ---------------------------------------------------------------- filter and write, packet by packet
        // frame index n -> LDS index; n in [-10, nfr + 10)
        for (int g = 0; g < np; ++g) {
            const int64_t pk = g0 + g;
            const int64_t pos = a.pos ? a.pos[pk] : (int64_t)((uint64_t)a.pos0 + (uint64_t)pk * (uint64_t)a.stride);
            if (pos >= a.n_out || pos <= -(int64_t)P) continue;          // nothing of it lies inside the recording
            const bool has_gain = IMPAIR && a.gain, has_cfo = IMPAIR && a.cfo;
            const float2 gk = has_gain ? a.gain[pk] : make_float2(1.f, 0.f);
            const double fk = has_cfo ? (double)a.cfo[pk] : 0.0;
            const int rows = TXP_ROWS + g * D * TXP_ROW;
            auto at = [&](int n, int &run) -> int {      // run: how far below n the map stays contiguous
                if (n < 320) { run = TXP_PAD; return TXP_PRE + TXP_PAD + n; }
                if (n >= nfr) { run = n - nfr; return TXP_ZERO + run; }
                const int x = n - 320, d = (int)(__umul24((unsigned)x, 52429u) >> 22), j = x - 80 * d;   // x / 80, x < 2^13
                run = j >= 16 ? j - 16 : j;
                return rows + d * TXP_ROW + (j >= 16 ? j - 16 : j + 48);                                  // [x(48:64) x]
            };
            const bool vec = (((uintptr_t)a.out + 8u * (uint64_t)pos) & 15u) == 0;
            const int qend = ACC ? (half + 63) & ~63 : half;
            for (int qb = 0; qb < qend; qb += TXP_THREADS) {
                const int q = qb + tid;
                if (ACC ? (q - lane >= half) : (q >= half)) continue;    // ACC: whole waves, for the shuffles
                const int qc = ACC ? min(q, half - 1) : q;
                int run, unused;
                const int a0 = at(qc, run), a10 = at(qc - TXP_PAD, unused) + TXP_PAD;
                float2 x[11];
#pragma unroll
                for (int t = 0; t < 11; ++t) x[t] = lds[(t <= run ? a0 : a10) - t];
                // Convolution(oversampled frame, RRC) (OFDM.c:342-364): ascending taps, as frame_wave_kernel
                float2 e0 = make_float2(0.f, 0.f), e1 = make_float2(0.f, 0.f);
#pragma unroll
                for (int t = 0; t < 11; ++t) {
                    e0.x = fmaf(a.taps[2 * t], x[t].x, e0.x);
                    e0.y = fmaf(a.taps[2 * t], x[t].y, e0.y);
                }
#pragma unroll
                for (int t = 0; t < 10; ++t) {
                    e1.x = fmaf(a.taps[2 * t + 1], x[t].x, e1.x);
                    e1.y = fmaf(a.taps[2 * t + 1], x[t].y, e1.y);
                }
                if (IMPAIR) {
                    e0 = cmul(txp_phasor(has_gain, gk, has_cfo, fk, 2 * qc), e0);
                    e1 = cmul(txp_phasor(has_gain, gk, has_cfo, fk, 2 * qc + 1), e1);
                }
                if (!ACC) {
                    const int64_t i0 = pos + 2 * q, i1 = i0 + 1;
                    if (i0 >= 0 && i1 < a.n_out) {
                        if (vec) *reinterpret_cast<float4 *>(a.out + i0) = make_float4(e0.x, e0.y, e1.x, e1.y);
                        else { a.out[i0] = e0; a.out[i1] = e1; }
                    } else {
                        if (i0 >= 0 && i0 < a.n_out) a.out[i0] = e0;
                        if (i1 >= 0 && i1 < a.n_out) a.out[i1] = e1;
                    }
                } else {
                    // the wave's pairs q - lane .. q - lane + 63 are 256 consecutive floats; instruction i adds
                    // floats 64 i .. 64 i + 63: float 64 i + l is component l & 3 of lane 16 i + (l >> 2)
                    const int kw = 2 * (q - lane);
                    float *const of = reinterpret_cast<float *>(a.out);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int src = 16 * i + (lane >> 2);
                        const float v0 = __shfl(e0.x, src), v1 = __shfl(e0.y, src), v2 = __shfl(e1.x, src),
                                    v3 = __shfl(e1.y, src);
                        const float v = (lane & 2) ? ((lane & 1) ? v3 : v2) : ((lane & 1) ? v1 : v0);
                        const int k = kw + 32 * i + (lane >> 1);
                        const int64_t idx = pos + k;
                        if (k < P && idx >= 0 && idx < a.n_out) atomicAdd(of + 2 * idx + (lane & 1), v);
                    }
                }
            }
        }
        __syncthreads();        // the next group's symbols overwrite the rows
    }
}

template <int CONV>
static void launch_transmit(hipStream_t st, const TxPkArgs &a, bool impair, bool acc, unsigned grid) {
    const dim3 g(grid), b(TXP_THREADS);
    if (impair) {
        if (acc) hipLaunchKernelGGL((transmit_kernel<CONV, true, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((transmit_kernel<CONV, true, false>), g, b, 0, st, a);
    } else {
        if (acc) hipLaunchKernelGGL((transmit_kernel<CONV, false, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((transmit_kernel<CONV, false, false>), g, b, 0, st, a);
    }
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_transmit_len(int32_t n_data, int32_t *len) {
    if (!len) return set_error(OFDM_E_ARG, "len is NULL");
    if (n_data < 1 || n_data > LONG_MAX_FRAMES)
        return set_error(OFDM_E_ARG, "n_data %d outside [1, %d]", n_data, LONG_MAX_FRAMES);
    *len = 2 * (320 + 80 * n_data) + 20;
    return OFDM_OK;
}

extern "C" int ofdm_transmit_packets(ofdm_ctx *ctx, const ofdm_tx_opts *opts, const void *d_words, int64_t n,
                                     const void *d_pos, int64_t pos0, int64_t stride, const void *d_gain,
                                     const void *d_cfo_hz, void *d_out, int64_t n_out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (!opts) return set_error(OFDM_E_ARG, "opts is NULL");
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (n_out < 0) return set_error(OFDM_E_ARG, "n_out %lld is negative", (long long)n_out);
    if (opts->n_data < 1 || opts->n_data > LONG_MAX_FRAMES)
        return set_error(OFDM_E_ARG, "n_data %d outside [1, %d]", opts->n_data, LONG_MAX_FRAMES);
    if (opts->conv != OFDM_CONV_C && opts->conv != OFDM_CONV_MATLAB) return set_error(OFDM_E_ARG, "bad conv %d", opts->conv);
    if (opts->flags & ~OFDM_TX_ACCUMULATE) return set_error(OFDM_E_ARG, "unknown flag bits 0x%x", opts->flags & ~OFDM_TX_ACCUMULATE);
    if (!d_words && n > 0) return set_error(OFDM_E_ARG, "d_words is required");
    if (!d_out && n_out > 0) return set_error(OFDM_E_ARG, "d_out is required");
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return set_error(OFDM_E_ARG, "d_out must be 8-byte aligned");
    if (n == 0 || n_out == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);

    TxPkArgs a{};
    a.words = (const uint32_t *)d_words;
    a.pos = (const int64_t *)d_pos;
    a.gain = (const float2 *)d_gain;
    a.cfo = (const float *)d_cfo_hz;
    a.out = (float2 *)d_out;
    a.n = n;
    a.n_out = n_out;
    a.pos0 = pos0;
    a.stride = stride;
    a.n_data = opts->n_data;
    a.per_group = TXP_GROUP_SYMS / opts->n_data;
    a.groups = (n + a.per_group - 1) / a.per_group;
    a.stf_scale = (float)std::sqrt(13.0 / 6.0);
    rrc_design(a.taps);
    // every block the same number of groups, and no more blocks than are resident at once
    const int64_t cap = (int64_t)TXP_BLOCKS_PER_CU * c->cus;
    const int64_t per_block = (a.groups + cap - 1) / cap;
    const unsigned grid = (unsigned)((a.groups + per_block - 1) / per_block);
    const bool impair = d_gain || d_cfo_hz, acc = (opts->flags & OFDM_TX_ACCUMULATE) != 0;
    c->tic(OFDM_K_TRANSMIT);
    if (opts->conv == OFDM_CONV_C) launch_transmit<OFDM_CONV_C>(c->stream, a, impair, acc, grid);
    else launch_transmit<OFDM_CONV_MATLAB>(c->stream, a, impair, acc, grid);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "transmit_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
