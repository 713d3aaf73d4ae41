// ofdm_fading.hip -- K10, K11: the per-packet fading transmitter and its tap generator
// (include/ofdm_mi355x_fading.h).
//
//   K10 transmit_faded_kernel : the packet transmitter with a FIR of its own for every packet between the RRC filter
//                        and the packet's gain and carrier offset.
//   K11 draw_taps_kernel : Rayleigh taps from the Philox stream of symbol mode's channel_taps (ofdm_rxcommon.h), one
//                        lane per (packet, pair of taps): one Philox block is four Gaussians, two complex taps.
//
// K10 keeps K7's block shape, group loop, IFFT and polyphase RRC pass with K7's arithmetic (ofdm_transmit.hip describes
// them); constants, sign table, txc_zero_pads, txc_at, txc_aligned16, txc_phasor and the host routines are
// ofdm_txchain.h's, as K7's are.  The group, packet and filter text stands in this body as in K7's: called from the
// header the instances read the whole argument block at the entry, took 1 to 6 more VGPRs, and every accumulate variant
// measured slower, the 32-tap ones 0.7 to 0.8 %, outside the former spread ("The shared transmit chain").  As
// written the eight instances are the machine code they were before the header existed, byte for byte;
// tests/test_gpu_fading.py holds K10's samples to K7's bit for bit.  Per packet:
//   filter   K7's pass; the lane's pair (e0, e1) = w[2 q], w[2 q + 1] goes to an LDS packet buffer, not to HBM.
//            The buffer holds [H + 4 zeros | w[0 .. P) | H + 4 zeros], H = n_taps - 1; the zeros are written once per
//            block (D and n_taps are the launch's) and the pass only ever writes the P samples in the middle.
//   fir      ofdm_channel.hip's shape (K8): a lane owns the four consecutive outputs 4 Q .. 4 Q + 3, keeps a window of
//            four samples in registers and reads one more LDS sample per tap (8 bytes and 16 fmaf per tap),
//            accumulating in ascending tap order with the header's fma order.  The loop takes four taps per step, so
//            the window moves by register renaming and the step's four LDS reads are issued ahead of its 64 fmaf.
//            The packet's taps are read from HBM once per packet, lane l of every wave holding tap l; the loop
//            broadcasts tap j with two v_readlane.
//   rotate   K7's phasor (txc_phasor) on sample m = 4 Q + s, counted from the packet's first sample.
//   store    two 16-byte stores per lane when the quad's address is 16-byte aligned -- a property of the packet --
//            and guarded 8-byte stores when not, at the recording's ends and in the packet's last quad.
//   add      OFDM_TX_ACCUMULATE: the wave's 256 samples are 512 floats; they are re-dealt with lane shuffles so
//            that each of eight atomic wave-instructions adds 64 consecutive floats (K7 deals 4 x 2 floats per lane the
//            same way; the two shuffle patterns share no text).
// Two barriers per packet: the FIR pass reads what every lane of the filter pass wrote, and the next packet's
// filter pass overwrites it.
#include "ofdm_txchain.h"
#include "ofdm_mi355x_fading.h"
#include <algorithm>

namespace ofdm {

// the launch's own constants (tests/test_scale_host.py reads them in this file)
constexpr int FD_GROUP_SYMS = 62;           // data symbols per group: the chain's lanes 0..61 of wave 0
constexpr int FD_BLOCKS_PER_CU = 2;         // resident blocks the launch is sized for (LDS: 2 x 61,040 B of 160 KiB)
static_assert(FD_GROUP_SYMS == TXC_GROUP_SYMS, "lanes 62 and 63 of wave 0 are the training symbols' rows");
constexpr int FD_MAX_P = txc_packet_len(LONG_MAX_FRAMES);                     // 3,060
// [H + 4 zeros | P | H + 4 zeros]: the history of n_taps - 1 samples on either side, in front the up to three samples
// more that a step of four taps reads, behind the up to three that the last quad's window reaches
constexpr int FD_BUF = FD_MAX_P + 2 * (OFDM_FADE_MAX_TAPS - 1) + 8;           // 3,130
constexpr int FD_LDS = TXC_LDS + FD_BUF;                                      // 7,630 complex samples = 61,040 B
static_assert(8 * FD_LDS <= 65536, "static LDS of one block");

// TxPkArgs' members with h and n_taps among them, in this kernel's own order: as TxPkArgs with the two behind it, only
// the prologue changed and every store variant measured 0.8 to 1.9 % slower ("The shared transmit chain")
struct FadeArgs {
    const uint32_t *words;       // [n][3 D]
    const int64_t *pos;          // [n] or null
    const float2 *gain;          // [n] or null
    const float *cfo;            // [n] or null
    const float2 *h;             // [n][n_taps]
    float2 *out;                 // [n_out]
    int64_t n, n_out, pos0, stride, groups;
    int32_t n_data, per_group;   // D; packets per group = FD_GROUP_SYMS / D
    int32_t n_taps;
    float stf_scale;             // sqrt(13/6) as the float of OFDM.c:479
    float taps[21];              // the RRC filter
};

__device__ __forceinline__ float fd_lane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

template <int CONV, bool IMPAIR, bool ACC>
__global__ __launch_bounds__(TXC_THREADS) void transmit_faded_kernel(FadeArgs a) {
    __shared__ float2 lds[FD_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int D = a.n_data, nfr = 320 + 80 * D, half = nfr + TXC_PAD, P = 2 * half;
    const int L = a.n_taps, H = L - 1, PL = P + H, quads = (PL + 3) >> 2, off = H + 4;     // w[0] at buf[off]
    float2 *const T = lds + TXC_ROWS;
    float2 *const buf = lds + TXC_LDS;
    txc_zero_pads(lds);
    for (int i = tid; i < FD_BUF; i += TXC_THREADS) buf[i] = make_float2(0.f, 0.f);
    bool first = true;
    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t g0 = grp * a.per_group;
        const int np = (int)min((int64_t)a.per_group, a.n - g0);
        // ---------------------------------------------------------------- the group's time symbols (K7's text)
        if (tid < 64) {
            const bool is_data = tid < np * D, is_pre = first && tid >= FD_GROUP_SYMS;
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
                    const float s = sgn * a.stf_scale * (float)txc_stf_sign(i);
                    X[i] = is_data ? data
                         : tid == FD_GROUP_SYMS ? make_float2(s, s)                           // (1+j) S_k scale
                         : make_float2(sgn * (float)ltf_sign(i), 0.f);                        // L_k
                });
                fft64<true>(X);
                static_for<0, 64>([&](auto nc) {
                    constexpr int n = decltype(nc)::value;
                    T[tid * TXC_ROW + n] = cscale(X[digit_rev4(n)], (n & 1) ? -1.0f / 64.0f : 1.0f / 64.0f);
                });
            }
        }
        __syncthreads();
        if (first) {
            // short = first 16 samples x10, long = [T(32:64) T T] (Preamble_Generator, OFDM.c:392-398)
            for (int n = tid; n < 320; n += TXC_THREADS)
                lds[TXC_PRE + TXC_PAD + n] = n < 160 ? T[FD_GROUP_SYMS * TXC_ROW + (n & 15)]
                                                     : T[(FD_GROUP_SYMS + 1) * TXC_ROW + ((n - 160 + 32) & 63)];
            __syncthreads();
            first = false;
        }
        // ---------------------------------------------------------------- filter, fade and write, packet by packet
        for (int g = 0; g < np; ++g) {
            const int64_t pk = g0 + g;
            const int64_t pos = a.pos ? a.pos[pk] : (int64_t)((uint64_t)a.pos0 + (uint64_t)pk * (uint64_t)a.stride);
            if (pos >= a.n_out || pos <= -(int64_t)PL) continue;         // nothing of it lies inside the recording
            const bool has_gain = IMPAIR && a.gain, has_cfo = IMPAIR && a.cfo;
            const float2 gk = has_gain ? a.gain[pk] : make_float2(1.f, 0.f);
            const double fk = has_cfo ? (double)a.cfo[pk] : 0.0;
            // lane l of every wave: tap l of this packet
            const float2 hv = lane < L ? a.h[pk * L + lane] : make_float2(0.f, 0.f);
            const int rows = TXC_ROWS + g * D * TXC_ROW;
            for (int q = tid; q < half; q += TXC_THREADS) {
                int run, unused;
                const int a0 = txc_at(q, nfr, rows, run), a10 = txc_at(q - TXC_PAD, nfr, rows, unused) + TXC_PAD;
                float2 x[11];
#pragma unroll
                for (int t = 0; t < 11; ++t) x[t] = lds[(t <= run ? a0 : a10) - t];
                // Convolution(oversampled frame, RRC) (OFDM.c:342-364): ascending taps, as transmit_kernel
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
                buf[off + 2 * q] = e0;                                   // 2 q + 1 < P: inside [off, off + P)
                buf[off + 2 * q + 1] = e1;
            }
            __syncthreads();
            const bool vec = txc_aligned16(a.out, pos);
            for (int qb = 0; qb < quads; qb += TXC_THREADS) {
                const int Q = qb + tid;
                if (Q - lane >= quads) continue;         // whole waves: the tap broadcast and the shuffles read every lane
                const int Qc = min(Q, quads - 1);
                // v[m] = sum_l h[l] w[m - l], m = 4 Qc + s, w[i] at buf[off + i].  Four taps per step: c[0..3] is the
                // window w[m + 3 - j] .. w[m - j] of tap j and c[4..7] the four samples behind it, so tap j + t reads
                // c[3 - s + t] and the window moves by renaming.  The lowest index read is off + 4 Qc - (j + 4) >= 0
                // (j + 4 <= H + 4 = off), the highest off + 4 Qc + 3 <= off + PL + 2 < FD_BUF.
                const int base = off + 4 * Qc;
                float2 c[8], y[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    c[3 - s] = buf[base + s];
                    y[s] = make_float2(0.f, 0.f);
                }
                for (int j = 0; j < L; j += 4) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) c[4 + t] = buf[base - (j + 1 + t)];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (j + t < L) {
                            const float hr = fd_lane(hv.x, j + t), hi = fd_lane(hv.y, j + t);
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const float2 w = c[3 - s + t];
                                y[s].x = fmaf(hr, w.x, y[s].x);
                                y[s].x = fmaf(-hi, w.y, y[s].x);
                                y[s].y = fmaf(hr, w.y, y[s].y);
                                y[s].y = fmaf(hi, w.x, y[s].y);
                            }
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) c[t] = c[4 + t];
                }
                if (IMPAIR) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) y[s] = cmul(txc_phasor(has_gain, gk, has_cfo, fk, 4 * Qc + s), y[s]);
                }
                if (!ACC) {
                    const int m0 = 4 * Q;
                    const int64_t i0 = pos + m0;
                    if (vec && m0 + 3 < PL && i0 >= 0 && i0 + 3 < a.n_out) {
                        *reinterpret_cast<float4 *>(a.out + i0) = make_float4(y[0].x, y[0].y, y[1].x, y[1].y);
                        *reinterpret_cast<float4 *>(a.out + i0 + 2) = make_float4(y[2].x, y[2].y, y[3].x, y[3].y);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            if (m0 + s < PL && i0 + s >= 0 && i0 + s < a.n_out) a.out[i0 + s] = y[s];
                    }
                } else {
                    // the wave's quads Q - lane .. Q - lane + 63 are 512 consecutive floats; instruction i adds
                    // floats 64 i .. 64 i + 63: float 64 i + l is component l & 1 of sample (l >> 1) & 3 of lane
                    // 8 i + (l >> 3)
                    const int kw = 4 * (Q - lane);
                    float *const of = reinterpret_cast<float *>(a.out);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int src = 8 * i + (lane >> 3);
                        float v[8];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            v[2 * s] = __shfl(y[s].x, src);
                            v[2 * s + 1] = __shfl(y[s].y, src);
                        }
                        const float v01 = (lane & 1) ? v[1] : v[0], v23 = (lane & 1) ? v[3] : v[2];
                        const float v45 = (lane & 1) ? v[5] : v[4], v67 = (lane & 1) ? v[7] : v[6];
                        const float val = (lane & 4) ? ((lane & 2) ? v67 : v45) : ((lane & 2) ? v23 : v01);
                        const int k = kw + 32 * i + (lane >> 1);         // the sample of the packet
                        const int64_t idx = pos + k;
                        if (k < PL && idx >= 0 && idx < a.n_out) atomicAdd(of + 2 * idx + (lane & 1), val);
                    }
                }
            }
            __syncthreads();        // the next packet's filter pass overwrites the buffer, the next group's IFFT the rows
        }
    }
}

struct DrawArgs {
    float2 *h;                   // [n][n_taps]
    int64_t n;
    uint64_t index0;
    uint32_t k0, k1;
    int32_t n_taps, pairs;       // pairs = (n_taps + 1) / 2 Philox blocks per packet
    float amp[OFDM_FADE_MAX_TAPS];
};

__global__ __launch_bounds__(256) void draw_taps_kernel(DrawArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n * a.pairs) return;
    const int64_t k = idx / a.pairs;
    const int b = (int)(idx - k * a.pairs);
    const uint64_t f = a.index0 + (uint64_t)k;
    // channel_taps (ofdm_rxcommon.h): block b holds taps 2 b and 2 b + 1
    const Gauss4 z = gauss4((uint32_t)f, (uint32_t)(f >> 32), (uint32_t)b, STREAM_CHAN, a.k0, a.k1);
    float2 *dst = a.h + k * a.n_taps + 2 * b;
    const float s0 = a.amp[2 * b];
    dst[0] = make_float2(s0 * z.z[0], s0 * z.z[1]);
    if (2 * b + 1 < a.n_taps) {
        const float s1 = a.amp[2 * b + 1];
        dst[1] = make_float2(s1 * z.z[2], s1 * z.z[3]);
    }
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_faded_len(int32_t n_data, int32_t n_taps, int32_t *len) {
    if (!len) return set_error(OFDM_E_ARG, "len is NULL");
    if (const int rc = txc_check_n_data(n_data)) return rc;
    if (n_taps < 1 || n_taps > OFDM_FADE_MAX_TAPS)
        return set_error(OFDM_E_ARG, "n_taps %d outside [1, %d]", n_taps, OFDM_FADE_MAX_TAPS);
    *len = txc_packet_len(n_data) + n_taps - 1;
    return OFDM_OK;
}

extern "C" int ofdm_draw_taps(ofdm_ctx *ctx, uint64_t seed, uint64_t index0, int64_t n, int32_t n_taps,
                              const float *pdp, void *d_taps) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (n_taps < 1 || n_taps > OFDM_FADE_MAX_TAPS)
        return set_error(OFDM_E_ARG, "n_taps %d outside [1, %d]", n_taps, OFDM_FADE_MAX_TAPS);
    if (!pdp) return set_error(OFDM_E_ARG, "pdp is NULL");
    for (int l = 0; l < n_taps; ++l)
        if (!std::isfinite(pdp[l]) || pdp[l] < 0.0f)
            return set_error(OFDM_E_ARG, "pdp[%d] = %g is not a finite value >= 0", l, (double)pdp[l]);
    if (!d_taps && n > 0) return set_error(OFDM_E_ARG, "d_taps is required");
    if (reinterpret_cast<uintptr_t>(d_taps) & 7u) return set_error(OFDM_E_ARG, "d_taps must be 8-byte aligned");
    DrawArgs a{};
    a.pairs = (n_taps + 1) / 2;
    const int64_t blocks = (n * a.pairs + 255) / 256;
    if (n > (INT64_MAX >> 8) || blocks > 0x7fffffff) return set_error(OFDM_E_ARG, "n %lld is too large", (long long)n);
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    a.h = (float2 *)d_taps;
    a.n = n;
    a.index0 = index0;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.n_taps = n_taps;
    for (int l = 0; l < n_taps; ++l) a.amp[l] = (float)std::sqrt((double)pdp[l] / 2.0);
    c->tic(OFDM_K_DRAW_TAPS);
    hipLaunchKernelGGL(draw_taps_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "draw_taps_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_transmit_faded(ofdm_ctx *ctx, const ofdm_tx_opts *opts, const void *d_words, int64_t n,
                                   const void *d_pos, int64_t pos0, int64_t stride, const void *d_gain,
                                   const void *d_cfo_hz, const void *d_taps, int32_t n_taps, void *d_out,
                                   int64_t n_out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    const TxcTapArgs fir{d_taps, n_taps, OFDM_FADE_MAX_TAPS};
    if (const int rc = txc_check_args(c, opts, d_words, n, d_out, n_out, &fir)) return rc;
    if (n == 0 || n_out == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);

    FadeArgs a{};
    txc_fill(a, opts, FD_GROUP_SYMS / opts->n_data, d_words, n, d_pos, pos0, stride, d_gain, d_cfo_hz, d_out, n_out);
    a.h = (const float2 *)d_taps;
    a.n_taps = n_taps;
    const dim3 grid(txc_grid(a.groups, (int64_t)FD_BLOCKS_PER_CU * c->cus)), block(TXC_THREADS);
    c->tic(OFDM_K_FADE);
    txc_dispatch(opts, d_gain || d_cfo_hz, [&](auto conv, auto impair, auto acc) {
        hipLaunchKernelGGL((transmit_faded_kernel<conv(), impair(), acc()>), grid, block, 0, c->stream, a);
    });
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "transmit_faded_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
