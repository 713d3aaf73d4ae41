// ofdm_txchain.h -- what the transmitters of Transmitter()'s chain (OFDM.c:467-618) hold in common, once: the packet
// transmitter (K7, ofdm_transmit.hip) and the fading transmitter (K10, ofdm_fading.hip) take the constants of the
// block's LDS layout, the sign table, txc_zero_pads, txc_at, txc_aligned16, txc_phasor and the host routines; frame
// mode's waveform kernel (K4a, ofdm_frame.hip) takes the sign table and txc_time_symbol.  The group stage, the packet
// stage and the filter pair are not here: called from a header they cost K7 and K10 speed, so each kernel keeps that
// text in its own body (the two units and DESIGN.md, "The shared transmit chain", say why), and
// tests/test_gpu_fading.py holds K10's samples to K7's bit for bit.  tests/test_gpu_transmit_exact.py pins all three.
#pragma once
#include <cmath>
#include <type_traits>
#include "ofdm_internal.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"
#include "ofdm_phasor.h"
#include "ofdm_mi355x_tx.h"

namespace ofdm {

constexpr int TXC_THREADS = 256;
constexpr int TXC_GROUP_SYMS = 62;           // data symbols per group: lanes 0..61 of wave 0; 62, 63: STF, LTF
constexpr int TXC_ROW = 65;                  // LDS pitch of a time symbol (complex samples)
constexpr int TXC_PAD = 10;                  // (RRC taps - 1) / 2: zeros in front of and behind the frame
constexpr int TXC_PRE = 0;                   // [10 zeros | 320 preamble samples]
constexpr int TXC_ZERO = TXC_PRE + TXC_PAD + 320;
constexpr int TXC_ROWS = TXC_ZERO + TXC_PAD;
constexpr int TXC_LDS = TXC_ROWS + 64 * TXC_ROW;     // 4,500 complex samples = 36,000 B
// samples of one packet: the 2x oversampled frame and the RRC tail
__host__ __device__ constexpr int txc_packet_len(int n_data) { return 2 * (320 + 80 * n_data) + 2 * TXC_PAD; }

// short training tones S_k at bins 6..58 (OFDM.c:483-490): +-1 on every 4th tone, times (1+j)
__host__ __device__ constexpr int txc_stf_sign(int bin) {
    constexpr int8_t S[53] = {0, 0, 1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 0,
                              0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0};
    return (bin >= 6 && bin <= 58) ? S[bin - 6] : 0;
}

// the argument block of K7 (K10's FadeArgs has these members and the packets' taps, in an order of its own).  A block
// of four waves takes groups of per_group = TXC_GROUP_SYMS / D packets
struct TxPkArgs {
    const uint32_t *words;       // [n][3 D]
    const int64_t *pos;          // [n] or null
    const float2 *gain;          // [n] or null
    const float *cfo;            // [n] or null
    float2 *out;                 // [n_out]
    int64_t n, n_out, pos0, stride, groups;
    int32_t n_data, per_group;   // D; packets per group = TXC_GROUP_SYMS / D
    float stf_scale;             // sqrt(13/6) as the float of OFDM.c:479
    float taps[21];              // the RRC filter
};

// ---- one lane's time symbol: the spectrum of a data symbol (is_data; payload words w), of the short (is_stf) or of
// the long training symbol, the inverse transform in registers and its (-1)^n / 64 scaled samples in natural order to
// `row`.  The kind is two flags and the spectrum two selects per bin: as one integer compared per bin the compiler
// branches around every bin (600 instructions more in K10) ----
template <int CONV>
__device__ __forceinline__ void txc_time_symbol(bool is_data, bool is_stf, const uint32_t (&w)[3], float stf_scale,
                                                float2 *row) {
    float2 X[64];
    static_for<0, 64>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr float sgn = (CONV == OFDM_CONV_C && (i & 1)) ? -1.0f : 1.0f;   // D5
        const float2 data = tx_bin<CONV, i>(w);
        const float s = sgn * stf_scale * (float)txc_stf_sign(i);
        X[i] = is_data ? data
             : is_stf ? make_float2(s, s)                                         // (1+j) S_k scale
             : make_float2(sgn * (float)ltf_sign(i), 0.f);                        // L_k
    });
    fft64<true>(X);
    static_for<0, 64>([&](auto nc) {
        constexpr int n = decltype(nc)::value;
        row[n] = cscale(X[digit_rev4(n)], (n & 1) ? -1.0f / 64.0f : 1.0f / 64.0f);
    });
}

// the ten zeros in front of the preamble and behind the frame, once per block
__device__ __forceinline__ void txc_zero_pads(float2 *lds) {
    if (threadIdx.x < TXC_PAD) {
        lds[TXC_PRE + threadIdx.x] = make_float2(0.f, 0.f);
        lds[TXC_ZERO + threadIdx.x] = make_float2(0.f, 0.f);
    }
}

// the packet's first sample sits on a 16-byte line of the recording: whole pairs and quads go out as 16-byte stores
__device__ __forceinline__ bool txc_aligned16(const float2 *out, int64_t pos) {
    return (((uintptr_t)out + 8u * (uint64_t)pos) & 15u) == 0;
}

// The frame is never laid out whole: index n in [-10, nfr + 10) maps to the shared preamble (ten zeros in front), to a
// symbol row from `rows` on (cyclic prefix = the row's last 16 samples) or to ten zeros behind the frame.  run: how far
// below n the map stays contiguous
__device__ __forceinline__ int txc_at(int n, int nfr, int rows, int &run) {
    if (n < 320) { run = TXC_PAD; return TXC_PRE + TXC_PAD + n; }
    if (n >= nfr) { run = n - nfr; return TXC_ZERO + run; }
    const int x = n - 320, d = (int)(__umul24((unsigned)x, 52429u) >> 22), j = x - 80 * d;   // x / 80, x < 2^13
    run = j >= 16 ? j - 16 : j;
    return rows + d * TXC_ROW + (j >= 16 ? j - 16 : j + 48);                                  // [x(48:64) x]
}

// g exp(j 2 pi f m Ts) at sample m of the packet: revolutions in fp64, reduced to [-1/2, 1/2], then the fp32 sine and
// cosine (carrier_phasor)
__device__ __forceinline__ float2 txc_phasor(bool has_gain, float2 g, bool has_cfo, double f, int m) {
    const float2 e = has_cfo ? carrier_phasor(f, (double)m) : make_float2(1.0f, 0.0f);
    return has_gain ? cmul(g, e) : e;
}

// ======================================================================== host side
inline int txc_check_n_data(int32_t n_data) {
    if (n_data < 1 || n_data > LONG_MAX_FRAMES)
        return set_error(OFDM_E_ARG, "n_data %d outside [1, %d]", n_data, LONG_MAX_FRAMES);
    return OFDM_OK;
}

// the per-packet taps of ofdm_transmit_faded, for the checks
struct TxcTapArgs {
    const void *d_taps;
    int32_t n_taps, max_taps;
};

// the arguments of ofdm_transmit_packets; with `fir` (ofdm_transmit_faded) also n_taps against [1, max_taps] and d_taps,
// at their places in the order
inline int txc_check_args(const void *ctx, const ofdm_tx_opts *opts, const void *d_words, int64_t n, const void *d_out,
                          int64_t n_out, const TxcTapArgs *fir = nullptr) {
    if (!ctx) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (!opts) return set_error(OFDM_E_ARG, "opts is NULL");
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (n_out < 0) return set_error(OFDM_E_ARG, "n_out %lld is negative", (long long)n_out);
    if (const int rc = txc_check_n_data(opts->n_data)) return rc;
    if (opts->conv != OFDM_CONV_C && opts->conv != OFDM_CONV_MATLAB) return set_error(OFDM_E_ARG, "bad conv %d", opts->conv);
    if (opts->flags & ~OFDM_TX_ACCUMULATE) return set_error(OFDM_E_ARG, "unknown flag bits 0x%x", opts->flags & ~OFDM_TX_ACCUMULATE);
    if (fir && (fir->n_taps < 1 || fir->n_taps > fir->max_taps))
        return set_error(OFDM_E_ARG, "n_taps %d outside [1, %d]", fir->n_taps, fir->max_taps);
    if (!d_words && n > 0) return set_error(OFDM_E_ARG, "d_words is required");
    if (fir && !fir->d_taps && n > 0) return set_error(OFDM_E_ARG, "d_taps is required");
    if (fir && (reinterpret_cast<uintptr_t>(fir->d_taps) & 7u)) return set_error(OFDM_E_ARG, "d_taps must be 8-byte aligned");
    if (!d_out && n_out > 0) return set_error(OFDM_E_ARG, "d_out is required");
    if (reinterpret_cast<uintptr_t>(d_out) & 7u) return set_error(OFDM_E_ARG, "d_out must be 8-byte aligned");
    return OFDM_OK;
}

// A: TxPkArgs or K10's FadeArgs, which has the same members by name; per_group: packets per group of the unit's kernel
template <typename A>
inline void txc_fill(A &a, const ofdm_tx_opts *opts, int32_t per_group, const void *d_words, int64_t n,
                     const void *d_pos, int64_t pos0, int64_t stride, const void *d_gain, const void *d_cfo_hz, void *d_out,
                     int64_t n_out) {
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
    a.per_group = per_group;
    a.groups = (n + a.per_group - 1) / a.per_group;
    a.stf_scale = (float)std::sqrt(13.0 / 6.0);
    rrc_design(a.taps);
}

// every block the same number of groups, and no more blocks than the `cap` that are resident at once
inline unsigned txc_grid(int64_t groups, int64_t cap) {
    const int64_t per_block = (groups + cap - 1) / cap;
    return (unsigned)((groups + per_block - 1) / per_block);
}

// launch(conv, impair, acc) with the three as integral constants: the <CONV, IMPAIR, ACC> instance of a kernel
template <typename F>
inline void txc_dispatch(const ofdm_tx_opts *opts, bool impair, F &&launch) {
    const bool acc = (opts->flags & OFDM_TX_ACCUMULATE) != 0;
    auto with = [&](auto conv) {
        if (impair) {
            if (acc) launch(conv, std::true_type{}, std::true_type{});
            else launch(conv, std::true_type{}, std::false_type{});
        } else {
            if (acc) launch(conv, std::false_type{}, std::true_type{});
            else launch(conv, std::false_type{}, std::false_type{});
        }
    };
    if (opts->conv == OFDM_CONV_C) with(std::integral_constant<int, OFDM_CONV_C>{});
    else with(std::integral_constant<int, OFDM_CONV_MATLAB>{});
}

}  // namespace ofdm
