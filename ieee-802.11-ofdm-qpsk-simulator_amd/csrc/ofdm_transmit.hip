// ofdm_transmit.hip -- K7: the batched packet transmitter (include/ofdm_mi355x_tx.h).
//
//   K7 transmit_kernel : Transmitter() (OFDM.c:467-618) for a batch of per-packet payloads, one period per packet,
//                        written into one device-resident recording at per-packet positions, with an optional
//                        complex gain and carrier offset per packet.
//
// A block of four waves takes groups of TXP_GROUP_SYMS / D packets.  Per group:
//   IFFT     the (packet, symbol) pairs of the group are flattened over the lanes of wave 0: 62 register-resident
//            64-point inverse transforms at once, into LDS rows of 65 complex samples (the odd pitch keeps the 64 lanes'
//            stores of one sample index on different banks).  In a block's first group lanes 62 and 63 build the short
//            and the long training symbol, which all threads then lay out as the 320 preamble samples every packet shares.
//   filter   all 256 lanes.  The zero-stuffed input makes the 21-tap RRC filter polyphase: outputs 2q and 2q + 1 both
//            read frame samples q - 10 .. q, the even one through the 11 even taps and the odd one through the 10 odd
//            taps, in ascending tap order with fmaf as frame_wave_kernel does, so the samples are ofdm_transmitter's bit
//            for bit.  A window of 11 crosses at most one seam of txc_at's map (seams are 16 or 64 samples apart), so a
//            lane resolves two addresses and selects per tap.
// The constants, sign table, argument block, txc_zero_pads, txc_at, txc_aligned16, txc_phasor and the host routines are
// ofdm_txchain.h's, shared with K10 (ofdm_fading.hip), which runs the same group, packet and filter text in its own
// body.  Those three stages, and the time symbol inside the first, are not called from the header: inlined from there
// they gave the same instructions in another order (the whole argument block read at the kernel's entry once a stage
// takes a reference to it; a.stf_scale read ahead of the bins once a stage is handed it as a value, which alone
// reorders 1,135 of the store instance's 2,033 instructions), and K7's store instances measured 1.7 to 3.4 % slower
// ("The shared transmit chain").  As written the eight instances are the machine code they were before the
// header existed, byte for byte.
//   store    a lane's pair is one 16-byte store, consecutive lanes consecutive pairs (1 KiB per wave-instruction),
//            when the pair's address is 16-byte aligned -- a property of the packet -- and two 8-byte stores when
//            not or when the pair straddles an end of the recording.
//   add      OFDM_TX_ACCUMULATE: the wave's 128 samples are 256 floats; they are re-dealt with lane shuffles so
//            that each of four atomic wave-instructions adds 64 consecutive floats (256 contiguous bytes), the shape
//            the memory side takes float atomics at full rate in.
#include "ofdm_txchain.h"
#include "ofdm_phasor.h"        // carrier_phasor, which txc_phasor turns the packet's samples by

namespace ofdm {

// the launch's own constants (tests/test_scale_host.py reads them in this file)
constexpr int TXP_GROUP_SYMS = 62;           // data symbols per group: the chain's lanes 0..61 of wave 0
constexpr int TXP_BLOCKS_PER_CU = 2;         // resident blocks the launch is sized for (200-210 VGPRs: 2 waves per SIMD)
static_assert(TXP_GROUP_SYMS == TXC_GROUP_SYMS, "lanes 62 and 63 of wave 0 are the training symbols' rows");

template <int CONV, bool IMPAIR, bool ACC>
__global__ __launch_bounds__(TXC_THREADS) void transmit_kernel(TxPkArgs a) {
    __shared__ float2 lds[TXC_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int D = a.n_data, nfr = 320 + 80 * D, half = nfr + TXC_PAD, P = 2 * half;
    float2 *const T = lds + TXC_ROWS;
    txc_zero_pads(lds);
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
                    const float s = sgn * a.stf_scale * (float)txc_stf_sign(i);
                    X[i] = is_data ? data
                         : tid == TXP_GROUP_SYMS ? make_float2(s, s)                          // (1+j) S_k scale
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
                lds[TXC_PRE + TXC_PAD + n] = n < 160 ? T[TXP_GROUP_SYMS * TXC_ROW + (n & 15)]
                                                     : T[(TXP_GROUP_SYMS + 1) * TXC_ROW + ((n - 160 + 32) & 63)];
            __syncthreads();
            first = false;
        }
        // ---------------------------------------------------------------- filter and write, packet by packet
        for (int g = 0; g < np; ++g) {
            const int64_t pk = g0 + g;
            const int64_t pos = a.pos ? a.pos[pk] : (int64_t)((uint64_t)a.pos0 + (uint64_t)pk * (uint64_t)a.stride);
            if (pos >= a.n_out || pos <= -(int64_t)P) continue;          // nothing of it lies inside the recording
            const bool has_gain = IMPAIR && a.gain, has_cfo = IMPAIR && a.cfo;
            const float2 gk = has_gain ? a.gain[pk] : make_float2(1.f, 0.f);
            const double fk = has_cfo ? (double)a.cfo[pk] : 0.0;
            const int rows = TXC_ROWS + g * D * TXC_ROW;
            const bool vec = txc_aligned16(a.out, pos);
            const int qend = ACC ? (half + 63) & ~63 : half;
            for (int qb = 0; qb < qend; qb += TXC_THREADS) {
                const int q = qb + tid;
                if (ACC ? (q - lane >= half) : (q >= half)) continue;    // ACC: whole waves, for the shuffles
                const int qc = ACC ? min(q, half - 1) : q;
                // Convolution(oversampled frame, RRC) (OFDM.c:342-364): ascending taps, as frame_wave_kernel
                int run, unused;
                const int a0 = txc_at(qc, nfr, rows, run), a10 = txc_at(qc - TXC_PAD, nfr, rows, unused) + TXC_PAD;
                float2 x[11];
#pragma unroll
                for (int t = 0; t < 11; ++t) x[t] = lds[(t <= run ? a0 : a10) - t];
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
                    e0 = cmul(txc_phasor(has_gain, gk, has_cfo, fk, 2 * qc), e0);
                    e1 = cmul(txc_phasor(has_gain, gk, has_cfo, fk, 2 * qc + 1), e1);
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

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_transmit_len(int32_t n_data, int32_t *len) {
    if (!len) return set_error(OFDM_E_ARG, "len is NULL");
    if (const int rc = txc_check_n_data(n_data)) return rc;
    *len = txc_packet_len(n_data);
    return OFDM_OK;
}

extern "C" int ofdm_transmit_packets(ofdm_ctx *ctx, const ofdm_tx_opts *opts, const void *d_words, int64_t n,
                                     const void *d_pos, int64_t pos0, int64_t stride, const void *d_gain,
                                     const void *d_cfo_hz, void *d_out, int64_t n_out) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (const int rc = txc_check_args(c, opts, d_words, n, d_out, n_out)) return rc;
    if (n == 0 || n_out == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);

    TxPkArgs a{};
    txc_fill(a, opts, TXP_GROUP_SYMS / opts->n_data, d_words, n, d_pos, pos0, stride, d_gain, d_cfo_hz, d_out, n_out);
    const dim3 grid(txc_grid(a.groups, (int64_t)TXP_BLOCKS_PER_CU * c->cus)), block(TXC_THREADS);
    c->tic(OFDM_K_TRANSMIT);
    txc_dispatch(opts, d_gain || d_cfo_hz, [&](auto conv, auto impair, auto acc) {
        hipLaunchKernelGGL((transmit_kernel<conv(), impair(), acc()>), grid, block, 0, c->stream, a);
    });
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "transmit_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
