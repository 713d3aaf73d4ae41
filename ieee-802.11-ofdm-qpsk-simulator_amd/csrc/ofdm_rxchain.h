// ofdm_rxchain.h -- Receiver()'s chain after packet selection (OFDM.c:773-1165), once, for the three kernels that run
// it with one wave per packet: capture_rx_kernel (ofdm_captures.hip), stream_decode_kernel (ofdm_stream.hip) and
// stream_decode_track_kernel (ofdm_stream_track.hip).  A kernel stages its samples, runs the matched filter at the
// down-sampled instants into fre[] / fim[] of its wave's LDS region, and from there its body is a sequence of the
// stages below, in this order.  Every stage is inlined: a stage is a span of the kernel's body, not a call, and the
// positions of the wave syncs and sched_fence()s inside and between the stages are part of what they are (the
// comments give what moving them costs in spilled VGPRs).  A packet's record is therefore the same arithmetic in the
// same order whichever kernel decoded it.  None of the three kernels is certified by build id (only the c2 / c3 / c5 /
// fft64 / frame / frame8 kernels are); resource rows in the host tests and byte parity with a recorded fixture on the
// GPU (tests/test_gpu_decode_exact.py) pin them.
#pragma once
#include <cmath>
#include "ofdm_mi355x_captures.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"

namespace ofdm {

constexpr int RXC_MAX_DATA = LONG_MAX_FRAMES;
constexpr int RXC_MAX_WAVES = 8;                      // 512 threads: two waves per SIMD, 256 VGPRs each
constexpr int RXC_ACC_WORDS = OFDM_NCOUNTERS;         // the block's counter row (64-bit words) ahead of the waves' regions
constexpr double RXC_TS = 1.0 / 20e6;                 // OFDM.c:16-17
constexpr int RXC_SPEC_PITCH = 130;                   // floats per parked spectrum (64 float2 + one: 8-byte accesses, 2 banks apart)
// long training tones with L_k = -1 (ofdm_device.h ltf_sign), bit k
constexpr uint64_t rxc_ltf_neg() {
    uint64_t v = 0;
    for (int b = 0; b < 64; ++b) v |= (uint64_t)(ltf_sign(b) < 0) << b;
    return v;
}
constexpr uint64_t RXC_LTF_NEG = rxc_ltf_neg();
static_assert(sizeof(ofdm_capture_result) == 48, "ofdm_capture_result is 48 bytes");

// floats of a wave's region that the parked spectra need: 4 ceil(D / 3) rows of the quads in use and one for the idle lanes
constexpr int rxc_spec_floats(int n_data) { return (4 * ((n_data + 2) / 3) + 1) * RXC_SPEC_PITCH; }

// LDS ordering between the lanes of one wave (the block's other waves run other packets)
__device__ __forceinline__ void rxc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float rxc_sum_f(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// rotate by exp(-j 2 pi f Ts i): the phase in revolutions in fp64, range-reduced, then v_sin / v_cos (OFDM.c:802,825)
__device__ __forceinline__ float2 rxc_rot(float2 v, double f_ts, int i) {
    const double rev = -f_ts * (double)i;
    const float fr = (float)(rev - rint(rev));
    const float s = __builtin_amdgcn_sinf(fr), c = __builtin_amdgcn_cosf(fr);
    return make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
}
// frame sample ii is one the receiver uses: STF tail [80, 112), LTF pair [192, 320), data symbols past their prefixes
__device__ __forceinline__ bool rxc_needed(int ii) {
    if (ii < 192) return ii >= 80 && ii < 112;
    if (ii < 320) return true;
    const int r = (ii - 320) % 80;
    return r >= 16;
}

// ---- Coarse_CFO_Estimation, Fine_CFO_Estimation (OFDM.c:773-828) ----
__device__ __forceinline__ void rxc_cfo(const float *fre, const float *fim, int lane, int float_cfo, double &fc, double &ff) {
    const int k = lane & 15;
    const float2 cu = make_float2(fre[80 + k], fim[80 + k]), cw = make_float2(fre[96 + k], fim[96 + k]);
    float2 pp = lane < 16 ? cmulc(cu, cw) : make_float2(0.f, 0.f);
    pp.x = rxc_sum_f(pp.x);
    pp.y = rxc_sum_f(pp.y);
    fc = (-1.0 / (2.0 * M_PI * 16.0 * RXC_TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (float_cfo) fc = (double)(float)fc;
    const float2 u = rxc_rot(make_float2(fre[192 + lane], fim[192 + lane]), fc * RXC_TS, 192 + lane);
    const float2 w = rxc_rot(make_float2(fre[256 + lane], fim[256 + lane]), fc * RXC_TS, 256 + lane);
    pp = cmulc(u, w);
    pp.x = rxc_sum_f(pp.x);
    pp.y = rxc_sum_f(pp.y);
    ff = (-1.0 / (2.0 * M_PI * 64.0 * RXC_TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (float_cfo) ff = (double)(float)ff;
}

// ---- the combined rotation in place, 64 samples per step: the LTF pair's sum over LTF1 (H = 0.5 (F1 + F2) conj(Lf) and
// fft() is linear), then the data windows ----
__device__ __forceinline__ void rxc_rotate(float *fre, float *fim, int lane, int nd, double fc, double ff) {
    const double fcf_ts = (fc + ff) * RXC_TS;
    const int k = 192 + lane;
    const float2 u = rxc_rot(make_float2(fre[k], fim[k]), fcf_ts, k);
    const float2 w = rxc_rot(make_float2(fre[k + 64], fim[k + 64]), fcf_ts, k + 64);
    fre[k] = u.x + w.x;
    fim[k] = u.y + w.y;
    for (int d = 0; d < nd; ++d) {
        const int kd = 336 + 80 * d + lane;
        const float2 v = rxc_rot(make_float2(fre[kd], fim[kd]), fcf_ts, kd);
        fre[kd] = v.x;
        fim[kd] = v.y;
    }
}

// ---- symbols: quad {LTF1 + LTF2, D_3q, D_3q+1, D_3q+2} ----
struct RxcQuad {
    int dsc;       // this lane's data symbol, clamped to D - 1 (lane 0 of a quad and the idle lanes transform one all the same)
    bool dlane;    // the lane holds a data symbol of the packet
    int k0;        // where its 64-sample window starts in fr[]
};
__device__ __forceinline__ RxcQuad rxc_quad(int lane, int nd) {
    const int role = lane & 3, dsym = 3 * (lane >> 2) + max(role - 1, 0), dsc = min(dsym, nd - 1);
    return RxcQuad{dsc, role >= 1 && dsym < nd, role == 0 ? 192 : 336 + 80 * dsc};
}
// a lane takes its window into registers, fft() = DFT(x (-1)^n), and runs the transform's first stage over the 16 columns
__device__ __forceinline__ void rxc_window(const float *fre, const float *fim, int k0, float2 (&x)[64]) {
    static_for<0, 64>([&](auto nc) {
        constexpr int n = decltype(nc)::value;
        const float vx = fre[k0 + n], vy = fim[k0 + n];
        x[n] = (n & 1) ? make_float2(-vx, -vy) : make_float2(vx, vy);
    });
    static_for<0, 16>([&](auto jc) { dif_stage1<false, decltype(jc)::value>(x); });
}
// Every window is in registers by now, so the wave's region is free: the quads in use park their finished spectra
// there (row pitch RXC_SPEC_PITCH floats: the lanes' 8-byte writes fall on distinct banks) for a pass with one
// subcarrier per lane.  No branch around the writes -- control flow inside the transform costs 60 spilled VGPRs: the
// idle lanes share one more row that nobody reads.
__device__ __forceinline__ float2 *rxc_spec_row(float *re, int lane, int nd) {
    return reinterpret_cast<float2 *>(re + min(lane, 4 * ((nd + 2) / 3)) * RXC_SPEC_PITCH);
}
// sub-transform R has finished bins 4 k + R
template <int R>
__device__ __forceinline__ void rxc_park(const float2 (&x)[64], float2 *spec_row) {
    static_for<0, 16>([&](auto kc) {
        constexpr int bin = 4 * decltype(kc)::value + R;
        spec_row[bin] = x[digit_rev4(bin)];
    });
}

// ---- the four sub-transforms with LS estimate, ZF, demap, EVM and BER in the lanes' registers (OFDM.c:830-1165, the
// helpers of ofdm_rxcommon.h); OUT: the spectra are parked as well, sub-block by sub-block ----
template <bool OUT>
__device__ __forceinline__ void rxc_demap(float2 (&x)[64], const uint32_t *dtable, int dsc, float *re, int lane, int nd, SymState &st) {
    const uint32_t wd[4] = {dtable[4 * dsc], dtable[4 * dsc + 1], dtable[4 * dsc + 2], dtable[4 * dsc + 3]};
    sym_init(st);
    auto Hof = [&](float2 Y, auto binc) { return ls_equalise<decltype(binc)::value>(Y); };
    [[maybe_unused]] float2 *spec_row = rxc_spec_row(re, lane, nd);
    if constexpr (OUT) rxc_wave_sync();
    static_for<0, 4>([&](auto rc) {
        constexpr int R = decltype(rc)::value;
        dif_sub16<false, R>(x);
        demap_sub<false, R, 2>(x, wd[R], Hof, nullptr, st);
        sched_fence();
        if constexpr (OUT) {
            rxc_park<R>(x, spec_row);
            sched_fence();
        }
    });
}

// the equalised subcarrier Z = Y / H = 2 Lf Y conj(S) / |S|^2 (OFDM.c:1044-1052) of data symbol d at `bin`, from the parked spectra
__device__ __forceinline__ float2 rxc_equalised(const float *re, int d, int bin) {
    const int l0 = 4 * (d / 3), ln = l0 + 1 + d % 3;
    const float2 Y = reinterpret_cast<const float2 *>(re + ln * RXC_SPEC_PITCH)[bin];
    const float2 S = reinterpret_cast<const float2 *>(re + l0 * RXC_SPEC_PITCH)[bin];
    const float r = __builtin_amdgcn_rcpf(fmaf(S.x, S.x, S.y * S.y));
    const float g = ((RXC_LTF_NEG >> bin) & 1ull) ? -2.0f * r : 2.0f * r;
    const float2 u = cmulc(Y, S);
    return make_float2(u.x * g, u.y * g);
}

// ---- the output pass: the equalised subcarriers and the decided bits (OFDM.c:852-908), one subcarrier per lane and
// step: coalesced stores, a 16-lane OR per word of 32 bits.  (Taken from the lanes' registers inside the metrics pass
// they cost 113 spilled VGPRs.) ----
__device__ __forceinline__ void rxc_outputs(const float *re, int lane, int nd, int64_t i, float2 *eq, uint32_t *bits) {
    rxc_wave_sync();
    const int nsc = 48 * nd;
    for (int j0 = 0; j0 < nsc; j0 += 64) {
        const int j = j0 + lane;
        const bool ok = j < nsc;
        const int jj = ok ? j : 0, d = jj / 48, m = jj - 48 * d, bin = data_bin(m);
        const float2 z = rxc_equalised(re, d, bin);
        if (eq && ok) eq[i * nsc + j] = z;
        const uint32_t pr = z.x > 0.f, pi = z.y > 0.f;
        uint32_t wv = ok ? (((pi ^ 1u) << 1) | (pr ^ pi)) << (30 - 2 * (lane & 15)) : 0u;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) wv |= (uint32_t)__shfl_xor((int)wv, o, 64);
        if (bits && ok && (lane & 15) == 0) bits[i * (3 * nd) + (j >> 4)] = wv;
    }
}

// ---- the packet's totals in symbol order ----
// A data symbol whose window lies wholly past the end of the samples (sample p + 2 (336 + 80 d) and all after it are
// at the end + 20 or beyond) reached the demapper as 64 exact zeros: Y = +-0 and u = +-0, and the sign bit of u, which
// demap_sub counts, is then an accident of S.  The reference decides "-" on both axes for a zero, as the output pass
// does, so that symbol's counts are the payload's own (ztable, zero_errors).  Those symbols are zfirst .. D - 1 (none
// unless oob); the branch is wave-uniform and rare, and it stands here, after the transforms (a branch inside them
// costs 60 spilled VGPRs).  Its EVM term needs nothing: u' = +-0 gives |0 - d|^2 either way.
__device__ __forceinline__ void rxc_totals(const SymState &st, bool dlane, int nd, int zfirst, const uint32_t *ztable,
                                           float &fe, uint32_t &ferr, uint32_t &fax) {
    const float fev = dlane ? finish_evm<2>(st) : 0.f;
    const uint32_t bev = dlane ? st.be : 0u, axv = dlane ? st.ax : 0u;
    fe = 0.f;
    ferr = 0u;
    fax = 0u;
    for (int d = 0; d < nd; ++d) {
        const int src = 4 * (d / 3) + 1 + d % 3;
        fe += __shfl(fev, src, 64);
        ferr += (uint32_t)__shfl((int)bev, src, 64);
        fax += (uint32_t)__shfl((int)axv, src, 64);
    }
    if (zfirst < nd) {
        for (int d = zfirst; d < nd; ++d) {
            const int src = 4 * (d / 3) + 1 + d % 3;
            const uint32_t z = ztable[d];
            ferr += (z & 0xffffu) - (uint32_t)__shfl((int)bev, src, 64);
            fax += (z >> 16) - (uint32_t)__shfl((int)axv, src, 64);
        }
    }
}

// ---- the decode half of the record and the packet's counter terms, from the totals (lane 0) ----
__device__ __forceinline__ void rxc_record(ofdm_capture_result *r, unsigned long long *acc, bool counters, int lane, int nd,
                                           float fe, uint32_t ferr, uint32_t fax) {
    if (lane == 0) {
        const float N = 48.0f * (float)nd;
        // a NaN sum (the long training symbols themselves past the end: S = 0, Z = 0 / 0) stays NaN, as the reference's
        const float db = fe > 0.f ? fmaxf(3.01029995663981195214f * __builtin_amdgcn_logf(fe / N), -400.f)
                                  : (fe == fe ? -400.f : fe);
        const float dbp = fax > 0u ? 3.01029995663981195214f * __builtin_amdgcn_logf(2.0f * (float)fax / N) : -INFINITY;
        r->bit_err = (int32_t)ferr;
        r->post_axis_err = (int32_t)fax;
        r->evm_pre_sum = fe;
        r->evm_db_pre = db;
        r->evm_db_post = dbp;
        r->ber = (float)ferr / (96.0f * (float)nd);
        if (counters) {
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
}

// the block's counter row, reduced in LDS, joins the caller's with 64-bit vector atomics
__device__ __forceinline__ void rxc_flush(const unsigned long long *acc, unsigned long long *counters) {
    __syncthreads();
    if (counters && threadIdx.x < RXC_ACC_WORDS && acc[threadIdx.x]) atomicAdd(&counters[threadIdx.x], acc[threadIdx.x]);
}

}  // namespace ofdm
