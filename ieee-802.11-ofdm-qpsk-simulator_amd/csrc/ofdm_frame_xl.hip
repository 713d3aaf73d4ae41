// ofdm_frame_xl.hip -- frame mode for long messages (ofdm_set_long_message: frames of 9..15 data symbols, captures of
// 6,447..9,394 samples) in a translation unit of its own.  The kernels of ofdm_frame.hip are budgeted to the byte for
// 1..8 symbols and PMC-certified by build id (codeobj.kernel_build_id), so nothing of theirs moves: these kernels take
// an argument block of their own (XlArgs = FrameArgs + the 15-symbol payload tables) and share only inlined device
// helpers with them.
//
//   frame_ring_xl_kernel  : the sweep's sync kernel.  frame_sync_long_kernel's capture ring carried to 4 or 5
//                           detection rounds: 11 waves per block and CU, 12,288 B of ring + mirror each.
//   frame_whole_xl_kernel : one-wave blocks holding the whole capture's real parts, any number of detection rounds:
//                           ofdm_receiver (external captures, every dump), word-length statistics, short user captures,
//                           OFDM_FRAME_NO_LONG=1 and every launch the ring kernel's LDS does not fit.  Same rounds, same
//                           lane starts, same arithmetic: every counter and packet_idx equals the ring kernel's.
//   frame_sym_xl_kernel   : frame_sym_kernel's quads for up to 16 hand-off windows per item.
#define OFDM_FRAME_XL_TU 1
#include "ofdm_frame.hip"

namespace ofdm {

using XlKArgs = const __attribute__((address_space(4))) XlArgs;
using FrKArgs = const __attribute__((address_space(4))) FrameArgs;

// ---- Packet_Detection (OFDM.c:659-683) of one lane's XL_CHUNK positions from n0: frame_sync_kernel's sliding sums
// and sign-bit crossings over register blocks of DET_B samples; tr_[k] / ti_[k] = Re / Im of sample n0 + k, k < 80.
// Crossing n0 + j at bit j of the result, positions from `npos` on masked. ----
__device__ __forceinline__ unsigned long long xl_detect_chunk(const __attribute__((address_space(3))) float *tr_,
                                                              const __attribute__((address_space(3))) float *ti_, int npos) {
    float sx = 0.f, sy = 0.f, pw = 0.f;
    uint32_t mlo = 0u, mhi = 0u;
    constexpr int nbat = (XL_CHUNK + DET_B - 1) / DET_B;
    float xr[nbat + 3][DET_B], xi[nbat + 3][DET_B];
    auto load_blk = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
#pragma unroll
        for (int k = 0; k < DET_B; ++k) { xr[j][k] = tr_[DET_B * j + k]; xi[j][k] = ti_[DET_B * j + k]; }
    };
    load_blk(std::integral_constant<int, 0>{});
    load_blk(std::integral_constant<int, 1>{});
    load_blk(std::integral_constant<int, 2>{});
    static_for<0, 2>([&](auto hc) {
        constexpr int h = decltype(hc)::value;
#pragma unroll
        for (int kk = 0; kk < DET_B; ++kk) {
            const float ux = xr[h][kk], uy = xi[h][kk], vx = xr[h + 1][kk], vy = xi[h + 1][kk];
            sx = fmaf(ux, vx, sx); sx = fmaf(-uy, vy, sx);
            sy = fmaf(ux, vy, sy); sy = fmaf(uy, vx, sy);
            pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
        }
    });
    static_for<0, nbat>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        load_blk(std::integral_constant<int, b + 3>{});
#pragma unroll
        for (int k = 0; k < DET_B; ++k) {
            const float o0x = xr[b][k], o0y = xi[b][k], o1x = xr[b + 1][k], o1y = xi[b + 1][k];
            const float i0x = xr[b + 2][k], i0y = xi[b + 2][k], i1x = xr[b + 3][k], i1y = xi[b + 3][k];
            const float num = fmaf(sx, sx, sy * sy), h = 0.75f * pw;
            const float tt = fmaf(h, pw, -num);
            mhi = __builtin_amdgcn_alignbit(mhi, mlo, 31);
            mlo = __builtin_amdgcn_alignbit(mlo, __float_as_uint(tt), 31);
            sx = fmaf(i0x, i1x, sx); sx = fmaf(-i0y, i1y, sx);
            sx = fmaf(-o0x, o1x, sx); sx = fmaf(o0y, o1y, sx);
            sy = fmaf(i0x, i1y, sy); sy = fmaf(i0y, i1x, sy);
            sy = fmaf(-o0x, o1y, sy); sy = fmaf(-o0y, o1x, sy);
            pw = fmaf(i1x, i1x, pw); pw = fmaf(i1y, i1y, pw);
            pw = fmaf(-o1x, o1x, pw); pw = fmaf(-o1y, o1y, pw);
        }
    });
    constexpr int J = nbat * DET_B;
    const unsigned long long rev = ((unsigned long long)__builtin_bitreverse32(mlo) << 32) | __builtin_bitreverse32(mhi);
    return (rev >> (64 - J)) & ((1ull << npos) - 1ull);           // 0 < npos <= XL_CHUNK < 64
}

// The rounds' crossing masks, one per lane and round, and Packet_Selection over them (frame_sync_long_kernel's)
struct XlCross {
    unsigned long long cm[XL_MAXR];     // lane l of round rho: crossing rho XL_ROUND + l XL_CHUNK + j at bit j
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int r = 0; r < XL_MAXR; ++r) cm[r] = 0ull;
    }
    // the crossing bit of position pos (inside the rounds detected) from the lane that owns it (ds_bpermute)
    __device__ __forceinline__ bool crossing(int pos, int R) const {
        const int rd = pos / XL_ROUND, rel = pos - rd * XL_ROUND;
        const int owner = rel / XL_CHUNK, bit = rel - owner * XL_CHUNK;
        unsigned long long w = 0ull;
        static_for<0, XL_MAXR>([&](auto r2c) {
            constexpr int r2 = decltype(r2c)::value;
            if (r2 < R) {
                const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)cm[r2], owner, 64);
                const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(cm[r2] >> 32), owner, 64);
                if (rd == r2) w = ((unsigned long long)hi << 32) | lo;
            }
        });
        return ((w >> bit) & 1ull) != 0ull;
    }
    // Packet_Selection (OFDM.c:685-771) over the first nr rounds: the least front whose +230 check is a crossing below
    // `limit` and that has a later front, or 0x7fffffff
    // (a lane's first and last crossing of a round are re-derived from its mask: 10 VGPRs less across the rounds)
    __device__ __forceinline__ int select(int nr, int limit, int lx) const {
        int vmin = 0x7fffffff, fmax_ = -1, carry = -1;
        static_for<0, XL_MAXR>([&](auto rc) {
            constexpr int rho = decltype(rc)::value;
            if (rho < nr) {
                const int n0 = rho * XL_ROUND + lx * XL_CHUNK;
                const int first = cm[rho] ? n0 + __builtin_ctzll(cm[rho]) : -1;
                const int last = cm[rho] ? n0 + 63 - __builtin_clzll(cm[rho]) : -1;
                const int pm = max(wave_prefix_max(last), carry);
                const int prev = max(wave_shr1(pm), carry);
                const int front = (first >= 0 && first - prev > 300) ? first : -1;
                carry = __builtin_amdgcn_readlane(pm, 63);
                const int pos = front + 230;
                const bool valid = crossing(pos < limit ? pos : 0, nr) && front >= 0 && pos < limit;
                vmin = min(vmin, valid ? front : 0x7fffffff);
                fmax_ = max(fmax_, front);
            }
        });
        const int cmin = wave_min_i(vmin), cmax = wave_max_i(fmax_);
        return cmin < cmax ? cmin : 0x7fffffff;
    }
};

// the matched filter's run u (frame_sync_kernel's runs of MF_RUN instants inside one needed range): instants [s0, e)
constexpr int XL_MF_RUN = 5, XL_MF_W = 2 * XL_MF_RUN + 19;
constexpr int XL_MF_C0 = (32 + XL_MF_RUN - 1) / XL_MF_RUN, XL_MF_C1 = XL_MF_C0 + (128 + XL_MF_RUN - 1) / XL_MF_RUN;
constexpr int XL_MF_CD = (64 + XL_MF_RUN - 1) / XL_MF_RUN;
constexpr int XL_MF_FIRST = 80;                       // the first run's first instant
__device__ __forceinline__ void xl_mf_range(int u, int &s0, int &e) {
    if (u < XL_MF_C0) {
        s0 = XL_MF_FIRST + XL_MF_RUN * u; e = 112;
    } else if (u < XL_MF_C1) {
        s0 = 192 + XL_MF_RUN * (u - XL_MF_C0); e = 320;
    } else {
        const int d = (u - XL_MF_C1) / XL_MF_CD, k = u - XL_MF_C1 - d * XL_MF_CD;
        s0 = 336 + 80 * d + XL_MF_RUN * k; e = 400 + 80 * d;
    }
    e = min(e, s0 + XL_MF_RUN);
}
// the outputs of one run from its window's samples (x[k] = sample n_lo + k): symmetric taps, 11 FMAs per component
__device__ __forceinline__ float2 xl_mf_out(const float (&xr)[XL_MF_W], const float (&xi)[XL_MF_W], const float (&tv)[11],
                                            int o) {
    float2 v = make_float2(xr[2 * o + 10] * tv[10], xi[2 * o + 10] * tv[10]);
#pragma unroll
    for (int tt = 0; tt < 10; ++tt) {
        v.x = fmaf(xr[2 * o + 20 - tt] + xr[2 * o + tt], tv[tt], v.x);
        v.y = fmaf(xi[2 * o + 20 - tt] + xi[2 * o + tt], tv[tt], v.y);
    }
    return v;
}
// the RRC taps scalar-loaded from the kernarg segment and moved to VGPRs (frame_sync_kernel)
__device__ __forceinline__ void xl_taps(float (&tv)[11]) {
    using kchar = __attribute__((address_space(4))) char;
    using kfloat = __attribute__((address_space(4))) float;
    const kfloat *tp = (const kfloat *)((const kchar *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(XlArgs, f) +
                                        offsetof(FrameArgs, taps));
    asm volatile("" : "+s"(tp));
#pragma unroll
    for (int j = 0; j < 11; ++j) asm volatile("v_mov_b32 %0, %1" : "=v"(tv[j]) : "s"(tp[j]));
}

// coarse / fine CFO (OFDM.c:773-828) from fr[] and the hand-off of the rotated windows (frame_sync_kernel's generic
// path); dbg_frame: the single-capture dump of every rotated sample, or null
template <typename A>
__device__ __forceinline__ void xl_cfo_handoff(const A &a, const float2 *fr, int lx, int n_data, int64_t i, float2 *dbg_frame) {
    const float2 cu = fr[80 + (lx & 15)], cw = fr[96 + (lx & 15)], l1 = fr[192 + lx], l2 = fr[256 + lx];
    float2 pp = make_float2(0.f, 0.f);
    if (lx < 16) pp = make_float2(cu.x * cw.x + cu.y * cw.y, cu.y * cw.x - cu.x * cw.y);
    pp.x = wave_sum_f(pp.x);
    pp.y = wave_sum_f(pp.y);
    double fc = (-1.0 / (2.0 * M_PI * 16.0 * TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (a.float_cfo) fc = (double)(float)fc;
    {
        const float2 u = cfo_rot(l1, fc * TS, 192 + lx), w = cfo_rot(l2, fc * TS, 256 + lx);
        pp = make_float2(u.x * w.x + u.y * w.y, u.y * w.x - u.x * w.y);
    }
    pp.x = wave_sum_f(pp.x);
    pp.y = wave_sum_f(pp.y);
    double ff = (-1.0 / (2.0 * M_PI * 64.0 * TS)) * (double)atan2_cfo(pp.y, pp.x);
    if (a.float_cfo) ff = (double)(float)ff;
    const int nw = 1 + n_data, nfr = fr_len(n_data);
    float2 *dst = win_item(a.win, a.ipb, nw, i);
    const double fcf_ts = (fc + ff) * TS;
    if (dbg_frame)
        for (int k = lx; k < nfr; k += 64) dbg_frame[k] = cfo_rot(fr[k], fcf_ts, k);
    // element j = sample j / nw of window j % nw (j / nw by a 16-bit reciprocal, exact for j < 64 nw <= 1,024)
    const uint32_t inv_nw = (65536u + (uint32_t)nw - 1u) / (uint32_t)nw;
    for (int j = lx; j < 64 * nw; j += 64) {
        const int n = (int)(((uint32_t)j * inv_nw) >> 16), w = j - n * nw;
        float2 v;
        if (w == 0) {
            const float2 u = cfo_rot(fr[192 + n], fcf_ts, 192 + n), x = cfo_rot(fr[256 + n], fcf_ts, 256 + n);
            v = make_float2(u.x + x.x, u.y + x.y);
        } else {
            const int k = 336 + 80 * (w - 1) + n;
            v = cfo_rot(fr[k], fcf_ts, k);
        }
        dst[win_off(n, a.ipb, nw) + w] = v;
    }
}

// capture_blocks' ring form for captures up to 4 XL_RING samples (three unsigned reductions of the ring position; the
// shared helper reduces twice, enough for 8 symbols): Philox blocks bs..be into the wave's ring, block b at float
// 4 (b - b0) mod XL_RING and, when that is below XL_EXT, also at its mirror past XL_RING.  The same draws and the same
// fp32 arithmetic per sample as capture_blocks.  TRIM: the last pass draws only as many blocks per lane as it stores.
template <bool TRIM, typename A>
__device__ __forceinline__ void capture_blocks_xl(const A &a, int wave_len, float *rbase, int b0, int bs, int be, int lane,
                                                  uint32_t t_lo, uint32_t t_hi, uint32_t qs, float sigma) {
    const PhiloxHead hd = philox_head(t_lo, t_hi, STREAM_NOISE | qs, a.k1);
    const float Ksig = noise_k(sigma);
    PhiloxKeysV vk;
    vk.init(a.k0, a.k1);
    const uint32_t pb = (uint32_t)(wave_len / (4 * FR_REPS)), nb_wave = (uint32_t)(wave_len / 4);
    uint32_t bm = (uint32_t)(bs + lane) % pb;
    const bool real = a.noise == OFDM_NOISE_REAL;
    auto pass = [&](auto uc, int p0) {
        constexpr int U = decltype(uc)::value;
        const int bb = p0 + lane;
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = bb + 64 * u;
            const float4 re = *reinterpret_cast<const float4 *>(a.wave_re + 4 * bm);     // bm < pb: inside the table
            const bool in = (uint32_t)b < nb_wave;                     // past the waveform's end: zeros
            v[u] = in ? re : make_float4(0.f, 0.f, 0.f, 0.f);
            bm = bm + 64 >= pb ? bm + 64 - pb : bm + 64;           // (bm + 64) mod pb (pb > 64)
        }
        if (real) {
            uint32_t c2[U];
            uint4 o[U];
#pragma unroll
            for (int u = 0; u < U; ++u) c2[u] = (uint32_t)(bb + 64 * u);
            philox10_c2_multi(hd, c2, vk, o);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Noise4 nz = noise4_of(o[u], Ksig);
                v[u].x = fmaf(nz.r0, nz.c0, v[u].x); v[u].y = fmaf(nz.r0, nz.s0, v[u].y);
                v[u].z = fmaf(nz.r1, nz.c1, v[u].z); v[u].w = fmaf(nz.r1, nz.s1, v[u].w);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (bb + 64 * u <= be) {
                uint32_t pos = 4u * (uint32_t)(bb + 64 * u - b0);       // < 4 XL_RING: three unsigned reductions
                pos = min(pos, pos - (uint32_t)XL_RING);
                pos = min(pos, pos - (uint32_t)XL_RING);
                pos = min(pos, pos - (uint32_t)XL_RING);
                *reinterpret_cast<float4 *>(rbase + pos) = v[u];
                if (pos < (uint32_t)XL_EXT) *reinterpret_cast<float4 *>(rbase + pos + XL_RING) = v[u];
            }
    };
    using U4 = std::integral_constant<int, FRAME_CAP_U>;
    int p0 = bs;
    if constexpr (TRIM) {
        for (; be - p0 >= 3 * 64; p0 += FRAME_CAP_U * 64) pass(U4{}, p0);
        if (be - p0 >= 2 * 64) pass(std::integral_constant<int, 3>{}, p0);
        else if (be - p0 >= 64) pass(std::integral_constant<int, 2>{}, p0);
        else if (be - p0 >= 0) pass(std::integral_constant<int, 1>{}, p0);
    } else {
        for (; p0 <= be; p0 += FRAME_CAP_U * 64) pass(U4{}, p0);
    }
}

// ---------------------------------------------------------------- the ring kernel (generated captures, sweeps)
// frame_sync_long_kernel's design for R = ceil((L - 47) / 1,984) = 4 or 5 rounds: the wave's ring always holds the last
// XL_RING - 3 samples generated, a round's piece [rho 1,984, +2,031) is generated before its detection, the crossing
// masks of every round stay in registers.  Lazy: after each round from the second on (but the last), Packet_Selection
// over the rounds done decides when their least valid front (its +230 check inside them) has a later front inside
// them -- fronts and checks depend only on earlier positions and every later front lies past it, so the full rule
// picks the same front -- and the remaining rounds and their samples are skipped (a.no_lazy: never).  Then the part of
// the matched-filter window [p + 140, p + 2 (nfr - 1) + 10] (at most 2,909 samples) that the ring lacks is generated
// again, forward past the resident samples or backward below them.  The imaginary parts come from a table of one
// period + XL_TABLE_REACH floats: a detection round reduces one uniform base (its lanes read up to 2,033 floats past
// it), a matched-filter run its own start (29 floats).
// LDS for 15 symbols at 16 SNR points: 256 + 20,432 + 11 x 12,288 = 155,856 B of the CU's 163,840: one block per CU,
// 3, 3, 3, 2 waves on its SIMDs.
constexpr int XL_MAXP = 4;                            // matched-filter passes of 64 runs (33 + 13 x 15 = 228 runs)
__global__ __launch_bounds__(64 * XL_RING_W, 3) void frame_ring_xl_kernel(XlArgs xa0) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const FrameArgs &a0 = xa0.f;
    const int L = a0.cap_len, Lc = L - 47;
    const int nfr = fr_len(a0.n_data);
    constexpr int ns = 2;
    unsigned long long *acc = smem;                                           // [n_snr][2]
    float *imt = reinterpret_cast<float *>(acc + a0.n_snr * ns);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *rbase = imt + ((a0.imt_len + 3) & ~3) + wv * XL_RING_REGION;
    for (int i = threadIdx.x; i < a0.n_snr * ns; i += 64 * XL_RING_W) acc[i] = 0ull;
    for (int k = threadIdx.x; k < a0.imt_len; k += 64 * XL_RING_W) imt[k] = a0.wave[k % a0.im_period].y;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int R = (Lc + XL_ROUND - 1) / XL_ROUND;                             // 4 or 5 (host-checked)
    const int nwaves = (int)gridDim.x * XL_RING_W;
    int64_t run_end = ((int64_t)blockIdx.x * XL_RING_W + wv) * FRAME_ITEM_RUN + FRAME_ITEM_RUN;
    int nxt = 0;
    for (int64_t i = run_end - FRAME_ITEM_RUN; i < a0.n_items;) {
        // the kernel arguments are re-read per item (frame_sync_kernel)
        XlKArgs *ap = (XlKArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ap));
        FrKArgs &a = ap->f;
        const int n_data = a.n_data, wave_len = a.wave_len;
        const ImMod im_mod{a.im_period, a.im_magic};
        if (lane == 0 && i == run_end - FRAME_ITEM_RUN) nxt = nwaves + (int)atomicAdd(a.work, 1ull);
        uint32_t qr;
        const int64_t ti = a.trial0 + snr_divmod((uint32_t)a.q0 + (uint32_t)i, (uint32_t)a.n_snr, a.snr_magic, qr);
        const int q = (int)qr;
        const uint64_t t = a.first_trial + (uint64_t)ti;
        const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32), qs = (uint32_t)(a.q_base + q);
        const float sigma = a.sigma[q];
        int rx_start = a.fixed_start;
        if (rx_start < 0) {
            const uint4 o = philox10(t_lo, t_hi, 0u, STREAM_START | qs, a.k0, a.k1);
            rx_start = (int)(o.x % (uint32_t)(wave_len - L));
        }
        rx_start = __builtin_amdgcn_readfirstlane(rx_start);
        const int off = rx_start & 3, b0 = rx_start >> 2;
        // capture sample n lives at ring float (n + off) mod XL_RING (and its mirror past XL_RING when < XL_EXT);
        // n + off < 3 XL_RING: two unsigned reductions
        auto ring = [&](int n) {
            uint32_t x = (uint32_t)(n + off);
            x = min(x, x - (uint32_t)XL_RING);
            x = min(x, x - (uint32_t)XL_RING);
            return (int)min(x, x - (uint32_t)XL_RING);
        };
        // samples [n_lo, n_hi) into the ring (whole Philox blocks: up to 3 samples either side, with their own values)
        auto gen = [&](int n_lo, int n_hi, auto trim) {
            capture_blocks_xl<decltype(trim)::value>(a, wave_len, rbase, b0, (rx_start + n_lo) >> 2, (rx_start + n_hi - 1) >> 2,
                                                     lane, t_lo, t_hi, qs, sigma);
        };
        const int im0 = im_mod(rx_start);
        int lx = lane;
        opaque(lx);
        XlCross cr;
        cr.clear();
        auto detect = [&](auto rc) {
            constexpr int rho = decltype(rc)::value;
            const int n0 = rho * XL_ROUND + lx * XL_CHUNK, n1 = min(n0 + XL_CHUNK, Lc);
            unsigned long long cmask = 0ull;
            if (n0 < n1) {
                using LdsF = const __attribute__((address_space(3))) float;
                LdsF *ti_ = (LdsF *)(imt + im_mod(im0 + rho * XL_ROUND) + lx * XL_CHUNK);   // uniform base + lane offset
                LdsF *tr_ = (LdsF *)(rbase + ring(n0));                 // 80 floats: inside ring + mirror
                opaque(ti_);
                opaque(tr_);
                cmask = xl_detect_chunk(tr_, ti_, n1 - n0);
            }
            cr.cm[rho] = cmask;
        };
        auto piece = [&](int rho) { gen(rho * XL_ROUND, min(L, rho * XL_ROUND + XL_PIECE), std::false_type{}); };
        piece(0);
        wave_lds_sync();
        detect(std::integral_constant<int, 0>{});
        int cand = 0x7fffffff, held = 0;
        static_for<1, XL_MAXR>([&](auto rc) {
            constexpr int rho = decltype(rc)::value;
            if (rho < R && cand == 0x7fffffff) {
                wave_lds_sync();                              // the round before's loads are done: this piece overwrites
                piece(rho);
                wave_lds_sync();
                detect(rc);
                held = rho;
                if (rho == R - 1) cand = cr.select(R, Lc, lx);
                else if (!a.no_lazy) cand = cr.select(rho + 1, (rho + 1) * XL_ROUND, lx);
            }
        });
        const bool sync_fail = cand == 0x7fffffff;
        const int p = sync_fail ? 0 : cand + 10 + 1;
        // ---- the matched filter's samples [lo, hi]: the ring holds [res_lo, res_hi) after the last piece ----
        {
            const int lo = p + 2 * XL_MF_FIRST - 20, hi = min(p + 2 * (nfr - 1) + 10, L - 1);
            const int res_hi = min(L, held * XL_ROUND + XL_PIECE), res_lo = res_hi + 3 - XL_RING;
            if (hi >= res_hi || lo < res_lo) {
                wave_lds_sync();                              // detection's loads are done
                const bool fwd = hi >= res_hi;
                gen(fwd ? max(lo, res_hi) : lo, fwd ? hi + 1 : min(hi + 1, res_lo), std::true_type{});
                wave_lds_sync();
            }
        }
        // ---- RRC matched filter at the needed instants, outputs held in registers until every lane's reads are done ----
        bool oob_l = false;
        float tv[11];
        xl_taps(tv);
        const int par_r = (off + p) & 1, par_i = (im0 + p) & 1;    // ring floats keep the parity (XL_RING even)
        const int n_runs = XL_MF_C1 + XL_MF_CD * n_data;
        const int im_mf = im0 + p - 20 + a.im_period;            // table index of sample p - 20 before reduction (uniform)
        float2 mfo[XL_MAXP][XL_MF_RUN];
        static_for<0, XL_MAXP>([&](auto pc) {
            constexpr int pi = decltype(pc)::value;
            const int u = lx + 64 * pi;
            int s0 = 0, e = 0;
            if (u < n_runs) xl_mf_range(u, s0, e);
            const int n_lo = p + 2 * s0 - 20;
            if (u < n_runs && n_lo >= 0 && p + 2 * (e - 1) < L) {
                float xr[XL_MF_W], xi[XL_MF_W];
                const int si = im_mod(im_mf + 2 * s0);                        // < 2^14; 29 floats from it: inside the table
                const int rl = ring(n_lo);                                    // 29 floats: inside ring + mirror
                if (par_r) lds_readn<1, FRAME_MF_B64_GEN>(rbase, rl, xr); else lds_readn<0, FRAME_MF_B64_GEN>(rbase, rl, xr);
                if (par_i) lds_readn<1, FRAME_MF_B64_GEN>(imt, si, xi); else lds_readn<0, FRAME_MF_B64_GEN>(imt, si, xi);
#pragma unroll
                for (int o = 0; o < XL_MF_RUN; ++o) mfo[pi][o] = xl_mf_out(xr, xi, tv, o);
            } else {
#pragma unroll
                for (int o = 0; o < XL_MF_RUN; ++o) {        // the per-instant path (windows leaving the capture)
                    const int n = p + 2 * (s0 + o);
                    float2 v = make_float2(0.f, 0.f);
                    if (u < n_runs && s0 + o < e) {
                        if (n >= L + 20) {
                            oob_l = true;
                        } else {
                            for (int tt = 0; tt < 21; ++tt) {
                                const int m = n - tt;
                                const int mc = min(max(m, 0), L - 1);
                                const bool in = m >= 0 && m < L;
                                const float xr = in ? rbase[ring(mc)] : 0.f, xi = in ? imt[im_mod(im0 + mc)] : 0.f;
                                const float h = tv[tt <= 10 ? tt : 20 - tt];
                                v.x = fmaf(xr, h, v.x);
                                v.y = fmaf(xi, h, v.y);
                            }
                        }
                    }
                    mfo[pi][o] = v;
                }
            }
        });
        const bool oob = __ballot(oob_l) != 0ull;
        wave_lds_sync();                                      // every lane's capture reads are done
        float2 *fr = reinterpret_cast<float2 *>(rbase);       // fr[] overwrites the region (2 nfr <= XL_RING_REGION floats)
        static_for<0, XL_MAXP>([&](auto pc) {
            constexpr int pi = decltype(pc)::value;
            const int u = lx + 64 * pi;
            int s0 = 0, e = 0;
            if (u < n_runs) xl_mf_range(u, s0, e);
#pragma unroll
            for (int o = 0; o < XL_MF_RUN; ++o)
                if (s0 + o < e) fr[s0 + o] = mfo[pi][o];
        });
        wave_lds_sync();
        xl_cfo_handoff(a, fr, lx, n_data, i, nullptr);
        if (lx == 0) {
            a.info[i] = make_int4(p, sync_fail, oob, rx_start);
            if (sync_fail) atomicAdd(&acc[q * ns + 0], 1ull);
            if (oob) atomicAdd(&acc[q * ns + 1], 1ull);
            if (a.pidx_out) a.pidx_out[(int64_t)q * a.n_trials + ti] = p;
        }
        if (i + 1 < run_end) {
            ++i;
        } else {
            i = (int64_t)__builtin_amdgcn_readfirstlane(nxt) * FRAME_ITEM_RUN;
            run_end = i + FRAME_ITEM_RUN;
        }
        wave_lds_sync();                                      // the next capture overwrites this item's region
    }
    __syncthreads();
    for (int k = threadIdx.x; k < a0.n_snr; k += 64 * XL_RING_W) {
        unsigned long long *c = a0.counters + k * OFDM_NCOUNTERS;
        const unsigned long long *sl = acc + k * ns;
        if (sl[0]) atomicAdd(&c[OFDM_C_SYNC_FAIL], sl[0]);
        if (sl[1]) atomicAdd(&c[OFDM_C_OOB], sl[1]);
    }
}

// ---------------------------------------------------------------- the whole-capture kernel (one wave per block)
// frame_sync_kernel<0, 0, 1>'s generic path -- generated or external captures, the parity dumps, the word-length
// statistics, fr[] in the part of the region the matched filter does not read -- with the detection in
// R = ceil((L - 47) / 1,984) rounds of 64 lanes x 31 positions (any R <= XL_MAXR) and no lazy capture.  15 symbols: 37.7 KB
// of capture + a 12.8 KB table per block, three blocks per CU (a four-wave block would need more than the CU has).
__global__ __launch_bounds__(64) void frame_whole_xl_kernel(XlArgs xa0) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const FrameArgs &a0 = xa0.f;
    const int L = a0.cap_len, Lc = L - 47;
    const int nfr = fr_len(a0.n_data);
    const int ns = acc_slots(a0.word_stats);
    unsigned long long *acc = smem;                                           // [n_snr][ns]
    float *imt = reinterpret_cast<float *>(acc + a0.n_snr * ns);
    float *rbase = imt + ((a0.imt_len + 3) & ~3);
    float2 *const fr_sep = reinterpret_cast<float2 *>(rbase + a0.region_floats - 2 * nfr);   // when !fr_in_cap
    for (int i = threadIdx.x; i < a0.n_snr * ns; i += 64) {
        const int k = i % ns;
        acc[i] = k == 2 ? (unsigned long long)INT64_MAX : k == 3 ? (unsigned long long)INT64_MIN : 0ull;
    }
    // generated captures: imt[k] = Im wave[k mod nfilt]; an external capture its own imaginary parts, zero past L
    for (int k = threadIdx.x; k < a0.imt_len; k += 64)
        imt[k] = a0.ext ? (k < L ? a0.ext[k].y : 0.f) : a0.wave[k % a0.im_period].y;
    __syncthreads();
    const int lane = threadIdx.x;
    const int R = (Lc + XL_ROUND - 1) / XL_ROUND;
    const int nwaves = (int)gridDim.x;
    int64_t run_end = (int64_t)blockIdx.x * FRAME_ITEM_RUN + FRAME_ITEM_RUN;
    int nxt = 0;
    for (int64_t i = run_end - FRAME_ITEM_RUN; i < a0.n_items;) {
        XlKArgs *ap = (XlKArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ap));
        FrKArgs &a = ap->f;
        const int n_data = a.n_data, wave_len = a.wave_len;
        const bool word_stats = a.word_stats;
        const ImMod im_mod{a.im_period, a.im_magic};
        if (lane == 0 && i == run_end - FRAME_ITEM_RUN) nxt = nwaves + (int)atomicAdd(a.work, 1ull);
        const int64_t g = a.item0 + i;
        uint32_t qr;
        const int64_t ti = a.trial0 + snr_divmod((uint32_t)a.q0 + (uint32_t)i, (uint32_t)a.n_snr, a.snr_magic, qr);
        const int q = (int)qr;
        const uint64_t t = a.first_trial + (uint64_t)ti;
        const uint32_t t_lo = (uint32_t)t, t_hi = (uint32_t)(t >> 32), qs = (uint32_t)(a.q_base + q);
        const float sigma = a.sigma[q];
        const bool first_item = g == 0;
        const bool ext = a.ext && first_item;
        int rx_start = a.fixed_start;
        if (rx_start < 0) {
            const uint4 o = philox10(t_lo, t_hi, 0u, STREAM_START | qs, a.k0, a.k1);
            rx_start = (int)(o.x % (uint32_t)(wave_len - L));
        }
        rx_start = __builtin_amdgcn_readfirstlane(rx_start);
        const int off = rx_start & 3;
        const float *r = rbase + off;                       // r[n] = Re capture sample n
        const int im0 = ext ? 0 : im_mod(rx_start);
        if (ext) {
            for (int n = lane; n < L; n += 64) rbase[off + n] = a.ext[n].x;
        } else {
            const int b0 = rx_start >> 2, b1 = (rx_start + L - 1) >> 2;
            capture_blocks(a, wave_len, rbase, b0, b0, b1, lane, t_lo, t_hi, qs, sigma);
        }
        wave_lds_sync();
        int lx = lane;
        opaque(lx);
        // ---- Word_Optimization_Analysis(Rx_filter_signal) (OFDM.c:38-73, 962-967), opt-in ----
        if (word_stats) {
            float mn = 1e9f, mx = -1e9f;
            for (int k = lx; k < L + 20; k += 64) {
                float2 v = make_float2(0.f, 0.f);
#pragma unroll
                for (int j = 0; j < 21; ++j) {
                    const int m = k - j;
                    if (m >= 0 && m < L) {
                        const int mi = im_mod(im0 + m);
                        v.x = fmaf(r[m], a.taps[j], v.x);
                        v.y = fmaf(imt[mi], a.taps[j], v.y);
                    }
                }
                mn = fminf(mn, fminf(v.x, v.y));
                mx = fmaxf(mx, fmaxf(v.x, v.y));
            }
            mn = wave_min_f(mn);
            mx = wave_max_f(mx);
            if (lx == 0) {
                atomicMin(reinterpret_cast<long long *>(&acc[q * ns + 2]), (long long)__float2ll_rn(mn * (float)OFDM_EVM_Q_SCALE));
                atomicMax(reinterpret_cast<long long *>(&acc[q * ns + 3]), (long long)__float2ll_rn(mx * (float)OFDM_EVM_Q_SCALE));
            }
        }
        // ---- Packet_Detection in R rounds (the ring kernel's lane starts), then Packet_Selection over all of them ----
        XlCross cr;
        cr.clear();
        static_for<0, XL_MAXR>([&](auto rc) {
            constexpr int rho = decltype(rc)::value;
            if (rho < R) {
                const int n0 = rho * XL_ROUND + lx * XL_CHUNK, n1 = min(n0 + XL_CHUNK, Lc);
                unsigned long long cmask = 0ull;
                if (n0 < n1) {
                    using LdsF = const __attribute__((address_space(3))) float;
                    LdsF *ti_ = (LdsF *)(imt + im_mod(im0 + n0));      // 80 floats from it: inside the table's IMT_EXT
                    LdsF *tr_ = (LdsF *)(r + n0);                      // 80 floats: inside the region (xl_cap_region)
                    opaque(ti_);
                    opaque(tr_);
                    cmask = xl_detect_chunk(tr_, ti_, n1 - n0);
                }
                cr.cm[rho] = cmask;
            }
        });
        if (a.dbg_corr && first_item) {             // Corr_Out for ofdm_receiver's parity dump
            for (int n = lx; n < Lc; n += 64) {
                float sx = 0.f, sy = 0.f, pw = 0.f;
                for (int k = 0; k < 32; ++k) {
                    const float ux = r[n + k], uy = imt[im_mod(im0 + n + k)];
                    const float vx = r[n + k + 16], vy = imt[im_mod(im0 + n + k + 16)];
                    sx += ux * vx - uy * vy;
                    sy += ux * vy + uy * vx;
                    pw += vx * vx + vy * vy;
                }
                a.dbg_corr[n] = (sx * sx + sy * sy) / (pw * pw);
            }
        }
        const int cand = cr.select(R, Lc, lx);
        const bool sync_fail = cand == 0x7fffffff;
        const int p = sync_fail ? 0 : cand + 10 + 1;           // len_RRC_rx + 1 (OFDM.c:758)
        // fr[] (float2) in the unread prefix [0, off + lo) or the unread suffix (off + hi, region) of the region
        float2 *fr = fr_sep;
        if (a.fr_in_cap) {
            const int lo = max(p - 20, 0), hi = min(p + 2 * nfr - 2, L - 1);
            fr = off + lo >= 2 * nfr ? reinterpret_cast<float2 *>(rbase)
                                     : reinterpret_cast<float2 *>(rbase + ((off + hi + 2) & ~1));
        }
        // ---- RRC matched filter at the down-sampled instants (frame_sync_kernel's runs; every instant for the dump) ----
        const bool dbg = a.dbg_frame && first_item;
        bool oob_l = false;
        float tv[11];
        xl_taps(tv);
        const int par_r = (off + p) & 1, par_i = (im0 + p) & 1;
        auto mf_one = [&](int ii) {
            const int n = p + 2 * ii;
            float2 v = make_float2(0.f, 0.f);
            if (n >= L + 20) {
                oob_l = true;                                    // the reference reads past its buffer
            } else {
#pragma unroll
                for (int tt = 0; tt < 21; ++tt) {
                    const int m = n - tt;
                    const int mc = min(max(m, 0), L - 1);
                    const bool in = m >= 0 && m < L;
                    const float xr = in ? r[mc] : 0.f, xi = in ? imt[im_mod(im0 + mc)] : 0.f;
                    const float h = tv[tt <= 10 ? tt : 20 - tt];
                    v.x = fmaf(xr, h, v.x);
                    v.y = fmaf(xi, h, v.y);
                }
            }
            fr[ii] = v;                                          // outside every lane's reads
        };
        if (dbg) {
            for (int j = lx; j < nfr; j += 64) mf_one(j);
        } else {
            const int n_runs = XL_MF_C1 + XL_MF_CD * n_data;
            for (int u = lx; u < n_runs; u += 64) {
                int s0, e;
                xl_mf_range(u, s0, e);
                const int n_lo = p + 2 * s0 - 20;                // first sample read
                if (n_lo >= 0 && p + 2 * (e - 1) < L) {
                    float xr[XL_MF_W], xi[XL_MF_W];
                    const int si = im_mod(im0 + n_lo);
                    if (par_r) lds_readn<1, FRAME_MF_B64_GEN>(rbase, off + n_lo, xr); else lds_readn<0, FRAME_MF_B64_GEN>(rbase, off + n_lo, xr);
                    if (par_i) lds_readn<1, FRAME_MF_B64_GEN>(imt, si, xi); else lds_readn<0, FRAME_MF_B64_GEN>(imt, si, xi);
#pragma unroll
                    for (int o = 0; o < XL_MF_RUN; ++o)
                        if (s0 + o < e) fr[s0 + o] = xl_mf_out(xr, xi, tv, o);
                } else {
                    for (int ii = s0; ii < e; ++ii) mf_one(ii);
                }
            }
        }
        const bool oob = __ballot(oob_l) != 0ull;
        wave_lds_sync();
        xl_cfo_handoff(a, fr, lx, n_data, i, dbg ? a.dbg_frame : nullptr);
        if (lx == 0) {
            a.info[i] = make_int4(p, sync_fail, oob, rx_start);
            if (sync_fail) atomicAdd(&acc[q * ns + 0], 1ull);
            if (oob) atomicAdd(&acc[q * ns + 1], 1ull);
            if (a.pidx_out) a.pidx_out[(int64_t)q * a.n_trials + ti] = p;
            if (first_item && a.dbg_ints) { a.dbg_ints[0] = p; a.dbg_ints[1] = sync_fail; a.dbg_ints[2] = oob; a.dbg_ints[3] = rx_start; }
        }
        if (i + 1 < run_end) {
            ++i;
        } else {
            i = (int64_t)__builtin_amdgcn_readfirstlane(nxt) * FRAME_ITEM_RUN;
            run_end = i + FRAME_ITEM_RUN;
        }
        wave_lds_sync();                                      // the next capture overwrites this item's region
    }
    __syncthreads();
    for (int k = threadIdx.x; k < a0.n_snr; k += 64) {
        unsigned long long *c = a0.counters + k * OFDM_NCOUNTERS;
        const unsigned long long *sl = acc + k * ns;
        if (sl[0]) atomicAdd(&c[OFDM_C_SYNC_FAIL], sl[0]);
        if (sl[1]) atomicAdd(&c[OFDM_C_OOB], sl[1]);
        if (ns == 4) {          // word_stats
            atomicMin(reinterpret_cast<long long *>(&c[OFDM_C_WL_MIN_Q]), (long long)sl[2]);
            atomicMax(reinterpret_cast<long long *>(&c[OFDM_C_WL_MAX_Q]), (long long)sl[3]);
        }
    }
}

// ---------------------------------------------------------------- symbols of the synced frames, up to 16 windows
// frame_sym_kernel's quads -- {LTF, D_3k, D_3k+1, D_3k+2}: 3..5 quads per item for 9..15 data symbols, whole items per
// wave (15 symbols: 5 quads, 3 items per wave, 12 per tile) -- reading the long argument block's demap words.
template <bool DUMP>   // DUMP: item 0's bits / subcarriers / metrics for ofdm_receiver
__global__ __launch_bounds__(SYM_THREADS, DUMP ? FRAME_SYM_MINB : 3) void frame_sym_xl_kernel(XlArgs xa) {
    const FrameArgs &a = xa.f;
    const int n_data = a.n_data;
    __shared__ unsigned long long acc[OFDM_MAX_SNR][8];
    constexpr int DPQ_MAX = 3;
    __shared__ float part_e[SYM_THREADS / 4][DPQ_MAX];       // per quad: EVM of its data symbols
    __shared__ uint32_t part_b[SYM_THREADS / 4][DPQ_MAX], part_a[SYM_THREADS / 4][DPQ_MAX];
    for (int k = threadIdx.x; k < a.n_snr * 8; k += SYM_THREADS) (&acc[0][0])[k] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, quad = threadIdx.x >> 2, role = lane & 3;
    const int qpi = (SYM_THREADS / 4) / a.ipb;                                  // quads per item from the tile size
    const int dpq = max(2, (n_data + qpi - 1) / qpi), r0 = 4 - dpq;             // data lanes per quad, first data role
    const int ipw = 16 / qpi, ipb = 4 * ipw;                               // items per wave, per block
    const int wq = quad & 15, item_l = (quad >> 4) * ipw + wq / qpi, qi = wq - (wq / qpi) * qpi;
    const int dsym = dpq == 2 ? 2 * qi + (role & 1) : 3 * qi + max(role - 1, 0);
    const int nw = 1 + n_data;
    const int dsc = min(dsym, n_data - 1);
    const int w = role < r0 ? 0 : 1 + dsc;
    for (int64_t base = (int64_t)blockIdx.x * ipb; base < a.n_items; base += (int64_t)gridDim.x * ipb) {
        const int64_t i = base + item_l;
        const bool item_ok = wq < ipw * qpi && i < a.n_items;
        const bool dlane = item_ok && role >= r0 && dsym < n_data;
        const float2 *src = win_item(a.win, ipb, nw, item_ok ? i : base) + w;
        float2 x[64];
        static_for<0, 4>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            gcf2 *sp = (gcf2 *)src;
            opaque(sp);
            static_for<0, 16>([&](auto pc) {
                constexpr int n = 16 * (decltype(pc)::value >> 2) + 4 * g + (decltype(pc)::value & 3);
                const float2 v = gld(sp, win_off(n, ipb, nw));
                x[n] = (n & 1) ? make_float2(-v.x, -v.y) : v;
            });
            if constexpr ((g + 1) % FRAME_SYM_GROUPS == 0) {
                static_for<0, 4 * FRAME_SYM_GROUPS>([&](auto ic) {
                    dif_stage1<false, 4 * (g + 1 - FRAME_SYM_GROUPS) + decltype(ic)::value>(x);
                });
                sched_fence();
            }
        });
        const uint32_t wd[4] = {xa.dtable[4 * dsc], xa.dtable[4 * dsc + 1], xa.dtable[4 * dsc + 2], xa.dtable[4 * dsc + 3]};
        SymState st;
        sym_init(st);
        const bool dump = DUMP && a.dbg_eq && item_ok && a.item0 + i == 0 && dlane;
        float2 *deq = dump ? a.dbg_eq + 48 * dsym : nullptr;
        auto Hof = [&](float2 Y, auto binc) { return ls_equalise<decltype(binc)::value>(Y); };
        static_for<0, 4>([&](auto rc) {
            constexpr int R = decltype(rc)::value;
            dif_sub16<false, R>(x);
            demap_sub<DUMP, R, 2>(x, wd[R], Hof, deq, st);
            sched_fence();
        });
        if (role >= r0) {
            const int sl = dpq == 2 ? role & 1 : role - 1;
            part_e[quad][sl] = dlane ? finish_evm<2>(st) : 0.f;
            part_b[quad][sl] = dlane ? st.be : 0u;
            part_a[quad][sl] = dlane ? st.ax : 0u;
        }
        if (DUMP && dump && a.dbg_bits) { a.dbg_bits[3 * dsym] = st.d[0]; a.dbg_bits[3 * dsym + 1] = st.d[1]; a.dbg_bits[3 * dsym + 2] = st.d[2]; }
        // an item's quads are in one wave (ipw whole items per wave): its totals need a wave's sync, not the block's
        if constexpr (!DUMP) wave_lds_sync(); else __syncthreads();
        if (item_ok && qi == 0 && role == 0) {
            // the item's totals in symbol order (deterministic), then the trial's metrics
            float fe = 0.f;
            uint32_t ferr = 0u, fax = 0u;
            for (int k = 0; k < qpi; ++k)
                for (int r2 = 0; r2 < dpq; ++r2) {
                    fe += part_e[quad + k][r2]; ferr += part_b[quad + k][r2]; fax += part_a[quad + k][r2];
                }
            const int64_t g = a.item0 + i;
            uint32_t q;
            (void)snr_divmod((uint32_t)a.q0 + (uint32_t)i, (uint32_t)a.n_snr, a.snr_magic, q);
            unsigned long long *sl = acc[q];
            atomicAdd(&sl[0], (unsigned long long)ferr);
            atomicAdd(&sl[1], (unsigned long long)(ferr > 0u));
            atomicAdd(&sl[2], (unsigned long long)fax);
            const float N = 48.0f * (float)n_data;
            atomicAdd(&sl[5], (unsigned long long)(int64_t)__float2ll_rn(fe * (float)OFDM_EVM_Q_SCALE));
            const float db = fe > 0.f ? fmaxf(3.01029995663981195214f * __builtin_amdgcn_logf(fe / N), -400.f) : -400.f;
            atomicAdd(&sl[6], (unsigned long long)(int64_t)__float2ll_rn(db * (float)OFDM_EVM_Q_SCALE));
            float dbp = -INFINITY;
            if (fax > 0u) {
                dbp = 3.01029995663981195214f * __builtin_amdgcn_logf(2.0f * (float)fax / N);
                atomicAdd(&sl[7], (unsigned long long)(int64_t)__float2ll_rn(dbp * (float)OFDM_EVM_Q_SCALE));
                atomicAdd(&sl[4], 1ull);
            }
            if (DUMP && g == 0 && a.dbg_res) { a.dbg_res[0] = db; a.dbg_res[1] = dbp; a.dbg_res[2] = (float)ferr / (96.0f * n_data); }
        }
        if constexpr (!DUMP) wave_lds_sync(); else __syncthreads();
    }
    if constexpr (!DUMP) __syncthreads();     // every wave's counter adds are in before the flush
    for (int k = threadIdx.x; k < a.n_snr * 6; k += SYM_THREADS) {
        const int q = k / 6, s2 = k % 6;
        const int slot = s2 < 3 ? s2 : s2 + 1;           // 0 bit_err, 1 frame_err, 2 axis, 4 finite, 5 pre, 6 dbpre, 7 dbpost
        const unsigned long long v = acc[q][slot];
        if (!v) continue;
        const int c = slot == 0 ? OFDM_C_BIT_ERR : slot == 1 ? OFDM_C_FRAME_ERR : slot == 2 ? OFDM_C_EVM_POST_AXIS
                    : slot == 4 ? OFDM_C_EVMDB_POST_FINITE : slot == 5 ? OFDM_C_EVM_PRE_Q : OFDM_C_EVMDB_PRE_Q;
        atomicAdd(&a.counters[q * OFDM_NCOUNTERS + c], v);
    }
    for (int q = threadIdx.x; q < a.n_snr; q += SYM_THREADS)
        if (acc[q][7]) atomicAdd(&a.counters[q * OFDM_NCOUNTERS + OFDM_C_EVMDB_POST_Q], acc[q][7]);
    if (blockIdx.x == 0 && a.add_totals) {
        for (int q = threadIdx.x; q < a.n_snr; q += SYM_THREADS) {
            unsigned long long *c = a.counters + q * OFDM_NCOUNTERS;
            const unsigned long long nt = (unsigned long long)a.n_trials, nd = (unsigned long long)a.n_data;
            atomicAdd(&c[OFDM_C_FRAMES], nt);
            atomicAdd(&c[OFDM_C_SYMBOLS], nd * nt);
            atomicAdd(&c[OFDM_C_BITS], 96ull * nd * nt);
            atomicAdd(&c[OFDM_C_EVM_TERMS], 48ull * nd * nt);
        }
    }
}

// launchers and occupancy handles
const void *frame_ring_xl_kernel_ptr() { return reinterpret_cast<const void *>(&frame_ring_xl_kernel); }
const void *frame_whole_xl_kernel_ptr() { return reinterpret_cast<const void *>(&frame_whole_xl_kernel); }
void launch_frame_ring_xl(hipStream_t st, const XlArgs &a, dim3 grid, size_t lds) {
    hipLaunchKernelGGL(frame_ring_xl_kernel, grid, dim3(64 * XL_RING_W), lds, st, a);
}
void launch_frame_whole_xl(hipStream_t st, const XlArgs &a, dim3 grid, size_t lds) {
    hipLaunchKernelGGL(frame_whole_xl_kernel, grid, dim3(64), lds, st, a);
}
void launch_frame_sym_xl(hipStream_t st, const XlArgs &a, int cus) {
    const int ipb = a.f.ipb;
    const bool dump = a.f.dbg_eq || a.f.dbg_bits || a.f.dbg_res;
    const void *k = dump ? reinterpret_cast<const void *>(&frame_sym_xl_kernel<true>)
                         : reinterpret_cast<const void *>(&frame_sym_xl_kernel<false>);
    const dim3 grid(occupancy_grid(k, SYM_THREADS, 0, cus, (a.f.n_items + ipb - 1) / ipb));
    if (dump) hipLaunchKernelGGL((frame_sym_xl_kernel<true>), grid, dim3(SYM_THREADS), 0, st, a);
    else hipLaunchKernelGGL((frame_sym_xl_kernel<false>), grid, dim3(SYM_THREADS), 0, st, a);
}

}  // namespace ofdm
