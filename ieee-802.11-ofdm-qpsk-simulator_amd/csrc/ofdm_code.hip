// ofdm_code.hip -- the coded link (include/ofdm_mi355x_code.h: ofdm_code_encode, ofdm_stream_csi, ofdm_code_decode).
// A translation unit of its own, a layer over what the library already exchanges: payload words in, equalised
// subcarriers out.  No other translation unit changes.
//
//   code_encode_kernel : one thread per output word.  The thread takes the 54 information bits its data symbol's 48
//     steps see (u_48d-6 .. u_48d+47, from at most three input words) into one 64-bit register, MSB first, forms all 48
//     A_t and all 48 B_t by five shifts and XORs each -- no serial chain -- and picks its 32 interleaved, precoded
//     bits out of them.
//   stream_csi_kernel : one wave per packet, CSI_WAVES waves per block, looping over d_count as the decode kernels.
//     Per branch: ofdm_stream_decode.h's staging over [p + 364, p + 638], the span the matched filter reads for the
//     frame instants 192 .. 319, the filter in the decode's tap order, rxc_rot by fc + ff read from the record, then
//     one bin per lane of the 64-point transform of LTF1 + LTF2: 64 steps of a broadcast LDS read against a 64-entry
//     twiddle table.  The lane adds |S|^2 / 4 over the branches; lanes 0 .. 47 fetch their data bin's and store.
//   code_decode_kernel : one wave per row, CDEC_WAVES waves per block, lane = trellis state; see the layout there.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_code.h"
#include "ofdm_stream_decode.h"
#include "twiddle64.h"

namespace ofdm {

static_assert(OFDM_K_CODE_ENCODE == Ctx::K_CODE_ENCODE && OFDM_K_STREAM_CSI == Ctx::K_STREAM_CSI &&
              OFDM_K_CODE_DECODE == Ctx::K_CODE_DECODE && Ctx::K_CODE_DECODE < Ctx::NK, "the code kernels' ids are the context's");
static_assert(OFDM_CODE_MAX_DATA_SYMBOLS == RXC_MAX_DATA, "a coded packet is a packet of the stream receiver");

constexpr int CODE_TAIL = OFDM_CODE_TAIL_BITS;
constexpr int CENC_THREADS = 256;
constexpr int CSI_WAVES = 4;
constexpr int CSI_BLOCKS_PER_CU = 8;                         // the grid's cap: the waves loop past it
constexpr int CSI_FIRST = 192, CSI_SPAN = 128;               // the frame instants that are filtered: the two long training symbols
constexpr int CSI_LEN = 2 * CSI_SPAN + 19;                   // staged samples: [p + 2 CSI_FIRST - 20, p + 2 (CSI_FIRST + CSI_SPAN - 1)]
constexpr int CSI_PLANE = (CSI_LEN + 3) & ~3;
constexpr int CDEC_WAVES = 4;                                // 45 KiB of LDS per block at D = 15: three blocks per CU
constexpr int CDEC_ROWS_PER_WAVE = 2;                        // the grid gives every wave two rows where there are that many
constexpr int CDEC_BLOCKS_PER_CU = 8;
constexpr float CODE_CLAMP = 0x1p100f;

// position j of a data symbol holds coded bit k = 16 (j mod 6) + j / 6 (the inverse of j = 6 (k mod 16) + k / 16)
__host__ __device__ constexpr int code_deinterleave(int j) { return 16 * (j % 6) + j / 6; }

// ---- encoder ----
struct EncArgs {
    const uint32_t *info;    // [n][wi]
    uint32_t *words;         // [n][3 nd]
    int64_t total;           // n 3 nd output words
    int32_t nd, wi;
    uint32_t last_mask;      // the information bits of a packet's last word
};

__global__ __launch_bounds__(CENC_THREADS) void code_encode_kernel(EncArgs a) {
    const int wpp = 3 * a.nd;
    for (int64_t o = (int64_t)blockIdx.x * CENC_THREADS + threadIdx.x; o < a.total; o += (int64_t)gridDim.x * CENC_THREADS) {
        const int64_t i = o / wpp;
        const int w = (int)(o - i * wpp), d = w / 3, part = w - 3 * d;
        const uint32_t *row = a.info + i * a.wi;
        // word q of the row, zero outside it, the last word without its unused bits (the tail is zero whatever they hold)
        auto word = [&](int q) -> uint32_t {
            if (q < 0 || q >= a.wi) return 0u;
            const uint32_t v = row[q];
            return q == a.wi - 1 ? v & a.last_mask : v;
        };
        // X: u_t0+i at bit 63 - i, t0 = 48 d - 6, i = 0 .. 53
        const int t0 = 48 * d - CODE_TAIL, q0 = (t0 + 32) / 32 - 1, sh = t0 - 32 * q0;       // floor division for t0 = -6
        const uint64_t hi = ((uint64_t)word(q0) << 32) | word(q0 + 1);
        const uint64_t X = sh ? (hi << sh) | ((uint64_t)word(q0 + 2) >> (32 - sh)) : hi;
        // step tau of the symbol sits at i = tau + 6: (X >> s) brings u_t-s there
        const uint64_t A = X ^ (X >> 2) ^ (X >> 3) ^ (X >> 5) ^ (X >> 6);
        const uint64_t B = X ^ (X >> 1) ^ (X >> 2) ^ (X >> 3) ^ (X >> 6);
        auto coded = [&](int k) -> uint32_t { return (uint32_t)(((k & 1) ? B : A) >> (57 - (k >> 1))) & 1u; };
        uint32_t out = 0u;
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const int j = 32 * part + 2 * mm;
            const uint32_t g0 = coded(code_deinterleave(j)), g1 = coded(code_deinterleave(j + 1));
            out |= ((g0 << 1) | (g0 ^ g1)) << (30 - 2 * mm);
        }
        a.words[o] = out;
    }
}

// ---- gains ----
struct CsiBranches {
    const float2 *x[OFDM_DIVERSITY_MAX_BRANCHES];
    int32_t nb;
};
struct CsiArgs {
    CsiBranches br;
    int64_t n, max_packets;
    const int64_t *count;
    const ofdm_stream_packet *pk;
    float *csi;              // [max_packets][48]
    float taps[21];
};

__global__ __launch_bounds__(64 * CSI_WAVES) void stream_csi_kernel(CsiArgs a) {
    __shared__ __attribute__((aligned(16))) float planes[CSI_WAVES][2][CSI_PLANE];
    __shared__ float frames[CSI_WAVES][2][CSI_SPAN];
    __shared__ float2 tw[64];                                         // exp(-2 pi j k / 64)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (threadIdx.x < 64) tw[threadIdx.x] = make_float2(kCos64[threadIdx.x], -kSin64[threadIdx.x]);
    __syncthreads();
    float *re = planes[wave][0], *im = planes[wave][1], *fre = frames[wave][0], *fim = frames[wave][1];
    const int64_t cnt = std::min<int64_t>(a.count[1], a.max_packets);
    for (int64_t i = (int64_t)blockIdx.x * CSI_WAVES + wave; i < cnt; i += (int64_t)gridDim.x * CSI_WAVES) {
        const ofdm_stream_packet *pkt = a.pk + i;
        int64_t p;
        int last_front;
        sdec_packet(pkt, p, last_front);
        const double f_ts = ((double)pkt->r.cfo_coarse_hz + (double)pkt->r.cfo_fine_hz) * RXC_TS;
        float g = 0.f;
#pragma unroll 1
        for (int b = 0; b < a.br.nb; ++b) {
            const float2 *x = a.br.x[b];
            const int q = (int)((reinterpret_cast<uintptr_t>(x) >> 3) & 1u);
            // plane index m is stream sample p + 2 CSI_FIRST - 20 + m
            sdec_stage(x, a.n, p + 2 * CSI_FIRST, q, CSI_LEN, lane, re, im);
            rxc_wave_sync();
            // frame instant CSI_FIRST + ii: sdec_filter's sum, tap for tap
#pragma unroll
            for (int r = 0; r < CSI_SPAN / 64; ++r) {
                const int ii = lane + 64 * r, n = 20 + 2 * ii;
                float vx = 0.f, vy = 0.f;
#pragma unroll
                for (int tt = 0; tt < 21; ++tt) {
                    vx = fmaf(re[n - tt], a.taps[tt], vx);
                    vy = fmaf(im[n - tt], a.taps[tt], vy);
                }
                fre[ii] = vx;
                fim[ii] = vy;
            }
            rxc_wave_sync();
            // rxc_rotate's first step: the rotated pair's sum over LTF1
            {
                const int k = CSI_FIRST + lane;
                const float2 u = rxc_rot(make_float2(fre[lane], fim[lane]), f_ts, k);
                const float2 w = rxc_rot(make_float2(fre[lane + 64], fim[lane + 64]), f_ts, k + 64);
                rxc_wave_sync();
                fre[lane] = u.x + w.x;
                fim[lane] = u.y + w.y;
            }
            rxc_wave_sync();
            // fft() = DFT(x (-1)^n): bin `lane` is sum_n s[n] exp(-2 pi j n (lane + 32) / 64)
            float sx = 0.f, sy = 0.f;
            const int step = (lane + 32) & 63;
#pragma unroll 8
            for (int n = 0; n < 64; ++n) {
                const float2 t = tw[(n * step) & 63];
                const float vx = fre[n], vy = fim[n];
                sx = fmaf(vx, t.x, sx); sx = fmaf(-vy, t.y, sx);
                sy = fmaf(vx, t.y, sy); sy = fmaf(vy, t.x, sy);
            }
            g += 0.25f * fmaf(sx, sx, sy * sy);                       // |H|^2 = |L S / 2|^2 on the used bins
            rxc_wave_sync();                                           // the next branch overwrites the planes and the frame
        }
        const float out = __shfl(g, data_bin(lane < 48 ? lane : 0), 64);
        if (lane < 48) a.csi[i * 48 + lane] = out;
    }
}

// ---- decoder ----
// One wave per row, lane = new state s' = u_t << 5 | s >> 1; its predecessors are the lanes p0 = (2 s') & 63 and
// p0 | 1.  The wave's LDS region: 48 D decision words of 64 bits (step t: bit s' set where p1 won), then the 96 D soft
// values in trellis order.  Per step: one 8-byte broadcast LDS read of the step's two soft values, two cross-lane reads
// of the predecessors' metrics (ds_bpermute, registers only), the sign flips (two XORs with the lane's constant sign
// masks; the complements ride on the additions' negate modifiers), four additions, one compare whose 64-bit result is
// the ballot, one select and lane 0's 8-byte LDS write of the decision word: 9 vector instructions for every lane, 3
// for lane 0's write, and 4 LDS instructions.
// Traceback: 64 decision words at a time, one per lane, and a wave-uniform walk that reads them with v_readlane.
struct CdecArgs {
    const float2 *eq;        // [n][48 nd]
    const float *csi;        // optional, [n][48]
    const int64_t *count;    // optional: [1] rows at most
    uint32_t *info;          // [n][wi]
    float *path;             // optional, [n]
    int64_t n;
    int32_t nd, wi;
};

constexpr size_t cdec_wave_bytes(int nd) { return (size_t)48 * nd * sizeof(unsigned long long) + (size_t)96 * nd * sizeof(float); }

__device__ __forceinline__ float code_flip(float v, uint32_t sign) { return __uint_as_float(__float_as_uint(v) ^ sign); }

__global__ __launch_bounds__(64 * CDEC_WAVES) void code_decode_kernel(CdecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long cdec_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nd = a.nd, steps = 48 * nd, nsoft = 96 * nd, kinfo = steps - CODE_TAIL;
    unsigned long long *dw = cdec_smem + (size_t)wave * (48 * nd + 48 * nd);       // 768 D bytes per wave: 96 D words of 8
    float *soft = reinterpret_cast<float *>(dw + steps);
    // the lane's constants: its predecessors and the coded bits (A, B) of the branch p0 -> lane as sign masks; the
    // branch p1 -> lane carries their complements (both generators tap u_t-6)
    const int p0 = (2 * lane) & 63, p1 = p0 | 1;
    const uint32_t a0 = ((lane >> 5) ^ (lane >> 3) ^ (lane >> 2) ^ lane) & 1u;
    const uint32_t b0 = ((lane >> 5) ^ (lane >> 4) ^ (lane >> 3) ^ (lane >> 2)) & 1u;
    const uint32_t sa0 = a0 << 31, sb0 = b0 << 31, sa1 = sa0 ^ 0x80000000u, sb1 = sb0 ^ 0x80000000u;
    int64_t rows = a.n;
    if (a.count) rows = std::min<int64_t>(rows, a.count[1]);
    for (int64_t i = (int64_t)blockIdx.x * CDEC_WAVES + wave; i < rows; i += (int64_t)gridDim.x * CDEC_WAVES) {
        // ---- the soft values, into trellis order ----
        const float2 *zrow = a.eq + i * (48 * nd);
        for (int e0 = 0; e0 < nsoft; e0 += 64) {
            const int e = e0 + lane;
            if (e < nsoft) {
                const int d = e / 96, j = e - 96 * d, m = j >> 1;
                const float2 z = zrow[48 * d + m];
                const float w = a.csi ? a.csi[i * 48 + m] : 1.0f;
                float lam = w * ((j & 1) ? z.x : z.y);
                if (!(fabsf(lam) < INFINITY)) lam = 0.f;
                lam = fminf(fmaxf(lam, -CODE_CLAMP), CODE_CLAMP);
                soft[96 * d + code_deinterleave(j)] = lam;
            }
        }
        rxc_wave_sync();
        // ---- add, compare, select ----
        float M = lane == 0 ? 0.f : -INFINITY;
        for (int t = 0; t < steps; ++t) {
            const float2 l = reinterpret_cast<const float2 *>(soft)[t];
            const float m0 = __shfl(M, p0, 64), m1 = __shfl(M, p1, 64);
            const float c0 = m0 + (code_flip(l.x, sa0) + code_flip(l.y, sb0));
            const float c1 = m1 + (code_flip(l.x, sa1) + code_flip(l.y, sb1));
            const bool win = c1 > c0;
            M = win ? c1 : c0;
            const unsigned long long word = __ballot(win);
            if (lane == 0) dw[t] = word;
        }
        if (a.path && lane == 0) a.path[i] = M;
        rxc_wave_sync();
        // ---- traceback from state 0: step t's input is bit 5 of the state it leads to ----
        int s = 0;
        uint32_t cur = 0u, mine = 0u;
        for (int c0 = (steps - 1) & ~63; c0 >= 0; c0 -= 64) {
            const int t = c0 + lane;
            const unsigned long long wv = t < steps ? dw[t] : 0ull;
            const int lo = (int)(uint32_t)wv, hi = (int)(uint32_t)(wv >> 32);
            for (int tl = std::min(63, steps - 1 - c0); tl >= 0; --tl) {
                const int tt = c0 + tl;
                const uint32_t half = (uint32_t)((s & 32) ? __builtin_amdgcn_readlane(hi, tl) : __builtin_amdgcn_readlane(lo, tl));
                if (tt < kinfo) {
                    cur |= (uint32_t)(s >> 5) << (31 - (tt & 31));
                    if ((tt & 31) == 0) {
                        if (lane == (tt >> 5)) mine = cur;
                        cur = 0u;
                    }
                }
                s = ((2 * s) & 63) | (int)((half >> (s & 31)) & 1u);
            }
        }
        if (lane < a.wi) a.info[i * a.wi + lane] = mine;
        rxc_wave_sync();                                               // the next row overwrites the wave's region
    }
}

// a device pointer aligned to `align` bytes (a power of two)
static bool code_aligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0; }

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_code_encode(ofdm_ctx *ctx, int32_t n_data, const void *d_info, int64_t n, void *d_words) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n_data < 1 || n_data > OFDM_CODE_MAX_DATA_SYMBOLS)
        return set_error(OFDM_E_ARG, "n_data must be in [1, %d], got %d", OFDM_CODE_MAX_DATA_SYMBOLS, (int)n_data);
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_info) return set_error(OFDM_E_ARG, "d_info is NULL");
    if (!d_words) return set_error(OFDM_E_ARG, "d_words is NULL");
    if (!code_aligned(d_info, 4)) return set_error(OFDM_E_ARG, "d_info must be 4-byte aligned");
    if (!code_aligned(d_words, 4)) return set_error(OFDM_E_ARG, "d_words must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    EncArgs a{};
    a.info = (const uint32_t *)d_info;
    a.words = (uint32_t *)d_words;
    a.nd = n_data;
    a.wi = OFDM_CODE_INFO_WORDS(n_data);
    a.total = n * 3 * n_data;
    const int valid = OFDM_CODE_INFO_BITS(n_data) - 32 * (a.wi - 1);          // 1 .. 32
    a.last_mask = valid == 32 ? 0xffffffffu : ~0u << (32 - valid);
    const int64_t blocks = (a.total + CENC_THREADS - 1) / CENC_THREADS;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 64 * (int64_t)c->cus));
    c->tic(OFDM_K_CODE_ENCODE);
    hipLaunchKernelGGL(code_encode_kernel, grid, dim3(CENC_THREADS), 0, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "code_encode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_stream_csi(ofdm_ctx *ctx, const void *const *d_branches, int32_t n_branches, int64_t n_samples,
                               const void *d_packets, const void *d_count, int64_t max_packets, void *d_csi) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n_branches < 1 || n_branches > OFDM_DIVERSITY_MAX_BRANCHES)
        return set_error(OFDM_E_ARG, "n_branches must be in [1, %d], got %d", OFDM_DIVERSITY_MAX_BRANCHES, (int)n_branches);
    if (n_samples < 0) return set_error(OFDM_E_ARG, "n_samples %lld is negative", (long long)n_samples);
    if (max_packets < 0) return set_error(OFDM_E_ARG, "max_packets %lld is negative", (long long)max_packets);
    if (!d_branches) return set_error(OFDM_E_ARG, "d_branches is NULL");
    if (n_samples > 0)
        for (int b = 0; b < n_branches; ++b) {
            if (!d_branches[b]) return set_error(OFDM_E_ARG, "d_branches[%d] is NULL", b);
            if (!code_aligned(d_branches[b], 8)) return set_error(OFDM_E_ARG, "d_branches[%d] must be 8-byte aligned", b);
        }
    if (!d_count) return set_error(OFDM_E_ARG, "d_count is NULL");
    if (!code_aligned(d_count, 8)) return set_error(OFDM_E_ARG, "d_count must be 8-byte aligned");
    if (max_packets > 0) {
        if (!d_packets) return set_error(OFDM_E_ARG, "d_packets is NULL");
        if (!d_csi) return set_error(OFDM_E_ARG, "d_csi is NULL");
    }
    if (!code_aligned(d_packets, 8)) return set_error(OFDM_E_ARG, "d_packets must be 8-byte aligned");
    if (!code_aligned(d_csi, 4)) return set_error(OFDM_E_ARG, "d_csi must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (max_packets == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    CsiArgs a{};
    a.br.nb = n_branches;
    for (int b = 0; b < n_branches; ++b) a.br.x[b] = (const float2 *)d_branches[b];
    a.n = n_samples;
    a.max_packets = max_packets;
    a.count = (const int64_t *)d_count;
    a.pk = (const ofdm_stream_packet *)d_packets;
    a.csi = (float *)d_csi;
    rrc_design(a.taps);
    const int64_t blocks = (max_packets + CSI_WAVES - 1) / CSI_WAVES;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, CSI_BLOCKS_PER_CU * (int64_t)c->cus));
    c->tic(OFDM_K_STREAM_CSI);
    hipLaunchKernelGGL(stream_csi_kernel, grid, dim3(64 * CSI_WAVES), 0, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "stream_csi_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_code_decode(ofdm_ctx *ctx, int32_t n_data, const void *d_eq, const void *d_csi, const void *d_count,
                                int64_t n, void *d_info, void *d_path) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (n_data < 1 || n_data > OFDM_CODE_MAX_DATA_SYMBOLS)
        return set_error(OFDM_E_ARG, "n_data must be in [1, %d], got %d", OFDM_CODE_MAX_DATA_SYMBOLS, (int)n_data);
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_eq) return set_error(OFDM_E_ARG, "d_eq is NULL");
    if (!d_info) return set_error(OFDM_E_ARG, "d_info is NULL");
    if (!code_aligned(d_eq, 8)) return set_error(OFDM_E_ARG, "d_eq must be 8-byte aligned");
    if (!code_aligned(d_csi, 4)) return set_error(OFDM_E_ARG, "d_csi must be 4-byte aligned");
    if (!code_aligned(d_count, 8)) return set_error(OFDM_E_ARG, "d_count must be 8-byte aligned");
    if (!code_aligned(d_info, 4)) return set_error(OFDM_E_ARG, "d_info must be 4-byte aligned");
    if (!code_aligned(d_path, 4)) return set_error(OFDM_E_ARG, "d_path must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    CdecArgs a{};
    a.eq = (const float2 *)d_eq;
    a.csi = (const float *)d_csi;
    a.count = (const int64_t *)d_count;
    a.info = (uint32_t *)d_info;
    a.path = (float *)d_path;
    a.n = n;
    a.nd = n_data;
    a.wi = OFDM_CODE_INFO_WORDS(n_data);
    const size_t lds = CDEC_WAVES * cdec_wave_bytes(n_data);
    // every wave two rows where there are that many, at most CDEC_BLOCKS_PER_CU blocks per CU; the waves loop over the rows
    const int64_t blocks = (n + CDEC_WAVES * CDEC_ROWS_PER_WAVE - 1) / (CDEC_WAVES * CDEC_ROWS_PER_WAVE);
    const dim3 grid((unsigned)std::min<int64_t>(blocks, CDEC_BLOCKS_PER_CU * (int64_t)c->cus));
    c->tic(OFDM_K_CODE_DECODE);
    hipLaunchKernelGGL(code_decode_kernel, grid, dim3(64 * CDEC_WAVES), lds, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "code_decode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
