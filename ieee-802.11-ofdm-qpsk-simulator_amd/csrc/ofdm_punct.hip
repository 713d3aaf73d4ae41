// ofdm_punct.hip -- the punctured rates of the coded link (include/ofdm_mi355x_punct.h: ofdm_punct_encode,
// ofdm_punct_decode).  A translation unit of its own over ofdm_mi355x_code.h's rules; ofdm_code.hip and every other
// translation unit stay as they are.
//
//   punct_encode_kernel : one thread per output word.  The thread takes the S + 6 (54, 70 or 78) information bits its data
//     symbol's S steps see (u_Sd-6 .. u_Sd+S-1, from at most four input words) into a 128-bit pair of registers, MSB
//     first, forms all A_t and all B_t by five shifts and XORs each -- no serial chain -- and picks its 32 interleaved,
//     precoded bits out of the ones the rate sends.
//   punct_decode_kernel : one wave per row, PDEC_WAVES waves per block, lane = trellis state; code_decode_kernel's layout
//     with S D decision words and the 96 D sent soft values in sent order; see there.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_punct.h"
#include "ofdm_stream_decode.h"

namespace ofdm {

static_assert(OFDM_K_CODE_ENCODE == Ctx::K_CODE_ENCODE && OFDM_K_CODE_DECODE == Ctx::K_CODE_DECODE,
              "the punctured kernels are timed under the coded link's encoder and decoder ids");
static_assert(OFDM_PUNCT_TAIL_BITS == OFDM_CODE_TAIL_BITS && OFDM_PUNCT_STEPS(OFDM_PUNCT_RATE_1_2) == 48 &&
              OFDM_PUNCT_INFO_BITS(2, 0) == OFDM_CODE_INFO_BITS(2) && OFDM_PUNCT_INFO_WORDS(15, 0) == OFDM_CODE_INFO_WORDS(15),
              "rate code 0 is the coded link's packet");
static_assert(OFDM_PUNCT_STEPS(1) * 3 == 96 * 2 && OFDM_PUNCT_STEPS(2) * 4 == 96 * 3, "96 sent bits per data symbol");
static_assert(OFDM_PUNCT_INFO_WORDS(OFDM_CODE_MAX_DATA_SYMBOLS, OFDM_PUNCT_RATE_3_4) <= 64, "one lane per information word");

constexpr int PUNCT_TAIL = OFDM_PUNCT_TAIL_BITS;
constexpr int PENC_THREADS = 256;
constexpr int PDEC_WAVES = 2;                                // 28,800 B of LDS per block at rate 3/4, D = 15: five blocks per CU
constexpr int PDEC_ROWS_PER_WAVE = 2;                        // the grid gives every wave two rows where there are that many
constexpr int PDEC_BLOCKS_PER_CU = 16;                       // the grid's cap: the waves loop past it
constexpr float PUNCT_CLAMP = 0x1p100f;

// position j of a data symbol holds sent bit k = 16 (j mod 6) + j / 6 (the inverse of j = 6 (k mod 16) + k / 16)
__host__ __device__ constexpr int punct_deinterleave(int j) { return 16 * (j % 6) + j / 6; }
__host__ __device__ constexpr int punct_steps(int rate) { return OFDM_PUNCT_STEPS(rate); }

// ---- encoder ----
struct PencArgs {
    const uint32_t *info;    // [n][wi]
    uint32_t *words;         // [n][3 nd]
    int64_t total;           // n 3 nd output words
    int32_t nd, wi, rate;
    uint32_t last_mask;      // the information bits of a packet's last word
};

struct Bits128 {
    uint64_t hi, lo;         // bit i of the sequence at bit 63 - i of hi (i < 64) or 127 - i of lo
};
__device__ __forceinline__ Bits128 punct_shr(Bits128 x, int s) { return {x.hi >> s, (x.lo >> s) | (x.hi << (64 - s))}; }   // 0 < s < 64
__device__ __forceinline__ Bits128 operator^(Bits128 a, Bits128 b) { return {a.hi ^ b.hi, a.lo ^ b.lo}; }
__device__ __forceinline__ uint32_t punct_bit(Bits128 x, int i) {
    return (uint32_t)(i < 64 ? x.hi >> (63 - i) : x.lo >> (127 - i)) & 1u;
}

__global__ __launch_bounds__(PENC_THREADS) void punct_encode_kernel(PencArgs a) {
    const int wpp = 3 * a.nd, rate = a.rate, S = punct_steps(rate);
    for (int64_t o = (int64_t)blockIdx.x * PENC_THREADS + threadIdx.x; o < a.total; o += (int64_t)gridDim.x * PENC_THREADS) {
        const int64_t i = o / wpp;
        const int w = (int)(o - i * wpp), d = w / 3, part = w - 3 * d;
        const uint32_t *row = a.info + i * a.wi;
        // word q of the row, zero outside it, the last word without its unused bits (the tail is zero whatever they hold)
        auto word = [&](int q) -> uint32_t {
            if (q < 0 || q >= a.wi) return 0u;
            const uint32_t v = row[q];
            return q == a.wi - 1 ? v & a.last_mask : v;
        };
        // X: u_t0+i at sequence bit i, t0 = S d - 6, i = 0 .. S + 5 <= 77; sh + 78 <= 109 bits of the four words
        const int t0 = S * d - PUNCT_TAIL, q0 = (t0 + 32) / 32 - 1, sh = t0 - 32 * q0;       // floor division for t0 = -6
        const uint64_t hi = ((uint64_t)word(q0) << 32) | word(q0 + 1), lo = ((uint64_t)word(q0 + 2) << 32) | word(q0 + 3);
        const Bits128 X = sh ? Bits128{(hi << sh) | (lo >> (64 - sh)), lo << sh} : Bits128{hi, lo};
        // step tau of the symbol sits at i = tau + 6: punct_shr(X, s) brings u_t-s there
        const Bits128 X2 = punct_shr(X, 2), X3 = punct_shr(X, 3), X6 = punct_shr(X, 6);
        const Bits128 A = X ^ X2 ^ X3 ^ punct_shr(X, 5) ^ X6;
        const Bits128 B = X ^ punct_shr(X, 1) ^ X2 ^ X3 ^ X6;
        // sent bit k of the symbol: rate 1/2 A_p B_p; 2/3 A_2p B_2p A_2p+1; 3/4 A_3p B_3p A_3p+1 B_3p+2
        auto coded = [&](int k) -> uint32_t {
            int tau, b;
            if (rate == OFDM_PUNCT_RATE_1_2) {
                tau = k >> 1, b = k & 1;
            } else if (rate == OFDM_PUNCT_RATE_2_3) {
                const int p = k / 3, r = k - 3 * p;
                tau = 2 * p + (r == 2), b = r == 1;
            } else {
                const int p = k >> 2, r = k & 3;
                tau = 3 * p + (r == 2) + 2 * (r == 3), b = r & 1;
            }
            return punct_bit(b ? B : A, tau + PUNCT_TAIL);
        };
        uint32_t out = 0u;
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const int j = 32 * part + 2 * mm;
            const uint32_t g0 = coded(punct_deinterleave(j)), g1 = coded(punct_deinterleave(j + 1));
            out |= ((g0 << 1) | (g0 ^ g1)) << (30 - 2 * mm);
        }
        a.words[o] = out;
    }
}

// ---- decoder ----
// code_decode_kernel's wave: lane = new state s' = u_t << 5 | s >> 1 with the predecessors p0 = (2 s') & 63 and p0 | 1,
// per step two ds_bpermute reads of their metrics, the sign flips, the additions, one compare whose 64-bit result is the
// ballot, one select and lane 0's 8-byte LDS write of the decision word.  The wave's LDS region: S D decision words of 64
// bits, then the 96 D soft values in sent order -- the staging is code_decode_kernel's, since a symbol's sent bit k sits
// where its coded bit k sat.  The steps run in periods of the puncturing pattern: one step at rate 1/2 (an 8-byte read),
// two at 2/3 (three values) and three at 3/4 (a 16-byte read); a stolen value is the constant +0.0f, whose addition
// the compiler folds: no metric is ever -0.0f, so a candidate is the same with and without it (the header's decoder rule).
// Traceback: code_decode_kernel's, over S D steps.
struct PdecArgs {
    const float2 *eq;        // [n][48 nd]
    const float *csi;        // optional, [n][48]
    const int64_t *count;    // optional: [1] rows at most
    uint32_t *info;          // [n][wi]
    float *path;             // optional, [n]
    int64_t n;
    int32_t nd, wi, rate;
};

constexpr size_t pdec_wave_bytes(int nd, int rate) {
    return (size_t)punct_steps(rate) * nd * sizeof(unsigned long long) + (size_t)96 * nd * sizeof(float);
}

__device__ __forceinline__ float punct_flip(float v, uint32_t sign) { return __uint_as_float(__float_as_uint(v) ^ sign); }

__global__ __launch_bounds__(64 * PDEC_WAVES) void punct_decode_kernel(PdecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long pdec_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nd = a.nd, rate = a.rate, steps = punct_steps(rate) * nd, nsoft = 96 * nd, kinfo = steps - PUNCT_TAIL;
    unsigned long long *dw = pdec_smem + (size_t)wave * (steps + 48 * nd);         // (8 S + 384) D bytes per wave, a multiple of 16
    float *soft = reinterpret_cast<float *>(dw + steps);
    // the lane's constants: its predecessors and the coded bits (A, B) of the branch p0 -> lane as sign masks; the
    // branch p1 -> lane carries their complements (both generators tap u_t-6)
    const int p0 = (2 * lane) & 63, p1 = p0 | 1;
    const uint32_t a0 = ((lane >> 5) ^ (lane >> 3) ^ (lane >> 2) ^ lane) & 1u;
    const uint32_t b0 = ((lane >> 5) ^ (lane >> 4) ^ (lane >> 3) ^ (lane >> 2)) & 1u;
    const uint32_t sa0 = a0 << 31, sb0 = b0 << 31, sa1 = sa0 ^ 0x80000000u, sb1 = sb0 ^ 0x80000000u;
    int64_t rows = a.n;
    if (a.count) rows = std::min<int64_t>(rows, a.count[1]);
    for (int64_t i = (int64_t)blockIdx.x * PDEC_WAVES + wave; i < rows; i += (int64_t)gridDim.x * PDEC_WAVES) {
        // ---- the soft values, into sent order ----
        const float2 *zrow = a.eq + i * (48 * nd);
        for (int e0 = 0; e0 < nsoft; e0 += 64) {
            const int e = e0 + lane;
            if (e < nsoft) {
                const int d = e / 96, j = e - 96 * d, m = j >> 1;
                const float2 z = zrow[48 * d + m];
                const float w = a.csi ? a.csi[i * 48 + m] : 1.0f;
                float lam = w * ((j & 1) ? z.x : z.y);
                if (!(fabsf(lam) < INFINITY)) lam = 0.f;
                lam = fminf(fmaxf(lam, -PUNCT_CLAMP), PUNCT_CLAMP);
                soft[96 * d + punct_deinterleave(j)] = lam;
            }
        }
        rxc_wave_sync();
        // ---- add, compare, select ----
        float M = lane == 0 ? 0.f : -INFINITY;
        auto acs = [&](float lx, float ly, int t) {
            const float m0 = __shfl(M, p0, 64), m1 = __shfl(M, p1, 64);
            const float c0 = m0 + (punct_flip(lx, sa0) + punct_flip(ly, sb0));
            const float c1 = m1 + (punct_flip(lx, sa1) + punct_flip(ly, sb1));
            const bool win = c1 > c0;
            M = win ? c1 : c0;
            const unsigned long long word = __ballot(win);
            if (lane == 0) dw[t] = word;
        };
        // a stolen value alone: the inner sum is the kept value's flip
        auto acs1 = [&](float l, uint32_t s0, uint32_t s1, int t) {
            const float m0 = __shfl(M, p0, 64), m1 = __shfl(M, p1, 64);
            const float c0 = m0 + punct_flip(l, s0);
            const float c1 = m1 + punct_flip(l, s1);
            const bool win = c1 > c0;
            M = win ? c1 : c0;
            const unsigned long long word = __ballot(win);
            if (lane == 0) dw[t] = word;
        };
        if (rate == OFDM_PUNCT_RATE_1_2) {
            for (int t = 0; t < steps; ++t) {
                const float2 l = reinterpret_cast<const float2 *>(soft)[t];
                acs(l.x, l.y, t);
            }
        } else if (rate == OFDM_PUNCT_RATE_2_3) {
            for (int q = 0; 2 * q < steps; ++q) {                       // A_2q B_2q A_2q+1
                const float l0 = soft[3 * q], l1 = soft[3 * q + 1], l2 = soft[3 * q + 2];
                acs(l0, l1, 2 * q);
                acs1(l2, sa0, sa1, 2 * q + 1);
            }
        } else {
            for (int q = 0; 3 * q < steps; ++q) {                       // A_3q B_3q A_3q+1 B_3q+2
                const float4 l = reinterpret_cast<const float4 *>(soft)[q];
                acs(l.x, l.y, 3 * q);
                acs1(l.z, sa0, sa1, 3 * q + 1);
                acs1(l.w, sb0, sb1, 3 * q + 2);
            }
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
static bool punct_aligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0; }

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_punct_encode(ofdm_ctx *ctx, int32_t rate, int32_t n_data, const void *d_info, int64_t n, void *d_words) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (rate < 0 || rate >= OFDM_PUNCT_RATES)
        return set_error(OFDM_E_ARG, "rate must be 0 (1/2), 1 (2/3) or 2 (3/4), got %d", (int)rate);
    if (n_data < 1 || n_data > OFDM_CODE_MAX_DATA_SYMBOLS)
        return set_error(OFDM_E_ARG, "n_data must be in [1, %d], got %d", OFDM_CODE_MAX_DATA_SYMBOLS, (int)n_data);
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_info) return set_error(OFDM_E_ARG, "d_info is NULL");
    if (!d_words) return set_error(OFDM_E_ARG, "d_words is NULL");
    if (!punct_aligned(d_info, 4)) return set_error(OFDM_E_ARG, "d_info must be 4-byte aligned");
    if (!punct_aligned(d_words, 4)) return set_error(OFDM_E_ARG, "d_words must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    PencArgs a{};
    a.info = (const uint32_t *)d_info;
    a.words = (uint32_t *)d_words;
    a.nd = n_data;
    a.rate = rate;
    a.wi = OFDM_PUNCT_INFO_WORDS(n_data, rate);
    a.total = n * 3 * n_data;
    const int valid = OFDM_PUNCT_INFO_BITS(n_data, rate) - 32 * (a.wi - 1);   // 1 .. 32
    a.last_mask = valid == 32 ? 0xffffffffu : ~0u << (32 - valid);
    const int64_t blocks = (a.total + PENC_THREADS - 1) / PENC_THREADS;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 64 * (int64_t)c->cus));
    c->tic(OFDM_K_CODE_ENCODE);
    hipLaunchKernelGGL(punct_encode_kernel, grid, dim3(PENC_THREADS), 0, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "punct_encode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_punct_decode(ofdm_ctx *ctx, int32_t rate, int32_t n_data, const void *d_eq, const void *d_csi,
                                 const void *d_count, int64_t n, void *d_info, void *d_path) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (rate < 0 || rate >= OFDM_PUNCT_RATES)
        return set_error(OFDM_E_ARG, "rate must be 0 (1/2), 1 (2/3) or 2 (3/4), got %d", (int)rate);
    if (n_data < 1 || n_data > OFDM_CODE_MAX_DATA_SYMBOLS)
        return set_error(OFDM_E_ARG, "n_data must be in [1, %d], got %d", OFDM_CODE_MAX_DATA_SYMBOLS, (int)n_data);
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_eq) return set_error(OFDM_E_ARG, "d_eq is NULL");
    if (!d_info) return set_error(OFDM_E_ARG, "d_info is NULL");
    if (!punct_aligned(d_eq, 8)) return set_error(OFDM_E_ARG, "d_eq must be 8-byte aligned");
    if (!punct_aligned(d_csi, 4)) return set_error(OFDM_E_ARG, "d_csi must be 4-byte aligned");
    if (!punct_aligned(d_count, 8)) return set_error(OFDM_E_ARG, "d_count must be 8-byte aligned");
    if (!punct_aligned(d_info, 4)) return set_error(OFDM_E_ARG, "d_info must be 4-byte aligned");
    if (!punct_aligned(d_path, 4)) return set_error(OFDM_E_ARG, "d_path must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    PdecArgs a{};
    a.eq = (const float2 *)d_eq;
    a.csi = (const float *)d_csi;
    a.count = (const int64_t *)d_count;
    a.info = (uint32_t *)d_info;
    a.path = (float *)d_path;
    a.n = n;
    a.nd = n_data;
    a.rate = rate;
    a.wi = OFDM_PUNCT_INFO_WORDS(n_data, rate);
    const size_t lds = PDEC_WAVES * pdec_wave_bytes(n_data, rate);
    // every wave two rows where there are that many, at most PDEC_BLOCKS_PER_CU blocks per CU; the waves loop over the rows
    const int64_t blocks = (n + PDEC_WAVES * PDEC_ROWS_PER_WAVE - 1) / (PDEC_WAVES * PDEC_ROWS_PER_WAVE);
    const dim3 grid((unsigned)std::min<int64_t>(blocks, PDEC_BLOCKS_PER_CU * (int64_t)c->cus));
    c->tic(OFDM_K_CODE_DECODE);
    hipLaunchKernelGGL(punct_decode_kernel, grid, dim3(64 * PDEC_WAVES), lds, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "punct_decode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
