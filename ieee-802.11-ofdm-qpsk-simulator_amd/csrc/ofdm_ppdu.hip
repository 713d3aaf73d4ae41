// ofdm_ppdu.hip -- self-describing coded packets (include/ofdm_mi355x_ppdu.h: ofdm_ppdu_encode, ofdm_ppdu_decode).  A
// translation unit of its own over ofdm_mi355x_punct.h's rules; ofdm_code.hip, ofdm_punct.hip and every other translation
// unit stay as they are, which is why the encoder's bit picking and the decoder's add-compare-select are restated here
// and not shared through a header: the older kernels keep their code objects byte for byte.
//
//   ppdu_info_kernel   : one thread per packet.  Header word, FCS over the body by a byte table in LDS, the PSDU moved
//     down by the 16 SERVICE bits, the scrambler run bit by bit, the pad: the packet's row of d_info.
//   ppdu_encode_kernel : punct_encode_kernel's thread per output word, with the row, the rate and the symbol index taken
//     per packet: symbol 0 is the header at rate 1/2, symbol d > 0 is symbol d - 1 of the data part at the rate the header
//     word names (a RATE field of 0, the info kernel's mark of a refused packet, encodes its zero data at rate 1/2).
//   ppdu_decode_kernel : one wave per row, PPDU_WAVES waves per block, lane = trellis state; punct_decode_kernel's layout
//     with the LDS region sized for rate 3/4, the header's decisions and soft values lying where the data part's decisions
//     go afterwards.  Header steps, traceback, scalar header check, then the data part in the branch of the header's rate,
//     traceback into lane-resident words, descrambling, SERVICE check and FCS.
#include <algorithm>
#include <cmath>
#include "ofdm_mi355x_ppdu.h"
#include "ofdm_stream_decode.h"

namespace ofdm {

static_assert(OFDM_PPDU_INFO_WORDS >= 2 + OFDM_PUNCT_INFO_WORDS(OFDM_CODE_MAX_DATA_SYMBOLS - 1, OFDM_PUNCT_RATE_3_4) &&
                  OFDM_PUNCT_INFO_WORDS(1, OFDM_PUNCT_RATE_1_2) == 2,
              "an info row holds the header's two words and the longest data part");
static_assert(4 * OFDM_PPDU_PSDU_WORDS >= (OFDM_PUNCT_INFO_BITS(OFDM_CODE_MAX_DATA_SYMBOLS - 1, OFDM_PUNCT_RATE_3_4) - 16) / 8,
              "a psdu row holds the longest PSDU");

constexpr int PPDU_TAIL = OFDM_PUNCT_TAIL_BITS;
constexpr int PPDU_HEADER_STEPS = OFDM_PUNCT_STEPS(OFDM_PUNCT_RATE_1_2);
constexpr int PPDU_MAX_STEPS = OFDM_PUNCT_STEPS(OFDM_PUNCT_RATE_3_4);
constexpr int PPDU_DATA_WORDS = OFDM_PPDU_INFO_WORDS - 2;
constexpr int PPDU_THREADS = 256;
constexpr int PPDU_WAVES = 2;                                // 26,880 B of LDS per block at D = 15: six blocks per CU
constexpr int PPDU_ROWS_PER_WAVE = 2;                        // the grid gives every wave two rows where there are that many
constexpr int PPDU_BLOCKS_PER_CU = 16;                       // the grid's cap: the waves loop past it
constexpr float PPDU_CLAMP = 0x1p100f;
constexpr uint32_t PPDU_CRC32_POLY = 0xEDB88320u;

__host__ __device__ constexpr int ppdu_deinterleave(int j) { return 16 * (j % 6) + j / 6; }
__host__ __device__ constexpr int ppdu_steps(int rate) { return OFDM_PUNCT_STEPS(rate); }
// cap(D, rate): the PSDU bytes that fit behind the SERVICE bits
__host__ __device__ constexpr int ppdu_cap(int nd, int rate) {
    return (ppdu_steps(rate) * (nd - 1) - PPDU_TAIL - OFDM_PPDU_SERVICE_BITS) / 8;
}
// the bits of a string's word that lie below bit `nbits` of the string, for the word that starts at bit 32 q
__host__ __device__ constexpr uint32_t ppdu_mask(int nbits, int q) {
    const int k = nbits - 32 * q;
    return k >= 32 ? 0xffffffffu : k <= 0 ? 0u : ~0u << (32 - k);
}

// ---- the header word ----
// CRC-8 of the top 18 bits of w: c = 0xFF; f = b ^ (c >> 7), c = ((c << 1) & 0xFF) ^ (f ? 7 : 0); the field is ~c
__host__ __device__ constexpr uint32_t ppdu_crc8(uint32_t w) {
    uint32_t c = 0xFFu;
    for (int k = 0; k < 18; ++k) {
        const uint32_t f = ((w >> (31 - k)) ^ (c >> 7)) & 1u;
        c = ((c << 1) & 0xFFu) ^ (f ? 0x07u : 0u);
    }
    return c ^ 0xFFu;
}
// word 0 of a header (word 1 is zero): RATE field, LENGTH, parity, CRC-8
__host__ __device__ constexpr uint32_t ppdu_header_word(uint32_t field, uint32_t length) {
    uint32_t w = (field << 28) | (length << 15), x = w >> 15;
    x ^= x >> 16, x ^= x >> 8, x ^= x >> 4, x ^= x >> 2, x ^= x >> 1;
    w |= (x & 1u) << 14;
    return w | (ppdu_crc8(w) << 6);
}
static_assert(ppdu_header_word(7, 123) == 0x703DF9C0u, "the header's known answer");
// the rate code of a valid header for nd symbols, -1 otherwise; *length is set with it
__device__ __forceinline__ int ppdu_header_check(uint32_t w0, uint32_t w1, int nd, int *length) {
    const int field = (int)(w0 >> 28), len = (int)((w0 >> 15) & 0xFFFu);
    if (field < 5 || field > 7 || w1 != 0u || w0 != ppdu_header_word((uint32_t)field, (uint32_t)len)) return -1;
    if (len < OFDM_PPDU_MIN_LENGTH || len > ppdu_cap(nd, field - 5)) return -1;
    *length = len;
    return field - 5;
}

// ---- the scrambler ----
// word i of the all-ones seed's 127-bit sequence repeated, MSB first: 160 bits serve every 32-bit window
__host__ __device__ constexpr uint32_t ppdu_seq_word(int i) {
    uint32_t s = 127u, w = 0u;
    for (int k = 0; k < 32 * (i + 1); ++k) {
        if (k % 127 == 0) s = 127u;
        const uint32_t b = ((s >> 6) ^ (s >> 3)) & 1u;
        s = ((s << 1) | b) & 127u;
        w = (w << 1) | b;
    }
    return w;
}
static_assert(ppdu_seq_word(0) == 0x0EF2C902u, "00001110 11110010 11001001 00000010");
// the 32 sequence bits from position p (0 .. 126) on
__device__ __forceinline__ uint32_t ppdu_seq_window(int p) {
    constexpr uint32_t q0 = ppdu_seq_word(0), q1 = ppdu_seq_word(1), q2 = ppdu_seq_word(2), q3 = ppdu_seq_word(3), q4 = ppdu_seq_word(4);
    const int i = p >> 5;
    const uint32_t hi = i == 0 ? q0 : i == 1 ? q1 : i == 2 ? q2 : q3, lo = i == 0 ? q1 : i == 1 ? q2 : i == 2 ? q3 : q4;
    return (uint32_t)(((((uint64_t)hi << 32) | lo) << (p & 31)) >> 32);
}

__device__ __forceinline__ uint32_t ppdu_crc32_entry(uint32_t c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (PPDU_CRC32_POLY & (0u - (c & 1u)));
    return c;
}

// ---- encoder, launch 1: the information rows ----
struct PpduInfoArgs {
    const uint32_t *psdu;    // [n][31]
    const int32_t *len, *rate, *seed;
    uint32_t *info;          // [n][36]
    int64_t n;
    int32_t nd;
};

__global__ __launch_bounds__(PPDU_THREADS) void ppdu_info_kernel(PpduInfoArgs a) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x] = ppdu_crc32_entry(threadIdx.x);
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * PPDU_THREADS + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * PPDU_THREADS) {
        const uint32_t *row = a.psdu + i * OFDM_PPDU_PSDU_WORDS;
        uint32_t *out = a.info + i * OFDM_PPDU_INFO_WORDS;
        const int rate = a.rate[i], len = a.len[i], seed = a.seed[i];
        const bool ok = rate >= 0 && rate < OFDM_PUNCT_RATES && len >= OFDM_PPDU_MIN_LENGTH && len <= ppdu_cap(a.nd, rate) &&
                        seed >= 1 && seed <= 127;
        out[1] = 0u;
        if (!ok) {                                                     // the refused packet: RATE field 0, LENGTH 0, zero data
            out[0] = ppdu_header_word(0u, 0u);
            for (int q = 0; q < PPDU_DATA_WORDS; ++q) out[2 + q] = 0u;
            continue;
        }
        out[0] = ppdu_header_word(5u + (uint32_t)rate, (uint32_t)len);
        const int body = len - 4, kinfo = ppdu_steps(rate) * (a.nd - 1) - PPDU_TAIL;
        auto byte_of = [&](int j) -> uint32_t { return (row[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu; };
        uint32_t crc = 0xffffffffu;
        for (int j = 0; j < body; ++j) crc = (crc >> 8) ^ tab[(crc ^ byte_of(j)) & 0xFFu];
        crc = ~crc;
        // word k of the PSDU as it is sent: the body, the FCS big-endian, zeros
        auto sent = [&](int k) -> uint32_t {
            uint32_t v = 0u;
            for (int b = 0; b < 4; ++b) {
                const int j = 4 * k + b;
                v = (v << 8) | (j < body ? byte_of(j) : j < len ? (crc >> (24 - 8 * (j - body))) & 0xFFu : 0u);
            }
            return v;
        };
        uint32_t s = (uint32_t)seed, prev = 0u;
        for (int q = 0; q < PPDU_DATA_WORDS; ++q) {
            const uint32_t cur = 4 * q < len ? sent(q) : 0u;
            uint32_t seq = 0u;
            for (int k = 0; k < 32; ++k) {
                const uint32_t b = ((s >> 6) ^ (s >> 3)) & 1u;
                s = ((s << 1) | b) & 127u;
                seq = (seq << 1) | b;
            }
            out[2 + q] = (((prev << 16) | (cur >> 16)) ^ seq) & ppdu_mask(kinfo, q);
            prev = cur;
        }
    }
}

// ---- encoder, launch 2: punct_encode_kernel's word per thread ----
struct PpduEncArgs {
    const uint32_t *info;    // [n][36]
    uint32_t *words;         // [n][3 nd]
    int64_t total;           // n 3 nd output words
    int32_t nd;
};

struct PpduBits128 {
    uint64_t hi, lo;         // bit i of the sequence at bit 63 - i of hi (i < 64) or 127 - i of lo
};
__device__ __forceinline__ PpduBits128 ppdu_shr(PpduBits128 x, int s) { return {x.hi >> s, (x.lo >> s) | (x.hi << (64 - s))}; }   // 0 < s < 64
__device__ __forceinline__ PpduBits128 operator^(PpduBits128 a, PpduBits128 b) { return {a.hi ^ b.hi, a.lo ^ b.lo}; }
__device__ __forceinline__ uint32_t ppdu_bit(PpduBits128 x, int i) {
    return (uint32_t)(i < 64 ? x.hi >> (63 - i) : x.lo >> (127 - i)) & 1u;
}

__global__ __launch_bounds__(PPDU_THREADS) void ppdu_encode_kernel(PpduEncArgs a) {
    const int wpp = 3 * a.nd;
    for (int64_t o = (int64_t)blockIdx.x * PPDU_THREADS + threadIdx.x; o < a.total; o += (int64_t)gridDim.x * PPDU_THREADS) {
        const int64_t i = o / wpp;
        const int w = (int)(o - i * wpp), sym = w / 3, part = w - 3 * sym;
        const uint32_t *head = a.info + i * OFDM_PPDU_INFO_WORDS;
        const uint32_t field = head[0] >> 28;
        // the header is a one-symbol rate-1/2 packet; the data part D - 1 symbols at the header's rate
        const int rate = sym == 0 || field < 5u ? OFDM_PUNCT_RATE_1_2 : (int)field - 5;
        const int S = ppdu_steps(rate), d = sym == 0 ? 0 : sym - 1;
        const int kinfo = S * (sym == 0 ? 1 : a.nd - 1) - PPDU_TAIL, wi = (kinfo + 31) / 32;
        const uint32_t *row = sym == 0 ? head : head + 2;
        auto word = [&](int q) -> uint32_t { return q < 0 || q >= wi ? 0u : row[q] & ppdu_mask(kinfo, q); };
        // X: u_t0+i at sequence bit i, t0 = S d - 6, i = 0 .. S + 5 <= 77; sh + 78 <= 109 bits of the four words
        const int t0 = S * d - PPDU_TAIL, q0 = (t0 + 32) / 32 - 1, sh = t0 - 32 * q0;       // floor division for t0 = -6
        const uint64_t hi = ((uint64_t)word(q0) << 32) | word(q0 + 1), lo = ((uint64_t)word(q0 + 2) << 32) | word(q0 + 3);
        const PpduBits128 X = sh ? PpduBits128{(hi << sh) | (lo >> (64 - sh)), lo << sh} : PpduBits128{hi, lo};
        const PpduBits128 X2 = ppdu_shr(X, 2), X3 = ppdu_shr(X, 3), X6 = ppdu_shr(X, 6);
        const PpduBits128 A = X ^ X2 ^ X3 ^ ppdu_shr(X, 5) ^ X6;
        const PpduBits128 B = X ^ ppdu_shr(X, 1) ^ X2 ^ X3 ^ X6;
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
            return ppdu_bit(b ? B : A, tau + PPDU_TAIL);
        };
        uint32_t out = 0u;
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const int j = 32 * part + 2 * mm;
            const uint32_t g0 = coded(ppdu_deinterleave(j)), g1 = coded(ppdu_deinterleave(j + 1));
            out |= ((g0 << 1) | (g0 ^ g1)) << (30 - 2 * mm);
        }
        a.words[o] = out;
    }
}

// ---- decoder ----
// punct_decode_kernel's wave (lane = new state, two ds_bpermute reads of the predecessors' metrics, the ballot as the
// decision word, lane 0's LDS write, the readlane traceback), run twice per row: over the header's 48 steps, and, if the
// header holds, over the S (D - 1) steps of the data part in the branch of its rate.  The wave's LDS region: 72 (D - 1)
// decision words of 64 bits -- the rate is not known before the header is read -- then the 96 (D - 1) soft values of the
// data symbols in sent order.  The header's 48 decision words and its 96 soft values (48 words) lie at the head of the
// decision area: they are dead once the header is traced back, before the data part's first decision is written, so the
// header costs no LDS (at D = 2 the area is these 96 words, more than the 72 the data part needs).  At D = 15 that is
// 8,064 + 5,376 = 13,440 B per wave, the region of punct_decode_kernel at rate 2/3, and six blocks per CU; with the
// header's words kept apart it would be 14,208 B and five.  Everything between the two decodes and behind the second is
// wave-uniform: the compiler keeps it on the scalar unit, but for the lanes' own words.
struct PpduDecArgs {
    const float2 *eq;        // [n][48 nd]
    const float *csi;        // optional, [n][48]
    const int64_t *count;    // optional: [1] rows at most
    int32_t *meta;           // [n][4]: status, rate, length, seed
    uint32_t *psdu;          // [n][31]
    float *path;             // optional, [n][2]
    int64_t n;
    int32_t nd;
};

// the decision area: the data part's words at rate 3/4, at least the header's 48 decisions and 48 words of soft values
constexpr size_t ppdu_decision_words(int nd) { return std::max<size_t>((size_t)PPDU_MAX_STEPS * (nd - 1), 2 * PPDU_HEADER_STEPS); }
constexpr size_t ppdu_wave_words(int nd) { return ppdu_decision_words(nd) + 48 * (size_t)(nd - 1); }

__device__ __forceinline__ float ppdu_flip(float v, uint32_t sign) { return __uint_as_float(__float_as_uint(v) ^ sign); }

__global__ __launch_bounds__(64 * PPDU_WAVES) void ppdu_decode_kernel(PpduDecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long ppdu_smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nd = a.nd, nsoft = 96 * nd;
    unsigned long long *dw = ppdu_smem + (size_t)wave * ppdu_wave_words(nd);      // a multiple of 16 bytes per wave
    float *hsoft = reinterpret_cast<float *>(dw + PPDU_HEADER_STEPS);             // the header's 96 values, dead after its steps
    float *softd = reinterpret_cast<float *>(dw + ppdu_decision_words(nd));       // the data symbols' 96 (D - 1) values
    const int p0 = (2 * lane) & 63, p1 = p0 | 1;
    const uint32_t a0 = ((lane >> 5) ^ (lane >> 3) ^ (lane >> 2) ^ lane) & 1u;
    const uint32_t b0 = ((lane >> 5) ^ (lane >> 4) ^ (lane >> 3) ^ (lane >> 2)) & 1u;
    const uint32_t sa0 = a0 << 31, sb0 = b0 << 31, sa1 = sa0 ^ 0x80000000u, sb1 = sb0 ^ 0x80000000u;
#ifndef OFDM_PPDU_CRC_BITWISE
    // the CRC-32 byte table, entry 64 k + lane in tk
    const uint32_t t0 = ppdu_crc32_entry(lane), t1 = ppdu_crc32_entry(64 + lane), t2 = ppdu_crc32_entry(128 + lane),
                   t3 = ppdu_crc32_entry(192 + lane);
#endif
    int64_t rows = a.n;
    if (a.count) rows = std::min<int64_t>(rows, a.count[1]);
    for (int64_t i = (int64_t)blockIdx.x * PPDU_WAVES + wave; i < rows; i += (int64_t)gridDim.x * PPDU_WAVES) {
        // ---- the soft values of all D symbols, into sent order ----
        const float2 *zrow = a.eq + i * (48 * nd);
        for (int e0 = 0; e0 < nsoft; e0 += 64) {
            const int e = e0 + lane;
            if (e < nsoft) {
                const int d = e / 96, j = e - 96 * d, m = j >> 1;
                const float2 z = zrow[48 * d + m];
                const float w = a.csi ? a.csi[i * 48 + m] : 1.0f;
                float lam = w * ((j & 1) ? z.x : z.y);
                if (!(fabsf(lam) < INFINITY)) lam = 0.f;
                lam = fminf(fmaxf(lam, -PPDU_CLAMP), PPDU_CLAMP);
                (d == 0 ? hsoft : softd + 96 * (d - 1))[ppdu_deinterleave(j)] = lam;
            }
        }
        rxc_wave_sync();
        float M = lane == 0 ? 0.f : -INFINITY;
        auto acs = [&](float lx, float ly, int t) {
            const float m0 = __shfl(M, p0, 64), m1 = __shfl(M, p1, 64);
            const float c0 = m0 + (ppdu_flip(lx, sa0) + ppdu_flip(ly, sb0));
            const float c1 = m1 + (ppdu_flip(lx, sa1) + ppdu_flip(ly, sb1));
            const bool win = c1 > c0;
            M = win ? c1 : c0;
            const unsigned long long word = __ballot(win);
            if (lane == 0) dw[t] = word;
        };
        // a stolen value alone: the inner sum is the kept value's flip
        auto acs1 = [&](float l, uint32_t s0, uint32_t s1, int t) {
            const float m0 = __shfl(M, p0, 64), m1 = __shfl(M, p1, 64);
            const float c0 = m0 + ppdu_flip(l, s0);
            const float c1 = m1 + ppdu_flip(l, s1);
            const bool win = c1 > c0;
            M = win ? c1 : c0;
            const unsigned long long word = __ballot(win);
            if (lane == 0) dw[t] = word;
        };
        // traceback from state 0 over the first `steps` decision words: information word l lands in lane l
        auto traceback = [&](int steps) -> uint32_t {
            const int kinfo = steps - PPDU_TAIL;
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
            return mine;
        };
        // ---- the header: a one-symbol rate-1/2 packet ----
        for (int t = 0; t < PPDU_HEADER_STEPS; ++t) {
            const float2 l = reinterpret_cast<const float2 *>(hsoft)[t];
            acs(l.x, l.y, t);
        }
        const float path0 = M;
        rxc_wave_sync();
        const uint32_t hw = traceback(PPDU_HEADER_STEPS);
        rxc_wave_sync();                                               // the data part's decisions overwrite the header's words
        int length = 0;
        const int rate = ppdu_header_check((uint32_t)__builtin_amdgcn_readlane((int)hw, 0),
                                           (uint32_t)__builtin_amdgcn_readlane((int)hw, 1), nd, &length);
        int status = OFDM_PPDU_BAD_HEADER, seed = 0;
        uint32_t pw = 0u;                                              // the lane's PSDU word
        if (rate >= 0) {
            // ---- the data part: D - 1 symbols at the header's rate, from state 0 ----
            const int steps = ppdu_steps(rate) * (nd - 1), kinfo = steps - PPDU_TAIL;
            M = lane == 0 ? 0.f : -INFINITY;
            if (rate == OFDM_PUNCT_RATE_1_2) {
                for (int t = 0; t < steps; ++t) {
                    const float2 l = reinterpret_cast<const float2 *>(softd)[t];
                    acs(l.x, l.y, t);
                }
            } else if (rate == OFDM_PUNCT_RATE_2_3) {
                for (int q = 0; 2 * q < steps; ++q) {                   // A_2q B_2q A_2q+1
                    const float l0 = softd[3 * q], l1 = softd[3 * q + 1], l2 = softd[3 * q + 2];
                    acs(l0, l1, 2 * q);
                    acs1(l2, sa0, sa1, 2 * q + 1);
                }
            } else {
                for (int q = 0; 3 * q < steps; ++q) {                   // A_3q B_3q A_3q+1 B_3q+2
                    const float4 l = reinterpret_cast<const float4 *>(softd)[q];
                    acs(l.x, l.y, 3 * q);
                    acs1(l.z, sa0, sa1, 3 * q + 1);
                    acs1(l.w, sb0, sb1, 3 * q + 2);
                }
            }
            if (a.path && lane == 0) a.path[2 * i + 1] = M;
            rxc_wave_sync();
            uint32_t mine = traceback(steps);
            // ---- the scrambler: the first seven bits are its state; where they stand in the 127-bit sequence gives the
            // seed (the seven bits before them) and every lane's 32 sequence bits ----
            const uint32_t state = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0) >> 25;
            status = 0;
            if (state) {
                const unsigned long long f0 = __ballot(ppdu_seq_window(lane) >> 25 == state);
                const unsigned long long f1 = __ballot(lane < 63 && ppdu_seq_window(64 + lane) >> 25 == state);
                const int at = f0 ? __builtin_ctzll(f0) : 64 + __builtin_ctzll(f1);
                seed = (int)(ppdu_seq_window((at + 120) % 127) >> 25);
                mine = (mine ^ ppdu_seq_window((at + 32 * lane) % 127)) & ppdu_mask(kinfo, lane);
            } else {
                status = OFDM_PPDU_BAD_SERVICE;                        // seven zeros are no state: nothing is descrambled
            }
            if ((uint32_t)__builtin_amdgcn_readlane((int)mine, 0) >> 16) status |= OFDM_PPDU_BAD_SERVICE;
            // ---- the PSDU: the LENGTH bytes behind the 16 SERVICE bits ----
            const uint32_t next = __shfl(mine, (lane + 1) & 63, 64);
            pw = ((mine << 16) | (next >> 16)) & ppdu_mask(8 * length, lane);
            // ---- the FCS, wave-uniform: CRC-32 over the body against the four bytes behind it ----
            const int body = length - 4;
            uint32_t crc = 0xffffffffu, got = 0u;
            for (int k = 0; 4 * k < length; ++k) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)pw, k);
                for (int b = 0; b < 4; ++b) {
                    const int j = 4 * k + b;
                    const uint32_t byte = (w >> (24 - 8 * b)) & 0xFFu;
                    if (j < body) {
#ifdef OFDM_PPDU_CRC_BITWISE
                        crc ^= byte;
                        for (int r = 0; r < 8; ++r) crc = (crc >> 1) ^ (PPDU_CRC32_POLY & (0u - (crc & 1u)));
#else
                        const uint32_t x = (crc ^ byte) & 0xFFu, sel = x >> 6;
                        const uint32_t tv = sel == 0 ? t0 : sel == 1 ? t1 : sel == 2 ? t2 : t3;
                        crc = (crc >> 8) ^ (uint32_t)__builtin_amdgcn_readlane((int)tv, x & 63u);
#endif
                    } else if (j < length) {
                        got = (got << 8) | byte;
                    }
                }
            }
            if (got != ~crc) status |= OFDM_PPDU_BAD_FCS;
        } else if (a.path && lane == 0) {
            a.path[2 * i + 1] = 0.f;
        }
        if (lane < OFDM_PPDU_PSDU_WORDS) a.psdu[i * OFDM_PPDU_PSDU_WORDS + lane] = pw;
        if (lane == 0) {
            if (a.path) a.path[2 * i] = path0;
            *reinterpret_cast<int4 *>(a.meta + 4 * i) = make_int4(status, rate, length, seed);
        }
        rxc_wave_sync();                                               // the next row overwrites the wave's region
    }
}

// a device pointer aligned to `align` bytes (a power of two)
static bool ppdu_aligned(const void *p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0; }

static int ppdu_check_n_data(int32_t n_data) {
    if (n_data < OFDM_PPDU_MIN_SYMBOLS || n_data > OFDM_CODE_MAX_DATA_SYMBOLS)
        return set_error(OFDM_E_ARG, "n_data must be in [%d, %d] (a header symbol and at least one data symbol), got %d",
                         OFDM_PPDU_MIN_SYMBOLS, OFDM_CODE_MAX_DATA_SYMBOLS, (int)n_data);
    return OFDM_OK;
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_ppdu_encode(ofdm_ctx *ctx, int32_t n_data, const void *d_psdu, const void *d_len, const void *d_rate,
                                const void *d_seed, int64_t n, void *d_info, void *d_words) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (const int rc = ppdu_check_n_data(n_data)) return rc;
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_psdu) return set_error(OFDM_E_ARG, "d_psdu is NULL");
    if (!d_len) return set_error(OFDM_E_ARG, "d_len is NULL");
    if (!d_rate) return set_error(OFDM_E_ARG, "d_rate is NULL");
    if (!d_seed) return set_error(OFDM_E_ARG, "d_seed is NULL");
    if (!d_info) return set_error(OFDM_E_ARG, "d_info is NULL");
    if (!d_words) return set_error(OFDM_E_ARG, "d_words is NULL");
    if (!ppdu_aligned(d_psdu, 4)) return set_error(OFDM_E_ARG, "d_psdu must be 4-byte aligned");
    if (!ppdu_aligned(d_len, 4)) return set_error(OFDM_E_ARG, "d_len must be 4-byte aligned");
    if (!ppdu_aligned(d_rate, 4)) return set_error(OFDM_E_ARG, "d_rate must be 4-byte aligned");
    if (!ppdu_aligned(d_seed, 4)) return set_error(OFDM_E_ARG, "d_seed must be 4-byte aligned");
    if (!ppdu_aligned(d_info, 4)) return set_error(OFDM_E_ARG, "d_info must be 4-byte aligned");
    if (!ppdu_aligned(d_words, 4)) return set_error(OFDM_E_ARG, "d_words must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    PpduInfoArgs ia{};
    ia.psdu = (const uint32_t *)d_psdu;
    ia.len = (const int32_t *)d_len;
    ia.rate = (const int32_t *)d_rate;
    ia.seed = (const int32_t *)d_seed;
    ia.info = (uint32_t *)d_info;
    ia.n = n;
    ia.nd = n_data;
    PpduEncArgs ea{};
    ea.info = (const uint32_t *)d_info;
    ea.words = (uint32_t *)d_words;
    ea.nd = n_data;
    ea.total = n * 3 * n_data;
    const int64_t cap = 64 * (int64_t)c->cus;
    const dim3 igrid((unsigned)std::min<int64_t>((n + PPDU_THREADS - 1) / PPDU_THREADS, cap));
    const dim3 egrid((unsigned)std::min<int64_t>((ea.total + PPDU_THREADS - 1) / PPDU_THREADS, cap));
    c->tic(OFDM_K_CODE_ENCODE);
    hipLaunchKernelGGL(ppdu_info_kernel, igrid, dim3(PPDU_THREADS), 0, c->stream, ia);
    hipLaunchKernelGGL(ppdu_encode_kernel, egrid, dim3(PPDU_THREADS), 0, c->stream, ea);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "ppdu encode launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

extern "C" int ofdm_ppdu_decode(ofdm_ctx *ctx, int32_t n_data, const void *d_eq, const void *d_csi, const void *d_count,
                                int64_t n, void *d_meta, void *d_psdu, void *d_path) {
    Ctx *c = reinterpret_cast<Ctx *>(ctx);
    if (const int rc = ppdu_check_n_data(n_data)) return rc;
    if (n < 0) return set_error(OFDM_E_ARG, "n %lld is negative", (long long)n);
    if (!d_eq) return set_error(OFDM_E_ARG, "d_eq is NULL");
    if (!d_meta) return set_error(OFDM_E_ARG, "d_meta is NULL");
    if (!d_psdu) return set_error(OFDM_E_ARG, "d_psdu is NULL");
    if (!ppdu_aligned(d_eq, 8)) return set_error(OFDM_E_ARG, "d_eq must be 8-byte aligned");
    if (!ppdu_aligned(d_csi, 4)) return set_error(OFDM_E_ARG, "d_csi must be 4-byte aligned");
    if (!ppdu_aligned(d_count, 8)) return set_error(OFDM_E_ARG, "d_count must be 8-byte aligned");
    if (!ppdu_aligned(d_meta, 16)) return set_error(OFDM_E_ARG, "d_meta must be 16-byte aligned");
    if (!ppdu_aligned(d_psdu, 4)) return set_error(OFDM_E_ARG, "d_psdu must be 4-byte aligned");
    if (!ppdu_aligned(d_path, 4)) return set_error(OFDM_E_ARG, "d_path must be 4-byte aligned");
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (n == 0) return OFDM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    PpduDecArgs a{};
    a.eq = (const float2 *)d_eq;
    a.csi = (const float *)d_csi;
    a.count = (const int64_t *)d_count;
    a.meta = (int32_t *)d_meta;
    a.psdu = (uint32_t *)d_psdu;
    a.path = (float *)d_path;
    a.n = n;
    a.nd = n_data;
    const size_t lds = PPDU_WAVES * ppdu_wave_words(n_data) * sizeof(unsigned long long);
    // every wave two rows where there are that many, at most PPDU_BLOCKS_PER_CU blocks per CU; the waves loop over the rows
    const int64_t blocks = (n + PPDU_WAVES * PPDU_ROWS_PER_WAVE - 1) / (PPDU_WAVES * PPDU_ROWS_PER_WAVE);
    const dim3 grid((unsigned)std::min<int64_t>(blocks, PPDU_BLOCKS_PER_CU * (int64_t)c->cus));
    c->tic(OFDM_K_CODE_DECODE);
    hipLaunchKernelGGL(ppdu_decode_kernel, grid, dim3(64 * PPDU_WAVES), lds, c->stream, a);
    c->toc();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "ppdu_decode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}
