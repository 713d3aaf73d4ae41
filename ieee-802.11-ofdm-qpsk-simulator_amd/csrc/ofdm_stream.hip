// ofdm_stream.hip -- the stream receiver (include/ofdm_mi355x_stream.h: ofdm_receive_stream): Packet_Detection and
// Packet_Selection (OFDM.c:659-771) once over one device-resident recording of any length, then Receiver()'s chain
// (OFDM.c:962-1165) on every packet found.  A translation unit of its own beside ofdm_captures.hip (one capture per
// wave, at most one packet per capture): the two share the inlined device helpers of ofdm_rxcommon.h and the
// post-selection chain of ofdm_rxchain.h, which each kernel runs on samples it has staged its own way.
//
//   stream_detect_kernel<METRIC> : a block takes OFDM_STREAM_TILE positions.  It stages TILE + 47 samples once
//     (16-byte loads, real and imaginary planes in LDS; the 47-sample halo is the only re-read), a lane owns one run
//     of OFDM_STREAM_RUN contiguous positions (odd: the lanes' strides fall on distinct banks), opens it with the
//     direct 32-term sum and slides in fp32 as capture_rx_kernel does.  RUN BOUNDARIES ARE FIXED IN ABSOLUTE STREAM
//     COORDINATES -- run j is [j RUN, (j + 1) RUN), tile t is runs [256 t, 256 (t + 1)) -- so every M[i] and every
//     crossing is bit-identical whatever the grid, the tile-to-block assignment or the alignment of the samples.
//     Crossings are gathered in an LDS bitmap and leave as whole 32-bit words, 16 bytes per lane.
//   stream_select_kernel<PHASE> : integer logic on the bitmap alone.  0: a thread owns one slot of 301 positions (at
//     most one front: fronts are more than 300 apart), finds the slot's front (a set bit whose predecessor is clear,
//     at position >= 300 -- the virtual crossing at -1 -- with 300 clear bits behind it, read from the neighbouring
//     words in global memory) and its +230 confirmation; per block the number of confirmed fronts and the largest
//     front.  1: one block scans the blocks' counts in order, reduces the largest front and writes d_count.
//     2: ordered compaction -- slot order is position order -- of the first max_packets confirmed fronts into
//     packet_pos, with the LAST_FRONT flag.  No arrival-order append anywhere: the output is deterministic.
//   stream_decode_kernel<OUT> : one wave per packet, W waves per block, looping over d_count.  A wave stages only
//     [p - 20, p + 2 nfr - 2] (2 nfr + 19 samples, zero outside the stream) and runs the chain of ofdm_rxchain.h on it.
// ofdm_receive_stream_ex (ofdm_stream_conj.hip) enters through stream_receive with a detector of its own
// (ofdm_stream_detect.h): another detection launch, then the selection and decode launches of this file.
// ofdm_receive_stream_timed (ofdm_stream_timing.hip) adds a refiner through the same door: one launch of its own
// between stream_select_kernel<2> and stream_decode_kernel that rewrites packet_pos.
// ofdm_receive_stream_tracked (ofdm_stream_track.hip) adds a decoder: its own kernel in place of stream_decode_kernel,
// launched with the same arguments, grid and LDS.  DecArgs and the staging, filter and sync record of the two decode
// kernels live in ofdm_stream_decode.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "ofdm_mi355x_stream.h"
#include "ofdm_ctx.h"
#include "ofdm_rxcommon.h"
#include "ofdm_stream_detect.h"
#include "ofdm_stream_decode.h"

namespace ofdm {

constexpr int SD_RUN = OFDM_STREAM_RUN;
constexpr int SD_THREADS = 256;
constexpr int SD_TILE = OFDM_STREAM_TILE;
constexpr int SD_SAMPLES = SD_TILE + 47;
constexpr int SD_PLANE = (SD_SAMPLES + 3) & ~3;
constexpr int SD_WORDS = SD_TILE / 32;
constexpr int SD_LOADS = (SD_SAMPLES / 2 + SD_THREADS - 1) / SD_THREADS;      // 16-byte loads per lane and tile
static_assert(SD_TILE == SD_RUN * SD_THREADS && SD_TILE % 128 == 0 && (SD_RUN & 1), "tile = 256 odd runs, whole 16-byte groups of bitmap words");
static_assert(SD_RUN <= 147, "no run longer than capture_rx_kernel's longest (the measured fp32 drift is the precedent)");
static_assert((2 * SD_PLANE + SD_WORDS) * 4 <= 64 * 1024, "static LDS");
constexpr int SS_THREADS = 256;           // slots per block of the selection kernel
constexpr int SS_SLOT = 301;              // positions per slot: fronts are at least 301 apart
constexpr int SS_SCAN_THREADS = 1024;

constexpr int SDEC_MAX_WAVES = 8;                     // packets per decode block at most: 512 threads, two waves per SIMD
static_assert(SDEC_MAX_WAVES <= RXC_MAX_WAVES, "the block stream_receive sizes fits both decode kernels' launch bounds");
static_assert(sizeof(ofdm_stream_packet) == 64, "ofdm_stream_packet is 64 bytes");

// DetArgs: ofdm_stream_detect.h (shared with the detectors of ofdm_stream_conj.hip)
template <bool METRIC>
__global__ __launch_bounds__(SD_THREADS) void stream_detect_kernel(DetArgs a) {
    __shared__ __attribute__((aligned(16))) float re[SD_PLANE];
    __shared__ __attribute__((aligned(16))) float im[SD_PLANE];
    __shared__ __attribute__((aligned(16))) uint32_t bm[SD_WORDS];
    const int tid = threadIdx.x;
    // 1: the stream starts 8 bytes off a 16-byte line; tiles start at even samples, so every tile shares it
    const int head = (int)((reinterpret_cast<uintptr_t>(a.x) >> 3) & 1u);
    for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const int64_t t0 = t * SD_TILE;
        // ---- stage [t0, t0 + TILE + 47) clipped to the stream; the rest of the planes and the bitmap zeroed ----
        {
            const float2 *row = a.x + t0;
            const int cnt = (int)std::min<int64_t>(SD_SAMPLES, a.n - t0);
            if (head && tid == 0) { const float2 v = row[0]; re[0] = v.x; im[0] = v.y; }
            const f4v *r4 = reinterpret_cast<const f4v *>(row + head);
            const int np = (cnt - head) >> 1;
            // every load of the tile is in flight before the first LDS write (issued one after the other, each behind
            // the LDS writes of the one before, the kernel measured 1.00 ms on a 2^28-sample stream against 0.71 ms)
            f4v v[SD_LOADS];
#pragma unroll
            for (int j = 0; j < SD_LOADS; ++j) {
                const int k = tid + j * SD_THREADS;
                if (k < np) v[j] = __builtin_nontemporal_load(r4 + k);
            }
#pragma unroll
            for (int j = 0; j < SD_LOADS; ++j) {
                const int k = tid + j * SD_THREADS;
                if (k >= np) continue;
                if (head) {
                    const int m = 1 + 2 * k;
                    re[m] = v[j].x; im[m] = v[j].y; re[m + 1] = v[j].z; im[m + 1] = v[j].w;
                } else {
                    *reinterpret_cast<float2 *>(re + 2 * k) = make_float2(v[j].x, v[j].z);
                    *reinterpret_cast<float2 *>(im + 2 * k) = make_float2(v[j].y, v[j].w);
                }
            }
            if (((cnt - head) & 1) && tid == 0) { const float2 v = row[cnt - 1]; re[cnt - 1] = v.x; im[cnt - 1] = v.y; }
            for (int k = cnt + tid; k < SD_PLANE; k += SD_THREADS) { re[k] = 0.f; im[k] = 0.f; }
            if (tid < SD_WORDS) bm[tid] = 0u;
        }
        __syncthreads();
        // ---- this lane's run: positions t0 + [n0, n0 + cnt) ----
        {
            const int n0 = tid * SD_RUN;
            const int cnt = (int)std::min<int64_t>(SD_RUN, a.lc - (t0 + n0));
            if (cnt > 0) {
                float sx = 0.f, sy = 0.f, pw = 0.f;
                int nz = 0;                                            // samples of the power window that are not zero
#pragma unroll 8
                for (int k = 0; k < 32; ++k) {
                    const float ux = re[n0 + k], uy = im[n0 + k], vx = re[n0 + k + 16], vy = im[n0 + k + 16];
                    sx = fmaf(ux, vx, sx); sx = fmaf(-uy, vy, sx);
                    sy = fmaf(ux, vy, sy); sy = fmaf(uy, vx, sy);
                    pw = fmaf(vx, vx, pw); pw = fmaf(vy, vy, pw);
                    nz += (vx != 0.f) | (vy != 0.f);
                }
                for (int j = 0; j < cnt; ++j) {
                    const int n = n0 + j;
                    // an all-zero power window has c = p = 0 exactly: what the slide left behind is rounding residue of
                    // the samples that have gone, and must not decide a crossing (idle gaps have none)
                    if (nz == 0) { sx = 0.f; sy = 0.f; pw = 0.f; }
                    const float num = fmaf(sx, sx, sy * sy), h = 0.75f * pw;
                    if (fmaf(h, pw, -num) < 0.f) atomicOr(&bm[n >> 5], 1u << (n & 31));     // |c|^2 / p^2 > 0.75
                    if constexpr (METRIC) a.metric[t0 + n] = num / (pw * pw);
                    if (j + 1 < cnt) {                                 // n + 48 <= t0 + n0 + cnt + 46 < the stream's end
                        const float o0x = re[n], o0y = im[n], o1x = re[n + 16], o1y = im[n + 16];
                        const float i0x = re[n + 32], i0y = im[n + 32], i1x = re[n + 48], i1y = im[n + 48];
                        sx = fmaf(i0x, i1x, sx); sx = fmaf(-i0y, i1y, sx);
                        sx = fmaf(-o0x, o1x, sx); sx = fmaf(o0y, o1y, sx);
                        sy = fmaf(i0x, i1y, sy); sy = fmaf(i0y, i1x, sy);
                        sy = fmaf(-o0x, o1y, sy); sy = fmaf(-o0y, o1x, sy);
                        pw = fmaf(i1x, i1x, pw); pw = fmaf(i1y, i1y, pw);
                        pw = fmaf(-o1x, o1x, pw); pw = fmaf(-o1y, o1y, pw);
                        nz += (int)((i1x != 0.f) | (i1y != 0.f)) - (int)((o1x != 0.f) | (o1y != 0.f));
                    }
                }
            }
        }
        __syncthreads();
        // ---- the tile's bitmap words: 16 bytes per lane into the scratch bitmap, and the caller's copy ----
        {
            const int64_t w0 = t0 >> 5;
            if (tid < SD_WORDS / 4 && w0 + 4 * tid < a.words)          // the scratch bitmap is padded to whole groups
                reinterpret_cast<uint4 *>(a.bitmap + w0)[tid] = reinterpret_cast<const uint4 *>(bm)[tid];
            if (a.cross && tid < SD_WORDS && w0 + tid < a.words) a.cross[w0 + tid] = bm[tid];
        }
        __syncthreads();                                               // the next tile overwrites the planes
    }
}

struct SelArgs {
    const uint32_t *bitmap;
    int64_t lc, nslots, nblocks, max_packets;
    int64_t *slots;        // [nslots] front << 1 | confirmed, or -1
    int64_t *blk_cnt;      // [nblocks] confirmed fronts of the block; after phase 1 their exclusive prefix
    int64_t *blk_max;      // [nblocks] largest front of the block, -1 when none; after phase 1 [0] the stream's
    int64_t *count;        // d_count
    ofdm_stream_packet *pk;
};

// bits [lo, hi) of the bitmap are all clear (0 <= lo < hi)
__device__ __forceinline__ bool stream_bits_clear(const uint32_t *bm, int64_t lo, int64_t hi) {
    for (int64_t w = (hi - 1) >> 5; w >= (lo >> 5); --w) {
        uint32_t x = bm[w];
        const int64_t base = w << 5;
        if (base < lo) x &= ~0u << (int)(lo - base);
        if (base + 32 > hi) x &= ~0u >> (int)(base + 32 - hi);
        if (x) return false;
    }
    return true;
}

// block-wide sum and maximum of 64-bit values (SS_THREADS threads; red has 2 x 4 words)
__device__ __forceinline__ void stream_block_reduce(int64_t cnt, int64_t mx, int64_t *red, int64_t &cnt_out, int64_t &mx_out) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        mx = max(mx, (int64_t)__shfl_xor(mx, o, 64));
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[wave] = cnt; red[16 + wave] = mx; }
    __syncthreads();
    cnt_out = 0;
    mx_out = -1;
    for (int k = 0; k < nw; ++k) { cnt_out += red[k]; mx_out = max(mx_out, red[16 + k]); }
}

template <int PHASE>
__global__ __launch_bounds__(PHASE == 1 ? SS_SCAN_THREADS : SS_THREADS) void stream_select_kernel(SelArgs a) {
    __shared__ int64_t red[32];
    if constexpr (PHASE == 0) {
        const int64_t s = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x;
        int64_t front = -1;
        bool conf = false;
        if (s < a.nslots) {
            const int64_t lo = s * SS_SLOT, hi = min(lo + SS_SLOT, a.lc);
            for (int64_t w = lo >> 5; w <= ((hi - 1) >> 5) && front < 0; ++w) {
                const uint32_t x = a.bitmap[w];
                const uint32_t prev = w > 0 ? a.bitmap[w - 1] >> 31 : 0u;
                uint32_t cand = x & ~((x << 1) | prev);                 // set bits whose predecessor is clear
                const int64_t base = w << 5;
                if (base < lo) cand &= ~0u << (int)(lo - base);
                if (base + 32 > hi) cand &= ~0u >> (int)(base + 32 - hi);
                while (cand) {
                    const int64_t i = base + (__ffs((int)cand) - 1);
                    cand &= cand - 1;
                    // previous crossing more than 300 back; none at all is the virtual crossing at -1
                    if (i >= 300 && stream_bits_clear(a.bitmap, i - 300, i)) { front = i; break; }
                }
            }
            if (front >= 0) {
                const int64_t j = front + 230;
                conf = j < a.lc && ((a.bitmap[j >> 5] >> (int)(j & 31)) & 1u);
            }
            a.slots[s] = front < 0 ? -1 : (front << 1) | (int64_t)conf;
        }
        int64_t c, m;
        stream_block_reduce((int64_t)conf, front, red, c, m);
        if (threadIdx.x == 0) { a.blk_cnt[blockIdx.x] = c; a.blk_max[blockIdx.x] = m; }
    } else if constexpr (PHASE == 1) {
        // one block: exclusive prefix of the blocks' counts in block order, the largest front, d_count
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int64_t carry = 0, mx = -1;
        for (int64_t b0 = 0; b0 < a.nblocks; b0 += SS_SCAN_THREADS) {
            const int64_t b = b0 + threadIdx.x;
            const int64_t v = b < a.nblocks ? a.blk_cnt[b] : 0;
            if (b < a.nblocks) mx = max(mx, a.blk_max[b]);
            int64_t inc = v;                                            // inclusive scan inside the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t u = __shfl_up(inc, o, 64);
                inc += lane >= o ? u : 0;
            }
            __syncthreads();
            if (lane == 63) red[wave] = inc;
            __syncthreads();
            int64_t before = 0, total = 0;
            for (int k = 0; k < SS_SCAN_THREADS / 64; ++k) { before += k < wave ? red[k] : 0; total += red[k]; }
            if (b < a.nblocks) a.blk_cnt[b] = carry + before + inc - v;
            carry += total;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (int64_t)__shfl_xor(mx, o, 64));
        __syncthreads();
        if (lane == 0) red[16 + wave] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < SS_SCAN_THREADS / 64; ++k) mx = max(mx, red[16 + k]);
            a.blk_max[0] = mx;
            a.count[0] = carry;
            a.count[1] = min(carry, a.max_packets);
        }
    } else {
        // ordered compaction: slot order is position order
        const int64_t s = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int64_t v = s < a.nslots ? a.slots[s] : -1;
        const bool conf = v >= 0 && (v & 1);
        const unsigned long long bal = __ballot(conf);
        if (lane == 0) red[wave] = __popcll(bal);
        __syncthreads();
        int64_t idx = a.blk_cnt[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; ++k) idx += red[k];
        if (conf && idx < a.max_packets) {
            const int64_t front = v >> 1, p = front + 11;              // len_RRC_rx + 1 (OFDM.c:758)
            ofdm_stream_packet *q = a.pk + idx;
            q->packet_pos = p;
            q->reserved = 0;
            q->r.flags = front == a.blk_max[0] ? OFDM_STREAM_LAST_FRONT : 0;   // the decode kernel adds the oob bit
        }
    }
}

// One wave per packet: ofdm_stream_decode.h's staging, filter and sync record, then ofdm_rxchain.h's stages -- the chain
// capture_rx_kernel runs from the matched filter on, so a packet's record is what that kernel gives for a window that
// contains it.
template <bool OUT>   // OUT: d_bits and / or d_eq are written
__global__ __launch_bounds__(64 * RXC_MAX_WAVES) void stream_decode_kernel(DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sdec_smem[];
    unsigned long long *acc = sdec_smem;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = blockDim.x >> 6;
    const int nd = a.n_data, nfr = 320 + 80 * nd, plane = a.plane, len = 2 * nfr + 19;
    float *re = reinterpret_cast<float *>(sdec_smem + RXC_ACC_WORDS) + (size_t)wave * a.wave_floats;
    float *im = re + plane;
    float *fre = re + 2 * plane, *fim = fre + nfr;
    if (threadIdx.x < RXC_ACC_WORDS) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t cnt = a.count[1];
    const int q = (int)((reinterpret_cast<uintptr_t>(a.x) >> 3) & 1u);     // sample s is 16-byte aligned when s + q is even
    for (int64_t i = (int64_t)blockIdx.x * W + wave; i < cnt; i += (int64_t)gridDim.x * W) {
        ofdm_stream_packet *pkt = a.pk + i;
        int64_t p;
        int last_front;
        sdec_packet(pkt, p, last_front);
        sdec_stage(a.x, a.n, p, q, len, lane, re, im);
        rxc_wave_sync();
        const bool oob = p + 2 * (int64_t)(nfr - 1) >= a.n + 20;       // the reference reads past its buffer
        // the first data symbol wholly past the end: the least d >= 0 with p + 2 (336 + 80 d) >= n + 20; D when none
        const int zfirst = (int)std::min<int64_t>(std::max<int64_t>((a.n - 652 - p + 159) / 160, 0), nd);
        sdec_filter(re, im, a.taps, nfr, lane, fre, fim);
        rxc_wave_sync();
        double fc, ff;
        rxc_cfo(fre, fim, lane, a.float_cfo, fc, ff);
        sdec_sync_record(&pkt->r, acc, a.counters != nullptr, lane, p, last_front, oob, fc, ff);
        rxc_rotate(fre, fim, lane, nd, fc, ff);
        rxc_wave_sync();
        const RxcQuad qd = rxc_quad(lane, nd);
        float2 x[64];
        rxc_window(fre, fim, qd.k0, x);
        SymState st;
        rxc_demap<OUT>(x, a.dtable, qd.dsc, re, lane, nd, st);
        if constexpr (OUT) rxc_outputs(re, lane, nd, i, a.eq, a.bits);
        float fe;
        uint32_t ferr, fax;
        rxc_totals(st, qd.dlane, nd, zfirst, a.ztable, fe, ferr, fax);
        rxc_record(&pkt->r, acc, a.counters != nullptr, lane, nd, fe, ferr, fax);
        rxc_wave_sync();                                             // the next packet overwrites the planes
    }
    rxc_flush(acc, a.counters);
}

// ofdm_receive_stream's body.  det (ofdm_stream_detect.h): another detection launch in place of stream_detect_kernel,
// with its own halo; everything after the bitmap -- selection, compaction, decode -- is the same launches either way.
int stream_receive(Ctx *c, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts, int payload,
                   int64_t max_packets, void *d_packets, void *d_count, void *d_bits, void *d_eq, void *d_counters,
                   void *d_metric, void *d_cross, const StreamDetector *det, const StreamRefiner *ref,
                   const StreamDecoder *dec) {
    const int halo = det ? det->halo : 47;
    if (!c) return set_error(OFDM_E_ARG, "ctx is NULL");
    if (!opts) return set_error(OFDM_E_ARG, "opts is NULL");
    if (n_samples < 0) return set_error(OFDM_E_ARG, "n_samples %lld is negative", (long long)n_samples);
    if (max_packets < 0) return set_error(OFDM_E_ARG, "max_packets %lld is negative", (long long)max_packets);
    if (payload != OFDM_PAYLOAD_MESSAGE && payload != OFDM_PAYLOAD_TESTER)
        return set_error(OFDM_E_ARG, "a stream is decoded against a fixed payload (MESSAGE or TESTER), got %d", payload);
    if (opts->word_stats) return set_error(OFDM_E_ARG, "word_stats is not available for a stream");
    if (!d_count) return set_error(OFDM_E_ARG, "d_count is required");
    if (!d_samples && n_samples > 0) return set_error(OFDM_E_ARG, "d_samples is required");
    if (!d_packets && max_packets > 0) return set_error(OFDM_E_ARG, "d_packets is required");
    if (reinterpret_cast<uintptr_t>(d_samples) & 7u) return set_error(OFDM_E_ARG, "d_samples must be 8-byte aligned");
    if (hipSetDevice(c->device) != hipSuccess) return set_error(OFDM_E_HIP, "hipSetDevice(%d) failed", c->device);
    if (n_samples <= halo) {                                         // no positions, no packets
        if (hipMemsetAsync(d_count, 0, 2 * sizeof(int64_t), c->stream) != hipSuccess)
            return set_error(OFDM_E_HIP, "hipMemsetAsync(d_count) failed");
        return OFDM_OK;
    }
    DecArgs da{};
    uint32_t table[3 * LONG_MAX_FRAMES];
    da.n_data = payload_table_long(payload, c->message, table);
    for (int d = 0; d < da.n_data; ++d) {
        demap_words(table + 3 * d, da.dtable + 4 * d);
        da.ztable[d] = zero_errors(table + 3 * d);
    }
    const int nfr = 320 + 80 * da.n_data;
    // the decode block's LDS, checked before anything is launched
    da.plane = (2 * nfr + 19 + 3) & ~3;
    da.wave_floats = (std::max(2 * da.plane + 2 * nfr, rxc_spec_floats(da.n_data)) + 3) & ~3;
    WaveBlock wb;
    if (wave_block(c, RXC_ACC_WORDS * sizeof(unsigned long long), (size_t)da.wave_floats * sizeof(float), SDEC_MAX_WAVES,
                   std::max<int64_t>(max_packets, 1), &wb))
        return OFDM_E_HIP;
    if (!wb.W)
        return set_error(OFDM_E_ARG, "a %d-symbol packet needs %zu bytes of LDS, above the %zu available", da.n_data,
                         wb.lds, wb.limit);
    const int W = wb.W;
    const size_t lds = wb.lds;

    // scratch: the crossing bitmap (whole 16-byte groups), the front slots, the selection blocks' counts and maxima
    const int64_t lc = n_samples - halo;
    const int64_t words = (lc + 31) / 32, tiles = (lc + SD_TILE - 1) / SD_TILE;
    const int64_t nslots = (lc + SS_SLOT - 1) / SS_SLOT, nblocks = (nslots + SS_THREADS - 1) / SS_THREADS;
    if (tiles > 0x7fffffffll || nblocks > 0x7fffffffll)
        return set_error(OFDM_E_ARG, "n_samples %lld is beyond one launch", (long long)n_samples);
    const size_t bm_bytes = (size_t)((words + 3) & ~(int64_t)3) * 4;
    const size_t total = bm_bytes + (size_t)(nslots + 2 * nblocks) * sizeof(int64_t);
    int rc = c->ensure(&c->d_scratch2, &c->cap_scratch2, total);
    if (rc) return rc;
    char *base = (char *)c->d_scratch2;
    if (ref && max_packets > 0 && (rc = ref->prepare(ref, c))) return rc;

    DetArgs ta{};
    ta.x = (const float2 *)d_samples;
    ta.n = n_samples;
    ta.lc = lc;
    ta.tiles = tiles;
    ta.words = words;
    ta.bitmap = (uint32_t *)base;
    ta.cross = (uint32_t *)d_cross;
    ta.metric = (float *)d_metric;
    SelArgs sa{};
    sa.bitmap = ta.bitmap;
    sa.lc = lc;
    sa.nslots = nslots;
    sa.nblocks = nblocks;
    sa.max_packets = max_packets;
    sa.slots = (int64_t *)(base + bm_bytes);
    sa.blk_cnt = sa.slots + nslots;
    sa.blk_max = sa.blk_cnt + nblocks;
    sa.count = (int64_t *)d_count;
    sa.pk = (ofdm_stream_packet *)d_packets;

    // one tile per block up to a grid the loop in the kernel wraps (the results do not depend on it)
    const dim3 dgrid((unsigned)std::min<int64_t>(tiles, 1 << 20));
    c->tic(det ? det->kernel : OFDM_K_STREAM_DETECT);
    if (det) det->launch(det, dgrid, c->stream, ta);
    else if (ta.metric) hipLaunchKernelGGL(stream_detect_kernel<true>, dgrid, dim3(SD_THREADS), 0, c->stream, ta);
    else hipLaunchKernelGGL(stream_detect_kernel<false>, dgrid, dim3(SD_THREADS), 0, c->stream, ta);
    c->toc();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return set_error(OFDM_E_HIP, "%s launch: %s", det ? det->name : "stream_detect_kernel", hipGetErrorString(e));
    c->tic(OFDM_K_STREAM_SELECT);
    hipLaunchKernelGGL(stream_select_kernel<0>, dim3((unsigned)nblocks), dim3(SS_THREADS), 0, c->stream, sa);
    hipLaunchKernelGGL(stream_select_kernel<1>, dim3(1), dim3(SS_SCAN_THREADS), 0, c->stream, sa);
    hipLaunchKernelGGL(stream_select_kernel<2>, dim3((unsigned)nblocks), dim3(SS_THREADS), 0, c->stream, sa);
    c->toc();
    e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "stream_select_kernel launch: %s", hipGetErrorString(e));
    if (max_packets == 0) return OFDM_OK;

    if (ref) {                                                       // between the selection and the decode
        RefineArgs ra{};
        ra.x = ta.x;
        ra.n = n_samples;
        ra.count = sa.count;
        ra.pk = sa.pk;
        ra.max_packets = max_packets;
        c->tic(ref->kernel);
        ref->launch(ref, c, c->stream, ra);
        c->toc();
        e = hipGetLastError();
        if (e != hipSuccess) return set_error(OFDM_E_HIP, "%s launch: %s", ref->name, hipGetErrorString(e));
    }

    da.x = ta.x;
    da.n = n_samples;
    da.count = sa.count;
    da.pk = sa.pk;
    da.bits = (uint32_t *)d_bits;
    da.eq = (float2 *)d_eq;
    da.counters = (unsigned long long *)d_counters;
    da.float_cfo = opts->float_cfo;
    rrc_design(da.taps);
    // the packet count stays on the device: enough blocks for max_packets, at most two per CU; the waves loop over d_count
    const int64_t blocks = (max_packets + W - 1) / W;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 2 * (int64_t)c->cus));
    if (dec) {                                                       // another decode kernel on the same arguments
        c->tic(dec->kernel);
        dec->launch(dec, grid, dim3(64 * W), lds, c->stream, da, table);
        c->toc();
        e = hipGetLastError();
        if (e != hipSuccess) return set_error(OFDM_E_HIP, "%s launch: %s", dec->name, hipGetErrorString(e));
        return OFDM_OK;
    }
    c->tic(OFDM_K_STREAM_DECODE);
    if (da.bits || da.eq) hipLaunchKernelGGL(stream_decode_kernel<true>, grid, dim3(64 * W), lds, c->stream, da);
    else hipLaunchKernelGGL(stream_decode_kernel<false>, grid, dim3(64 * W), lds, c->stream, da);
    c->toc();
    e = hipGetLastError();
    if (e != hipSuccess) return set_error(OFDM_E_HIP, "stream_decode_kernel launch: %s", hipGetErrorString(e));
    return OFDM_OK;
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_receive_stream(ofdm_ctx *ctx, const void *d_samples, int64_t n_samples, const ofdm_rx_opts *opts,
                                   int payload, int64_t max_packets, void *d_packets, void *d_count, void *d_bits,
                                   void *d_eq, void *d_counters, void *d_metric, void *d_cross) {
    return stream_receive(reinterpret_cast<Ctx *>(ctx), d_samples, n_samples, opts, payload, max_packets, d_packets,
                          d_count, d_bits, d_eq, d_counters, d_metric, d_cross, nullptr);
}
