// ofdm_stream_tile.h -- the parts of stream_detect_kernel's shape that the optional detection kernels share
// (ofdm_stream_conj.hip: stream_detect_conj_kernel and stream_detect_thr_kernel; ofdm_stream_div.hip:
// stream_detect_div_kernel): the tile's geometry, its staging, one position's decision and the tile's bitmap store.
// Every function is inlined into the kernel that calls it.
#pragma once
#include <algorithm>
#include "ofdm_mi355x_detect.h"
#include "ofdm_rxcommon.h"
#include "ofdm_stream_detect.h"

namespace ofdm {

constexpr int CD_RUN = OFDM_STREAM_RUN;
constexpr int CD_THREADS = 256;
constexpr int CD_TILE = OFDM_STREAM_TILE;
constexpr int CD_WORDS = CD_TILE / 32;
static_assert(CD_TILE == CD_RUN * CD_THREADS && CD_TILE % 128 == 0 && (CD_RUN & 1), "tile = 256 odd runs, whole 16-byte groups of bitmap words");

template <bool CONJ>
struct DetShape {
    static constexpr int LAG = CONJ ? 32 : 16;
    static constexpr int HALO = 31 + LAG;                              // a position reads [i, i + HALO]
    static constexpr int SAMPLES = CD_TILE + HALO;
    static constexpr int PLANE = (SAMPLES + 3) & ~3;
    static constexpr int LOADS = (SAMPLES / 2 + CD_THREADS - 1) / CD_THREADS;      // 16-byte loads per lane and tile
    static_assert((2 * PLANE + CD_WORDS) * 4 <= 64 * 1024, "static LDS");
};
static_assert(DetShape<true>::HALO == 63 && DetShape<false>::HALO == 47, "Lc = n - 63 and n - 47");
static_assert((2 * DetShape<true>::PLANE + CD_WORDS) * 4 == 64992, "two planes of 8,000 floats and 248 bitmap words");

// ---- the parts of stream_detect_kernel's shape the kernels share ----
// stage [t0, t0 + TILE + HALO) clipped to the stream; the rest of the planes and the bitmap zeroed
template <class S>
__device__ __forceinline__ void det_stage(const DetArgs &a, int64_t t0, int head, float *re, float *im, uint32_t *bm) {
    const int tid = threadIdx.x;
    const float2 *row = a.x + t0;
    const int cnt = (int)std::min<int64_t>(S::SAMPLES, a.n - t0);
    if (head && tid == 0) { const float2 v = row[0]; re[0] = v.x; im[0] = v.y; }
    const f4v *r4 = reinterpret_cast<const f4v *>(row + head);
    const int np = (cnt - head) >> 1;
    // every load of the tile is in flight before the first LDS write, as in stream_detect_kernel
    f4v v[S::LOADS];
#pragma unroll
    for (int j = 0; j < S::LOADS; ++j) {
        const int k = tid + j * CD_THREADS;
        if (k < np) v[j] = __builtin_nontemporal_load(r4 + k);
    }
#pragma unroll
    for (int j = 0; j < S::LOADS; ++j) {
        const int k = tid + j * CD_THREADS;
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
    for (int k = cnt + tid; k < S::PLANE; k += CD_THREADS) { re[k] = 0.f; im[k] = 0.f; }
    if (tid < CD_WORDS) bm[tid] = 0u;
}

// the tile's bitmap words: 16 bytes per lane into the scratch bitmap, and the caller's copy
__device__ __forceinline__ void det_store(const DetArgs &a, int64_t t0, const uint32_t *bm) {
    const int tid = threadIdx.x;
    const int64_t w0 = t0 >> 5;
    if (tid < CD_WORDS / 4 && w0 + 4 * tid < a.words)                  // the scratch bitmap is padded to whole groups
        reinterpret_cast<uint4 *>(a.bitmap + w0)[tid] = reinterpret_cast<const uint4 *>(bm)[tid];
    if (a.cross && tid < CD_WORDS && w0 + tid < a.words) a.cross[w0 + tid] = bm[tid];
}

// one position's decision and metric from its sums
template <bool METRIC>
__device__ __forceinline__ void det_decide(const DetArgs &a, int64_t t0, int n, float sx, float sy, float pw, float thr,
                                           uint32_t *bm) {
    const float num = fmaf(sx, sx, sy * sy), h = thr * pw;
    if (fmaf(h, pw, -num) < 0.f) atomicOr(&bm[n >> 5], 1u << (n & 31));             // |c|^2 / p^2 > thr
    if constexpr (METRIC) a.metric[t0 + n] = num / (pw * pw);
}

}  // namespace ofdm
