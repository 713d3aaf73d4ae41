// ofdm_ctx.h -- the opaque ofdm_ctx behind the C ABI (host-side state of one GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <string>
#include <vector>
#include "ofdm_mi355x_long.h"

namespace ofdm {

int set_error(int code, const char *fmt, ...);
int check_cfg(const ofdm_cfg *c);

constexpr int MSG_MAX_FRAMES = 8;           // data symbols per frame-mode frame (LDS budget)
constexpr int MSG_MAX_CHARS = 12 * MSG_MAX_FRAMES;
// payload words (MSB-first bits, 3 per data symbol) of the TESTER pattern or `message` padded with
// ' ' to whole symbols (Data_Generator, OFDM.c:435-465); returns the data symbols per frame
// (symbol mode's table: a message set through ofdm_set_long_message is cut at MSG_MAX_FRAMES symbols here, and the
// symbol-mode entry points refuse it first, check_symbol_payload)
int payload_table(int payload, const std::string &message, uint32_t table[3 * MSG_MAX_FRAMES]);
// long messages (include/ofdm_mi355x_long.h, frame mode only): up to 15 data symbols per frame, the largest frame
// whose matched-filter window (2,909 samples) fits the sync kernel's capture ring (2,973)
constexpr int LONG_MAX_FRAMES = OFDM_LONG_MAX_DATA_SYMBOLS;
constexpr int LONG_MSG_MAX_CHARS = OFDM_LONG_MSG_MAX_CHARS;
static_assert(LONG_MSG_MAX_CHARS == 12 * LONG_MAX_FRAMES, "12 characters per data symbol");
int payload_table_long(int payload, const std::string &message, uint32_t table[3 * LONG_MAX_FRAMES]);
// rcosdesign(0.5, 10, 2, 'sqrt') (Tester.m:112; OFDM.c:32 holds the same values as floats): the 21 RRC taps of frame
// mode, of the capture and stream receivers and of the packet and fading transmitters; symmetric to the bit (the sync
// kernels fold them)
void rrc_design(float out[21]);
// The errors of a data symbol that reaches the demapper as 64 exact zeros (its window lies wholly past the end of the
// samples; ofdm_rxchain.h rxc_totals): the reference's slicer decides "-" on both axes for a zero (Z > 0 fails,
// OFDM.c:858-866), the demapper then (1, 0) for every pair (OFDM.c:873-908), so the counts depend on the payload alone.
// w: the symbol's 96 payload bits, MSB first.  Returns bit errors | slicer axis errors << 16.
uint32_t zero_errors(const uint32_t w[3]);
struct Ctx;
constexpr size_t LDS_PER_CU = 160 * 1024;
// A block of one wave per item (capture, packet) in dynamic LDS: `head` bytes for the block and `per_wave` for each
// wave, against `limit`, the smaller of the device's limit per block and LDS_PER_CU.  W = min(max_waves, what fits,
// items) waves and their request `lds`; W = 0 when not even one wave fits (lds is then what one needs: the caller
// words that error).  Returns non-zero (OFDM_E_HIP, the error text set) when the device cannot be asked.
struct WaveBlock { int W; size_t lds, limit; };
int wave_block(const Ctx *c, size_t head, size_t per_wave, int max_waves, int64_t items, WaveBlock *out);
// OFDM_E_ARG when `payload` is MESSAGE and the message set has more than MSG_MAX_FRAMES symbols (symbol mode)
int check_symbol_payload(const Ctx *c, int payload);

struct Ctx {
    // 4..6: the stream receiver's kernels (OFDM_K_STREAM_* of ofdm_mi355x_stream.h), 7: the packet transmitter
    // (OFDM_K_TRANSMIT of ofdm_mi355x_tx.h), 8, 9: the channel and the scoring (OFDM_K_CHANNEL, OFDM_K_SCORE of
    // ofdm_mi355x_channel.h), 10, 11: the fading transmitter and its tap generator (OFDM_K_FADE, OFDM_K_DRAW_TAPS of
    // ofdm_mi355x_fading.h), 12: the stream receiver's conjugate-correlation detector (OFDM_K_STREAM_DETECT_CONJ of
    // ofdm_mi355x_detect.h), 13: its fine timing kernel (OFDM_K_STREAM_TIMING of ofdm_mi355x_timing.h), 14: its pilot-tracking
    // decode (OFDM_K_STREAM_DECODE_TRACK of ofdm_mi355x_track.h), 15..17: the diversity receiver's detection, timing and
    // decode (OFDM_K_STREAM_*_DIV of ofdm_mi355x_diversity.h), 18..20: the coded link's encoder, gains and Viterbi
    // decoder (OFDM_K_CODE_ENCODE, OFDM_K_STREAM_CSI, OFDM_K_CODE_DECODE of ofdm_mi355x_code.h), added at the tail
    enum { K_FFT = 0, K_TX = 1, K_RX = 2, K_FRAME = 3, K_STREAM_DETECT = 4, K_STREAM_SELECT = 5, K_STREAM_DECODE = 6,
           K_TRANSMIT = 7, K_CHANNEL = 8, K_SCORE = 9, K_FADE = 10, K_DRAW_TAPS = 11, K_STREAM_DETECT_CONJ = 12,
           K_STREAM_TIMING = 13, K_STREAM_DECODE_TRACK = 14, K_STREAM_DETECT_DIV = 15, K_STREAM_TIMING_DIV = 16,
           K_STREAM_DECODE_DIV = 17, K_CODE_ENCODE = 18, K_STREAM_CSI = 19, K_CODE_DECODE = 20, NK = 21 };
    int device = 0;
    int cus = 256;
    hipStream_t own = nullptr;       // created by the context
    hipStream_t stream = nullptr;    // where work is enqueued (own or external)
    float2 *d_ltf[2] = {nullptr, nullptr};
    float2 *d_ltf2_rows[2] = {nullptr, nullptr};   // LS staging column: [68][2] 2T[(r - 4) mod 64]
    std::string message = "Hey! I am Vivaswan";   // MESSAGE payload (OFDM.c:20), ofdm_set_message
    // sweep scratch (grown on demand, freed with the context)
    void *d_tx = nullptr, *d_bits = nullptr, *d_cnt = nullptr, *d_scratch = nullptr, *d_scratch2 = nullptr;
    // ofdm_symbol_sweep's pipeline: the second Tx batch and the stream the next chunk's Tx runs on
    void *d_tx2 = nullptr, *d_bits2 = nullptr;
    size_t cap_tx2 = 0, cap_bits2 = 0;
    hipStream_t tx_stream = nullptr;
    // ofdm_set_next_tx: a Tx batch the next ofdm_rx_frames call builds (fused into the packed receiver)
    bool nx_pending = false;
    ofdm_cfg nx_cfg{};
    uint64_t nx_first = 0;
    int64_t nx_n = 0;
    void *nx_tx = nullptr, *nx_bits = nullptr;
    hipEvent_t ev_start = nullptr, ev_tx[2] = {nullptr, nullptr}, ev_rx[2] = {nullptr, nullptr};
    void *d_wave = nullptr;
    void *d_work = nullptr;          // K3c's work-item counter (one receiver launch in flight per context)
    // K3c's table of lane-independent Philox words (pack_philox_table): a function of the seed and of the high word
    // of the launch's first frame, so it is uploaded again only when one of them (or the stream) changes
    void *d_philox = nullptr;
    bool philox_valid = false;
    uint32_t philox_key[3] = {0, 0, 0};
    hipStream_t philox_stream = nullptr;
    uint32_t h_philox[2 * 48 * 4] = {};
    // pinned host staging for the sweeps' counter read-back (a pageable destination costs HIP a staging copy kernel
    // and a host round trip per call); grown on demand, freed with the context
    void *h_cnt = nullptr;
    size_t cap_h_cnt = 0;
    size_t cap_tx = 0, cap_bits = 0, cap_cnt = 0, cap_scratch = 0, cap_scratch2 = 0, cap_wave = 0;
    // frame-mode waveform cache (per conv/payload/message)
    int wave_key = -1;
    int wave_frames = 0;
    int32_t wave_len = 0;
    double wave_power = 0.0;
    // the fine timing templates (ofdm_stream_timing.hip): w[394 .. 522) of Transmitter()'s waveform under
    // OFDM_CONV_C [0] and OFDM_CONV_MATLAB [1], each built on its first use
    bool ltf_ready[2] = {false, false};
    float2 ltf_template[2][128] = {};
    // kernel timing
    struct Ev { hipEvent_t a, b; int kernel; };
    bool timing = false;
    std::vector<Ev> open, done;
    std::vector<hipEvent_t> pool;
    double acc_ms[NK] = {};
    int64_t launches[NK] = {};

    void tic(int k);
    void toc();
    void resolve();
    int ensure(void **p, size_t *cap, size_t bytes);
    // d_cnt[0, bytes) -> host `out` on `stream` through the pinned staging buffer; returns after the copy has landed
    int read_counters(void *out, size_t bytes);
};

}  // namespace ofdm
