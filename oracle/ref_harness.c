/*
 * oracle/ref_harness.c -- TEST INFRASTRUCTURE ONLY (never shipped, never measured as the product).
 *
 * Builds the UNMODIFIED reference translation unit /root/reference/src/OFDM.c into a shared
 * library (oracle/_ref/libofdm_ref.so) so tests and bench.py's cpu_baseline leg can call the
 * reference's own stage functions.  Nothing is copied: the reference source is #included from
 * where it lies (path given by -DREF_OFDM_C=...).  Two hooks only:
 *   - `main`  -> `ofdm_reference_main`   (OFDM.c:1187, so the library has no entry point)
 *   - `rand`  -> `ref_hook_rand`         (OFDM.c:626-627 Box-Muller draws, OFDM.c:949 capture
 *                                         offset) so runs are reproducible and scriptable.
 * RAND_MAX stays glibc's 2^31-1 (OFDM.c:626 divides by it).
 *
 * Exported entry points are prefixed `ref_`; see oracle/ref.py for the Python side.
 */
#include <stdio.h>
#include <stdlib.h>
#include <complex.h>
#include <math.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <fcntl.h>

int ref_hook_rand(void);

#define rand ref_hook_rand
#define main ofdm_reference_main
#include REF_OFDM_C
#undef rand
#undef main

/* ------------------------------------------------------------------ rand hook */
static unsigned long long g_lcg = 0x80211AULL;
static const int *g_script = NULL;
static int g_script_n = 0, g_script_pos = 0;
static long long g_rand_calls = 0;

int ref_hook_rand(void)
{
    g_rand_calls++;
    if (g_script && g_script_pos < g_script_n)
        return g_script[g_script_pos++];
    /* 64-bit LCG (Knuth MMIX constants); top 31 bits -> [0, RAND_MAX] */
    g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL;
    return (int)(g_lcg >> 33);
}

void ref_seed(unsigned long long s) { g_lcg = s; g_script = NULL; g_script_n = g_script_pos = 0; }
void ref_script(const int *vals, int n) { g_script = vals; g_script_n = n; g_script_pos = 0; }
long long ref_rand_calls(void) { return g_rand_calls; }

/* ------------------------------------------------------------------ stdout silencer */
static int g_saved_fd = -1;
static void quiet_begin(void)
{
    fflush(stdout);
    g_saved_fd = dup(1);
    int devnull = open("/dev/null", O_WRONLY);
    if (devnull >= 0) { dup2(devnull, 1); close(devnull); }
}
static void quiet_end(void)
{
    fflush(stdout);
    if (g_saved_fd >= 0) { dup2(g_saved_fd, 1); close(g_saved_fd); g_saved_fd = -1; }
}

/* ------------------------------------------------------------------ transmitter (once) */
static float complex *g_tx = NULL;      /* the current frame's waveform: every ref_* entry below reads this one */
static float complex *g_tx_main = NULL; /* Transmitter()'s own output for message[] (OFDM.c:20), kept for comparison */
static int g_tx_main_len = 0;

/* Transmitter() mutates globals and leaks on re-entry (OFDM.c:467-618): call it exactly once. */
int ref_init(void)
{
    if (!g_tx) {
        quiet_begin();
        g_tx_main = g_tx = Transmitter();
        g_tx_main_len = len_Tx_Signal_repeated;
        quiet_end();
    }
    return len_Tx_Signal_repeated;
}

/* Transmitter()'s own waveform of the compiled-in message, whatever ref_set_message did since. */
int ref_tx_main_copy(float *out, int max_complex)
{
    ref_init();
    int n = g_tx_main_len < max_complex ? g_tx_main_len : max_complex;
    memcpy(out, g_tx_main, (size_t)n * sizeof(float complex));
    return n;
}

/*
 * The frame of another message (the message is a compile-time array in OFDM.c:20 and Transmitter() cannot run
 * twice), built from the reference's own stage functions in the order Transmitter() calls them: characters to bits
 * (Decimal_To_Binary, blanks up to a whole symbol), QPSK_Modulator, the subcarrier map with the four pilots
 * (Slice_Repeater), ifft, cyclic prefix, the two preambles (Preamble_Generator over the IEEE 802.11a short and long
 * training tones, as oracle/ofdm_oracle.c preamble_tones states them), 2x zero-stuffing, Convolution with
 * RRC_Filter_Tx, ten periods.  The globals Receiver() reads -- Data, Data_Payload_Mod, data_frames_number,
 * Data_Frame_Size, len_Tx_Signal_repeated -- and g_tx are replaced, so ref_trial / ref_time_trials / ref_mc_trials /
 * ref_receiver / ref_receiver_stages / ref_tx_copy / ref_globals / ref_init all see the new frame.  For the compiled-in
 * message the result equals Transmitter()'s output bit for bit (tests/test_ref_long.py).  Returns the new
 * len_Tx_Signal_repeated, or -1 for an empty message.
 */
int ref_set_message(const unsigned char *msg, int n)
{
    if (!msg || n < 1) return -1;
    ref_init();
    quiet_begin();
    if (Data_Payload_Mod) Deallocate_Array_2D(Data_Payload_Mod, data_frames_number);
    free(Data);
    if (g_tx != g_tx_main) free(g_tx);

    const int nf = (int)ceil(8 * n / 96.0);
    data_frames_number = nf;
    Data = Allocate_Array_1D(nf * 96);
    int eight[8];
    for (int c = 0; c < nf * 12; ++c) {
        Decimal_To_Binary(c < n ? msg[c] : ' ', eight);
        for (int b = 0; b < 8; ++b) Data[c * 8 + b] = eight[b];
    }
    float complex **payload = Allocate_Array_2D(nf, 96);
    for (int d = 0; d < nf; ++d) Slice_Repeater(Data, payload[d], 0, 96 * d, 96 * d + 96, 1);
    Data_Payload_Mod = Allocate_Array_2D(nf, 48);
    QPSK_Modulator(payload, Data_Payload_Mod, nf);
    Deallocate_Array_2D(payload, nf);

    static const signed char s_pat[53] = {0,0,1,0,0,0,-1,0,0,0,1,0,0,0,-1,0,0,0,-1,0,0,0,1,0,0,0,0,0,0,0,
                                           -1,0,0,0,-1,0,0,0,1,0,0,0,1,0,0,0,1,0,0,0,1,0,0};
    static const signed char l_pat[53] = {1,1,-1,-1,1,1,-1,1,-1,1,1,1,1,1,1,-1,-1,1,1,-1,1,-1,1,1,1,1,0,
                                           1,-1,-1,1,1,-1,1,-1,1,-1,-1,-1,-1,-1,1,1,-1,-1,1,-1,1,-1,1,1,1,1};
    /* 54 entries: Preamble_Generator copies P_k[0..54) (OFDM.c:381) and overwrites the last with a guard tone */
    float complex tones_s[54] = {0}, tones_l[54] = {0}, guard[11] = {0}, stf[160], ltf[160];
    for (int i = 0; i < 53; ++i) { tones_s[i] = s_pat[i] * (1 + 1 * I); tones_l[i] = l_pat[i]; }
    float scale = sqrt(13.0 / 6.0);
    Preamble_Generator(scale, tones_s, guard, stf, 0);
    Preamble_Generator(1, tones_l, guard, ltf, 1);          /* also rewrites Long_preamble_slot_Frequency: same values */

    Data_Frame_Size = nf * 80 + 320;
    float complex *frame = Allocate_Array_1D(Data_Frame_Size);
    Slice_Repeater(stf, frame, 0, 0, 160, 1);
    Slice_Repeater(ltf, frame, 160, 0, 160, 1);
    const int pilot[4] = {1, 1, 1, -1};
    for (int d = 0; d < nf; ++d) {
        float complex X[N_FFT] = {0}, x[N_FFT];
        float complex *q = Data_Payload_Mod[d];
        Slice_Repeater(q, X, 6, 0, 5, 1);    X[11] = pilot[0];
        Slice_Repeater(q, X, 12, 5, 18, 1);  X[25] = pilot[1];
        Slice_Repeater(q, X, 26, 18, 24, 1);
        Slice_Repeater(q, X, 33, 24, 30, 1); X[39] = pilot[2];
        Slice_Repeater(q, X, 40, 30, 43, 1); X[53] = pilot[3];
        Slice_Repeater(q, X, 54, 43, 48, 1);
        ifft(X, x, N_FFT);
        Slice_Repeater(x, frame, 320 + 80 * d, 48, 64, 1);
        Slice_Repeater(x, frame, 336 + 80 * d, 0, 64, 1);
    }
    const int n_over = 2 * Data_Frame_Size, n_period = n_over + len_RRC_Coeff - 1;
    float complex *over = Allocate_Array_1D(n_over);
    for (int i = 0; i < Data_Frame_Size; ++i) { over[2 * i] = frame[i]; over[2 * i + 1] = 0; }
    free(frame);
    float complex *period = Convolution(over, RRC_Filter_Tx, n_over, len_RRC_Coeff);
    free(over);
    len_Tx_Signal_repeated = 10 * n_period;
    g_tx = Allocate_Array_1D(len_Tx_Signal_repeated);
    Slice_Repeater(period, g_tx, 0, 0, n_period, 10);
    free(period);
    quiet_end();
    return len_Tx_Signal_repeated;
}

int ref_tx_copy(float *out, int max_complex)
{
    int n = ref_init();
    if (n > max_complex) n = max_complex;
    memcpy(out, g_tx, (size_t)n * sizeof(float complex));
    return n;
}

/* Data (OFDM.c:28, 96 bits per data symbol as float complex), Data_Payload_Mod (OFDM.c:30, 48 per data symbol),
 * Long_preamble_slot_Frequency (OFDM.c:34), data_frames_number, Data_Frame_Size: the caller sizes bits and
 * payload_mod for the current frame (dims alone first). */
void ref_globals(float *bits, float *payload_mod, float *ltf_freq, int *dims)
{
    ref_init();
    int nb = data_frames_number * 96;
    for (int i = 0; i < nb && bits; ++i) bits[i] = crealf(Data[i]);
    for (int f = 0; f < data_frames_number && payload_mod; ++f)
        for (int j = 0; j < 48; ++j) {
            payload_mod[(f * 48 + j) * 2 + 0] = crealf(Data_Payload_Mod[f][j]);
            payload_mod[(f * 48 + j) * 2 + 1] = cimagf(Data_Payload_Mod[f][j]);
        }
    for (int i = 0; i < N_FFT && ltf_freq; ++i) {
        ltf_freq[2 * i] = crealf(Long_preamble_slot_Frequency[i]);
        ltf_freq[2 * i + 1] = cimagf(Long_preamble_slot_Frequency[i]);
    }
    if (dims) { dims[0] = data_frames_number; dims[1] = Data_Frame_Size; dims[2] = len_Tx_Signal_repeated; }
}

void ref_rrc_taps(float *out21)
{
    for (int i = 0; i < 21; ++i) out21[i] = crealf(RRC_Filter_Tx[i]);
}

/* ------------------------------------------------------------------ FFT utilities */
void ref_fft(const float *in, float *out, int n)
{
    float complex x[256], y[256];
    memcpy(x, in, (size_t)n * sizeof(float complex));
    fft(x, y, n);
    memcpy(out, y, (size_t)n * sizeof(float complex));
}

void ref_ifft(const float *in, float *out, int n)
{
    float complex x[256], y[256];
    memcpy(x, in, (size_t)n * sizeof(float complex)); /* ifft mutates its input (OFDM.c:322) */
    ifft(x, y, n);
    memcpy(out, y, (size_t)n * sizeof(float complex));
}

/* Time n_transforms 64-point fft() (inverse 0) or ifft() (inverse 1) calls of the reference (OFDM.c:282-339) over
 * a buffer of distinct input vectors (CPU baseline of bench.py --workload fft64).  Returns wall seconds; *check
 * gets a sum of the outputs (keeps the work observable). */
double ref_time_fft(const float *in, int n_vectors, int n_transforms, int inverse, double *check)
{
    struct timespec t0, t1;
    float complex x[64], y[64];
    double acc = 0.0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int t = 0; t < n_transforms; ++t) {
        memcpy(x, in + (size_t)(t % n_vectors) * 128, sizeof x);   /* ifft mutates its input (OFDM.c:322) */
        if (inverse) ifft(x, y, 64); else fft(x, y, 64);
        acc += crealf(y[t & 63]);
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (check) *check = acc;
    return (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
}

void ref_convolution(const float *in, int n, float *out)
{
    quiet_begin();
    float complex *o = Convolution((float complex *)in, RRC_Filter_Tx, n, len_RRC_Coeff);
    quiet_end();
    memcpy(out, o, (size_t)(n + len_RRC_Coeff - 1) * sizeof(float complex));
    free(o);
}

/* ------------------------------------------------------------------ channel + receiver */
void ref_toa(const float *tx, float *out, float snr_db, int len)
{
    Transmission_Over_Air((float complex *)tx, (float complex *)out, snr_db, len);
}

void ref_receiver(const float *ota, int len, float *res3)
{
    ref_init();
    quiet_begin();
    Receiver((float complex *)ota, len, data_frames_number, res3);
    quiet_end();
}

/* One reference trial exactly as main() runs it per SNR point (OFDM.c:1206-1217). */
void ref_trial(float snr_db, float *res3)
{
    int n = ref_init();
    float complex *ota = Allocate_Array_1D(n);
    Transmission_Over_Air(g_tx, ota, snr_db, n);
    quiet_begin();
    Receiver(ota, n, data_frames_number, res3);
    quiet_end();
    free(ota);
}

/* Time n_trials reference trials (CPU baseline).  Returns wall seconds; res_sum gets Σ Res. */
double ref_time_trials(float snr_db, int n_trials, double *res_sum3)
{
    int n = ref_init();
    struct timespec t0, t1;
    float res[3];
    double acc[3] = {0, 0, 0};
    float complex *ota = Allocate_Array_1D(n);
    quiet_begin();
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int t = 0; t < n_trials; ++t) {
        Transmission_Over_Air(g_tx, ota, snr_db, n);
        Receiver(ota, n, data_frames_number, res);
        acc[0] += res[0]; acc[1] += res[1]; acc[2] += res[2];
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    quiet_end();
    free(ota);
    if (res_sum3) { res_sum3[0] = acc[0]; res_sum3[1] = acc[1]; res_sum3[2] = acc[2]; }
    return (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
}

/* The same trial loop with per-trial statistics for the Monte-Carlo fixture (tests/golden/gen_golden.py):
 * acc8 = {Σ EVM_dB, Σ EVM_AGC_dB, Σ BER, Σ BER², trials with BER > 0, trials with BER >= 1/4,
 *         Σ EVM_dB², trials with finite EVM_AGC_dB}.  The second moment gives the frame-clustered
 * sampling error of the mean BER (a failed sync costs ~half of a trial's 192 bits at once). */
double ref_mc_trials(float snr_db, int n_trials, double *acc8)
{
    int n = ref_init();
    struct timespec t0, t1;
    float res[3];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float complex *ota = Allocate_Array_1D(n);
    quiet_begin();
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int t = 0; t < n_trials; ++t) {
        Transmission_Over_Air(g_tx, ota, snr_db, n);
        Receiver(ota, n, data_frames_number, res);
        acc[0] += res[0]; acc[1] += res[1]; acc[2] += res[2];
        acc[3] += (double)res[2] * res[2];
        acc[4] += res[2] > 0; acc[5] += res[2] >= 0.25f;
        acc[6] += (double)res[0] * res[0];
        acc[7] += isfinite(res[1]) != 0;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    quiet_end();
    free(ota);
    if (acc8) memcpy(acc8, acc, sizeof(acc));
    return (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
}

/*
 * Receiver() with its intermediate values exposed.  The orchestration below follows
 * Receiver() (OFDM.c:941-1165) statement for statement and calls the reference's own stage
 * functions, so the result must equal ref_receiver() bit for bit (tested).  The capture offset
 * is passed in instead of drawn (OFDM.c:949).  Any output pointer may be NULL.
 *   corr      [len_corr]      real part of Corr_Out (OFDM.c:972)
 *   rx_frame  [fsz*2]         down-sampled frame (OFDM.c:992-996), fsz = Data_Frame_Size (480 for 2 symbols)
 *   coarse    [fsz*2]         after coarse CFO (OFDM.c:1004)
 *   fine      [fsz*2]         after fine CFO (OFDM.c:1012)
 *   H         [64*2]          channel estimate (OFDM.c:1020)
 *   Yf        [nf*64*2]       data FFT outputs (OFDM.c:1039)
 *   nopilot   [nf*48*2]       equalised data subcarriers (OFDM.c:1059-1069)
 *   bits      [nf*96]         demodulated bits (OFDM.c:1083-1100)
 *   res3      EVM_dB, EVM_AGC_dB, BER (OFDM.c:1163-1165)
 *   ints      [0]=packet_idx [1]=len_corr [2]=len_filtered
 */
void ref_receiver_stages(const float *ota_in, int len_Tx_Signal, int rx_start,
                         float *corr, float *rxf, float *coarse, float *fine, float *H,
                         float *Yf, float *nopilot, float *bits, float *res3, int *ints)
{
    ref_init();
    float complex *Tx_OTA_signal = (float complex *)ota_in;
    int nf = data_frames_number;
    quiet_begin();

    int len_Rx_Signal = len_Tx_Signal * 0.307;
    float complex *Rx_Signal = Allocate_Array_1D(len_Rx_Signal);
    Slice_Repeater(Tx_OTA_signal, Rx_Signal, 0, rx_start, rx_start + len_Rx_Signal, 1);
    int len_out_sig = len_Rx_Signal + len_RRC_Coeff - 1;
    float complex *Rx_filter_signal = Convolution(Rx_Signal, RRC_Filter_Tx, len_Rx_Signal, len_RRC_Coeff);

    int len_Corr_Out = 0;
    float complex *Corr_Out = Packet_Detection(Rx_Signal, len_Rx_Signal, &len_Corr_Out);
    free(Rx_Signal);
    if (corr) for (int i = 0; i < len_Corr_Out; ++i) corr[i] = crealf(Corr_Out[i]);
    int packet_idx = Packet_Selection(Corr_Out, len_Corr_Out);
    free(Corr_Out);

    int oversampling_rate = 2;
    int rx_frame_size = ((oversampling_rate * Data_Frame_Size + packet_idx - 1) - packet_idx) / oversampling_rate + 1;
    float complex *rx_frame = Allocate_Array_1D(rx_frame_size);
    /* The reference reads past the filtered buffer when packet_idx is late (UB); mirror the
     * in-bounds behaviour and zero-fill beyond it (flagged in ints[3]). */
    int index = 0, oob = 0;
    for (int i = packet_idx; i < oversampling_rate * Data_Frame_Size + packet_idx - 1; i += oversampling_rate) {
        if (i < len_out_sig) rx_frame[index] = Rx_filter_signal[i];
        else { rx_frame[index] = 0; oob = 1; }
        index += 1;
    }
    free(Rx_filter_signal);
    if (rxf) memcpy(rxf, rx_frame, (size_t)rx_frame_size * sizeof(float complex));

    float complex *rx_frame_after_coarse = Allocate_Array_1D(rx_frame_size);
    Coarse_CFO_Estimation(rx_frame, rx_frame_after_coarse, rx_frame_size);
    free(rx_frame);
    if (coarse) memcpy(coarse, rx_frame_after_coarse, (size_t)rx_frame_size * sizeof(float complex));

    float complex *rx_frame_after_fine = Allocate_Array_1D(rx_frame_size);
    Fine_CFO_Estimation(rx_frame_after_coarse, rx_frame_after_fine, rx_frame_size);
    free(rx_frame_after_coarse);
    if (fine) memcpy(fine, rx_frame_after_fine, (size_t)rx_frame_size * sizeof(float complex));

    float complex *H_est = Allocate_Array_1D(64);
    Channel_Estimation(rx_frame_after_fine, H_est, rx_frame_size);
    if (H) memcpy(H, H_est, 64 * sizeof(float complex));

    float complex **Rx_Payload_Time = Allocate_Array_2D(nf, N_FFT);
    for (int i = 0; i < nf; ++i)
        Slice_Repeater(rx_frame_after_fine, Rx_Payload_Time[i], 0, 320 + i * 80 + 16, 320 + (i + 1) * 80, 1);
    free(rx_frame_after_fine);
    float complex **Rx_Payload_Frequency = Allocate_Array_2D(nf, N_FFT);
    for (int i = 0; i < nf; ++i) fft(Rx_Payload_Time[i], Rx_Payload_Frequency[i], N_FFT);
    Deallocate_Array_2D(Rx_Payload_Time, nf);
    if (Yf) for (int i = 0; i < nf; ++i) memcpy(Yf + i * 128, Rx_Payload_Frequency[i], 64 * sizeof(float complex));

    float complex **Eq = Allocate_Array_2D(nf, N_FFT);
    for (int i = 0; i < nf; ++i)
        for (int j = 0; j < N_FFT; ++j) Eq[i][j] = Rx_Payload_Frequency[i][j] / H_est[j];
    free(H_est);
    Deallocate_Array_2D(Rx_Payload_Frequency, nf);

    float complex **NoPilot = Allocate_Array_2D(nf, 48);
    for (int i = 0; i < nf; ++i) {
        Slice_Repeater(Eq[i], NoPilot[i], 0, 6, 11, 1);
        Slice_Repeater(Eq[i], NoPilot[i], 5, 12, 25, 1);
        Slice_Repeater(Eq[i], NoPilot[i], 18, 26, 32, 1);
        Slice_Repeater(Eq[i], NoPilot[i], 24, 33, 39, 1);
        Slice_Repeater(Eq[i], NoPilot[i], 30, 40, 53, 1);
        Slice_Repeater(Eq[i], NoPilot[i], 43, 54, 59, 1);
    }
    Deallocate_Array_2D(Eq, nf);
    if (nopilot) for (int i = 0; i < nf; ++i) memcpy(nopilot + i * 96, NoPilot[i], 48 * sizeof(float complex));

    float complex **Final = Allocate_Array_2D(nf, 48);
    AGC_Receiver(NoPilot, Final);
    float complex **Demod = Allocate_Array_2D(nf, 96);
    QPSK_Demodulator(Final, Demod, nf);
    if (bits) for (int i = 0; i < nf; ++i) for (int j = 0; j < 96; ++j) bits[i * 96 + j] = crealf(Demod[i][j]);

    /* EVM / BER exactly as OFDM.c:1104-1161 */
    float error_square_sum = 0, data_payload_square_sum = 0;
    float complex error;
    for (int i = 0; i < nf; ++i) for (int j = 0; j < 48; ++j) {
        error = NoPilot[i][j] - Data_Payload_Mod[i][j];
        error_square_sum += pow(cabs(error), 2);
        data_payload_square_sum += pow(cabs(Data_Payload_Mod[i][j]), 2);
    }
    float evm = sqrt(error_square_sum / (nf * 48)) / sqrt(data_payload_square_sum / (nf * 48));
    float evm_dB = 20 * log10(evm);
    error_square_sum = 0; data_payload_square_sum = 0;
    for (int i = 0; i < nf; ++i) for (int j = 0; j < 48; ++j) {
        error = Final[i][j] - Data_Payload_Mod[i][j];
        error_square_sum += pow(cabs(error), 2);
        data_payload_square_sum += pow(cabs(Data_Payload_Mod[i][j]), 2);
    }
    float evm_AGC = sqrt(error_square_sum / (nf * 48)) / sqrt(data_payload_square_sum / (nf * 48));
    float evm_AGC_dB = 20 * log10(evm_AGC);
    float sum = 0;
    int total_bits = nf * 96;
    for (int i = 0; i < nf; ++i) for (int j = 0; j < 96; ++j)
        sum += abs(creal(Data[i * 96 + j]) - creal(Demod[i][j]));
    if (res3) { res3[0] = evm_dB; res3[1] = evm_AGC_dB; res3[2] = sum / total_bits; }
    Deallocate_Array_2D(NoPilot, nf);
    Deallocate_Array_2D(Final, nf);
    Deallocate_Array_2D(Demod, nf);
    quiet_end();
    if (ints) { ints[0] = packet_idx; ints[1] = len_Corr_Out; ints[2] = len_out_sig; ints[3] = oob; }
}

/* Individual stage access for fine-grained fixtures. */
void ref_packet_detection(const float *rx, int len, float *corr_out, int *len_out)
{
    float complex *c = Packet_Detection((float complex *)rx, len, len_out);
    for (int i = 0; i < *len_out; ++i) corr_out[i] = crealf(c[i]);
    free(c);
}

int ref_packet_selection(const float *corr_real, int len)
{
    float complex *c = Allocate_Array_1D(len);
    for (int i = 0; i < len; ++i) c[i] = corr_real[i];
    int p = Packet_Selection(c, len);
    free(c);
    return p;
}

void ref_channel_estimation(const float *frame480, float *H64)
{
    ref_init();
    float complex tmp[480];
    memcpy(tmp, frame480, sizeof(tmp));
    Channel_Estimation(tmp, (float complex *)H64, 480);
}

void ref_gaussian_noise(int n, float *out)
{
    for (int i = 0; i < n; ++i) out[i] = gaussian_noise(0, 1);
}

/*
 * CPU baseline for the symbol-mode workloads (bench.py cpu_baseline, configs c2/c3/c4/c5): the
 * genie-timed symbol chain of the GPU sweep composed from the reference's OWN stage functions,
 * timed on this host.  Per frame the Tx is built once (QPSK_Modulator OFDM.c:415-433, subcarrier
 * map as Transmitter OFDM.c:523-548, ifft OFDM.c:320-339, CP OFDM.c:559-565) and re-used for every
 * SNR point, as the GPU sweep re-uses its Tx batch.  Per SNR point: real-only noise from the
 * reference's gaussian_noise (OFDM.c:622-632, 651) on the samples the receiver reads (LTF pair +
 * 2 data windows), Channel_Estimation (OFDM.c:830-850), fft + ZF + demap (Receiver's inline loops
 * OFDM.c:1024-1069, restated), AGC_Receiver (852-871), QPSK_Demodulator (873-908), EVM and BER
 * sums (1104-1161, restated).  Noise var = kappa P_ref / 10^(snr/10).
 * flags bit 0 (config c5, no reference counterpart, D9): a 4-tap CN(0, 1/4) channel per frame
 * (restated) ahead of the same real-only noise.
 * flags bit 1 (config c2, ideal CSI): the known channel instead of the LTF estimate -- H is taken once
 * from Channel_Estimation of the noiseless frame (AWGN: the exact channel of the fft(ifft()) pair) and
 * the per-SNR Channel_Estimation is skipped, as the GPU's ideal-CSI receiver skips it.
 * flags bit 2 (fixture statistics, tests/golden/gen_golden.py --only chain): acc is double[5] and also gets
 * acc[3] += sum over (frame, SNR) of (bit errors of the frame)^2, acc[4] += frames with a bit error, the
 * frame-clustered variance of the BER estimate.
 * acc3 += {bit errors, bits, sum |z - d|^2}.  Returns wall seconds.
 */
static unsigned long long g_bits_state = 0x9E3779B97F4A7C15ULL;
static unsigned int bits_next(void)
{
    g_bits_state ^= g_bits_state << 13; g_bits_state ^= g_bits_state >> 7; g_bits_state ^= g_bits_state << 17;
    return (unsigned int)(g_bits_state >> 11);
}
/* payload bits of independent fixture jobs: any non-zero state */
void ref_seed_bits(unsigned long long s) { g_bits_state = s ? s : 0x9E3779B97F4A7C15ULL; }

double ref_time_symbol_chain(const float *snr_db, int n_snr, int n_frames, int flags, double *acc3)
{
    ref_init();
    const int rayleigh = flags & 1, ideal = (flags >> 1) & 1;
    const int D = data_frames_number;     /* 2 for the reference message (OFDM.c:439) */
    const int FR = 320 + 80 * D;          /* symbol-rate frame: 480 for it, more after ref_set_message */
    const int pilot[4] = {1, 1, 1, -1};
    float complex T[64], ltf[64];
    memcpy(ltf, Long_preamble_slot_Frequency, sizeof(ltf));
    ifft(ltf, T, 64);                                      /* long training symbol, C ifft (D5) */
    float complex **payload = Allocate_Array_2D(D, 96), **mod = Allocate_Array_2D(D, 48);
    float complex frame_tx[FR], frame_rx[FR], H[64];
    float complex **rx_time = Allocate_Array_2D(D, 64), **rx_freq = Allocate_Array_2D(D, 64);
    float complex **no_pilot = Allocate_Array_2D(D, 48), **final = Allocate_Array_2D(D, 48);
    float complex **demod = Allocate_Array_2D(D, 96);
    double be = 0, nb = 0, epre = 0, be2 = 0, fe = 0;
    struct timespec t0, t1;
    quiet_begin();
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int f = 0; f < n_frames; ++f) {
        memset(frame_tx, 0, sizeof(frame_tx));
        for (int i = 0; i < 64; ++i) { frame_tx[192 + i] = T[i]; frame_tx[256 + i] = T[i]; }
        for (int d = 0; d < D; ++d) {
            for (int j = 0; j < 96; j += 32) {
                unsigned int w = bits_next();
                for (int b = 0; b < 32; ++b) payload[d][j + b] = (w >> (31 - b)) & 1u;
            }
        }
        QPSK_Modulator(payload, mod, D);
        for (int d = 0; d < D; ++d) {
            float complex X[64] = {0}, x[64];
            Slice_Repeater(mod[d], X, 6, 0, 5, 1);   X[11] = pilot[0];
            Slice_Repeater(mod[d], X, 12, 5, 18, 1); X[25] = pilot[1];
            Slice_Repeater(mod[d], X, 26, 18, 24, 1);
            Slice_Repeater(mod[d], X, 33, 24, 30, 1); X[39] = pilot[2];
            Slice_Repeater(mod[d], X, 40, 30, 43, 1); X[53] = pilot[3];
            Slice_Repeater(mod[d], X, 54, 43, 48, 1);
            ifft(X, x, 64);
            Slice_Repeater(x, frame_tx, 320 + 80 * d, 48, 64, 1);
            Slice_Repeater(x, frame_tx, 336 + 80 * d, 0, 64, 1);
        }
        if (rayleigh) {          /* y[n] = sum_l h_l x[n - l], taps CN(0, 1/4) (Box-Muller on rand()) */
            float complex h[4], y[FR];
            for (int l = 0; l < 4; ++l) h[l] = 0.5f * (gaussian_noise(0, 0.5f) + I * gaussian_noise(0, 0.5f));
            for (int n = 0; n < FR; ++n) {
                y[n] = 0;
                for (int l = 0; l < 4 && l <= n; ++l) y[n] += h[l] * frame_tx[n - l];
            }
            memcpy(frame_tx, y, sizeof(y));
        }
        if (ideal) Channel_Estimation(frame_tx, H, FR);     /* known channel: noiseless LTF pair */
        for (int q = 0; q < n_snr; ++q) {
            const float kappa = 0.4980f;
            const float sd = sqrtf(kappa * 52.0f / 4096.0f / powf(10.0f, snr_db[q] / 10.0f));
            memcpy(frame_rx, frame_tx, sizeof(frame_rx));
            for (int i = 192; i < 320; ++i) frame_rx[i] += sd * gaussian_noise(0, 1);
            for (int d = 0; d < D; ++d)
                for (int i = 336 + 80 * d; i < 400 + 80 * d; ++i) frame_rx[i] += sd * gaussian_noise(0, 1);
            if (!ideal) Channel_Estimation(frame_rx, H, FR);
            for (int d = 0; d < D; ++d) {
                Slice_Repeater(frame_rx, rx_time[d], 0, 336 + 80 * d, 400 + 80 * d, 1);
                fft(rx_time[d], rx_freq[d], 64);
                for (int j = 0; j < 64; ++j) rx_freq[d][j] = rx_freq[d][j] / H[j];
                Slice_Repeater(rx_freq[d], no_pilot[d], 0, 6, 11, 1);
                Slice_Repeater(rx_freq[d], no_pilot[d], 5, 12, 25, 1);
                Slice_Repeater(rx_freq[d], no_pilot[d], 18, 26, 32, 1);
                Slice_Repeater(rx_freq[d], no_pilot[d], 24, 33, 39, 1);
                Slice_Repeater(rx_freq[d], no_pilot[d], 30, 40, 53, 1);
                Slice_Repeater(rx_freq[d], no_pilot[d], 43, 54, 59, 1);
            }
            AGC_Receiver(no_pilot, final);
            QPSK_Demodulator(final, demod, D);
            float es = 0;
            for (int d = 0; d < D; ++d)
                for (int j = 0; j < 48; ++j) es += pow(cabs(no_pilot[d][j] - mod[d][j]), 2);
            float sum = 0;
            for (int d = 0; d < D; ++d)
                for (int j = 0; j < 96; ++j) sum += abs(creal(payload[d][j]) - creal(demod[d][j]));
            be += sum; nb += 96 * D; epre += es; be2 += (double)sum * sum; fe += sum > 0;
        }
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    quiet_end();
    Deallocate_Array_2D(payload, D); Deallocate_Array_2D(mod, D);
    Deallocate_Array_2D(rx_time, D); Deallocate_Array_2D(rx_freq, D);
    Deallocate_Array_2D(no_pilot, D); Deallocate_Array_2D(final, D); Deallocate_Array_2D(demod, D);
    if (acc3) { acc3[0] += be; acc3[1] += nb; acc3[2] += epre; }
    if (acc3 && (flags & 4)) { acc3[3] += be2; acc3[4] += fe; }
    return (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec);
}
