"""ctypes binding of the C ABI in include/ofdm_mi355x.h (libofdm_mi355x.so).

The library is the product: there is no CPU or PyTorch fallback.  If the shared object is
missing or cannot be loaded, load_library() raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libofdm_mi355x.so"
HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x.h"

ABI_VERSION = 1

# enums (include/ofdm_mi355x.h)
CONV = {"c": 0, "matlab": 1}
PAYLOAD = {"random": 0, "message": 1, "tester": 2}
EST = {"ls": 0, "ideal": 1}
NOISE = {"real": 0, "complex": 1, "none": 2}
CHANNEL = {"awgn": 0, "rayleigh4": 1}

# counters
NCOUNTERS = 16
C_FRAMES, C_SYMBOLS, C_BITS, C_BIT_ERR, C_FRAME_ERR, C_SYNC_FAIL, C_EVM_TERMS, C_EVM_PRE_Q, \
    C_EVM_POST_AXIS, C_EVMDB_PRE_Q, C_EVMDB_POST_Q, C_EVMDB_POST_FINITE, C_OOB, \
    C_WL_MIN_Q, C_WL_MAX_Q, C_WL_BITS = range(16)
EVM_Q_SCALE = float(1 << 20)

# kernel ids for timing
K_FFT, K_TX, K_RX, K_FRAME = range(4)
K_STREAM_DETECT, K_STREAM_SELECT, K_STREAM_DECODE = 4, 5, 6     # OFDM_K_STREAM_* (ofdm_mi355x_stream.h)
K_TRANSMIT = 7                                                   # OFDM_K_TRANSMIT (ofdm_mi355x_tx.h)
K_CHANNEL, K_SCORE = 8, 9                                        # OFDM_K_CHANNEL, OFDM_K_SCORE (ofdm_mi355x_channel.h)
K_FADE, K_DRAW_TAPS = 10, 11                                     # OFDM_K_FADE, OFDM_K_DRAW_TAPS (ofdm_mi355x_fading.h)
K_STREAM_DETECT_CONJ = 12                                        # OFDM_K_STREAM_DETECT_CONJ (ofdm_mi355x_detect.h)
K_STREAM_TIMING = 13                                             # OFDM_K_STREAM_TIMING (ofdm_mi355x_timing.h)
K_STREAM_DECODE_TRACK = 14                                       # OFDM_K_STREAM_DECODE_TRACK (ofdm_mi355x_track.h)
K_STREAM_DETECT_DIV, K_STREAM_TIMING_DIV, K_STREAM_DECODE_DIV = 15, 16, 17   # OFDM_K_STREAM_*_DIV (ofdm_mi355x_diversity.h)

# every entry point of the header, with ctypes argument types
_V = C.c_void_p
_SIGS = {
    "ofdm_abi_version": (C.c_int, []),
    "ofdm_last_error": (C.c_char_p, []),
    "ofdm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ofdm_ctx_create": (C.c_int, [C.c_int, C.POINTER(_V)]),
    "ofdm_ctx_destroy": (C.c_int, [_V]),
    "ofdm_ctx_set_stream": (C.c_int, [_V, _V]),
    "ofdm_ctx_synchronize": (C.c_int, [_V]),
    "ofdm_ctx_trim": (C.c_int, [_V, C.POINTER(C.c_int64)]),
    "ofdm_ctx_scratch_bytes": (C.c_int, [_V, C.POINTER(C.c_int64)]),
    "ofdm_timing_enable": (C.c_int, [_V, C.c_int]),
    "ofdm_timing_query": (C.c_int, [_V, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ofdm_timing_reset": (C.c_int, [_V]),
    "ofdm_fft64": (C.c_int, [_V, _V, _V, C.c_int64, C.c_int, C.c_int]),
    "ofdm_tx_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ofdm_tx_frames": (C.c_int, [_V, _V, C.c_uint64, C.c_int64, _V, _V]),
    "ofdm_set_next_tx": (C.c_int, [_V, _V, C.c_uint64, C.c_int64, _V, _V]),
    "ofdm_rx_frames": (C.c_int, [_V, _V, _V, _V, C.c_uint64, C.c_int64, _V, C.c_int, _V]),
    "ofdm_txrx_frames": (C.c_int, [_V, _V, C.c_uint64, C.c_int64, _V, _V, _V, C.c_int, _V]),
    "ofdm_rx_frames_dump": (C.c_int, [_V, _V, _V, _V, C.c_uint64, C.c_int64, _V, C.c_int, _V, _V, _V]),
    "ofdm_symbol_sweep": (C.c_int, [_V, _V, _V, C.c_int, C.c_uint64, C.c_int64, C.c_int64, _V]),
    "ofdm_set_message": (C.c_int, [_V, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
    "ofdm_payload_frames": (C.c_int, [_V, C.c_int, C.POINTER(C.c_int32)]),
    "ofdm_transmitter": (C.c_int, [_V, C.c_int, C.c_int, C.c_int, _V, C.c_int32, C.POINTER(C.c_int32)]),
    "ofdm_transmission_over_air": (C.c_int, [_V, _V, _V, C.c_int32, C.c_double, C.c_uint64, C.c_uint64, C.c_int32]),
    "ofdm_receiver": (C.c_int, [_V, _V, _V, C.c_int, _V, _V, _V, _V]),
    "ofdm_word_length_report": (C.c_int, [_V, _V, C.c_int32, _V, C.POINTER(C.c_int32)]),
    "ofdm_frame_sweep": (C.c_int, [_V, _V, _V, _V, C.c_int, C.c_uint64, C.c_int64, _V, _V]),
}
EXPORTS = tuple(_SIGS)

# the extension header include/ofdm_mi355x_long.h (long messages: frames of up to 15 data symbols); the base
# header's function list (EXPORTS) and ABI_VERSION do not change with it
LONG_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_long.h"
_LONG_SIGS = {
    "ofdm_set_long_message": (C.c_int, [_V, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]),
}
LONG_EXPORTS = tuple(_LONG_SIGS)
MSG_MAX_CHARS = 96                 # ofdm_set_message
LONG_MSG_MAX_CHARS = 180           # ofdm_set_long_message (OFDM_LONG_MSG_MAX_CHARS)
LONG_MAX_DATA_SYMBOLS = 15

# the extension header include/ofdm_mi355x_captures.h (Receiver() over a device-resident batch of caller-supplied
# captures); EXPORTS, LONG_EXPORTS and ABI_VERSION do not change with it
CAPTURES_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_captures.h"
_CAPTURES_SIGS = {
    "ofdm_receive_captures": (C.c_int, [_V, _V, C.c_int64, C.c_int64, _V, C.c_int, _V, _V, _V, _V]),
}
CAPTURES_EXPORTS = tuple(_CAPTURES_SIGS)
CAPTURE_MAX_LEN = 9400             # OFDM_CAPTURE_MAX_LEN
CAPTURE_SYNC_FAIL, CAPTURE_OOB = 1, 2      # ofdm_capture_result.flags

# the extension header include/ofdm_mi355x_stream.h (detection once over one recording of any length, every packet
# decoded); the export lists above and ABI_VERSION do not change with it
STREAM_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_stream.h"
_STREAM_SIGS = {
    "ofdm_receive_stream": (C.c_int, [_V, _V, C.c_int64, _V, C.c_int, C.c_int64, _V, _V, _V, _V, _V, _V, _V]),
}
STREAM_EXPORTS = tuple(_STREAM_SIGS)
STREAM_LAST_FRONT = 4              # OFDM_STREAM_LAST_FRONT, ofdm_capture_result.flags bit 2
STREAM_RUN, STREAM_TILE = 31, 7936  # OFDM_STREAM_RUN, OFDM_STREAM_TILE

# the extension header include/ofdm_mi355x_tx.h (Transmitter() over a device-resident batch of per-packet payloads,
# written into a device-resident recording); the export lists above and ABI_VERSION do not change with it
TX_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_tx.h"
_TX_SIGS = {
    "ofdm_transmit_len": (C.c_int, [C.c_int32, C.POINTER(C.c_int32)]),
    "ofdm_transmit_packets": (C.c_int, [_V, _V, _V, C.c_int64, _V, C.c_int64, C.c_int64, _V, _V, _V, C.c_int64]),
}
TX_EXPORTS = list(_TX_SIGS)
TX_ACCUMULATE = 1                  # OFDM_TX_ACCUMULATE, ofdm_tx_opts.flags bit 0

# the extension header include/ofdm_mi355x_channel.h (multipath, carrier offset and Philox noise over a device-resident
# recording; received records scored against the transmitted packets); the export lists above and ABI_VERSION do not
# change with it
CHANNEL_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_channel.h"
_CHANNEL_SIGS = {
    "ofdm_impair_stream": (C.c_int, [_V, _V, _V, _V, _V, C.c_int64]),
    "ofdm_score_packets": (C.c_int, [_V, C.c_int32, _V, C.c_int64, _V, C.c_int64, C.c_int64, _V, _V, _V, C.c_int32,
                                     C.c_int32, _V, _V]),
}
CHANNEL_EXPORTS = tuple(_CHANNEL_SIGS)
NOISE_REAL, NOISE_COMPLEX, NOISE_NONE = NOISE["real"], NOISE["complex"], NOISE["none"]   # OFDM_NOISE_* (ofdm_mi355x.h)
CHANNEL_MAX_TAPS = 32              # OFDM_CHANNEL_MAX_TAPS
CHANNEL_TILE = 1024                # OFDM_CHANNEL_TILE
NSCORE = 8                         # OFDM_NSCORE
S_TRANSMITTED, S_MATCHED, S_RECEIVED, S_BITS, S_BIT_ERR, S_PACKET_ERR = range(6)     # the totals row
SCORE_MAX_WINDOW = 300             # off_hi - off_lo at most

# the extension header include/ofdm_mi355x_fading.h (a FIR of its own for every transmitted packet, and Rayleigh taps
# drawn on the device); the export lists above and ABI_VERSION do not change with it
FADING_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_fading.h"
_FADING_SIGS = {
    "ofdm_faded_len": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ofdm_draw_taps": (C.c_int, [_V, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, _V, _V]),
    "ofdm_transmit_faded": (C.c_int, [_V, _V, _V, C.c_int64, _V, C.c_int64, C.c_int64, _V, _V, _V, C.c_int32, _V,
                                      C.c_int64]),
}
FADING_EXPORTS = tuple(_FADING_SIGS)
FADE_MAX_TAPS = 32                 # OFDM_FADE_MAX_TAPS

# the extension header include/ofdm_mi355x_detect.h (an optional detector and a threshold for the stream receiver); the
# export lists above and ABI_VERSION do not change with it
DETECT_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_detect.h"
_DETECT_SIGS = {
    "ofdm_stream_positions": (C.c_int64, [C.c_int64, C.c_int]),
    "ofdm_receive_stream_ex": (C.c_int, [_V, _V, C.c_int64, _V, _V, C.c_int, C.c_int64, _V, _V, _V, _V, _V, _V, _V]),
}
DETECT_EXPORTS = tuple(_DETECT_SIGS)
DETECTOR = {"reference": 0, "conjugate": 1}      # OFDM_DETECT_REFERENCE, OFDM_DETECT_CONJUGATE
DETECT_THRESHOLD = 0.75                          # OFDM_DETECT_THRESHOLD
DETECT_HALO = {"reference": 47, "conjugate": 63}  # Lc = n - halo

# the extension header include/ofdm_mi355x_timing.h (fine timing for the stream receiver by cross-correlation against
# the long training field); the export lists above and ABI_VERSION do not change with it
TIMING_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_timing.h"
_TIMING_SIGS = {
    "ofdm_receive_stream_timed": (C.c_int, [_V, _V, C.c_int64, _V, _V, C.c_int, C.c_int, C.c_int64, _V, _V, _V, _V, _V, _V,
                                            _V, _V]),
}
TIMING_EXPORTS = tuple(_TIMING_SIGS)
TIMING = {"none": 0, "ltf": 1, "ltf-matlab": 2}  # OFDM_TIMING_NONE, OFDM_TIMING_LTF, OFDM_TIMING_LTF_MATLAB
TIMING_BACK, TIMING_FWD = 56, 8                  # OFDM_TIMING_BACK, OFDM_TIMING_FWD: shifts -56 .. +7

# the extension header include/ofdm_mi355x_track.h (pilot phase tracking in the stream receiver's decode); the export
# lists above and ABI_VERSION do not change with it
TRACK_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_track.h"
_TRACK_SIGS = {
    "ofdm_receive_stream_tracked": (C.c_int, [_V, _V, C.c_int64, _V, _V, C.c_int, C.c_int, C.c_int, C.c_int64, _V, _V, _V,
                                              _V, _V, _V, _V, _V, _V]),
}
TRACK_EXPORTS = tuple(_TRACK_SIGS)
TRACKING = {"none": 0, "pilots": 1}              # OFDM_TRACK_NONE, OFDM_TRACK_PILOTS

# the extension header include/ofdm_mi355x_diversity.h (receive diversity: 2 to 4 recordings combined in the stream
# receiver); the export lists above and ABI_VERSION do not change with it
DIVERSITY_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_diversity.h"
_DIVERSITY_SIGS = {
    "ofdm_receive_stream_diversity": (C.c_int, [_V, C.POINTER(_V), C.c_int32, C.c_int64, _V, _V, C.c_int, C.c_int, C.c_int,
                                                C.c_int64, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
}
DIVERSITY_FUNCTIONS = tuple(_DIVERSITY_SIGS)
DIVERSITY_MAX_BRANCHES = 4                       # OFDM_DIVERSITY_MAX_BRANCHES

# the extension header include/ofdm_mi355x_code.h (the coded link: K = 7 rate-1/2 encoder over the payload words, the
# per-subcarrier gains of received records and a CSI-weighted soft Viterbi decoder over d_eq); the export lists above and
# ABI_VERSION do not change with it
CODE_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_code.h"
_CODE_SIGS = {
    "ofdm_code_encode": (C.c_int, [_V, C.c_int32, _V, C.c_int64, _V]),
    "ofdm_stream_csi": (C.c_int, [_V, C.POINTER(_V), C.c_int32, C.c_int64, _V, _V, C.c_int64, _V]),
    "ofdm_code_decode": (C.c_int, [_V, C.c_int32, _V, _V, _V, C.c_int64, _V, _V]),
}
CODE_FUNCTIONS = tuple(_CODE_SIGS)
K_CODE_ENCODE, K_STREAM_CSI, K_CODE_DECODE = 18, 19, 20      # OFDM_K_CODE_ENCODE, OFDM_K_STREAM_CSI, OFDM_K_CODE_DECODE
CODE_TAIL_BITS = 6                               # OFDM_CODE_TAIL_BITS


def code_info_bits(n_data: int) -> int:
    """OFDM_CODE_INFO_BITS: 48 D - 6"""
    return 48 * int(n_data) - CODE_TAIL_BITS


def code_info_words(n_data: int) -> int:
    """OFDM_CODE_INFO_WORDS: ceil((48 D - 6) / 32)"""
    return (code_info_bits(n_data) + 31) // 32


CODE_DECODE_WAVES = 4                            # CDEC_WAVES (csrc/ofdm_code.hip): rows per block and sweep


def code_decode_lds_bytes(n_data: int) -> int:
    """The decode kernel's dynamic LDS per block: per wave 96 D floats (the soft values) and 48 D 64-bit words (the
    decisions), 11.25 KiB at D = 15; it has no static LDS."""
    return CODE_DECODE_WAVES * (96 * int(n_data) * 4 + 48 * int(n_data) * 8)


# the extension header include/ofdm_mi355x_punct.h (802.11a's punctured rates 2/3 and 3/4 of the coded link: an encoder
# and a Viterbi decoder that take a rate); the export lists above and ABI_VERSION do not change with it
PUNCT_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_punct.h"
_PUNCT_SIGS = {
    "ofdm_punct_encode": (C.c_int, [_V, C.c_int32, C.c_int32, _V, C.c_int64, _V]),
    "ofdm_punct_decode": (C.c_int, [_V, C.c_int32, C.c_int32, _V, _V, _V, C.c_int64, _V, _V]),
}
PUNCT_FUNCTIONS = tuple(_PUNCT_SIGS)
RATE = {"1/2": 0, "2/3": 1, "3/4": 2}            # OFDM_PUNCT_RATE_*
PUNCT_STEPS = (48, 64, 72)                       # OFDM_PUNCT_STEPS: trellis steps per data symbol, by rate code


def rate_code(rate: str) -> int:
    """OFDM_PUNCT_RATE_* of "1/2", "2/3" or "3/4"; ValueError for anything else"""
    if not isinstance(rate, str) or rate not in RATE:
        raise ValueError(f"rate must be one of {tuple(RATE)}, got {rate!r}")
    return RATE[rate]


def punct_info_bits(n_data: int, rate: str) -> int:
    """OFDM_PUNCT_INFO_BITS: S D - 6"""
    return PUNCT_STEPS[rate_code(rate)] * int(n_data) - CODE_TAIL_BITS


def punct_info_words(n_data: int, rate: str) -> int:
    """OFDM_PUNCT_INFO_WORDS: ceil((S D - 6) / 32)"""
    return (punct_info_bits(n_data, rate) + 31) // 32


PUNCT_DECODE_WAVES = 2                           # PDEC_WAVES (csrc/ofdm_punct.hip): rows per block and sweep


def punct_decode_lds_bytes(n_data: int, rate: str) -> int:
    """The punctured decode kernel's dynamic LDS per block: per wave S D 64-bit words (the decisions) and the 96 D sent
    soft values as floats, 14,400 bytes at rate 3/4 and D = 15; it has no static LDS."""
    return PUNCT_DECODE_WAVES * (PUNCT_STEPS[rate_code(rate)] * int(n_data) * 8 + 96 * int(n_data) * 4)


# the extension header include/ofdm_mi355x_ppdu.h (self-describing coded packets: a header symbol that names the rate and
# the length, 802.11a's scrambler and a CRC-32; an encoder and a fused decoder); the export lists above and ABI_VERSION do
# not change with it
PPDU_HEADER = PKG_DIR.parent / "include" / "ofdm_mi355x_ppdu.h"
_PPDU_SIGS = {
    "ofdm_ppdu_encode": (C.c_int, [_V, C.c_int32, _V, _V, _V, _V, C.c_int64, _V, _V]),
    "ofdm_ppdu_decode": (C.c_int, [_V, C.c_int32, _V, _V, _V, C.c_int64, _V, _V, _V]),
}
PPDU_FUNCTIONS = tuple(_PPDU_SIGS)                # not named *_EXPORTS: like the lists since the diversity header's
PPDU_MIN_SYMBOLS = 2                             # OFDM_PPDU_MIN_SYMBOLS: the header's symbol and one data symbol
PPDU_PSDU_WORDS, PPDU_INFO_WORDS = 31, 36        # OFDM_PPDU_PSDU_WORDS, OFDM_PPDU_INFO_WORDS
PPDU_SERVICE_BITS, PPDU_MIN_LENGTH = 16, 4       # OFDM_PPDU_SERVICE_BITS, OFDM_PPDU_MIN_LENGTH
PPDU_BAD_HEADER, PPDU_BAD_SERVICE, PPDU_BAD_FCS = 1, 2, 4       # OFDM_PPDU_BAD_*: d_meta's status bits
PPDU_DECODE_WAVES = 2                            # PPDU_WAVES (csrc/ofdm_ppdu.hip): rows per block and sweep


def ppdu_cap(n_data: int, rate: str) -> int:
    """cap(D, rate): the largest LENGTH of a packet of D symbols, (S (D - 1) - 6 - 16) // 8"""
    return (punct_info_bits(int(n_data) - 1, rate) - PPDU_SERVICE_BITS) // 8


def ppdu_decode_lds_bytes(n_data: int) -> int:
    """The fused decode kernel's dynamic LDS per block: per wave 72 (D - 1) 64-bit words (the data part's decisions at the
    worst rate; at least 96, since the header's 48 decisions and 96 soft values lie there first) and the data symbols'
    96 (D - 1) soft values as floats, 13,440 bytes at D = 15; it has no static LDS."""
    return PPDU_DECODE_WAVES * (max(72 * (int(n_data) - 1), 96) * 8 + 96 * (int(n_data) - 1) * 4)


class OfdmError(RuntimeError):
    pass


class Cfg(C.Structure):
    """ofdm_cfg"""
    _fields_ = [("seed", C.c_uint64), ("conv", C.c_int32), ("payload", C.c_int32), ("est", C.c_int32),
                ("noise", C.c_int32), ("channel", C.c_int32), ("data_per_frame", C.c_int32),
                ("kappa", C.c_double), ("p_ref", C.c_double)]


class RxOpts(C.Structure):
    """ofdm_rx_opts"""
    _fields_ = [("cap_len", C.c_int32), ("float_cfo", C.c_int32), ("matlab_slicer", C.c_int32),
                ("float_taps", C.c_int32), ("fixed_start", C.c_int32), ("word_stats", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class TxOpts(C.Structure):
    """ofdm_tx_opts (16 bytes)"""
    _fields_ = [("conv", C.c_int32), ("float_taps", C.c_int32), ("n_data", C.c_int32), ("flags", C.c_int32)]


class ChannelOpts(C.Structure):
    """ofdm_channel_opts (64 bytes)"""
    _fields_ = [("power", C.c_double), ("snr_db", C.c_double), ("cfo_hz", C.c_double), ("seed", C.c_uint64),
                ("trial", C.c_uint64), ("index0", C.c_int64), ("noise", C.c_int32), ("snr_index", C.c_int32),
                ("n_taps", C.c_int32), ("lead", C.c_int32)]


class Score(C.Structure):
    """ofdm_score (8 bytes, one per transmitted packet)"""
    _fields_ = [("rx_index", C.c_int32), ("bit_err", C.c_int32)]


def score_dtype():
    """numpy structured dtype of ofdm_score"""
    import numpy as np  # noqa: PLC0415
    return np.dtype([("rx_index", "<i4"), ("bit_err", "<i4")])


class CaptureResult(C.Structure):
    """ofdm_capture_result (48 bytes, one per capture)"""
    _fields_ = [("packet_idx", C.c_int32), ("flags", C.c_int32), ("bit_err", C.c_int32), ("post_axis_err", C.c_int32),
                ("evm_pre_sum", C.c_float), ("evm_db_pre", C.c_float), ("evm_db_post", C.c_float), ("ber", C.c_float),
                ("cfo_coarse_hz", C.c_float), ("cfo_fine_hz", C.c_float), ("reserved", C.c_int32 * 2)]


def capture_result_dtype():
    """numpy structured dtype of ofdm_capture_result (same names, offsets and size as CaptureResult)"""
    import numpy as np  # noqa: PLC0415
    return np.dtype([("packet_idx", "<i4"), ("flags", "<i4"), ("bit_err", "<i4"), ("post_axis_err", "<i4"),
                     ("evm_pre_sum", "<f4"), ("evm_db_pre", "<f4"), ("evm_db_post", "<f4"), ("ber", "<f4"),
                     ("cfo_coarse_hz", "<f4"), ("cfo_fine_hz", "<f4"), ("reserved", "<i4", (2,))])


class StreamOpts(C.Structure):
    """ofdm_stream_opts (32 bytes)"""
    _fields_ = [("detector", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32 * 6)]


def make_stream_opts(detector: str = "reference", threshold: float = DETECT_THRESHOLD) -> StreamOpts:
    """ofdm_stream_opts for Engine.receive_stream: ValueError for an unknown detector or a threshold that is NaN or
    outside (0, 1) -- what ofdm_receive_stream_ex refuses, refused before the call."""
    if detector not in DETECTOR:
        raise ValueError(f"detector must be one of {tuple(DETECTOR)}, got {detector!r}")
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold must be a number inside (0, 1), got {threshold!r}") from None
    if not 0.0 < C.c_float(thr).value < 1.0:
        raise ValueError(f"threshold must be inside (0, 1), got {threshold!r}")
    return StreamOpts(DETECTOR[detector], thr)


def stream_positions(n: int, detector: str = "reference") -> int:
    """Lc of ofdm_stream_positions: n - 47 (reference) or n - 63 (conjugate), 0 when there are no positions"""
    if detector not in DETECTOR:
        raise ValueError(f"detector must be one of {tuple(DETECTOR)}, got {detector!r}")
    return max(int(n) - DETECT_HALO[detector], 0)


class StreamTiming(C.Structure):
    """ofdm_stream_timing (16 bytes, one per record)"""
    _fields_ = [("coarse_pos", C.c_int64), ("quality", C.c_float), ("shift", C.c_int32)]


def stream_timing_dtype():
    """numpy structured dtype of ofdm_stream_timing"""
    import numpy as np  # noqa: PLC0415
    return np.dtype([("coarse_pos", "<i8"), ("quality", "<f4"), ("shift", "<i4")])


def timing_code(timing: str) -> int:
    """OFDM_TIMING_* of "none", "ltf" or "ltf-matlab"; ValueError for anything else"""
    if not isinstance(timing, str) or timing not in TIMING:
        raise ValueError(f"timing must be one of {tuple(TIMING)}, got {timing!r}")
    return TIMING[timing]


def tracking_code(tracking: str) -> int:
    """OFDM_TRACK_* of "none" or "pilots"; ValueError for anything else"""
    if not isinstance(tracking, str) or tracking not in TRACKING:
        raise ValueError(f"tracking must be one of {tuple(TRACKING)}, got {tracking!r}")
    return TRACKING[tracking]


class StreamPacket(C.Structure):
    """ofdm_stream_packet (64 bytes, one per packet)"""
    _fields_ = [("packet_pos", C.c_int64), ("reserved", C.c_int64), ("r", CaptureResult)]


def stream_packet_dtype():
    """numpy structured dtype of ofdm_stream_packet: packet_pos, reserved, then ofdm_capture_result's fields flat"""
    import numpy as np  # noqa: PLC0415
    return np.dtype([("packet_pos", "<i8"), ("reserved8", "<i8")] + capture_result_dtype().descr)


def reduce_capture_records(rec, frames: int):
    """The counters row ofdm_receive_captures adds for these records (the header's rule): int64 [NCOUNTERS].  A
    non-finite evm_pre_sum (the long training symbols themselves past the capture's end: Z = 0 / 0) is left out of
    EVM_PRE_Q and EVMDB_PRE_Q together with its evm_db_pre, as a -inf evm_db_post is left out of EVMDB_POST_Q."""
    import numpy as np  # noqa: PLC0415
    rec = np.asarray(rec)
    out = np.zeros(NCOUNTERS, np.int64)
    n = len(rec)
    out[C_FRAMES], out[C_SYMBOLS], out[C_BITS], out[C_EVM_TERMS] = n, n * frames, 96 * frames * n, 48 * frames * n
    out[C_BIT_ERR] = rec["bit_err"].astype(np.int64).sum()
    out[C_FRAME_ERR] = int((rec["bit_err"] > 0).sum())
    out[C_SYNC_FAIL] = int((rec["flags"] & CAPTURE_SYNC_FAIL != 0).sum())
    out[C_OOB] = int((rec["flags"] & CAPTURE_OOB != 0).sum())
    out[C_EVM_POST_AXIS] = rec["post_axis_err"].astype(np.int64).sum()
    q = lambda v: np.rint(v.astype(np.float64) * EVM_Q_SCALE).astype(np.int64)    # llrint of the stored fp32 value
    pre = np.isfinite(rec["evm_pre_sum"])
    out[C_EVM_PRE_Q] = q(rec["evm_pre_sum"][pre]).sum()
    out[C_EVMDB_PRE_Q] = q(rec["evm_db_pre"][pre]).sum()
    fin = np.isfinite(rec["evm_db_post"])
    out[C_EVMDB_POST_Q] = q(rec["evm_db_post"][fin]).sum()
    out[C_EVMDB_POST_FINITE] = int(fin.sum())
    return out


def make_cfg(seed: int = 0x80211A, conv: str = "c", payload: str = "random", est: str = "ls",
             noise: str = "real", channel: str = "awgn", kappa: float = 0.4980,
             p_ref: float = 52.0 / 4096.0) -> Cfg:
    return Cfg(seed, CONV[conv], PAYLOAD[payload], EST[est], NOISE[noise], CHANNEL[channel], 2, kappa, p_ref)


def wave_len(frames: int) -> int:
    """Transmitter() output length for `frames` data symbols (OFDM.c:569-612): 10 x (2 (320 + 80 D) + 20)."""
    return 10 * (2 * (320 + 80 * frames) + 20)


def packet_len(frames: int) -> int:
    """One period of Transmitter() for `frames` data symbols, a packet of ofdm_transmit_packets: 2 (320 + 80 D) + 20."""
    return 2 * (320 + 80 * frames) + 20


def faded_len(frames: int, n_taps: int) -> int:
    """A packet of ofdm_transmit_faded: packet_len(frames) + n_taps - 1 (ofdm_faded_len)."""
    return packet_len(frames) + n_taps - 1


def capture_len(frames: int) -> int:
    """Receiver() capture, int(0.307 x waveform length) (OFDM.c:945): 3008 for D = 2."""
    return int(wave_len(frames) * 0.307)


RX_OPT_FIELDS = ("cap_len", "float_cfo", "matlab_slicer", "float_taps")


def make_rx_opts(mode: str = "c", fixed_start: int = -1, opts: dict | None = None) -> RxOpts:
    """mode 'c': OFDM.c receiver (capture int(0.307 len), 3008 for the reference message; fp32 CFO,
    fp32 taps); 'matlab': IEEE_802_11_a_Code_Tester.m (capture 3000, MATLAB slicer, double taps).
    opts: single fields of ofdm_rx_opts (RX_OPT_FIELDS) set over the mode's, e.g. {"cap_len": 1100}."""
    if mode == "c":
        o = RxOpts(0, 1, 0, 1, fixed_start)
    elif mode == "matlab":
        o = RxOpts(3000, 0, 1, 0, fixed_start)
    else:
        raise ValueError(mode)
    for k, v in (opts or {}).items():
        if k not in RX_OPT_FIELDS or isinstance(v, float) or int(v) != v:
            raise ValueError(f"opts takes integer values for {RX_OPT_FIELDS}, got {k!r}: {v!r}")
        setattr(o, k, int(v))
    return o


_LIB = None
_LIB_FILE: Path | None = None


def library_file() -> Path:
    """The shared object load_library() loaded (or would load): bench.py reads its kernels' build ids."""
    return _LIB_FILE or Path(os.environ.get("OFDM_MI355X_LIB") or LIB_PATH)


def load_library(path: Path | str | None = None) -> C.CDLL:
    """Load libofdm_mi355x.so (build it first with build_lib.build()).  Raises if absent."""
    global _LIB, _LIB_FILE
    if _LIB is not None and path is None:
        return _LIB
    # OFDM_MI355X_LIB: load a variant build (tools/build_variants.py) instead of the default
    p = Path(path or os.environ.get("OFDM_MI355X_LIB") or LIB_PATH)
    try:
        # PyTorch ships its own libamdhip64 (same SONAME).  Loading it first makes this library
        # bind to that one HIP runtime instead of starting a second one from /opt/rocm, which
        # would then see no device.
        import torch  # noqa: F401,PLC0415
    except ImportError:
        pass
    if not p.exists():
        raise OfdmError(f"{p} not found: the HIP library must be built (build_lib.build()); "
                        "there is no CPU fallback")
    lib = C.CDLL(str(p))
    for name, (res, args) in {**_SIGS, **_LONG_SIGS, **_CAPTURES_SIGS, **_STREAM_SIGS, **_TX_SIGS,
                              **_CHANNEL_SIGS, **_FADING_SIGS, **_DETECT_SIGS, **_TIMING_SIGS, **_TRACK_SIGS,
                              **_DIVERSITY_SIGS, **_CODE_SIGS, **_PUNCT_SIGS, **_PPDU_SIGS}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ofdm_abi_version() != ABI_VERSION:
        raise OfdmError(f"ABI mismatch: library {lib.ofdm_abi_version()} != {ABI_VERSION}")
    if path is None:
        _LIB, _LIB_FILE = lib, p
    return lib


def check(lib: C.CDLL, rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib.ofdm_last_error()
        raise OfdmError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
