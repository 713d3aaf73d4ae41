"""Helpers of tests/test_timing_host.py and tests/test_gpu_timing.py: the template, the streams and the cuts of the
fine timing tests (include/ofdm_mi355x_timing.h), host code in fp64, no GPU."""
from __future__ import annotations

import numpy as np

import detect_ref as ref

CLEAN_CASES = [(d, cfo) for d in (1, 2, 15) for cfo in (0.0, -90e3, 200e3)]
CLEAN_PACKETS = 4
SPAN = 640                      # a packet is refined only when p + 640 < n

# The benefit stream (test_timing_host.test_refined_positions_decode_better): 216 unfaded packets of 2 data symbols at
# 10 dB complex noise and 40 kHz.  The conditions on the seeds: the conjugate detector finds at least 150 packets, and
# the coarse positions give bit errors at all (at least 10, so that "under a tenth" is not met by 0 < 0).  The first
# seeds tried, 0x716 for the payloads and 0x717 for the noise, meet them.
BENEFIT = dict(d=2, packets=216, snr_db=10.0, cfo_hz=40e3, words_seed=0x716, noise_seed=0x717)


def template(oracle, conv: str = "c") -> np.ndarray:
    """stream.ltf_template of the oracle's Transmitter() (one period, 2 data symbols) under the transform convention
    conv, "c" (OFDM_TIMING_LTF) or "matlab" (OFDM_TIMING_LTF_MATLAB): complex128 [256]"""
    from ofdm_amd.stream import ltf_template
    return ltf_template(oracle.frame_waveform(ref.bits_of(ref.rand_words(2, 1, 1))[0], conv, True, 1))


def clean_stream(oracle, d: int, cfo_hz: float, conv: str = "c"):
    """Four noise-free packets of d data symbols (transform convention conv) behind 500-sample gaps under a carrier
    offset: words, the fp64 stream and the packets' first samples"""
    words = ref.rand_words(d, CLEAN_PACKETS, 30 + d)
    x, pos = ref.packet_stream(oracle, words, cfo_hz=cfo_hz, conv=conv)
    return words, x, pos


def coarse_positions(x, detector: str = "conjugate") -> np.ndarray:
    from ofdm_amd.stream import detection_metric, select_packets
    return select_packets(detection_metric(x, detector))["positions"]


def offsets(rx_pos, tx_pos) -> np.ndarray:
    """packet_pos - first sample for every record, against the packet whose first sample is nearest before it"""
    rx, tx = np.asarray(rx_pos, np.int64), np.asarray(tx_pos, np.int64)
    k = np.clip(np.searchsorted(tx, rx, side="right") - 1, 0, len(tx) - 1)
    return rx - tx[k], k


def top_gap(metric) -> np.ndarray:
    """the relative gap between the two largest L of every row"""
    s = np.sort(np.asarray(metric, np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) / s[:, -1]


def benefit_stream(oracle):
    """words, the complex64 stream and the packets' first samples of BENEFIT"""
    b = BENEFIT
    words = ref.rand_words(b["d"], b["packets"], b["words_seed"])
    x, pos = ref.packet_stream(oracle, words, cfo_hz=b["cfo_hz"])
    plen = 2 * (320 + 80 * b["d"]) + 20
    return words, ref.add_noise(x, b["snr_db"], b["packets"] * plen, b["noise_seed"]).astype(np.complex64), pos
