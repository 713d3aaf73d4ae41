"""Helpers of tests/test_diversity_host.py and tests/test_gpu_diversity.py: the multi-branch streams of the receive
diversity tests (include/ofdm_mi355x_diversity.h) and the fp64 rules applied to the oracle's dumps, host code, no GPU."""
from __future__ import annotations

import numpy as np

import detect_ref as ref
import track_ref as tk

GAP = ref.GAP
# The parity streams: (D, B, SNR dB, CFO Hz) -> seed, base 21000 + 100 D + 10 B plus 1000 per replacement.  About 3e4
# samples per branch (more than three detection tiles), flat Rayleigh gains per packet and branch, complex noise of one
# power on every branch.  D = 1: a partly filled quad; 2: the common packet; 4: a subcarrier pass of exactly 3 x 64;
# 15: five quads, a ragged pass and the largest LDS need.  The conditions on a seed (test_diversity_host): no front or
# confirmation decision of the combined fp64 metric inside |M - 0.75| <= 0.75e-3 and at most 1 % of the positions in
# that band; every record's two largest L more than 1e-4 apart (relative); at most 0.2 % of the subcarriers inside
# track_ref.AXIS_BAND under the fp64 rule alone.
PARITY_SEEDS = {(1, 2, 14, 0.0): 21120, (2, 3, 12, 40e3): 21230, (4, 4, 10, -90e3): 22440, (15, 2, 16, 40e3): 22520,
                (15, 4, 12, 0.0): 22540, (2, 4, 14, -90e3): 21240}
CROSS_SEED = 0xD1F
CROSS_WEAK = 0.05
CROSS_PHASE = 2.1         # branch 1's arbitrary phase, radians


def packet_count(d: int) -> int:
    return max(28000 // (2 * (320 + 80 * d) + 20 + GAP), 4)


def branch_stream(oracle, words, gains, snr_db: float, cfo_hz: float, seed: int):
    """The packets `words` (uint32 [n, 3 D]) on B branches: gains complex [B, n], one flat gain per branch and packet
    (detect_ref.packet_stream with one-tap rows), one carrier offset, and independent complex noise of one power on
    every branch, snr_db against the mean power of a gain-1 packet's samples.  Returns complex64 [B, n_samples] and
    the packets' first samples."""
    gains = np.asarray(gains, np.complex128)
    d = words.shape[1] // 3
    plen = 2 * (320 + 80 * d) + 20
    xs, pos = [], None
    for g in gains:
        x, pos = ref.packet_stream(oracle, words, g.reshape(-1, 1), cfo_hz=cfo_hz)
        xs.append(x)
    unit, _ = ref.packet_stream(oracle, words[:1])
    power = float((np.abs(unit) ** 2).sum()) / plen
    s = np.sqrt(power / 10 ** (snr_db / 10) / 2)
    rng = np.random.default_rng(seed)
    out = [x + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))) for x in xs]
    return np.stack(out).astype(np.complex64), pos


def parity_stream(oracle, key, seed: int | None = None):
    """one of PARITY_SEEDS' streams (or the same stream under another seed): words, complex64 [B, n], the packets'
    first samples"""
    d, nb, snr, cfo = key
    seed = PARITY_SEEDS[key] if seed is None else seed
    n = packet_count(d)
    words = np.repeat(tk.blank_words(d), n, axis=0)                  # the receiver's fixed payload: bit_err means something
    rng = np.random.default_rng(seed + 1)
    gains = (rng.standard_normal((nb, n)) + 1j * rng.standard_normal((nb, n))) / np.sqrt(2)
    xs, pos = branch_stream(oracle, words, gains, snr, cfo, seed + 2)
    return words, xs, pos


def cross_faded(oracle, d: int = 2, packets: int = 8, snr_db: float = 20.0, cfo_hz: float = 40e3, seed: int = CROSS_SEED):
    """Packets cross-faded between two branches: branch 0 has gain 1 on even packets and CROSS_WEAK on odd ones, branch
    1 the reverse times exp(j CROSS_PHASE).  words, complex64 [2, n] and the packets' first samples."""
    words = np.repeat(tk.blank_words(d), packets, axis=0)
    even = np.arange(packets) % 2 == 0
    gains = np.stack([np.where(even, 1.0, CROSS_WEAK), np.where(even, CROSS_WEAK, 1.0) * np.exp(1j * CROSS_PHASE)])
    xs, pos = branch_stream(oracle, words, gains, snr_db, cfo_hz, seed + 2)
    return words, xs, pos


def frames_at(oracle, xs, p: int, truth):
    """Every branch's matched-filtered frame at stream position p (the oracle's rxframe dump; samples outside the
    stream read as zero): complex128 [B, 320 + 80 D], and whether the oracle reports the window out of bounds"""
    d = len(truth) // 96
    fr, oob = [], False
    for x in xs:
        cap, at, cap_len = tk.window(np.asarray(x), p, d)
        o = oracle.decode_at(cap, truth, at, dumps=True, cap_len=cap_len)
        fr.append(o["rxframe"])
        oob = oob or bool(o["oob"])
    return np.stack(fr), oob


def fp64_packet(oracle, xs, p: int, truth, tracking: str = "none") -> dict:
    """stream.combine_branches on the oracle's frames at position p and track_ref.metrics of its z: c (the rule's
    answer), m (bits, bit_err, axis, evm_pre_sum, evm_db_pre) and oob"""
    from ofdm_amd.stream import combine_branches
    fr, oob = frames_at(oracle, xs, p, truth)
    c = combine_branches(fr, tracking)
    return dict(c=c, m=tk.metrics(c["z"].reshape(-1), truth), oob=oob)


def fp64_receive(oracle, xs, template=None) -> dict:
    """the fp64 detection and timing rules over the branches: metric, sel (select_packets) and, with a template,
    tim (refine_timing_branches)"""
    from ofdm_amd import stream
    x64 = [np.asarray(x).astype(np.complex128) for x in xs]
    metric = stream.diversity_metric(x64)
    sel = stream.select_packets(metric)
    tim = None if template is None else stream.refine_timing_branches(x64, sel["positions"], template)
    return dict(metric=metric, sel=sel, tim=tim)


def c_template(oracle):
    """the fine timing template of C-convention packets (stream.ltf_template of the oracle's waveform)"""
    from ofdm_amd.stream import ltf_template
    return ltf_template(oracle.frame_waveform(tk.blank_truth(1), "c", True, 1))


def two_largest_apart(metric_rows) -> float:
    """the smallest relative distance between the two largest L of a row, over the rows that were refined"""
    worst = np.inf
    for lam in np.asarray(metric_rows):
        if not lam.max() > 0:
            continue
        a = np.sort(lam)
        worst = min(worst, float((a[-1] - a[-2]) / a[-1]))
    return worst
