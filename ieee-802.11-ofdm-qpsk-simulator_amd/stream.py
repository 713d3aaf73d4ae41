"""The stream receiver's rule in numpy, and the command lines of the stream receiver and the packet transmitter.

select_packets() is the executable specification of include/ofdm_mi355x_stream.h: the reference's Packet_Selection
(OFDM.c:685-771) over a whole recording, reporting every confirmed front instead of the first one.  The kernels
(csrc/ofdm_stream.hip) are tested against it bit for bit; it is host code for tests and tools and is never on a hot
path.  main() is `python ofdm_pkg.py stream`.  pack_messages() packs texts into the payload words both the receivers'
d_bits and ofdm_transmit_packets' d_words use; transmit_main() is `python ofdm_pkg.py transmit`.  score_packets() is
the executable specification of ofdm_score_packets (include/ofdm_mi355x_channel.h).  detection_metric() and
positions() are the executable specification of the two detectors of include/ofdm_mi355x_detect.h, refine_timing() that
of the fine timing of include/ofdm_mi355x_timing.h and track_pilots() that of the pilot phase tracking of
include/ofdm_mi355x_track.h; diversity_metric(), refine_timing_branches() and combine_branches() are those of the
receive diversity of include/ofdm_mi355x_diversity.h; conv_encode(), conv_soft(), viterbi_decode() and channel_gain()
those of the coded link of include/ofdm_mi355x_code.h.
"""
from __future__ import annotations

import argparse
import csv
import functools
import sys
from pathlib import Path

import numpy as np

THRESHOLD = 0.75          # OFDM.c:701
FRONT_GAP = 300           # a front's previous crossing is more than this far back (OFDM.c:716-741)
CONFIRM = 230             # the second look, front + 230 (OFDM.c:745-760)
PACKET_OFFSET = 11        # len_RRC_rx + 1 (OFDM.c:758)
LAST_FRONT = 4            # OFDM_STREAM_LAST_FRONT


DETECTORS = {"reference": (16, False), "conjugate": (32, True)}     # lag, conjugate; the window is 32 for both


def positions(n: int, detector: str = "reference") -> int:
    """Lc, the detection positions of a stream of n samples (ofdm_stream_positions): n - 47 for the reference's
    metric, n - 63 for the conjugate one, 0 when there are none."""
    if detector not in DETECTORS:
        raise ValueError(f"detector must be one of {tuple(DETECTORS)}, got {detector!r}")
    return max(int(n) - 31 - DETECTORS[detector][0], 0)


def detection_metric(x, detector: str = "reference") -> np.ndarray:
    """The detection metric M[i], 0 <= i < positions(len(x), detector), in double precision; NaN where the power is
    zero (no crossing).

    reference  M = |sum_{k<32} r[i+k] r[i+k+16]|^2 / (sum_{k<32} |r[i+k+16]|^2)^2, no conjugate (OFDM.c:659-683)
    conjugate  M = |sum_{k<32} r[i+k] conj(r[i+k+32])|^2 / (sum_{k<32} |r[i+k+32]|^2)^2: the short training field's
               period at 40 MS/s; |c| does not see the channel's phase or a carrier offset

    select_packets(M, thr) is the rest of either rule."""
    x = np.asarray(x).astype(np.complex128).reshape(-1)
    lc = positions(len(x), detector)
    if lc == 0:
        return np.zeros(0, np.float64)
    lag, conj = DETECTORS[detector]
    prod = x[:-lag] * (np.conj(x[lag:]) if conj else x[lag:])
    # windows are summed directly (no running sum): an idle gap of exact zeros gives exactly zero power, hence NaN
    c = np.lib.stride_tricks.sliding_window_view(prod, 32)[:lc].sum(axis=1)
    p = np.lib.stride_tricks.sliding_window_view((x.real ** 2 + x.imag ** 2)[lag:], 32)[:lc].sum(axis=1)
    with np.errstate(all="ignore"):
        return (c.real ** 2 + c.imag ** 2) / (p * p)


def unpack_cross(words, lc: int) -> np.ndarray:
    """The crossing bitmap of ofdm_receive_stream (bit i & 31 of word i >> 5) as a boolean array of lc positions."""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32, copy=False))
    if len(w) < (lc + 31) // 32:
        raise ValueError(f"{len(w)} words do not hold {lc} positions")
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    return bits[:lc].astype(bool)


def select_packets(cross_or_metric, thr: float = THRESHOLD) -> dict:
    """Every packet of a stream from its crossings (a boolean array) or its metric M (a float array, crossing where
    M > thr; NaN is no crossing).

    crossing  M[i] > thr
    front     a crossing i whose previous crossing b (-1 when there is none) has i - b > 300
    confirmed a front with i + 230 < Lc and a crossing at i + 230
    packets   every confirmed front, ascending, at front + 11; flag LAST_FRONT (4) on the packet whose front is the
              largest front of the stream, confirmed or not

    Returns fronts, confirmed (a mask over fronts), positions (int64) and flags (int32, 0 or 4)."""
    a = np.asarray(cross_or_metric)
    if a.ndim != 1:
        raise ValueError("one-dimensional crossings or metric expected")
    if a.dtype == bool:
        cross = a
    else:
        with np.errstate(invalid="ignore"):
            cross = a > thr
    lc = len(cross)
    idx = np.nonzero(cross)[0].astype(np.int64)
    prev = np.concatenate([[-1], idx[:-1]]).astype(np.int64)
    fronts = idx[(idx - prev) > FRONT_GAP]
    look = fronts + CONFIRM
    conf = np.zeros(len(fronts), bool)
    inside = look < lc
    conf[inside] = cross[look[inside]]
    pos = fronts[conf] + PACKET_OFFSET
    flags = np.zeros(len(pos), np.int32)
    if len(fronts):
        flags[fronts[conf] == fronts.max()] = LAST_FRONT
    return dict(fronts=fronts, confirmed=conf, positions=pos.astype(np.int64), flags=flags)


TIMINGS = ("none", "ltf", "ltf-matlab")      # "ltf-matlab": the template of a MATLAB-convention waveform
LTF_START = 394           # 2 * 192 + 10: the first long training symbol in one period of Transmitter()'s waveform
TIMING_BACK = 56          # OFDM_TIMING_BACK: candidate j is the shift j - 56
TIMING_FWD = 8            # OFDM_TIMING_FWD
TIMING_CANDIDATES = TIMING_BACK + TIMING_FWD
TIMING_FIRST = LTF_START - 16 - TIMING_BACK     # 322: candidate 0 reads from p + 322
TIMING_SPAN = TIMING_FIRST + TIMING_CANDIDATES - 1 + 256 - 1    # 640: the last sample a packet's search reads is p + 640
TIMING_SEGMENT = 32       # the non-coherent segments: the short training field's period


def ltf_template(wave) -> np.ndarray:
    """The 256-sample template of the fine timing rule (include/ofdm_mi355x_timing.h) from one period of
    Transmitter()'s 40 MS/s waveform: t[k] = wave[394 + (k mod 128)], the first long training symbol, which is cyclic
    on both sides and does not depend on the payload or on the number of data symbols.  complex128 [256].
    It does depend on the transform convention of the waveform: ltf_template(w_c) is the template of OFDM_TIMING_LTF
    ("ltf"), ltf_template(w_matlab) that of OFDM_TIMING_LTF_MATLAB ("ltf-matlab") and its specification; the second is
    the first rotated by half a period, np.roll(t_c, -64), exactly."""
    w = np.asarray(wave).astype(np.complex128).reshape(-1)
    if len(w) < LTF_START + 128:
        raise ValueError(f"a waveform of at least {LTF_START + 128} samples expected, got {len(w)}")
    return np.tile(w[LTF_START:LTF_START + 128], 2)


def refine_timing(x, positions, template) -> dict:
    """The fine timing rule in double precision, the executable specification of ofdm_receive_stream_timed with
    OFDM_TIMING_LTF: every coarse packet_pos p is moved to p - 56 + argmax_j L[j] over the 64 candidates j (the
    smallest j wins a tie), where candidate j reads 256 samples from q = p + 322 + j and
        L[j] = sum_{s<8} | sum_{k<32} x[q + 32 s + k] conj(t[32 s + k]) |^2 .
    A packet whose search window [p + 322, p + 640] does not lie inside the stream, or whose every L[j] is 0, keeps p
    with shift 0 and quality 0.  quality = L[j*] / sum_s (sum_k |t[32 s + k]|^2 sum_k |x[q* + 32 s + k]|^2), inside
    [0, 1] and invariant to the scale of x and of t.

    Returns positions (int64, refined), coarse (int64), shift (int32), quality (float64) and metric (float64
    [n, 64], L; zeros for a packet that was not refined).
    The rule takes any template: with ltf_template of a C-convention waveform it specifies OFDM_TIMING_LTF, with that
    of a MATLAB-convention waveform OFDM_TIMING_LTF_MATLAB.  The template has to be of the recording's convention:
    the other one moves every packet 4 samples late at a quality near 0.3, and at large carrier offsets further."""
    x = np.asarray(x).astype(np.complex128).reshape(-1)
    t = np.asarray(template).astype(np.complex128).reshape(-1)
    if len(t) != 256:
        raise ValueError(f"a template of 256 samples expected (ltf_template), got {len(t)}")
    coarse = np.asarray(positions, np.int64).reshape(-1)
    n, m = len(x), len(coarse)
    pos, shift = coarse.copy(), np.zeros(m, np.int32)
    quality, metric = np.zeros(m, np.float64), np.zeros((m, TIMING_CANDIDATES), np.float64)
    tc = np.conj(t).reshape(8, TIMING_SEGMENT)
    te = (np.abs(t) ** 2).reshape(8, TIMING_SEGMENT).sum(axis=1)
    for i, p in enumerate(coarse):
        p = int(p)
        if p + TIMING_FIRST < 0 or p + TIMING_SPAN >= n:
            continue
        win = np.lib.stride_tricks.sliding_window_view(x[p + TIMING_FIRST:p + TIMING_SPAN + 1], 256)    # [64, 256]
        seg = (win.reshape(TIMING_CANDIDATES, 8, TIMING_SEGMENT) * tc).sum(axis=2)
        lam = (seg.real ** 2 + seg.imag ** 2).sum(axis=1)
        metric[i] = lam
        j = int(np.argmax(lam))
        if not lam[j] > 0.0:
            continue
        xe = (np.abs(win[j]) ** 2).reshape(8, TIMING_SEGMENT).sum(axis=1)
        pos[i] = p - TIMING_BACK + j
        shift[i] = j - TIMING_BACK
        quality[i] = lam[j] / float((te * xe).sum())
    return dict(positions=pos, coarse=coarse, shift=shift, quality=quality, metric=metric)


TRACKINGS = ("none", "pilots")
PILOT_BINS = (11, 25, 39, 53)             # in the reference's bin order (pilot_at, csrc/ofdm_device.h)
PILOT_VALUES = (1.0, 1.0, 1.0, -1.0)      # OFDM.c:523
DATA_BINS = tuple(b for b in range(6, 59) if b != 32 and b not in PILOT_BINS)    # the 48 data bins, ascending


def track_pilots(Y, H) -> dict:
    """The pilot phase tracking rule in double precision, the executable specification of ofdm_receive_stream_tracked
    with OFDM_TRACK_PILOTS (include/ofdm_mi355x_track.h).  Y: the data symbols' spectra in the reference's bin order,
    complex [D, 64] (or [64 D]: the oracle's Yf dump); H: the LS estimate, complex [64] (the oracle's H dump).
        P_d   = sum over the pilot bins k = 11, 25, 39, 53 of p_k Y_d[k] conj(H[k]),  p = (+1, +1, +1, -1)
        u_d   = P_d / |P_d|, or 1 when |P_d| is 0 or P_d is not finite
        z'_d  = (Y_d[k_j] / H[k_j]) conj(u_d) over the 48 data bins k_j
    A symbol with u_d = 1 by the fallback keeps z = Y / H as it is (a NaN included) and has phase 0.

    Returns u (complex128 [D]), phase (float64 [D], the angle of P_d, radians), z (complex128 [D, 48], z'), P
    (complex128 [D]) and fallback (bool [D])."""
    H = np.asarray(H).astype(np.complex128).reshape(-1)
    if len(H) != 64:
        raise ValueError(f"an estimate of 64 bins expected, got {len(H)}")
    Y = np.asarray(Y).astype(np.complex128)
    if Y.size % 64:
        raise ValueError(f"spectra of 64 bins expected, got {Y.shape}")
    Y = Y.reshape(-1, 64)
    pb, db = list(PILOT_BINS), list(DATA_BINS)
    with np.errstate(all="ignore"):
        P = (np.asarray(PILOT_VALUES) * Y[:, pb] * np.conj(H[pb])).sum(axis=1)
        mag = np.abs(P)
        fallback = ~(np.isfinite(P.real) & np.isfinite(P.imag) & np.isfinite(mag) & (mag > 0))
        u = np.where(fallback, 1.0 + 0.0j, P / np.where(fallback, 1.0, mag))
        phase = np.where(fallback, 0.0, np.angle(np.where(fallback, 1.0, P)))
        z0 = Y[:, db] / H[db]
        z = np.where(fallback[:, None], z0, z0 * np.conj(u)[:, None])
    return dict(u=u, phase=phase, z=z, P=P, fallback=fallback)


def slice_bits(z) -> np.ndarray:
    """The C slicer and demapper (OFDM.c:852-908) on equalised subcarriers z [..., 48 D]: int32 [..., 96 D]; an axis
    that is zero or NaN decides "-", so such a subcarrier gives the bits (1, 0)."""
    z = np.asarray(z)
    with np.errstate(invalid="ignore"):
        pr, pi = z.real > 0, z.imag > 0
    return np.stack([~pi, pr ^ pi], axis=-1).astype(np.int32).reshape(*z.shape[:-1], 2 * z.shape[-1])


MAX_BRANCHES = 4          # OFDM_DIVERSITY_MAX_BRANCHES
# the long training tones L_k in the reference's bin order (OFDM.c:494; ltf_sign, csrc/ofdm_device.h): +-1 on the 52
# used bins 6..58, 0 at bin 32 and outside
LTF_SIGNS = np.array([0] * 6 + [1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
                                1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1]
                     + [0] * 5, np.float64)
USED_BINS = tuple(int(b) for b in np.nonzero(LTF_SIGNS)[0])      # the 48 data bins and the 4 pilots
SAMPLE_TIME = 1.0 / 20e6  # the frame's sample time after the matched filter's down-sampling (OFDM.c:16-17)


def fft64(x) -> np.ndarray:
    """The reference's transform convention (OFDM.c fft): DFT(x (-1)^n) over the last axis of 64 samples, so that bin 32
    is the carrier and bins 6..58 are the used subcarriers in ascending frequency."""
    x = np.asarray(x).astype(np.complex128)
    if x.shape[-1] != 64:
        raise ValueError(f"64 samples expected along the last axis, got {x.shape}")
    return np.fft.fft(x * (1.0 - 2.0 * (np.arange(64) & 1)), axis=-1)


def _branches(xs) -> np.ndarray:
    """B recordings of one length as complex128 [B, n]; ValueError unless 1 <= B <= MAX_BRANCHES"""
    rows = [np.asarray(x).astype(np.complex128).reshape(-1) for x in xs]
    if not 1 <= len(rows) <= MAX_BRANCHES:
        raise ValueError(f"1 to {MAX_BRANCHES} branches expected, got {len(rows)}")
    if len({len(r) for r in rows}) != 1:
        raise ValueError(f"branches of one length expected, got {[len(r) for r in rows]}")
    return np.stack(rows)


def diversity_metric(xs) -> np.ndarray:
    """The combined detection metric of include/ofdm_mi355x_diversity.h in double precision, over B recordings xs of
    one length n: with c_b and p_b the sums of the conjugate rule (detection_metric) on branch b,
        c[i] = sum_b c_b[i],  p[i] = sum_b p_b[i],  M[i] = |c[i]|^2 / p[i]^2,  0 <= i < n - 63,
    NaN where the power is zero (no crossing).  |c_b| does not see the phase of branch b's channel or a carrier
    offset, and c_b's own phase is that of the common offset alone, so the branches add coherently.
    diversity_metric([x]) is detection_metric(x, "conjugate"), bit for bit; select_packets(M, thr) is the rest."""
    x = _branches(xs)
    lc = positions(x.shape[1], "conjugate")
    if lc == 0:
        return np.zeros(0, np.float64)
    c = np.zeros(lc, np.complex128)
    p = np.zeros(lc, np.float64)
    for r in x:
        prod = r[:-32] * np.conj(r[32:])
        c = c + np.lib.stride_tricks.sliding_window_view(prod, 32)[:lc].sum(axis=1)
        p = p + np.lib.stride_tricks.sliding_window_view((r.real ** 2 + r.imag ** 2)[32:], 32)[:lc].sum(axis=1)
    with np.errstate(all="ignore"):
        return (c.real ** 2 + c.imag ** 2) / (p * p)


def refine_timing_branches(xs, positions, template) -> dict:
    """refine_timing over B recordings xs (include/ofdm_mi355x_diversity.h): L[j] = sum_b L_b[j] over the same 64
    candidates, the largest L with the smallest j wins, and
        quality = L[j*] / sum_b sum_s (sum_k |t[32 s + k]|^2 sum_k |x_b[q* + 32 s + k]|^2).
    The window rule, the arguments and the result are refine_timing's; with one branch it is refine_timing."""
    x = _branches(xs)
    t = np.asarray(template).astype(np.complex128).reshape(-1)
    if len(t) != 256:
        raise ValueError(f"a template of 256 samples expected (ltf_template), got {len(t)}")
    coarse = np.asarray(positions, np.int64).reshape(-1)
    n, m = x.shape[1], len(coarse)
    pos, shift = coarse.copy(), np.zeros(m, np.int32)
    quality, metric = np.zeros(m, np.float64), np.zeros((m, TIMING_CANDIDATES), np.float64)
    tc = np.conj(t).reshape(8, TIMING_SEGMENT)
    te = (np.abs(t) ** 2).reshape(8, TIMING_SEGMENT).sum(axis=1)
    for i, p in enumerate(coarse):
        p = int(p)
        if p + TIMING_FIRST < 0 or p + TIMING_SPAN >= n:
            continue
        wins = [np.lib.stride_tricks.sliding_window_view(r[p + TIMING_FIRST:p + TIMING_SPAN + 1], 256) for r in x]
        lam = np.zeros(TIMING_CANDIDATES, np.float64)
        for win in wins:
            seg = (win.reshape(TIMING_CANDIDATES, 8, TIMING_SEGMENT) * tc).sum(axis=2)
            lam = lam + (seg.real ** 2 + seg.imag ** 2).sum(axis=1)
        metric[i] = lam
        j = int(np.argmax(lam))
        if not lam[j] > 0.0:
            continue
        den = sum(float((te * (np.abs(win[j]) ** 2).reshape(8, TIMING_SEGMENT).sum(axis=1)).sum()) for win in wins)
        pos[i] = p - TIMING_BACK + j
        shift[i] = j - TIMING_BACK
        quality[i] = lam[j] / den
    return dict(positions=pos, coarse=coarse, shift=shift, quality=quality, metric=metric)


def _rotate(frames, f_hz: float) -> np.ndarray:
    """frame sample i times exp(-j 2 pi f Ts i) (OFDM.c:802,825)"""
    return frames * np.exp(-2j * np.pi * f_hz * SAMPLE_TIME * np.arange(frames.shape[-1]))


def combine_branches(frames, tracking: str = "none", float_cfo: bool = True) -> dict:
    """The diversity decode rule of include/ofdm_mi355x_diversity.h in double precision, its executable specification.
    frames: complex [B, 320 + 80 D], every branch's matched-filtered frame at the packet's position (the oracle's
    rxframe dump); one-dimensional input is one branch.
        coarse CFO  fc = -angle(sum_b sum_{k<16} f_b[80 + k] conj(f_b[96 + k])) / (2 pi 16 Ts)
        fine CFO    ff = -angle(sum_b sum_{k<64} g_b[192 + k] conj(g_b[256 + k])) / (2 pi 64 Ts), g_b = f_b rotated by fc
                    (float_cfo: each rounded to fp32 as it is formed, the C receiver's)
        rotation    every branch by fc + ff
        spectra     S_b = fft64(LTF1 + LTF2), H_b = LTF_SIGNS S_b / 2, Y_{b,d} = fft64 of data symbol d past its prefix
        combining   N_d[k] = sum_b Y_{b,d}[k] conj(H_b[k]),  G[k] = sum_b |H_b[k]|^2,  z_d = N_d / G on the 48 data bins
        tracking    "pilots": P_d = sum_pilots p_k N_d[k]; u_d, the fallback and z' = z conj(u_d) as track_pilots
        gain        gain[b] = sum over the 52 used bins of |H_b[k]|^2 / 52
    With one branch H, Y and z are the reference's own (the oracle's H, Yf and nopilot dumps).

    Returns z (complex128 [D, 48]: z, or z' with tracking), N ([D, 64]), G ([64]), H ([B, 64]), Y ([B, D, 64]), gain
    ([B]), cfo (fc, ff), and with tracking u, phase, P and fallback ([D]) as track_pilots gives them (else None)."""
    if tracking not in TRACKINGS:
        raise ValueError(f"tracking must be one of {TRACKINGS}, got {tracking!r}")
    f = np.asarray(frames).astype(np.complex128)
    f = f.reshape(1, -1) if f.ndim == 1 else f
    nfr = f.shape[-1]
    if f.ndim != 2 or not 1 <= len(f) <= MAX_BRANCHES or nfr < 400 or (nfr - 320) % 80:
        raise ValueError(f"frames [B, 320 + 80 D] with 1 <= B <= {MAX_BRANCHES} expected, got {f.shape}")
    d = (nfr - 320) // 80
    rnd = (lambda v: float(np.float32(v))) if float_cfo else float
    with np.errstate(all="ignore"):
        pp = (f[:, 80:96] * np.conj(f[:, 96:112])).sum()
        fc = rnd(-np.arctan2(pp.imag, pp.real) / (2 * np.pi * 16 * SAMPLE_TIME))
        g = _rotate(f, fc)
        pp = (g[:, 192:256] * np.conj(g[:, 256:320])).sum()
        ff = rnd(-np.arctan2(pp.imag, pp.real) / (2 * np.pi * 64 * SAMPLE_TIME))
        r = _rotate(f, fc + ff)
        H = _channel(r)
        Y = fft64(np.stack([r[:, 336 + 80 * s:400 + 80 * s] for s in range(d)], axis=1))       # [B, D, 64]
        N = (Y * np.conj(H)[:, None, :]).sum(axis=0)
        G = (np.abs(H) ** 2).sum(axis=0)
        db = list(DATA_BINS)
        z = N[:, db] / G[db]
        gain = (np.abs(H[:, list(USED_BINS)]) ** 2).sum(axis=1) / len(USED_BINS)
        out = dict(z=z, N=N, G=G, H=H, Y=Y, gain=gain, cfo=(fc, ff), u=None, phase=None, P=None, fallback=None)
        if tracking == "pilots":
            # track_pilots on (N, G): P_d = sum p_k N_d[k] conj(G[k]) would weigh the pilots by G, so the rule is spelt out
            P = (np.asarray(PILOT_VALUES) * N[:, list(PILOT_BINS)]).sum(axis=1)
            mag = np.abs(P)
            fallback = ~(np.isfinite(P.real) & np.isfinite(P.imag) & np.isfinite(mag) & (mag > 0))
            u = np.where(fallback, 1.0 + 0.0j, P / np.where(fallback, 1.0, mag))
            phase = np.where(fallback, 0.0, np.angle(np.where(fallback, 1.0, P)))
            out.update(z=np.where(fallback[:, None], z, z * np.conj(u)[:, None]), u=u, phase=phase, P=P, fallback=fallback)
    return out


def first_packet(sel: dict) -> int:
    """Packet_Selection's answer from select_packets': the first packet that is not the last front's, 0 when none."""
    keep = sel["positions"][sel["flags"] & LAST_FRONT == 0]
    return int(keep[0]) if len(keep) else 0


def synthetic_segments(period: int, frames: int, gap: int) -> list:
    """`frames` whole frames of the repeated waveform, each behind an idle gap, and a closing gap"""
    seg = []
    for k in range(frames):
        seg += [("gap", gap), ("wave", (k % 10) * period, (k % 10 + 1) * period)]
    return seg + [("gap", gap)]


MAX_DATA_SYMBOLS = 15     # OFDM_LONG_MAX_DATA_SYMBOLS


def pack_messages(texts, n_data: int | None = None):
    """Payload words of one packet per text: (uint32 [n, 3 D], D), three MSB-first words per data symbol -- the layout
    of ofdm_receive_stream's d_bits and of ofdm_transmit_packets' d_words.  Every text (str, latin-1, or bytes) is
    padded with ' ' to D whole symbols of 12 characters (Data_Generator, OFDM.c:435-465); D is n_data, or the largest
    number of symbols any text needs (at least 1).  ValueError for a text that needs more than 15 symbols or more
    than n_data.  fileio.decode_message of a row's bits gives the padded text back."""
    rows = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in texts]
    need = [max((8 * len(b) + 95) // 96, 1) for b in rows]
    for b, k in zip(rows, need):
        if k > MAX_DATA_SYMBOLS:
            raise ValueError(f"a text of {len(b)} characters needs {k} data symbols, a packet carries at most "
                             f"{MAX_DATA_SYMBOLS} ({12 * MAX_DATA_SYMBOLS} characters)")
    d = max(need, default=1) if n_data is None else int(n_data)
    if not 1 <= d <= MAX_DATA_SYMBOLS:
        raise ValueError(f"n_data must be in [1, {MAX_DATA_SYMBOLS}], got {n_data!r}")
    if need and max(need) > d:
        raise ValueError(f"a text needs {max(need)} data symbols, n_data is {d}")
    buf = np.full((len(rows), 12 * d), 0x20, np.uint8)
    for k, b in enumerate(rows):
        buf[k, :len(b)] = np.frombuffer(b, np.uint8)
    return buf.view(">u4").astype(np.uint32), d


SCORE_MAX_WINDOW = 300    # off_hi - off_lo at most: fronts are at least 301 apart, so a window holds one record
NSCORE = 8                # OFDM_NSCORE


def score_packets(tx_pos, tx_words, rx_pos, rx_words, window=(8, 40)) -> dict:
    """The scoring rule of include/ofdm_mi355x_channel.h in numpy, as select_packets is the detection rule:
    transmitted packet k (position tx_pos[k], payload words tx_words[k]) matches the received record j with the
    smallest j for which off_lo <= rx_pos[j] - tx_pos[k] <= off_hi (rx_pos ascending); rx_index = j and bit_err = the
    differing bits of the two rows of words, or -1 and 0 without a match.

    Returns rx_index and bit_err (int32 [n_tx]) and totals (int64 [8]: transmitted, matched, received, bits
    compared, bit errors, matched packets with at least one bit error, 0, 0)."""
    lo, hi = (int(v) for v in window)
    if not (0 <= lo <= hi and hi - lo <= SCORE_MAX_WINDOW):
        raise ValueError(f"window needs 0 <= off_lo <= off_hi and off_hi - off_lo <= {SCORE_MAX_WINDOW}, got {window!r}")
    tx_pos = np.asarray(tx_pos, np.int64).reshape(-1)
    rx_pos = np.asarray(rx_pos, np.int64).reshape(-1)
    n_tx, n_rx = len(tx_pos), len(rx_pos)
    tw = np.asarray(tx_words).astype(np.uint32, copy=False)
    rw = np.asarray(rx_words).astype(np.uint32, copy=False)
    if tw.ndim != 2 or rw.ndim != 2 or len(tw) != n_tx or len(rw) != n_rx or tw.shape[1] != rw.shape[1]:
        raise ValueError(f"tx_words [{n_tx}, W] and rx_words [{n_rx}, W] expected, got {tw.shape} and {rw.shape}")
    if n_rx > 1 and (np.diff(rx_pos) < 0).any():
        raise ValueError("rx_pos must be ascending")
    j = np.searchsorted(rx_pos, tx_pos + lo, side="left")               # the first record at or behind pos + off_lo
    hit = j < n_rx
    hit[hit] = rx_pos[j[hit]] - tx_pos[hit] <= hi
    rx_index = np.where(hit, j, -1).astype(np.int32)
    bit_err = np.zeros(n_tx, np.int32)
    if hit.any():
        x = tw[hit] ^ rw[j[hit]]
        bit_err[hit] = np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=1).sum(axis=1)
    totals = np.zeros(NSCORE, np.int64)
    totals[:6] = (n_tx, int(hit.sum()), n_rx, 32 * tw.shape[1] * int(hit.sum()), int(bit_err.sum()),
                  int((bit_err > 0).sum()))
    return dict(rx_index=rx_index, bit_err=bit_err, totals=totals)


# ---- the coded link (include/ofdm_mi355x_code.h): 802.11a's K = 7 rate-1/2 mother code over the payload words ----
CODE_TAIL = 6             # zero tail bits: the trellis ends in state 0
CODE_STATES = 64
CODE_CLAMP = 2.0 ** 100   # |soft value| at most: 1,440 of them cannot overflow fp32
# generators 133 and 171 (octal) over (u_t, u_t-1, .., u_t-6)
CODE_TAPS_A = (0, 2, 3, 5, 6)
CODE_TAPS_B = (0, 1, 2, 3, 6)


def INFO_BITS(n_data: int) -> int:
    """K_info = 48 D - 6 information bits of a packet of D data symbols"""
    d = int(n_data)
    if d != n_data or not 1 <= d <= MAX_DATA_SYMBOLS:
        raise ValueError(f"n_data must be in [1, {MAX_DATA_SYMBOLS}], got {n_data!r}")
    return 48 * d - CODE_TAIL


def INFO_WORDS(n_data: int) -> int:
    """W_i = ceil(K_info / 32) words of uint32 per packet, MSB first"""
    return (INFO_BITS(n_data) + 31) // 32


def pack_coded_messages(texts, n_data: int | None = None, rate: str = "1/2"):
    """Information words of one coded packet per text: (uint32 [n, W_i], D).  A text (str, latin-1, or bytes) fills the
    first 8 len information bits, MSB first, and is padded with ' ' to the K_info // 8 whole characters a packet holds;
    the few bits past them are 0.  D is n_data, or the smallest with S D - 6 >= 8 len for every text (at least 1); S is
    48, or RATE_STEPS[rate] at a punctured rate (include/ofdm_mi355x_punct.h).
    ValueError for a text that needs more than 15 symbols or more than n_data."""
    if rate not in RATE_STEPS:
        raise ValueError(f"rate must be one of {tuple(RATE_STEPS)}, got {rate!r}")
    s = RATE_STEPS[rate]
    kinfo = lambda d: s * d - CODE_TAIL
    rows = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in texts]
    need = [max((8 * len(b) + CODE_TAIL + s - 1) // s, 1) for b in rows]
    for b, k in zip(rows, need):
        if k > MAX_DATA_SYMBOLS:
            raise ValueError(f"a text of {len(b)} characters needs {k} data symbols, a coded packet carries at most "
                             f"{MAX_DATA_SYMBOLS} ({kinfo(MAX_DATA_SYMBOLS) // 8} characters)")
    d = max(need, default=1) if n_data is None else int(n_data)
    if not 1 <= d <= MAX_DATA_SYMBOLS:
        raise ValueError(f"n_data must be in [1, {MAX_DATA_SYMBOLS}], got {n_data!r}")
    if need and max(need) > d:
        raise ValueError(f"a text needs {max(need)} data symbols, n_data is {d}")
    buf = np.zeros((len(rows), 4 * ((kinfo(d) + 31) // 32)), np.uint8)
    buf[:, :kinfo(d) // 8] = 0x20
    for k, b in enumerate(rows):
        buf[k, :len(b)] = np.frombuffer(b, np.uint8)
    return buf.view(">u4").astype(np.uint32), d


def interleave_index() -> np.ndarray:
    """802.11a's first permutation for N_CBPS = 96 (the second is the identity for QPSK): coded bit k of a data symbol
    goes to position j[k] = 6 (k mod 16) + k // 16"""
    k = np.arange(96)
    return 6 * (k % 16) + k // 16


def _info_bits(info_words, n_data: int) -> np.ndarray:
    """uint32 [n, W_i] -> uint8 [n, K_info], MSB first; the unused low bits of the last word are dropped"""
    w = np.ascontiguousarray(np.asarray(info_words).astype(np.uint32, copy=False))
    if w.ndim != 2 or w.shape[1] != INFO_WORDS(n_data):
        raise ValueError(f"information words [n, {INFO_WORDS(n_data)}] expected for {n_data} data symbols, got {w.shape}")
    return np.unpackbits(w.astype(">u4").view(np.uint8), axis=1)[:, :INFO_BITS(n_data)]


def _pack_bits(bits) -> np.ndarray:
    """uint8 [n, k] -> uint32 [n, ceil(k / 32)], MSB first, the last word's unused low bits 0"""
    b = np.asarray(bits, np.uint8)
    pad = (-b.shape[1]) % 32
    b = np.concatenate([b, np.zeros((len(b), pad), np.uint8)], axis=1)
    return np.ascontiguousarray(np.packbits(b, axis=1)).view(">u4").astype(np.uint32)


def conv_code_bits(u) -> np.ndarray:
    """The mother code on bit rows u [n, T] (u_t = 0 for t < 0): uint8 [n, 2 T], c[2 t] = A_t, c[2 t + 1] = B_t"""
    u = np.asarray(u, np.uint8)
    pad = np.concatenate([np.zeros((len(u), 6), np.uint8), u], axis=1)
    t = u.shape[1]
    a = np.zeros_like(u)
    b = np.zeros_like(u)
    for s in CODE_TAPS_A:
        a ^= pad[:, 6 - s:6 - s + t]
    for s in CODE_TAPS_B:
        b ^= pad[:, 6 - s:6 - s + t]
    return np.stack([a, b], axis=-1).reshape(len(u), 2 * t)


def conv_encode(info_words, n_data: int, precode: bool = True) -> np.ndarray:
    """The encoder of include/ofdm_mi355x_code.h, its executable specification: information words uint32 [n, W_i]
    (MSB first) -> payload words uint32 [n, 3 D] for ofdm_transmit_packets.  K_info information bits and six zero tail
    bits through the K = 7 rate-1/2 code (generators 133, 171 octal), each data symbol's 96 coded bits through
    interleave_index(), and the interleaved bits g precoded for the reference's QPSK map: b[2 m] = g[2 m],
    b[2 m + 1] = g[2 m] ^ g[2 m + 1], so that im > 0 iff g[2 m] = 0 and re > 0 iff g[2 m + 1] = 0.
    precode=False feeds g to the map as it is (what the precoding is measured against, not a mode of the library)."""
    u = _info_bits(info_words, n_data)
    n = len(u)
    u = np.concatenate([u, np.zeros((n, CODE_TAIL), np.uint8)], axis=1)
    c = conv_code_bits(u).reshape(n, n_data, 96)
    g = np.zeros_like(c)
    g[:, :, interleave_index()] = c
    if precode:
        g = g.copy()
        g[:, :, 1::2] ^= g[:, :, 0::2]
    return _pack_bits(g.reshape(n, 96 * n_data))


def conv_soft(eq, csi=None) -> np.ndarray:
    """The soft values of include/ofdm_mi355x_code.h in trellis order: float32 [n, 96 D], the two of step t at 2 t and
    2 t + 1.  eq: complex [n, 48 D] equalised subcarriers (d_eq); csi: [n, 48] gains (d_csi) or None for 1.  At
    position j of data symbol d, subcarrier m = j >> 1: v = Im z for even j, Re z for odd j, z = eq[48 d + m];
    lam = csi[m] v as one fp32 product; a non-finite lam is 0; |lam| is clamped to 2^100; positive means bit 0."""
    z = np.asarray(eq).astype(np.complex64)
    if z.ndim != 2 or z.shape[1] % 48 or not 1 <= z.shape[1] // 48 <= MAX_DATA_SYMBOLS:
        raise ValueError(f"eq [n, 48 D] with 1 <= D <= {MAX_DATA_SYMBOLS} expected, got {z.shape}")
    n, d = len(z), z.shape[1] // 48
    v = np.stack([z.imag, z.real], axis=-1).reshape(n, d, 96)                 # position j = 2 m + (0: Im, 1: Re)
    with np.errstate(all="ignore"):
        if csi is not None:
            w = np.asarray(csi).astype(np.float32)
            if w.shape != (n, 48):
                raise ValueError(f"csi [{n}, 48] expected, got {w.shape}")
            v = v * np.repeat(w, 2, axis=1)[:, None, :]
        v = v.astype(np.float32)
        v = np.where(np.isfinite(v), v, np.float32(0))
        v = np.clip(v, np.float32(-CODE_CLAMP), np.float32(CODE_CLAMP))
    return np.ascontiguousarray(v[:, :, interleave_index()].reshape(n, 96 * d), np.float32)


def _trellis():
    """State s = u_t-1 << 5 | .. | u_t-6; the step's input u_t = s' >> 5 leads to s' = u_t << 5 | s >> 1, so the
    predecessors of s' are p0 = (2 s') & 63 and p1 = p0 | 1 (u_t-6 = 0 and 1).  Returns p0 [64] and the coded bits
    (A, B) on the branch p0 -> s' [64]; those on p1 -> s' are their complements (both generators tap u_t-6)."""
    s = np.arange(CODE_STATES)
    bit = lambda k: (s >> k) & 1                                     # u_t-i sits at bit 5 - i of s' for i = 0..5
    a0 = bit(5) ^ bit(3) ^ bit(2) ^ bit(0)
    b0 = bit(5) ^ bit(4) ^ bit(3) ^ bit(2)
    return (2 * s) & 63, a0.astype(bool), b0.astype(bool)


def _viterbi(lam) -> dict:
    """The recursion and traceback of viterbi_decode over float32 [n, 2 T] values, T steps of which the last six are
    the tail"""
    n, steps = len(lam), lam.shape[1] // 2
    p0, a0, b0 = _trellis()
    p1 = p0 | 1
    m = np.full((n, CODE_STATES), -np.inf, np.float32)
    m[:, 0] = 0
    dec = np.zeros((steps, n, CODE_STATES), bool)
    with np.errstate(invalid="ignore"):
        for t in range(steps):
            l0, l1 = lam[:, 2 * t, None], lam[:, 2 * t + 1, None]
            sa, sb = np.where(a0, -l0, l0), np.where(b0, -l1, l1)
            c0 = m[:, p0] + (sa + sb)
            c1 = m[:, p1] + ((-sa) + (-sb))
            dec[t] = c1 > c0
            m = np.where(dec[t], c1, c0)
    assert m.dtype == np.float32
    s = np.zeros(n, np.int64)
    u = np.zeros((n, steps), np.uint8)
    rows = np.arange(n)
    for t in range(steps - 1, -1, -1):
        u[:, t] = s >> 5
        s = ((2 * s) & 63) | dec[t, rows, s]
    return dict(info=_pack_bits(u[:, :steps - CODE_TAIL]), path=m[:, 0].copy())


def viterbi_decode(soft) -> dict:
    """The decoder of include/ofdm_mi355x_code.h in fp32, its executable specification, vectorised over packets.
    soft: float32 [n, 96 D] in trellis order (conv_soft).  A Viterbi decoder over the 64 states with a correlation
    metric that is maximised: M = 0 for state 0 and -inf for the others; per step and new state the two candidates
    c_p = M[p] + ((+-lam[2 t]) + (+-lam[2 t + 1])), the sign "-" where the branch's coded bit is 1, the inner sum
    rounded to fp32 first, then the outer one; p1 wins iff c_p1 > c_p0 (a tie takes p0); traceback from state 0.
    Returns info (uint32 [n, W_i], MSB first, the last word's unused bits 0) and path (float32 [n], the final metric
    of state 0)."""
    lam = np.asarray(soft)
    if lam.dtype != np.float32 or lam.ndim != 2 or lam.shape[1] % 96 or not 1 <= lam.shape[1] // 96 <= MAX_DATA_SYMBOLS:
        raise ValueError(f"soft float32 [n, 96 D] with 1 <= D <= {MAX_DATA_SYMBOLS} expected, got {lam.dtype} {lam.shape}")
    return _viterbi(lam)


# ---- the punctured rates (include/ofdm_mi355x_punct.h): 802.11a's 2/3 and 3/4 of the same code ----
RATES = ("1/2", "2/3", "3/4")                          # OFDM_PUNCT_RATE_*: the C codes 0, 1, 2
RATE_STEPS = {"1/2": 48, "2/3": 64, "3/4": 72}         # S: trellis steps per data symbol of 96 sent bits
# the period of each pattern as (step, 0: A, 1: B) in sent order
_RATE_PERIOD = {"1/2": (1, ((0, 0), (0, 1))),
                "2/3": (2, ((0, 0), (0, 1), (1, 0))),
                "3/4": (3, ((0, 0), (0, 1), (1, 0), (2, 1)))}


def _rate(rate) -> str:
    if not isinstance(rate, str) or rate not in RATES:
        raise ValueError(f"rate must be one of {RATES}, got {rate!r}")
    return rate


def puncture_index(rate: str) -> np.ndarray:
    """The 96 kept places of a data symbol's 2 S coded bits (place 2 tau + 0 is A_tau, 2 tau + 1 is B_tau), in sent
    order.  802.11a's patterns, restarting at every symbol: rate 2/3 sends A_tau always and B_tau for even tau; rate
    3/4 sends A_tau for tau mod 3 != 2 and B_tau for tau mod 3 != 1; rate 1/2 sends everything."""
    period, kept = _RATE_PERIOD[_rate(rate)]
    s = RATE_STEPS[rate]
    idx = np.array([2 * (period * p + tau) + ab for p in range(s // period) for tau, ab in kept], np.int64)
    assert len(idx) == 96
    return idx


def rate_info_bits(n_data: int, rate: str = "1/2") -> int:
    """K_info = S D - 6 information bits of a packet of D data symbols at a rate"""
    return INFO_BITS(n_data) + (RATE_STEPS[_rate(rate)] - 48) * int(n_data)


def rate_info_words(n_data: int, rate: str = "1/2") -> int:
    """W_i = ceil(K_info / 32) words of uint32 per packet, MSB first"""
    return (rate_info_bits(n_data, rate) + 31) // 32


def conv_encode_rate(info_words, n_data: int, rate: str = "1/2") -> np.ndarray:
    """The encoder of include/ofdm_mi355x_punct.h, its executable specification: information words uint32
    [n, rate_info_words(n_data, rate)] -> payload words uint32 [n, 3 D].  K_info = S D - 6 information bits and six zero
    tail bits through the mother code; of each data symbol's 2 S coded bits the 96 of puncture_index(rate) are sent,
    through conv_encode's interleaver and precoding.  Rate "1/2" is conv_encode."""
    kinfo, wi = rate_info_bits(n_data, rate), rate_info_words(n_data, rate)
    w = np.ascontiguousarray(np.asarray(info_words).astype(np.uint32, copy=False))
    if w.ndim != 2 or w.shape[1] != wi:
        raise ValueError(f"information words [n, {wi}] expected for {n_data} data symbols at rate {rate}, got {w.shape}")
    u = np.unpackbits(w.astype(">u4").view(np.uint8), axis=1)[:, :kinfo]
    n = len(u)
    u = np.concatenate([u, np.zeros((n, CODE_TAIL), np.uint8)], axis=1)
    c = conv_code_bits(u).reshape(n, n_data, 2 * RATE_STEPS[rate])[:, :, puncture_index(rate)]
    g = np.zeros_like(c)
    g[:, :, interleave_index()] = c
    g[:, :, 1::2] ^= g[:, :, 0::2]
    return _pack_bits(g.reshape(n, 96 * n_data))


def conv_soft_rate(eq, csi=None, rate: str = "1/2") -> np.ndarray:
    """The soft values of include/ofdm_mi355x_punct.h: float32 [n, 2 S D], the two of step t at 2 t and 2 t + 1.  A sent
    position's value is conv_soft's (eq, csi: as there); a stolen place holds +0.0."""
    idx = puncture_index(rate)
    sent = conv_soft(eq, csi)
    n, d, s = len(sent), sent.shape[1] // 96, RATE_STEPS[rate]
    out = np.zeros((n, d, 2 * s), np.float32)
    out[:, :, idx] = sent.reshape(n, d, 96)
    return out.reshape(n, 2 * s * d)


def viterbi_decode_rate(soft, rate: str = "1/2") -> dict:
    """The decoder of include/ofdm_mi355x_punct.h in fp32: viterbi_decode's rule, unchanged, over the S D steps of
    conv_soft_rate's float32 [n, 2 S D]; an erased value takes part as the +0.0 it is.  Returns info (uint32
    [n, rate_info_words(D, rate)]) and path (float32 [n])."""
    s2 = 2 * RATE_STEPS[_rate(rate)]
    lam = np.asarray(soft)
    if lam.dtype != np.float32 or lam.ndim != 2 or lam.shape[1] % s2 or not 1 <= lam.shape[1] // s2 <= MAX_DATA_SYMBOLS:
        raise ValueError(f"soft float32 [n, {s2} D] with 1 <= D <= {MAX_DATA_SYMBOLS} expected at rate {rate}, got "
                         f"{lam.dtype} {lam.shape}")
    return _viterbi(lam)


# ---- self-describing packets (include/ofdm_mi355x_ppdu.h): a header symbol, 802.11a's scrambler and a CRC-32 ----
PPDU_PSDU_WORDS = 31      # OFDM_PPDU_PSDU_WORDS: 124 bytes >= ppdu_cap(15, "3/4")
PPDU_INFO_WORDS = 36      # OFDM_PPDU_INFO_WORDS: the 2 header words and room for 34 more (rate_info_words(14, "3/4") = 32 in use)
PPDU_HEADER_BITS = 42     # INFO_BITS(1): the header symbol is a one-symbol rate-1/2 packet
PPDU_SERVICE_BITS = 16
PPDU_MIN_LENGTH = 4       # the FCS alone
PPDU_BAD_HEADER, PPDU_BAD_SERVICE, PPDU_BAD_FCS = 1, 2, 4       # OFDM_PPDU_BAD_*: the status bits
PPDU_MIN_DATA_SYMBOLS = 2


def scramble_sequence(seed: int, n: int) -> np.ndarray:
    """The first n output bits of 802.11a's scrambler x^7 + x^4 + 1 from the state `seed` (1 .. 127, x7 the top bit):
    per bit out = x7 ^ x4, shifted in at x1.  uint8 [n]; the period is 127."""
    s = int(seed)
    if s != seed or not 1 <= s <= 127:
        raise ValueError(f"seed must be in [1, 127], got {seed!r}")
    return np.resize(_scramble_period(s), int(n))


@functools.lru_cache(maxsize=None)
def _scramble_period(s: int) -> np.ndarray:
    out = np.zeros(127, np.uint8)
    for k in range(127):
        b = ((s >> 6) ^ (s >> 3)) & 1
        out[k] = b
        s = ((s << 1) | b) & 127
    out.setflags(write=False)
    return out


def fcs32(data) -> int:
    """The frame check sequence of a body (bytes): CRC-32 as zlib.crc32 computes it, bit by bit -- reflected polynomial
    0xEDB88320, the register starts at 0xFFFFFFFF, a byte enters at the low end, the result is complemented."""
    c = 0xFFFFFFFF
    for byte in bytes(data):
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def crc8(bits) -> int:
    """The header's CRC-8 over a bit sequence: c = 0xFF; per bit b, f = b ^ (c >> 7), c = ((c << 1) & 0xFF) ^ (7 if f
    else 0); the field is ~c."""
    c = 0xFF
    for b in bits:
        f = (int(b) & 1) ^ (c >> 7)
        c = ((c << 1) & 0xFF) ^ (0x07 if f else 0)
    return c ^ 0xFF


def _ppdu_n_data(n_data) -> int:
    d = int(n_data)
    if d != n_data or not PPDU_MIN_DATA_SYMBOLS <= d <= MAX_DATA_SYMBOLS:
        raise ValueError(f"n_data must be in [{PPDU_MIN_DATA_SYMBOLS}, {MAX_DATA_SYMBOLS}] (a header symbol and at least one "
                         f"data symbol), got {n_data!r}")
    return d


def _ppdu_rate(rate) -> str:
    """a rate as "1/2", "2/3", "3/4" or as its code 0, 1, 2"""
    if isinstance(rate, (int, np.integer)) and not isinstance(rate, bool) and 0 <= int(rate) < len(RATES):
        return RATES[int(rate)]
    return _rate(rate)


def ppdu_cap(n_data: int, rate: str) -> int:
    """The largest LENGTH (PSDU bytes, the four FCS bytes among them) of a packet of D symbols at a rate:
    (S (D - 1) - 6 - 16) // 8.  D = 2 at rate 1/2 gives 3, under the smallest LENGTH of 4."""
    return (rate_info_bits(_ppdu_n_data(n_data) - 1, _ppdu_rate(rate)) - PPDU_SERVICE_BITS) // 8


def _ppdu_header_bits(rate_field: int, length: int) -> np.ndarray:
    b = np.zeros(PPDU_HEADER_BITS, np.uint8)
    b[0:4] = [(rate_field >> (3 - k)) & 1 for k in range(4)]
    b[5:17] = [(length >> (11 - k)) & 1 for k in range(12)]
    b[17] = b[:17].sum() & 1
    c = crc8(b[:18])
    b[18:26] = [(c >> (7 - k)) & 1 for k in range(8)]
    return b


def ppdu_header(rate, length: int) -> np.ndarray:
    """The 42 header bits as 2 words, MSB first: RATE = 5 + the rate's code in bits 0..3, bit 4 zero, LENGTH in bits 5..16,
    even parity over bits 0..16 in bit 17, crc8 of bits 0..17 in bits 18..25, zeros to bit 41.  LENGTH is any 12-bit
    value: ppdu_encode is what refuses one a packet cannot hold."""
    ln = int(length)
    if ln != length or not 0 <= ln < 4096:
        raise ValueError(f"length must be in [0, 4095], got {length!r}")
    return _pack_bits(_ppdu_header_bits(5 + RATES.index(_ppdu_rate(rate)), ln)[None])[0]


def ppdu_header_check(words, n_data: int | None = None):
    """(valid, rate, length) of header words uint32 [n, 2] (or [2]): valid iff RATE is 5, 6 or 7, bit 4 is 0, the parity
    and the CRC-8 are right, bits 26..41 are zero and, with n_data, 4 <= LENGTH <= ppdu_cap(n_data, rate).  rate is the
    rate's code (int32, -1 where invalid) and length int32 (0 where invalid)."""
    w = np.asarray(words).astype(np.uint32, copy=False)
    single = w.ndim == 1
    w = np.ascontiguousarray(w.reshape(-1, 2))
    bits = np.unpackbits(w.astype(">u4").view(np.uint8), axis=1)
    field = bits[:, 0:4] @ (8, 4, 2, 1)
    length = (bits[:, 5:17].astype(np.int64) @ (1 << np.arange(11, -1, -1))).astype(np.int64)
    crc = np.full(len(bits), 0xFF, np.int64)                          # crc8 of bits 0..17, all rows at once
    for k in range(18):
        f = bits[:, k] ^ (crc >> 7)
        crc = ((crc << 1) & 0xFF) ^ (0x07 * f)
    crc ^= 0xFF
    valid = (field >= 5) & (field <= 7) & (bits[:, 4] == 0) & (bits[:, :18].sum(axis=1) % 2 == 0)
    valid &= (bits[:, 18:26] @ (1 << np.arange(7, -1, -1))) == crc
    valid &= ~bits[:, 26:].any(axis=1)
    valid &= length >= PPDU_MIN_LENGTH
    if n_data is not None:
        caps = np.array([ppdu_cap(n_data, r) for r in RATES])
        valid &= length <= caps[np.clip(field - 5, 0, 2)]
    rate = np.where(valid, field - 5, -1).astype(np.int32)
    length = np.where(valid, length, 0).astype(np.int32)
    return (bool(valid[0]), int(rate[0]), int(length[0])) if single else (valid, rate, length)


def ppdu_fill(psdu_words, lengths) -> np.ndarray:
    """The PSDUs as they are sent: uint32 [n, 31] with, per row, the first LENGTH - 4 bytes of psdu_words (MSB first),
    their fcs32 big-endian in the next four and zeros behind; whatever psdu_words hold from byte LENGTH - 4 on is
    ignored."""
    w = np.ascontiguousarray(np.asarray(psdu_words).astype(np.uint32, copy=False))
    ln = np.asarray(lengths, np.int64).reshape(-1)
    if w.ndim != 2 or w.shape[1] != PPDU_PSDU_WORDS or len(ln) != len(w):
        raise ValueError(f"psdu words [n, {PPDU_PSDU_WORDS}] and n lengths expected, got {w.shape} and {ln.shape}")
    if len(ln) and (ln.min() < PPDU_MIN_LENGTH or ln.max() > 4 * PPDU_PSDU_WORDS):
        raise ValueError(f"a LENGTH must be in [{PPDU_MIN_LENGTH}, {4 * PPDU_PSDU_WORDS}]")
    by = w.astype(">u4").view(np.uint8).reshape(len(w), 4 * PPDU_PSDU_WORDS).copy()
    # fcs32 of every row's body at once: the rule's eight steps per byte folded into a table, one byte column at a time
    table = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        table = (table >> 1) ^ np.where(table & 1, np.uint32(0xEDB88320), np.uint32(0))
    crc = np.full(len(w), 0xFFFFFFFF, np.uint32)
    for j in range(int(ln.max()) - 4 if len(ln) else 0):
        crc = np.where(j < ln - 4, (crc >> 8) ^ table[(crc ^ by[:, j]) & 0xFF], crc)
    crc ^= np.uint32(0xFFFFFFFF)
    col = np.arange(by.shape[1])[None, :]
    k = col - (ln[:, None] - 4)                                      # 0..3 in the FCS's place
    fcs = (crc[:, None] >> (8 * (3 - np.clip(k, 0, 3))).astype(np.uint32)) & 0xFF
    by = np.where(k < 0, by, np.where(k < 4, fcs, 0)).astype(np.uint8)
    return np.ascontiguousarray(by).view(">u4").astype(np.uint32)


def ppdu_encode(psdu_words, lengths, rates, seeds, n_data: int, strict: bool = True):
    """The encoder of include/ofdm_mi355x_ppdu.h, its executable specification.  psdu_words: uint32 [n, 31]; lengths, rates
    (codes 0..2 or "1/2", "2/3", "3/4") and seeds (1..127): one per packet; n_data: D symbols, the header's among them.
    Returns (payload words uint32 [n, 3 D], info words uint32 [n, 36]).  An info row holds the 2 header words and then the
    data part's W_i = rate_info_words(D - 1, rate) words: 16 SERVICE zeros, the ppdu_fill PSDU and zeros up to K =
    rate_info_bits(D - 1, rate) bits, all K XORed with scramble_sequence(seed, K); the rest of the row is 0.  The payload
    is conv_encode_rate(header, 1, "1/2") followed by conv_encode_rate(data, D - 1, rate).
    ValueError for a LENGTH outside [4, ppdu_cap], a seed outside [1, 127] or an unknown rate.  strict=False is the
    device encoder's rule for such a packet instead: LENGTH 0 under a RATE field of 0, which no receiver takes for a
    header, and an all-zero data part at rate 1/2."""
    d = _ppdu_n_data(n_data)
    w = np.ascontiguousarray(np.asarray(psdu_words).astype(np.uint32, copy=False))
    n = len(w)
    if w.ndim != 2 or w.shape[1] != PPDU_PSDU_WORDS:
        raise ValueError(f"psdu words [n, {PPDU_PSDU_WORDS}] expected, got {w.shape}")
    ln = np.asarray(lengths).reshape(-1)
    sd = np.asarray(seeds).reshape(-1)
    rt = list(rates) if not isinstance(rates, (str, int, np.integer)) else [rates] * n
    if not (len(ln) == len(sd) == len(rt) == n):
        raise ValueError(f"{n} lengths, rates and seeds expected, got {len(ln)}, {len(rt)} and {len(sd)}")
    info = np.zeros((n, PPDU_INFO_WORDS), np.uint32)
    words = np.zeros((n, 3 * d), np.uint32)
    code = np.full(n, -1)                                            # -1: a refused packet (strict=False)
    for i in range(n):
        try:
            rate = _ppdu_rate(rt[i])
            if int(ln[i]) != ln[i] or not PPDU_MIN_LENGTH <= int(ln[i]) <= ppdu_cap(d, rate):
                raise ValueError(f"packet {i}: LENGTH must be in [{PPDU_MIN_LENGTH}, {ppdu_cap(d, rate)}] for {d} symbols "
                                 f"at rate {rate}, got {ln[i]!r}")
            if int(sd[i]) != sd[i] or not 1 <= int(sd[i]) <= 127:
                raise ValueError(f"packet {i}: seed must be in [1, 127], got {sd[i]!r}")
        except ValueError:
            if strict:
                raise
            info[i, :2] = _pack_bits(_ppdu_header_bits(0, 0)[None])[0]
            continue
        k, wi = rate_info_bits(d - 1, rate), rate_info_words(d - 1, rate)
        bits = np.zeros(k, np.uint8)
        body = ppdu_fill(w[i:i + 1], [int(ln[i])])
        bits[16:16 + 8 * int(ln[i])] = np.unpackbits(body.astype(">u4").view(np.uint8))[:8 * int(ln[i])]
        bits ^= scramble_sequence(int(sd[i]), k)
        info[i, :2] = ppdu_header(rate, int(ln[i]))
        info[i, 2:2 + wi] = _pack_bits(bits[None])[0]
        code[i] = RATES.index(rate)
    words[:, :3] = conv_encode_rate(info[:, :2], 1, "1/2")
    for c, rate in enumerate(RATES):
        rows = np.nonzero(code == c)[0]
        words[rows, 3:] = conv_encode_rate(info[rows, 2:2 + rate_info_words(d - 1, rate)], d - 1, rate)
    return words, info


def _scrambler_seed(state7: int) -> int:
    """the seed whose first seven output bits are `state7`, MSB first: seven steps of the register backwards (0 for 0)"""
    s = int(state7)
    for _ in range(7):
        s = (s >> 1) | (((s & 1) ^ ((s >> 4) & 1)) << 6)
    return s


def ppdu_decode(eq, csi=None) -> dict:
    """The decoder of include/ofdm_mi355x_ppdu.h in fp32, its executable specification.  eq: complex [n, 48 D], 2 <= D <= 15;
    csi: [n, 48] or None.  Columns [0, 48) are decoded as a one-symbol rate-1/2 packet (conv_soft_rate,
    viterbi_decode_rate) and checked (ppdu_header_check with D).  A row whose header fails gets status PPDU_BAD_HEADER,
    rate -1, length 0, seed 0, a zero psdu and path[1] = 0.  Otherwise columns [48, 48 D) are decoded at the header's rate
    with the same gains; the first seven decoded bits are the scrambler's state, from which the seed (seven steps back)
    and the sequence follow -- seven zeros are no state: seed 0, nothing descrambled, PPDU_BAD_SERVICE; descrambled bits
    7..15 other than zero are PPDU_BAD_SERVICE as well; the psdu is the LENGTH bytes behind the 16 SERVICE bits, zeros
    after them; PPDU_BAD_FCS unless its last four bytes are fcs32 of the ones before.
    Returns status, rate, length, seed (int32 [n]), psdu (uint32 [n, 31]) and path (float32 [n, 2]: header, data)."""
    z = np.asarray(eq).astype(np.complex64)
    if z.ndim != 2 or z.shape[1] % 48 or not PPDU_MIN_DATA_SYMBOLS <= z.shape[1] // 48 <= MAX_DATA_SYMBOLS:
        raise ValueError(f"eq [n, 48 D] with {PPDU_MIN_DATA_SYMBOLS} <= D <= {MAX_DATA_SYMBOLS} expected, got {z.shape}")
    n, d = len(z), z.shape[1] // 48
    head = viterbi_decode_rate(conv_soft_rate(z[:, :48], csi, "1/2"), "1/2")
    valid, rate, length = ppdu_header_check(head["info"], d) if n else (np.zeros(0, bool),) * 3
    status = np.where(valid, 0, PPDU_BAD_HEADER).astype(np.int32)
    seed = np.zeros(n, np.int32)
    psdu = np.zeros((n, PPDU_PSDU_WORDS), np.uint32)
    path = np.zeros((n, 2), np.float32)
    path[:, 0] = head["path"]
    w = None if csi is None else np.asarray(csi)
    for code, name in enumerate(RATES):
        rows = np.nonzero(valid & (rate == code))[0]
        if not len(rows):
            continue
        k = rate_info_bits(d - 1, name)
        out = viterbi_decode_rate(conv_soft_rate(z[rows, 48:], None if w is None else w[rows], name), name)
        path[rows, 1] = out["path"]
        bits = np.unpackbits(out["info"].astype(">u4").view(np.uint8), axis=1)[:, :k]
        state = bits[:, :7] @ (64, 32, 16, 8, 4, 2, 1)
        seed[rows] = [_scrambler_seed(v) for v in state]
        sequences = np.zeros((128, k), np.uint8)                      # row 0: seven zeros are no state
        for v in set(seed[rows].tolist()) - {0}:
            sequences[v] = scramble_sequence(v, k)
        bits = bits ^ sequences[seed[rows]]
        status[rows[(state == 0) | bits[:, 7:16].any(axis=1)]] |= PPDU_BAD_SERVICE
        body = np.zeros((len(rows), 8 * 4 * PPDU_PSDU_WORDS), np.uint8)
        room = min(k - 16, body.shape[1])
        body[:, :room] = bits[:, 16:16 + room]
        body[np.arange(body.shape[1])[None, :] >= 8 * length[rows, None]] = 0
        by = np.packbits(body, axis=1)
        psdu[rows] = np.ascontiguousarray(by).view(">u4").astype(np.uint32)
        for i, row, ln in zip(rows, by, length[rows]):
            if int.from_bytes(row[ln - 4:ln].tobytes(), "big") != fcs32(row[:ln - 4].tobytes()):
                status[i] |= PPDU_BAD_FCS
    return dict(status=status, rate=rate, length=length, seed=seed, psdu=psdu, path=path)


def pack_ppdu_messages(texts, n_data: int | None = None, rate="1/2"):
    """One packet per text for ppdu_encode: (psdu words uint32 [n, 31], lengths int32 [n], D).  A text (str, latin-1, or
    bytes) is the PSDU's body, so LENGTH = len + 4; rate is one rate or one per text.  D is n_data, or the smallest
    number of symbols that holds every text at its rate.  ValueError for a text that needs more than 15 symbols or
    more than n_data."""
    rows = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in texts]
    rates = [_ppdu_rate(rate)] * len(rows) if isinstance(rate, (str, int, np.integer)) else [_ppdu_rate(r) for r in rate]
    if len(rates) != len(rows):
        raise ValueError(f"{len(rows)} rates expected, got {len(rates)}")
    need = [next((d for d in range(PPDU_MIN_DATA_SYMBOLS, MAX_DATA_SYMBOLS + 1) if ppdu_cap(d, r) >= len(b) + 4), None)
            for b, r in zip(rows, rates)]
    for b, r, k in zip(rows, rates, need):
        if k is None:
            raise ValueError(f"a text of {len(b)} characters does not fit a packet at rate {r}: {MAX_DATA_SYMBOLS} symbols "
                             f"carry at most {ppdu_cap(MAX_DATA_SYMBOLS, r) - 4}")
    d = max(need, default=PPDU_MIN_DATA_SYMBOLS) if n_data is None else _ppdu_n_data(n_data)
    if need and max(need) > d:
        raise ValueError(f"a text needs {max(need)} symbols, n_data is {d}")
    buf = np.zeros((len(rows), 4 * PPDU_PSDU_WORDS), np.uint8)
    for k, b in enumerate(rows):
        buf[k, :len(b)] = np.frombuffer(b, np.uint8)
    return buf.view(">u4").astype(np.uint32), np.array([len(b) + 4 for b in rows], np.int32), d


def rrc_taps() -> np.ndarray:
    """rcosdesign(0.5, 10, 2, 'sqrt') rounded to fp32 and made symmetric: the receivers' 21 matched-filter taps
    (rrc_design, csrc/ofdm_capi.hip), float64 [21]"""
    beta, sps = 0.5, 2.0
    h = np.zeros(21)
    for i in range(21):
        t = (i - 10) / sps
        q = 4 * beta * t
        if t == 0.0:
            h[i] = -1.0 / (np.pi * sps) * (np.pi * (beta - 1) - 4 * beta)
        elif abs(abs(q) - 1.0) < 1e-12:
            h[i] = 1.0 / (2 * np.pi * sps) * (np.pi * (beta + 1) * np.sin(np.pi * (beta + 1) / (4 * beta))
                                               - 4 * beta * np.sin(np.pi * (beta - 1) / (4 * beta))
                                               + np.pi * (beta - 1) * np.cos(np.pi * (beta - 1) / (4 * beta)))
        else:
            h[i] = -4 * beta / sps * (np.cos((1 + beta) * np.pi * t) + np.sin((1 - beta) * np.pi * t) / q) / (np.pi * (q * q - 1))
    out = (h / np.sqrt((h * h).sum())).astype(np.float32)
    out[11:] = out[:10][::-1]
    return out.astype(np.float64)


def _channel(r) -> np.ndarray:
    """H = L S / 2, S = fft64(LTF1 + LTF2), of rotated frames r [..., >= 320]"""
    return LTF_SIGNS * fft64(r[..., 192:256] + r[..., 256:320]) / 2


def channel_gain(branches, positions, cfo_hz, taps=None) -> np.ndarray:
    """The rule of ofdm_stream_csi (include/ofdm_mi355x_code.h) in double precision: float64 [n_packets, 48],
    csi[i][m] = sum_b |H_b[bin(m)]|^2 over the 48 data bins in d_eq's order.  branches: B recordings [B, n] (or one,
    [n]); positions: the records' packet_pos; cfo_hz: per packet, (double) cfo_coarse_hz + (double) cfo_fine_hz of the
    record -- read, not re-estimated.  Per packet and branch: the matched filter at the frame instants 192 .. 319
    (frame sample ii = sum_tt x[p + 2 ii - tt] taps[tt], samples outside [0, n) read as zero), the rotation by
    exp(-j 2 pi f Ts ii), and H_b = L S_b / 2 with S_b = fft64(LTF1 + LTF2) as combine_branches forms them."""
    xs = np.asarray(branches)
    x = _branches([xs] if xs.ndim == 1 else xs)
    n = x.shape[1]
    h = rrc_taps() if taps is None else np.asarray(taps, np.float64)
    pos = np.asarray(positions, np.int64).reshape(-1)
    f = np.broadcast_to(np.asarray(cfo_hz, np.float64).reshape(-1), pos.shape)
    out = np.zeros((len(pos), 48), np.float64)
    ii = np.arange(192, 320)
    pad = np.zeros((x.shape[0], 640 + 20), np.complex128)
    for i, p in enumerate(pos):
        p = int(p)
        # stream samples p - 20 .. p + 639 at pad index s - (p - 20), zero outside the recording
        pad[:] = 0
        lo, hi = max(p - 20, 0), min(p + 640, n)
        if lo < hi:
            pad[:, lo - (p - 20):hi - (p - 20)] = x[:, lo:hi]
        fr = np.zeros((x.shape[0], 320), np.complex128)
        for tt in range(21):
            fr[:, 192:] += pad[:, 20 + 2 * ii - tt] * h[tt]
        H = _channel(_rotate(fr, float(f[i])))
        out[i] = (np.abs(H[:, list(DATA_BINS)]) ** 2).sum(axis=0)
    return out


def transmit_main(argv=None) -> int:
    """python ofdm_pkg.py transmit: one packet per line of --messages, each behind --gap idle samples (and a closing
    gap), with per-packet carrier offsets and gains, written as a complex64 .npy recording that
    `python ofdm_pkg.py stream --in` decodes line for line."""
    ap = argparse.ArgumentParser(prog="ofdm_pkg.py transmit", description=transmit_main.__doc__)
    ap.add_argument("--messages", required=True, help="a text file, one packet per line (at most 180 characters)")
    ap.add_argument("--out", required=True, help="the recording, a .npy file of complex64 samples at 40 MS/s")
    ap.add_argument("--gap", type=int, default=500, help="idle samples before every packet and after the last")
    ap.add_argument("--n-data", type=int, default=None, help="data symbols per packet (default: what the longest line needs)")
    ap.add_argument("--cfo-hz", default=None, help="carrier offsets in Hz, comma separated, cycled over the packets")
    ap.add_argument("--gain", default=None, help="complex gains, comma separated, cycled, e.g. 1,0.5j,-0.8+0.3j")
    ap.add_argument("--snr", type=float, default=20.0, help="dB, against the mean power of the packets' samples")
    ap.add_argument("--noise", default="none", choices=("real", "complex", "none"))
    ap.add_argument("--taps", default=None, help="multipath FIR over the recording, e.g. 1,0,0.4+0.3j")
    ap.add_argument("--seed", type=int, default=0x80211A)
    a = ap.parse_args(argv)
    if a.gap < 0:
        raise SystemExit("--gap must not be negative")
    import torch  # noqa: PLC0415
    from . import abi  # noqa: PLC0415
    from .channel import impair_stream, parse_taps  # noqa: PLC0415
    from .engine import Engine  # noqa: PLC0415
    texts = [ln for ln in Path(a.messages).read_text(encoding="latin-1").splitlines() if ln]
    if not texts:
        raise SystemExit(f"{a.messages}: no lines")
    words, d = pack_messages(texts, a.n_data)
    n, plen = len(texts), abi.packet_len(d)
    cyc = lambda text, conv, dt: None if text is None else np.resize(np.array([conv(t) for t in text.split(",") if t.strip()], dt), n)
    cfo, gain = cyc(a.cfo_hz, float, np.float32), cyc(a.gain, complex, np.complex64)
    with Engine(0) as eng:
        rec = eng.transmit_packets(words, d, pos0=a.gap, stride=plen + a.gap, gains=gain, cfo_hz=cfo,
                                   n_out=n * (plen + a.gap) + a.gap)
        if a.noise != "none" or a.taps is not None:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(a.seed)
            power = float((rec.real.double() ** 2 + rec.imag.double() ** 2).sum()) / (n * plen)
            rec = impair_stream(rec, power, a.snr, taps=None if a.taps is None else parse_taps(a.taps), noise=a.noise,
                                generator=gen)
        x = rec.cpu().numpy()
    np.save(a.out, x)
    print(f"{n} packets of {d} data symbols ({plen} samples each), {len(x)} samples -> {a.out}", file=sys.stderr)
    return 0


def main(argv=None) -> int:
    """python ofdm_pkg.py stream: decode every packet of a recording (--in rec.npy, complex64) or of a synthetic
    stream; one line per packet and packets.csv under --out."""
    ap = argparse.ArgumentParser(prog="ofdm_pkg.py stream", description=main.__doc__)
    ap.add_argument("--in", dest="rec", help="a .npy file of complex samples at 40 MS/s")
    ap.add_argument("--out", default="stream_out")
    ap.add_argument("--message", default=None, help="the MESSAGE payload packets are checked against")
    ap.add_argument("--frames", type=int, default=8, help="synthetic stream: packets")
    ap.add_argument("--gap", type=int, default=500, help="synthetic stream: idle samples between packets")
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--cfo-hz", type=float, default=0.0)
    ap.add_argument("--taps", default=None, help="multipath FIR, e.g. 1,0,0.4+0.3j")
    ap.add_argument("--noise", default="real", choices=("real", "complex", "none"))
    ap.add_argument("--seed", type=int, default=0x80211A)
    ap.add_argument("--max-packets", type=int, default=None)
    ap.add_argument("--detector", choices=tuple(DETECTORS), default="reference",
                    help="the detection metric: the reference's, or delay-and-correlate with the conjugate at lag 32")
    ap.add_argument("--threshold", type=float, default=THRESHOLD, help="a crossing is M > threshold, inside (0, 1)")
    ap.add_argument("--timing", choices=TIMINGS, default="none",
                    help="ltf: refine every packet's position against the long training field before the decode "
                         "(packets.csv then has a coarse_pos column); ltf-matlab: the same for a recording made "
                         "with the MATLAB transform convention")
    ap.add_argument("--tracking", choices=TRACKINGS, default="none",
                    help="pilots: turn every data symbol back by its four pilots' common phase before the slicer "
                         "(for long packets; costs a little BER on 2-symbol packets)")
    a = ap.parse_args(argv)
    if not 0.0 < a.threshold < 1.0:
        raise SystemExit("--threshold must be inside (0, 1)")
    import torch  # noqa: PLC0415
    from . import abi  # noqa: PLC0415
    from .channel import make_stream, parse_taps  # noqa: PLC0415
    from .engine import Engine  # noqa: PLC0415
    with Engine(0) as eng:
        if a.message is not None:
            eng.set_long_message(a.message)
        if a.rec:
            x = np.load(a.rec)
            if x.ndim != 1 or not np.iscomplexobj(x):
                raise SystemExit(f"{a.rec}: a one-dimensional complex array expected, got {x.dtype} {x.shape}")
            samples = torch.from_numpy(np.ascontiguousarray(x, np.complex64)).cuda()
        else:
            w = torch.from_numpy(eng.transmitter("c", "message")).cuda()
            gen = torch.Generator(device="cuda")
            gen.manual_seed(a.seed)
            samples = make_stream(w, synthetic_segments(len(w) // 10, a.frames, a.gap), a.snr, a.cfo_hz,
                                  taps=None if a.taps is None else parse_taps(a.taps), noise=a.noise, generator=gen)
        out = eng.receive_stream(samples, max_packets=a.max_packets, detector=a.detector, threshold=a.threshold,
                                 timing=a.timing, tracking=a.tracking)
    rec = out["records"]
    timed = a.timing != "none"
    d = Path(a.out)
    d.mkdir(parents=True, exist_ok=True)
    with open(d / "packets.csv", "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["packet_pos", "flags", "cfo_coarse_hz", "cfo_fine_hz", "bit_err", "evm_db_pre", "message"]
                    + (["coarse_pos"] if timed else []))
        for k in range(out["count"]):
            r = rec[k]
            row = [int(r["packet_pos"]), int(r["flags"]), float(r["cfo_coarse_hz"]), float(r["cfo_fine_hz"]),
                   int(r["bit_err"]), float(r["evm_db_pre"]), out["messages"][k]]
            wr.writerow(row + ([int(out["coarse_pos"][k])] if timed else []))
            tags = "".join(t for bit, t in ((abi.CAPTURE_OOB, " oob"), (abi.STREAM_LAST_FRONT, " last-front")) if row[1] & bit)
            print(f"{row[0]:>12d}  flags {row[1]}{tags:<15s} cfo {row[2] + row[3]:+10.1f} Hz  bit_err {row[4]:4d}  {row[6]!r}")
    print(f"{out['found']} packets found, {out['count']} decoded of {len(samples)} samples -> {d / 'packets.csv'}",
          file=sys.stderr)
    return 0


__all__ = ["diversity_metric", "refine_timing_branches", "combine_branches", "fft64", "LTF_SIGNS", "USED_BINS", "MAX_BRANCHES", "SAMPLE_TIME",
           "track_pilots", "slice_bits", "TRACKINGS", "PILOT_BINS", "PILOT_VALUES", "DATA_BINS", "ltf_template", "refine_timing", "TIMINGS", "LTF_START", "TIMING_BACK", "TIMING_FWD", "TIMING_CANDIDATES", "TIMING_FIRST", "TIMING_SPAN",
           "select_packets", "detection_metric", "positions", "DETECTORS", "unpack_cross", "first_packet", "synthetic_segments", "main", "pack_messages",
           "transmit_main", "score_packets", "SCORE_MAX_WINDOW", "NSCORE", "MAX_DATA_SYMBOLS", "THRESHOLD", "FRONT_GAP", "CONFIRM", "PACKET_OFFSET", "LAST_FRONT"]
