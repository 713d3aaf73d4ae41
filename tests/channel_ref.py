"""Helpers of tests/test_gpu_channel.py: the 12-packet recording the channel tests share, and the channel of
include/ofdm_mi355x_channel.h in fp64 with the oracle's Gaussians (host code, no GPU)."""
from __future__ import annotations

import numpy as np

TS = 25e-9
STREAM_NOISE = 0x5A000000
GAPS = (700, 400, 301, 1000, 700, 350, 512, 301, 900, 333, 640, 450)
TAIL = 400
N_DATA = 2
PLEN = 2 * (320 + 80 * N_DATA) + 20
SEED = 0x80211A


def layout():
    """positions (int64 [12]) of the packets, each behind its gap, and the recording's length (18,747)"""
    pos, at = [], 0
    for g in GAPS:
        at += g
        pos.append(at)
        at += PLEN
    return np.array(pos, np.int64), at + TAIL


def words():
    return np.random.default_rng(0x11C0).integers(0, 1 << 32, (12, 6), dtype=np.uint64).astype(np.uint32)


def fir64(x, taps) -> np.ndarray:
    """y[i] = sum_j h[j] x[i - j] in fp64, x = 0 in front of the recording, truncated to its length"""
    x = np.asarray(x, np.complex128)
    if taps is None or len(taps) == 0:
        return x.copy()
    return np.convolve(x, np.asarray(taps, np.complex64).astype(np.complex128))[:len(x)]


def rotation64(cfo_hz: float, index0: int, n: int) -> np.ndarray:
    """exp(j 2 pi cfo_hz k 25e-9), k = index0 .. index0 + n - 1, with the revolutions reduced in extended precision"""
    k = np.arange(n, dtype=np.longdouble) + np.longdouble(index0)
    rev = np.longdouble(cfo_hz) * k * np.longdouble(TS)
    frac = (rev - np.rint(rev)).astype(np.float64)
    return np.exp(2j * np.pi * frac)


def noise64(oracle, n: int, sigma2: float, noise: str, trial: int, q: int, seed: int = SEED, index0: int = 0):
    """The header's noise layout with the oracle's Gaussians, in fp64: complex128 [n]"""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    ctr = lambda b: [trial & 0xFFFFFFFF, trial >> 32, b, STREAM_NOISE | q]
    k = np.arange(index0, index0 + n)
    if noise == "real":
        blocks = {int(b): oracle.gauss4(ctr(int(b)), key) for b in np.unique(k >> 2)}
        g = np.array([blocks[int(i) >> 2][int(i) & 3] for i in k])
        return (np.sqrt(sigma2) * g).astype(np.complex128)
    if noise == "complex":
        blocks = {int(b): oracle.gauss4(ctr(int(b)), key) for b in np.unique(k >> 1)}
        g = np.array([complex(blocks[int(i) >> 1][2 * (int(i) & 1)], blocks[int(i) >> 1][2 * (int(i) & 1) + 1]) for i in k])
        return np.sqrt(0.5 * sigma2) * g
    return np.zeros(n, np.complex128)


def channel64(oracle, x, power: float, snr_db: float, cfo_hz: float, taps, noise: str, trial: int, q: int,
              seed: int = SEED) -> np.ndarray:
    """filter, rotation, noise -- all in fp64 -- over the fp32 recording x"""
    y = fir64(x, taps)
    if cfo_hz:
        y = y * rotation64(cfo_hz, 0, len(y))
    return y + noise64(oracle, len(y), power / 10.0 ** (snr_db / 10.0), noise, trial, q, seed)
