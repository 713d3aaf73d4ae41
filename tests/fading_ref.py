"""Helpers of tests/test_gpu_fading.py and tests/test_fading_host.py: the shapes, the caller taps and the tap stream
of include/ofdm_mi355x_fading.h in fp64 with the oracle's Gaussians (host code, no GPU)."""
from __future__ import annotations

import numpy as np

STREAM_CHAN = 0xC4A00000
SEED = 0x80211A
N = 67
DS = (1, 2, 7, 15)
LS = (1, 2, 4, 5, 32)
EDGE_PACKETS = (0, 61, 62, 66)               # D = 1: a group of 62 packets ends at 61
# g_k [1, 0, 0.4 + 0.3j]: the gains of the loopback
LOOP_GAINS = np.array([1, 0.5j, -0.8 + 0.6j, 0.25 - 0.1j, 2 * np.exp(2.1j)], np.complex128)
LOOP_PROFILE = np.array([1, 0, 0.4 + 0.3j], np.complex128)
LOOP_GAPS = (700, 400, 301, 1000, 700)


def rand_words(d: int, n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, 3 * d), dtype=np.uint64).astype(np.uint32)


def rand_taps(n: int, L: int, seed: int) -> np.ndarray:
    """random complex64 x 0.25, [n, L]"""
    rng = np.random.default_rng(seed)
    return (0.25 * (rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L)))).astype(np.complex64)


def bits_of(words: np.ndarray) -> np.ndarray:
    """[n, 96 D] int32, MSB first"""
    w = np.asarray(words, np.uint32)
    return ((w[..., None] >> np.arange(31, -1, -1, dtype=np.uint32)) & 1).astype(np.int32).reshape(len(w), -1)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def taps64(oracle, seed: int, index0: int, n: int, pdp) -> np.ndarray:
    """The header's tap stream with the oracle's Gaussians in fp64: complex128 [n, len(pdp)].  The amplitude is the
    fp32 value the library multiplies with."""
    pdp = np.asarray(pdp, np.float32)
    amp = np.sqrt(pdp.astype(np.float64) / 2.0).astype(np.float32).astype(np.float64)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    out = np.zeros((n, len(pdp)), np.complex128)
    for k in range(n):
        f = (index0 + k) & 0xFFFFFFFFFFFFFFFF
        for b in range((len(pdp) + 1) // 2):
            z = oracle.gauss4([f & 0xFFFFFFFF, f >> 32, b, STREAM_CHAN], key)
            out[k, 2 * b] = amp[2 * b] * complex(z[0], z[1])
            if 2 * b + 1 < len(pdp):
                out[k, 2 * b + 1] = amp[2 * b + 1] * complex(z[2], z[3])
    return out
