"""A deliberately plain second implementation of the coded link's rules (include/ofdm_mi355x_code.h), to test
stream.conv_encode, stream.conv_soft and stream.viterbi_decode against: per-packet Python loops, a shift-register
encoder and a forward-formulated Viterbi decoder on np.float32 scalars; and the subcarrier-level link model of
tests/test_code_host.py.  Host code, no GPU."""
from __future__ import annotations

import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)
CLAMP = F32(2.0 ** 100)


def info_bits(n_data: int) -> int:
    return 48 * n_data - 6


def info_words(n_data: int) -> int:
    return -(-info_bits(n_data) // 32)


def unpack(words, nbits: int) -> list:
    return [(int(words[t // 32]) >> (31 - t % 32)) & 1 for t in range(nbits)]


def pack(bits) -> list:
    out = [0] * (-(-len(bits) // 32))
    for t, b in enumerate(bits):
        out[t // 32] |= int(b) << (31 - t % 32)
    return out


def step(reg: list, u: int):
    """one step of the K = 7 shift register reg = [u_t-1, .., u_t-6]: (A, B, the new register)"""
    a = u ^ reg[1] ^ reg[2] ^ reg[4] ^ reg[5]            # 133 octal: 1 011 011
    b = u ^ reg[0] ^ reg[1] ^ reg[2] ^ reg[5]            # 171 octal: 1 111 001
    return a, b, [u] + reg[:5]


def code_bits(u) -> list:
    reg, out = [0] * 6, []
    for bit in u:
        a, b, reg = step(reg, int(bit))
        out += [a, b]
    return out


def interleave(k: int) -> int:
    return 6 * (k % 16) + k // 16


def encode_packet(words, n_data: int, precode: bool = True) -> list:
    """information words of one packet -> its 3 D payload words"""
    u = unpack(words, info_bits(n_data)) + [0] * 6
    c = code_bits(u)
    g = [0] * (96 * n_data)
    for d in range(n_data):
        for k in range(96):
            g[96 * d + interleave(k)] = c[96 * d + k]
    b = list(g)
    if precode:
        for m in range(48 * n_data):
            b[2 * m + 1] = g[2 * m] ^ g[2 * m + 1]
    return pack(b)


def qpsk_map(bits) -> np.ndarray:
    """the reference's map on payload bits [.., 2 m]: re > 0 iff b0 == b1, im > 0 iff b0 == 0; unit power"""
    b = np.asarray(bits).reshape(-1, 2)
    re = np.where(b[:, 0] == b[:, 1], 1.0, -1.0)
    im = np.where(b[:, 0] == 0, 1.0, -1.0)
    return (re + 1j * im) / np.sqrt(2)


def soft_packet(eq, csi, n_data: int) -> np.ndarray:
    """one record's soft values in trellis order, float32 [96 D]"""
    z = np.asarray(eq, np.complex64)
    out = np.zeros(96 * n_data, F32)
    for d in range(n_data):
        for k in range(96):
            j = interleave(k)
            m = j // 2
            v = F32(z[48 * d + m].real) if j % 2 else F32(z[48 * d + m].imag)
            w = F32(1) if csi is None else F32(csi[m])
            with np.errstate(all="ignore"):
                lam = F32(w * v)
            if not np.isfinite(lam):
                lam = F32(0)
            lam = min(max(lam, -CLAMP), CLAMP)
            out[96 * d + k] = lam
    return out


def viterbi_packet(soft):
    """One packet, forward formulation: every old state pushes its two branches; a new state keeps the larger candidate
    and on a tie the one from the numerically smaller old state.  The state number is u_t-1 << 5 | .. | u_t-6.
    Returns (information words, the path metric of state 0)."""
    lam = np.asarray(soft, F32)
    steps = len(lam) // 2
    regs = [[(s >> (5 - i)) & 1 for i in range(6)] for s in range(64)]
    number = lambda reg: sum(bit << (5 - i) for i, bit in enumerate(reg))
    metric = [NEG_INF] * 64
    metric[0] = F32(0)
    history = []
    for t in range(steps):
        l0, l1 = lam[2 * t], lam[2 * t + 1]
        new, came = [None] * 64, [None] * 64
        for s in range(64):                               # ascending: a later (larger) old state must be strictly better
            for u in (0, 1):
                a, b, reg = step(regs[s], u)
                inner = F32((-l0 if a else l0) + (-l1 if b else l1))
                cand = F32(metric[s] + inner)
                ns = number(reg)
                if new[ns] is None or cand > new[ns]:
                    new[ns], came[ns] = cand, s
        metric = new
        history.append(came)
    s, u = 0, [0] * steps
    for t in range(steps - 1, -1, -1):
        u[t] = s >> 5
        s = history[t][s]
    return pack(u[:steps - 6]), metric[0]


# ---- test inputs ----
def rand_info(n_data: int, n: int, seed: int) -> np.ndarray:
    """random information words [n, W_i] with the last word's unused bits 0"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, info_bits(n_data)), dtype=np.uint8)
    return np.array([pack(row) for row in bits], np.uint32)


def bits_of(words, nbits=None) -> np.ndarray:
    w = np.ascontiguousarray(np.asarray(words, np.uint32))
    b = np.unpackbits(w.astype(">u4").view(np.uint8), axis=-1)
    return b if nbits is None else b[..., :nbits]


def ideal_eq(words) -> np.ndarray:
    """payload words [n, 3 D] -> the noise-free equalised subcarriers complex64 [n, 48 D]"""
    return qpsk_map(bits_of(words)).reshape(len(words), -1).astype(np.complex64)


# ---- the subcarrier-level link model ----
def model_channel(rng, n: int, pdp) -> np.ndarray:
    """Rayleigh taps of power profile pdp at 40 MS/s seen by the 48 data subcarriers of a 20 MS/s 64-point symbol:
    complex [n, 48], unit mean power; pdp None is the flat unit channel"""
    from ofdm_amd.stream import DATA_BINS
    if pdp is None:
        return np.ones((n, 48), np.complex128)
    p = np.asarray(pdp, np.float64)
    p = p / p.sum()
    h = (rng.standard_normal((n, len(p))) + 1j * rng.standard_normal((n, len(p)))) * np.sqrt(p / 2)
    k = np.asarray(DATA_BINS) - 32
    return h @ np.exp(-2j * np.pi * np.outer(np.arange(len(p)), k) / 128)


def model_receive(rng, payload_bits, H, snr_db: float):
    """payload bits [n, 96 D] through the map, the channel H [n, 48], complex noise, an LS estimate from two training
    symbols and zero-forcing: (z [n, 48 D], |H^|^2 [n, 48])"""
    n, d = len(payload_bits), payload_bits.shape[1] // 96
    x = qpsk_map(payload_bits).reshape(n, d, 48)
    sigma = np.sqrt(10 ** (-snr_db / 10) / 2)
    noise = lambda *shape: sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    y = H[:, None, :] * x + noise(n, d, 48)
    hest = H + (noise(n, 48) + noise(n, 48)) / 2
    return (y / hest[:, None, :]).reshape(n, 48 * d), np.abs(hest) ** 2
