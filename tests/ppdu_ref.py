"""A deliberately plain second implementation of the self-describing packets' rules (include/ofdm_mi355x_ppdu.h), to test
stream.ppdu_* against: Python lists of bits, a shift-register scrambler written from the polynomial, the header built and
parsed field by field, and zlib.crc32 for the FCS.  It imports nothing from stream.py.  Host code, no GPU."""
from __future__ import annotations

import zlib

import numpy as np

STEPS = (48, 64, 72)                  # trellis steps per data symbol, by rate code
RATE_NAMES = ("1/2", "2/3", "3/4")
PSDU_WORDS, INFO_WORDS = 31, 36
BAD_HEADER, BAD_SERVICE, BAD_FCS = 1, 2, 4


def data_bits(n_data: int, rate: int) -> int:
    """K: the information bits of the D - 1 data symbols"""
    return STEPS[rate] * (n_data - 1) - 6


def cap(n_data: int, rate: int) -> int:
    return (data_bits(n_data, rate) - 16) // 8


def scrambler(seed: int, n: int) -> list:
    """x^7 + x^4 + 1 on a register x[1..7] (x[7] the oldest): out = x[7] ^ x[4], then everything moves up one place and
    out enters at x[1].  The seed's top bit is x[7]."""
    x = [None] + [(seed >> k) & 1 for k in range(7)]          # x[1] = bit 0 .. x[7] = bit 6
    out = []
    for _ in range(n):
        b = x[7] ^ x[4]
        out.append(b)
        x = [None, b] + x[1:7]
    return out


def crc8(bits) -> int:
    c = 0xFF
    for b in bits:
        f = b ^ (c >> 7)
        c = (c << 1) & 0xFF
        if f:
            c ^= 0x07
    return ~c & 0xFF


def to_bits(value: int, width: int) -> list:
    return [(value >> (width - 1 - k)) & 1 for k in range(width)]


def from_bits(bits) -> int:
    v = 0
    for b in bits:
        v = 2 * v + int(b)
    return v


def header_bits(rate_field: int, length: int) -> list:
    """the 42 header bits for a RATE field (5 + the rate's code for a real packet) and a LENGTH"""
    b = to_bits(rate_field, 4) + [0] + to_bits(length, 12)
    b.append(sum(b) % 2)
    b += to_bits(crc8(b), 8)
    return b + [0] * 16


def parse_header(bits, n_data: int | None = None):
    """(valid, rate code or -1, LENGTH or 0) of 42 header bits"""
    bits = [int(v) for v in bits]
    field, length = from_bits(bits[0:4]), from_bits(bits[5:17])
    ok = field in (5, 6, 7) and bits[4] == 0 and sum(bits[:18]) % 2 == 0 and from_bits(bits[18:26]) == crc8(bits[:18])
    ok = ok and not any(bits[26:42]) and length >= 4
    if ok and n_data is not None:
        ok = length <= cap(n_data, field - 5)
    return (True, field - 5, length) if ok else (False, -1, 0)


def bytes_to_bits(data: bytes) -> list:
    return [(byte >> (7 - k)) & 1 for byte in data for k in range(8)]


def bits_to_bytes(bits) -> bytes:
    return bytes(from_bits(bits[k:k + 8]) for k in range(0, len(bits), 8))


def build(body: bytes, rate: int, seed: int, n_data: int):
    """(the 42 header bits, the K scrambled data bits, the PSDU bytes as sent) of a packet whose PSDU is body + FCS"""
    psdu = body + zlib.crc32(body).to_bytes(4, "big")
    k = data_bits(n_data, rate)
    assert 4 <= len(psdu) <= cap(n_data, rate) and 1 <= seed <= 127
    plain = [0] * 16 + bytes_to_bits(psdu)
    plain += [0] * (k - len(plain))
    return header_bits(5 + rate, len(psdu)), [p ^ s for p, s in zip(plain, scrambler(seed, k))], psdu


def parse_data(bits, length: int):
    """(status bits, seed, the LENGTH PSDU bytes) of K decoded data bits: the first seven are the scrambler's state after
    seven steps, so the seed is found by trying all 127"""
    bits = [int(v) for v in bits]
    status, seed = 0, 0
    for s in range(1, 128):
        if scrambler(s, 7) == bits[:7]:
            seed = s
    if seed:
        bits = [b ^ s for b, s in zip(bits, scrambler(seed, len(bits)))]
    else:
        status |= BAD_SERVICE
    if any(bits[7:16]):
        status |= BAD_SERVICE
    psdu = bits_to_bytes(bits[16:16 + 8 * length])
    if zlib.crc32(psdu[:-4]) != int.from_bytes(psdu[-4:], "big"):
        status |= BAD_FCS
    return status, seed, psdu


def pack_words(bits, words: int | None = None) -> np.ndarray:
    """bits -> uint32 words, MSB first, zero padded (to `words` words)"""
    n = -(-len(bits) // 32) if words is None else words
    out = [0] * n
    for t, b in enumerate(bits):
        out[t // 32] |= int(b) << (31 - t % 32)
    return np.array(out, np.uint32)


def psdu_words(data: bytes) -> np.ndarray:
    return pack_words(bytes_to_bits(data), PSDU_WORDS)


def random_packets(n_data: int, n: int, seed: int, rates=None, lengths=None):
    """n packets for a test: (bodies, rate codes, lengths, seeds); rate code i % 3 (1 + i % 2 where D = 2, which holds
    no rate-1/2 packet) and a random LENGTH in [4, cap] unless given"""
    rng = np.random.default_rng(seed)
    if rates is None:
        rates = [(1 + i % 2) if n_data == 2 else i % 3 for i in range(n)]
    if lengths is None:
        lengths = [int(rng.integers(4, cap(n_data, r) + 1)) for r in rates]
    bodies = [rng.integers(0, 256, k - 4, dtype=np.uint8).tobytes() for k in lengths]
    seeds = [int(v) for v in rng.integers(1, 128, n)]
    return bodies, list(rates), list(lengths), seeds
