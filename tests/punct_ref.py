"""A deliberately plain second implementation of the punctured rates' rules (include/ofdm_mi355x_punct.h), to test
stream.conv_encode_rate, stream.conv_soft_rate and stream.viterbi_decode_rate against: a per-packet shift-register encoder
with an explicit steal table, written as the standard's sent-order strings, and depuncturing by loops.  The register
step, the Viterbi decoder and the word packing are tests/code_ref.py's.  Host code, no GPU."""
from __future__ import annotations

import numpy as np

from code_ref import F32, interleave, pack, soft_packet, step, unpack, viterbi_packet

# one period of each pattern as 802.11a writes it: the sent bits in order, "A1" the first generator's bit of the period's
# step 1 (IEEE 802.11a-1999, figure 115; the steps of a period counted from 0)
SENT_ORDER = {"1/2": "A0 B0", "2/3": "A0 B0 A1", "3/4": "A0 B0 A1 B2"}
PERIOD = {"1/2": 1, "2/3": 2, "3/4": 3}
STEPS = {"1/2": 48, "2/3": 64, "3/4": 72}
RATE_CODE = {"1/2": 0, "2/3": 1, "3/4": 2}


def steal_table(rate: str) -> list:
    """the kept (step inside the period, 0: A, 1: B) pairs of one period, in sent order"""
    return [(int(name[1:]), "AB".index(name[0])) for name in SENT_ORDER[rate].split()]


def info_bits(n_data: int, rate: str) -> int:
    return STEPS[rate] * n_data - 6


def info_words(n_data: int, rate: str) -> int:
    return -(-info_bits(n_data, rate) // 32)


def sent_bits(u, rate: str) -> list:
    """the bits that are sent for the input bits u (whole periods), the register starting at zero"""
    reg, out, pending = [0] * 6, [], []
    for t, bit in enumerate(u):
        a, b, reg = step(reg, int(bit))
        pending.append((a, b))
        if len(pending) == PERIOD[rate]:
            out += [pending[tau][ab] for tau, ab in steal_table(rate)]
            pending = []
    assert not pending
    return out


def encode_packet(words, n_data: int, rate: str) -> list:
    """information words of one packet -> its 3 D payload words"""
    c = sent_bits(unpack(words, info_bits(n_data, rate)) + [0] * 6, rate)
    assert len(c) == 96 * n_data
    g = [0] * (96 * n_data)
    for d in range(n_data):
        for k in range(96):
            g[96 * d + interleave(k)] = c[96 * d + k]
    b = list(g)
    for m in range(48 * n_data):
        b[2 * m + 1] = g[2 * m] ^ g[2 * m + 1]
    return pack(b)


def depuncture(sent, rate: str) -> np.ndarray:
    """the sent soft values of one record (float32 [96 D], sent order) at their (step, A/B) places: float32 [2 S D], +0.0
    where a bit was stolen"""
    table, period = steal_table(rate), PERIOD[rate]
    out = np.zeros(2 * len(sent) * period // len(table), F32)
    for k, v in enumerate(sent):
        p, r = divmod(k, len(table))
        tau, ab = table[r]
        out[2 * (period * p + tau) + ab] = v
    return out


def soft_packet_rate(eq, csi, n_data: int, rate: str) -> np.ndarray:
    return depuncture(soft_packet(eq, csi, n_data), rate)


def decode_packet(soft):
    """(information words, path metric) of one depunctured row"""
    return viterbi_packet(soft)


def rand_info(n_data: int, n: int, seed: int, rate: str) -> np.ndarray:
    """random information words [n, W_i] with the last word's unused bits 0"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (n, info_bits(n_data, rate)), dtype=np.uint8)
    return np.array([pack(row) for row in bits], np.uint32)


def free_distance(rate: str) -> int:
    """The smallest number of sent ones on a path that leaves the zero state and returns to it, over every puncture
    phase it can leave at: a shortest-path search (Dijkstra) over (register, phase)."""
    import heapq
    kept = {}
    for tau, ab in steal_table(rate):
        kept.setdefault(tau, []).append(ab)
    best = None
    for phase0 in range(PERIOD[rate]):
        def weight(reg, u, phase):
            a, b, new = step(list(reg), u)
            return sum((a, b)[ab] for ab in kept.get(phase, [])), tuple(new)
        w0, reg0 = weight((0,) * 6, 1, phase0)
        heap, seen = [(w0, reg0, (phase0 + 1) % PERIOD[rate])], {}
        while heap:
            w, reg, phase = heapq.heappop(heap)
            if not any(reg):
                best = w if best is None else min(best, w)
                break
            if seen.get((reg, phase), 1 << 30) <= w:
                continue
            seen[(reg, phase)] = w
            for u in (0, 1):
                dw, new = weight(reg, u, phase)
                heapq.heappush(heap, (w + dw, new, (phase + 1) % PERIOD[rate]))
    return best
