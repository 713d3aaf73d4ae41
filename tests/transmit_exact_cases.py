"""The runs behind tests/golden/transmit_chain_parent.npz, shared by the test that compares with the fixture
(test_gpu_transmit_exact.py) and the script that records it (tools/record_transmit_exact.py).

The fixture pins the transmit chain of transmit_kernel (K7), transmit_faded_kernel (K10) and frame_wave_kernel (K4a) to
the raw output bytes of the library before what the three kernels share went into csrc/ofdm_txchain.h.

Words, positions, gains, carrier offsets, taps and the recording's base are made on the host from fixed seeds, so the
recorder and the test see the same bytes (their sha256 is in the fixture).  Every recording starts from a non-zero base,
so samples a kernel must not touch count.  Outputs are kept as 32-bit words: a short recording raw, a long one as the
sha256 of the whole and, per packet, the first DIGEST bytes of the sha256 of its window [pos, pos + len) inside the
recording.  Accumulate runs use packets that do not overlap: every float then receives one atomic add, and the result
does not depend on the order of the adds.

PACKETS, the same shapes for K7 and for K10 (whose packets are L - 1 samples longer; L in brackets):
  d1             D = 1, 63 packets: a full first group of 62 lanes and a second group of one packet; pos0 = 3 and
                 stride = len + 1, so packets on and off a 16-byte line alternate; store, no impairment [L = 1];
  d2-ends        D = 2, MATLAB convention, gain and carrier offset, explicit positions, the recording 8 bytes off a
                 16-byte line: a packet across the recording's start, one at an odd position, one across its end (K10:
                 the end cuts its tail of L - 1 samples), one past the end and one wholly in front, both skipped; raw
                 [L = 3];
  d7-acc         D = 7, carrier offset only, accumulate: eight packets fill 56 lanes and x / 80 runs across seven
                 symbols; pos0 = 2 - len, so the first packet's last two samples (K10: of its tail, which the skip rule
                 must count) are all of it that lies inside [L = 5];
  d15-acc-*      D = 15, nine packets in groups of 4 + 4 + 1, gain only, accumulate, both conventions [L = 32];
  d15-many       D = 15, 2,053 packets, store: on 256 CUs 514 groups on 257 blocks, every block twice round its loop
                 (first = false and the trailing barrier), the last group of one packet; digests only [L = 4];
  d3-*           D = 3, 21 packets (groups of 20 + 1) through every <CONV, IMPAIR, ACC> instance: both conventions,
                 with and without gain and carrier offset, store and accumulate [L = 2].
WAVES: Engine.transmitter for both conventions and messages of 1, 2, 8, 9 and 15 data symbols (set_message up to 8,
set_long_message beyond): the first period raw and the sha256 of the ten repeats.
SWEEPS: one 64-trial frame_sweep at two SNR points of the reference message per convention: integer counters that
depend on every sample of K4a's waveform, on its mean power and on the RRC taps the sync kernel folds."""
import hashlib

import numpy as np

CONVS = ("c", "matlab")
DEFAULT_MSG = b"Hey! I am Vivaswan"
TEXT = (b"One transmit chain for the packet, fading and frame transmitters: the same bytes as before. " * 3)[:180]
DIGEST = 8
RAW_MAX = 4096                   # recordings up to this many samples are kept raw
WAVE_SYMBOLS = (1, 2, 8, 9, 15)
SWEEP_SNRS = (6.0, 10.0)
SWEEP_TRIALS = 64


def _packets(fading):
    L = lambda taps: taps if fading else 1
    c = {"d1": dict(D=1, conv="c", n=63, pos0=3, gap=1, L=L(1), seed=21),
         "d2-ends": dict(D=2, conv="matlab", n=5, ends=True, gain=True, cfo=True, odd=True, L=L(3), seed=22),
         "d7-acc": dict(D=7, conv="c", n=8, pos0="tail", gap=3, cfo=True, acc=True, L=L(5), seed=23)}
    for conv in CONVS:
        c[f"d15-acc-{conv}"] = dict(D=15, conv=conv, n=9, pos0=11, gap=1, gain=True, acc=True, L=L(32), seed=24)
    c["d15-many"] = dict(D=15, conv="c", n=2053, pos0=0, gap=0, L=L(4), seed=25)
    for conv in CONVS:
        for imp in (False, True):
            for acc in (False, True):
                c[f"d3-{conv}-{'impaired' if imp else 'clean'}-{'acc' if acc else 'store'}"] = dict(
                    D=3, conv=conv, n=21, pos0=1, gap=1, gain=imp, cfo=imp, acc=acc, L=L(2), seed=26)
    return c


PACKETS = {"k7": _packets(False), "k10": _packets(True)}


def packet_len(case):
    return 2 * (320 + 80 * case["D"]) + 20 + case["L"] - 1


def layout(kernel, name):
    """(positions, n_out) of a case, on the host"""
    case = PACKETS[kernel][name]
    n, plen = case["n"], packet_len(case)
    if case.get("ends"):
        n_out = 2400 if kernel == "k7" else 2600
        last = n_out - 500 if kernel == "k7" else n_out - plen + 1
        pos = np.array([-400, 601, last, n_out + 10, -plen], np.int64)
        assert len(pos) == n and 601 + plen <= last
        return pos, n_out
    pos0 = 2 - plen if case["pos0"] == "tail" else case["pos0"]
    stride = plen + case["gap"]
    return pos0 + stride * np.arange(n, dtype=np.int64), pos0 + n * stride + (5 if case["gap"] else 0)


def is_raw(kernel, name):
    return layout(kernel, name)[1] <= RAW_MAX


def packet_inputs(kernel, name):
    """words, positions, gains, cfo_hz, taps, base of a case (None where the case has none), all from its seed"""
    case = PACKETS[kernel][name]
    n, D, L = case["n"], case["D"], case["L"]
    rng = np.random.default_rng(case["seed"])
    pos, n_out = layout(kernel, name)
    words = rng.integers(0, 1 << 32, (n, 3 * D), dtype=np.uint64).astype(np.uint32)
    g = rng.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    f = rng.uniform(-100e3, 100e3, n)
    h = (rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))) / np.sqrt(2 * L)
    pattern = (rng.standard_normal(4099) + 1j * rng.standard_normal(4099)).astype(np.complex64)
    return dict(words=words, positions=pos, gains=g.astype(np.complex64) if case.get("gain") else None,
                cfo_hz=f.astype(np.float32) if case.get("cfo") else None,
                taps=h.astype(np.complex64) if kernel == "k10" else None, base=np.resize(pattern, n_out))


def sha(*arrays):
    h = hashlib.sha256()
    for x in arrays:
        if x is not None:
            h.update(np.ascontiguousarray(x).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def window_digests(rec32, pos, plen):
    """per packet the first DIGEST bytes of the sha256 of its window's words (two per sample) inside the recording"""
    n_out = len(rec32) // 2
    return np.stack([sha(rec32[2 * min(max(int(p), 0), n_out):2 * min(max(int(p) + plen, 0), n_out)])[:DIGEST] for p in pos])


def packet_key(kernel, name, field):
    return f"{kernel}|{name}|{field}"


def packet_fields(kernel, name):
    return ("input", "raw") if is_raw(kernel, name) else ("input", "whole", "packets")


def wave_key(conv, nd, field):
    return f"k4a|{conv}|d{nd}|{field}"


def sweep_key(conv):
    return f"sweep|{conv}|counters"


def all_keys():
    keys = [packet_key(k, n, f) for k in PACKETS for n in PACKETS[k] for f in packet_fields(k, n)]
    keys += [wave_key(c, nd, f) for c in CONVS for nd in WAVE_SYMBOLS for f in ("period", "repeats")]
    return keys + [sweep_key(c) for c in CONVS]


def run_packets(engine, kernel, name):
    """{key: array} of one packet case: its inputs' sha256 and the recording the library left, as 32-bit words"""
    import torch
    case = PACKETS[kernel][name]
    x = packet_inputs(kernel, name)
    n_out, odd = len(x["base"]), bool(case.get("odd"))
    dev = torch.device("cuda", engine.device)
    buf = torch.zeros(n_out + 1, dtype=torch.complex64, device=dev)
    rec = buf[1:] if odd else buf[:-1]
    assert (rec.data_ptr() >> 3) & 1 == int(odd)
    rec.copy_(torch.from_numpy(x["base"]))
    dense = not case.get("ends")
    args = dict(positions=None if dense else x["positions"], gains=x["gains"], cfo_hz=x["cfo_hz"], out=rec,
                accumulate=bool(case.get("acc")), conv=case["conv"])
    if dense:
        args.update(pos0=int(x["positions"][0]), stride=packet_len(case) + case["gap"])
    if kernel == "k7":
        engine.transmit_packets(x["words"], case["D"], **args)
    else:
        engine.transmit_faded(x["words"], case["D"], x["taps"], **args)
    torch.cuda.synchronize()
    rec32 = torch.view_as_real(rec).contiguous().cpu().numpy().view(np.uint32).ravel().copy()
    out = {packet_key(kernel, name, "input"): sha(*(x[k] for k in ("words", "positions", "gains", "cfo_hz", "taps", "base")))}
    if is_raw(kernel, name):
        out[packet_key(kernel, name, "raw")] = rec32
    else:
        out[packet_key(kernel, name, "whole")] = sha(rec32)
        out[packet_key(kernel, name, "packets")] = window_digests(rec32, x["positions"], packet_len(case))
    return out


def run_wave(engine, conv, nd):
    """{key: array} of Engine.transmitter for a message of nd data symbols: the first period and the ten repeats' sha256"""
    try:
        msg = TEXT[:12 * nd]
        assert (engine.set_long_message(msg) if nd > 8 else engine.set_message(msg)) == nd
        w = engine.transmitter(conv, "message").view(np.uint32)
        P = 2 * (320 + 80 * nd) + 20
        assert len(w) == 2 * 10 * P
        return {wave_key(conv, nd, "period"): w[:2 * P].copy(), wave_key(conv, nd, "repeats"): sha(w)}
    finally:
        engine.set_message(DEFAULT_MSG)


def run_sweep(engine, pkg, conv):
    """{key: array} of the reference message's frame sweep: the counter rows"""
    engine.set_message(DEFAULT_MSG)
    cnt = engine.frame_sweep(pkg.make_cfg(conv=conv, payload="message"), list(SWEEP_SNRS), SWEEP_TRIALS)
    return {sweep_key(conv): np.asarray(cnt, np.int64).copy()}
