"""The runs behind tests/golden/decode_chain_parent.npz, shared by the test that compares with the fixture
(test_gpu_decode_exact.py) and the script that records it (tools/record_decode_exact.py).

The fixture pins the post-selection decode chain (csrc/ofdm_rxchain.h) of capture_rx_kernel, stream_decode_kernel and
stream_decode_track_kernel to the raw output bytes of the library before the three kernels' copies of it became one.

Inputs are made on the host from fixed seeds, so the recorder and the test see the same bytes (their sha256 is in the
fixture): Engine.transmitter's waveform of the case's message, through the two-tap channel TAPS (notches at a quarter of the band
either side, deep enough for bit errors at an SNR the detector still works at), turned by a CFO, under complex noise of np.random.default_rng.

Streams are zeros(700) | packets x period | zeros(400), cut `cut` samples after the last packet's first sample where the
case has one; each is decoded plain (ofdm_receive_stream) and tracked (ofdm_receive_stream_tracked, pilots):
  d1, d3, d4, d15    1, 3, 4 and 15 data symbols, two or three packets, float_cfo 0 and 1, every combination of
                     d_bits / d_eq (both decode variants) and with and without d_counters;
  d4-odd             the recording passed one sample into its allocation: 8 bytes off a 16-byte line;
  d15-w1             max_packets 1: one wave per block, and a second packet found but not decoded;
  d15-oob, d4-oob    the last packet runs past the stream's end inside its data: oob, 0 < zfirst < D (with and without
                     d_bits / d_eq);
  d4-noltf           the stream ends before the last packet's long training symbols: the NaN rule.
Captures are rows of one batch (every row is named in CAPTURES), pitch odd where the case says so:
  c2, c2-bare        D = 2, cap_len 3008 (fr beside the samples, fr_sep = 0), odd pitch: a packet early in the capture,
                     one so late that lo >= nfr, noise alone (sync fail) and one that runs past the end (oob); with
                     both outputs and with none;
  c2-short           D = 2, cap_len 1400 (fr_sep = 1): past the end, whole, noise alone;
  c15, c15-short     D = 15 at cap_len 9394 (fr_sep = 0) and 4000 (fr_sep = 1) with the same kinds of rows."""
import ctypes as C
import hashlib

import numpy as np

FS = 20e6
TAPS = np.array([1.0, 0.0, 0.0, 0.0, 0.7])
DEFAULT_MSG = b"Hey! I am Vivaswan"
TEXT = (b"One decode chain for the capture, stream and tracking receivers: the same bytes as before. " * 3)[:180]
TRACKING = ("none", "pilots")


def message(nd):
    return TEXT[:12 * nd]


# name -> D, packets, SNR dB, CFO Hz, float_cfo, d_bits, d_eq, d_counters, max_packets, odd offset, cut, seed
STREAMS = {
    "d1": (1, 3, 12.0, 30e3, 1, True, True, True, None, False, None, 11),
    "d3": (3, 2, 10.0, -50e3, 0, False, False, True, None, False, None, 12),
    "d4-odd": (4, 3, 10.0, 10e3, 1, True, False, False, None, True, None, 13),
    "d15-w1": (15, 2, 12.0, 20e3, 1, False, True, True, 1, False, None, 14),
    "d15-oob": (15, 3, 12.0, -15e3, 0, True, True, True, None, False, 16 + 640 + 160 * 7 + 100, 15),
    "d4-oob": (4, 2, 10.0, 0.0, 1, False, False, True, None, True, 16 + 640 + 160 * 2 + 60, 16),
    "d4-noltf": (4, 2, 15.0, 5e3, 1, True, True, True, None, False, 300, 17),
}
NOISY_STREAMS = ("d1", "d3", "d4-odd", "d15-w1", "d15-oob")      # whole packets at 10 or 12 dB behind the notches

# rows of a capture batch: (kind, seed); kinds: see capture_row
ROWS = (("early", 1), ("late", 2), ("noise", 3), ("oob", 4), ("early", 5))
# name -> D, cap_len, odd pitch, SNR dB, CFO Hz, float_cfo, d_bits, d_eq, d_counters
CAPTURES = {
    "c2": (2, 3008, True, 12.0, 25e3, 1, True, True, True),
    "c2-bare": (2, 3008, True, 12.0, 25e3, 1, False, False, False),
    "c2-short": (2, 1400, False, 12.0, -40e3, 0, True, False, True),
    "c15": (15, 9394, True, 12.0, 12e3, 0, False, True, True),
    "c15-short": (15, 4000, False, 12.0, -8e3, 1, False, False, True),
}


def stream_key(name, tracking, field):
    return f"stream|{name}|{tracking}|{field}"


def capture_key(name, field):
    return f"captures|{name}|{field}"


STREAM_FIELDS = ("count", "records", "words", "eq", "counters", "phase")
CAPTURE_FIELDS = ("records", "words", "eq", "counters")


def all_keys():
    keys = [f"input|stream|{n}" for n in STREAMS] + [f"input|captures|{n}" for n in CAPTURES]
    keys += [stream_key(n, t, f) for n in STREAMS for t in TRACKING for f in STREAM_FIELDS]
    keys += [capture_key(n, f) for n in CAPTURES for f in CAPTURE_FIELDS]
    return keys


def sha(x):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8).copy()


def _impair(x, power, snr_db, cfo_hz, seed):
    """the channel TAPS, the CFO, then complex noise at snr_db below `power`, in fp64; complex64 out"""
    x = np.convolve(np.asarray(x, np.complex128), TAPS)[:len(x)]
    x = x * np.exp(2j * np.pi * cfo_hz / FS * np.arange(len(x)))
    rng = np.random.default_rng(seed)
    s = np.sqrt(power / 10 ** (snr_db / 10) / 2)
    return (x + s * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))).astype(np.complex64)


def _wave(engine, nd):
    """Engine.transmitter's ten periods of the nd-symbol message (the engine keeps the message), in fp64"""
    msg = message(nd)
    assert (engine.set_long_message(msg) if nd > 8 else engine.set_message(msg)) == nd
    w = engine.transmitter("c", "message").astype(np.complex128)
    assert len(w) == 10 * (2 * (320 + 80 * nd) + 20)
    return w


def stream_input(wave, name):
    _, packets, snr, cfo, _, _, _, _, _, _, cut, seed = STREAMS[name]
    P = len(wave) // 10
    x = np.concatenate([np.zeros(700), wave[:packets * P], np.zeros(400)])
    x = _impair(x, np.mean(np.abs(wave) ** 2), snr, cfo, seed)
    return x if cut is None else x[:700 + (packets - 1) * P + cut].copy()


def capture_row(wave, nd, L, kind, snr, cfo, seed):
    """early: zeros(300) | the wave (packet_idx near 316); late: the wave from sample 100 on, so the first front that
    counts is the second period's (lo >= nfr); noise: no packet; oob: a packet whose data the capture's end cuts, then
    the 100 samples of another front that the rule needs (tests/test_oob_host.py's construction)"""
    P, power = len(wave) // 10, np.mean(np.abs(wave) ** 2)
    if kind == "early":
        x = np.concatenate([np.zeros(300), wave])[:L]
    elif kind == "late":
        x = wave[100:100 + L]
    elif kind == "noise":
        x = np.zeros(L)
    else:
        keep = 640 + 160 * (nd // 3) + 20                         # the cut falls inside data symbol nd // 3; later ones are zero
        x = np.concatenate([np.zeros(L - keep - 100), wave[:keep], wave[:100]])
    assert len(x) == L and P > 0
    return _impair(x, power, snr, cfo, seed)


def capture_input(wave, name):
    nd, L, _, snr, cfo = CAPTURES[name][:5]
    return np.stack([capture_row(wave, nd, L, kind, snr, cfo, 100 * nd + seed) for kind, seed in ROWS])


def _u32(t):
    """a device tensor's bytes as a host uint32 array: NaN payloads and signed zeros count"""
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint32).copy()


def run_stream(engine, pkg, name):
    """{key: array} of one stream case: its input's sha256 and, plain and tracked, the raw bytes of everything the
    library wrote for the records it counted"""
    import torch
    abi = pkg.abi
    nd, _, _, _, float_cfo, bits, eq, counters, max_packets, odd, _, _ = STREAMS[name]
    out = {}
    try:
        x = stream_input(_wave(engine, nd), name)
        out[f"input|stream|{name}"] = sha(x)
        dev = torch.device("cuda", engine.device)
        buf = torch.zeros(len(x) + 1, dtype=torch.complex64, device=dev)
        t = buf[1:] if odd else buf[:-1]
        assert (t.data_ptr() >> 3) & 1 == int(odd)
        t.copy_(torch.from_numpy(x))
        mp = len(x) // 301 + 1 if max_packets is None else max_packets
        for tracking in TRACKING:
            row = engine.new_counters(1)[0] if counters else None
            pk, cnt, words, zeq, _, _, _, ph = engine._launch_receive_stream(
                t, abi.make_rx_opts("c", opts=dict(float_cfo=float_cfo)), "message", nd, mp, bits, eq, False, False, row,
                abi.make_stream_opts(), abi.timing_code("none"), abi.tracking_code(tracking))
            torch.cuda.synchronize()
            found, count = (int(v) for v in cnt.cpu())
            empty = np.zeros(0, np.uint32)
            res = dict(count=np.array([found, count], np.int64), records=_u32(pk[:count]),
                       words=_u32(words[:count]) if bits else empty, eq=_u32(zeq[:count]) if eq else empty,
                       counters=row.cpu().numpy().copy() if counters else np.zeros(0, np.int64),
                       phase=_u32(ph[:count]) if ph is not None else empty)
            for f in STREAM_FIELDS:
                out[stream_key(name, tracking, f)] = res[f]
    finally:
        engine.set_message(DEFAULT_MSG)
    return out


def run_captures(engine, pkg, name):
    """{key: array} of one capture case: its input's sha256 and the raw bytes of ofdm_receive_captures' outputs"""
    import torch
    abi = pkg.abi
    nd, L, odd, _, _, float_cfo, bits, eq, counters = CAPTURES[name]
    out = {}
    try:
        caps = capture_input(_wave(engine, nd), name)
        out[f"input|captures|{name}"] = sha(caps)
        dev = torch.device("cuda", engine.device)
        n, pitch = len(caps), L + 1 if odd else L
        buf = torch.zeros((n, pitch), dtype=torch.complex64, device=dev)
        buf[:, :L] = torch.from_numpy(caps).to(dev)
        rec = torch.empty((n, C.sizeof(abi.CaptureResult)), dtype=torch.uint8, device=dev)
        words = torch.empty((n, 3 * nd), dtype=torch.int32, device=dev) if bits else None
        zeq = torch.empty((n, 48 * nd), dtype=torch.complex64, device=dev) if eq else None
        row = engine.new_counters(1)[0] if counters else None
        ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())
        opts = abi.make_rx_opts("c", opts=dict(cap_len=L, float_cfo=float_cfo))
        abi.check(engine.lib, engine.lib.ofdm_receive_captures(engine.ctx, ptr(buf), n, pitch, C.byref(opts),
                                                               abi.PAYLOAD["message"], ptr(rec), ptr(words), ptr(zeq),
                                                               ptr(row)), "receive_captures")
        torch.cuda.synchronize()
        empty = np.zeros(0, np.uint32)
        res = dict(records=_u32(rec), words=_u32(words) if bits else empty, eq=_u32(zeq) if eq else empty,
                   counters=row.cpu().numpy().copy() if counters else np.zeros(0, np.int64))
        for f in CAPTURE_FIELDS:
            out[capture_key(name, f)] = res[f]
    finally:
        engine.set_message(DEFAULT_MSG)
    return out
