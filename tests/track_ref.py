"""Helpers of tests/test_track_host.py and tests/test_gpu_track.py: the streams of the pilot tracking tests
(include/ofdm_mi355x_track.h) and the fp64 rule applied to the oracle's dumps, host code, no GPU."""
from __future__ import annotations

import numpy as np

import detect_ref as ref

GAP = 500
INV_SQRT2 = 1.0 / np.sqrt(2.0)
TAPS3 = (1.0, 0.0, 0.35 + 0.25j)          # the one multipath stream of the parity test
# the parity streams: (D, SNR dB, noise, CFO Hz, taps) -> seed of make_stream's generator.  D = 1: a partly filled quad and
# a subcarrier pass of 48 lanes; 3 -> 4: the step from one quad to two; 4: a pass of exactly 3 x 64; 15: five quads and a
# ragged pass (720 = 11 x 64 + 16).  The condition on a seed (test_track_host): under the fp64 rule alone, at most 0.2 %
# of the subcarriers have an axis inside 1e-4 of the packet's largest |z'|.
PARITY_SEEDS = {(1, 14, "real", 0.0, None): 3101, (1, 8, "complex", 40e3, None): 3102,
                (2, 14, "complex", -90e3, None): 3201, (2, 8, "real", 0.0, None): 3202,
                (3, 14, "real", 40e3, None): 3301, (3, 8, "complex", -90e3, None): 3302,
                (4, 14, "complex", 0.0, None): 3401, (4, 8, "real", 40e3, None): 3402,
                (15, 14, "real", -90e3, None): 4501, (15, 8, "complex", 0.0, None): 4502,
                (15, 14, "complex", 40e3, TAPS3): 4503}
PARITY_PACKETS = 6
AXIS_BAND = 1e-4                          # an axis this close to 0 (of the packet's largest |z'|) may decide either way
# the phase steps of the step test, one per data symbol of a 15-symbol packet, reaching +-1.2 rad
PHI = (0.0, 0.3, -0.5, 0.9, -1.2, 1.2, 0.6, -0.9, 1.0, -0.2, 0.8, -1.1, 0.1, 1.2, -0.7)


def blank_words(d: int) -> np.ndarray:
    """the payload words of d data symbols of blanks, what Engine.set_long_message(" " * 12 d) makes the truth"""
    from ofdm_amd.stream import pack_messages
    return pack_messages([" " * (12 * d)], d)[0]


def blank_truth(d: int) -> np.ndarray:
    return ref.bits_of(blank_words(d))[0]


def noisy_stream(oracle, d: int, snr_db: float, noise: str, cfo_hz: float, taps, seed: int, packets: int = PARITY_PACKETS,
                 gap: int = GAP):
    """`packets` packets of d data symbols of blanks, each behind `gap` idle samples, and a closing gap, through
    channel.make_stream on the CPU: the complex64 recording and the packets' first samples"""
    import torch
    from ofdm_amd.channel import make_stream
    wave = oracle.frame_waveform(blank_truth(d))
    period = len(wave) // 10
    seg = []
    for k in range(packets):
        seg += [("gap", gap), ("wave", (k % 10) * period, (k % 10 + 1) * period)]
    seg.append(("gap", gap))
    gen = torch.Generator()
    gen.manual_seed(seed)
    x = make_stream(torch.from_numpy(wave.astype(np.complex64)), seg, snr_db, cfo_hz, taps=None if taps is None else list(taps),
                    noise=noise, generator=gen).numpy()
    return x, gap + (period + gap) * np.arange(packets, dtype=np.int64)


def window(x, p: int, d: int):
    """the samples the decode at stream position p reads, zero outside the stream, p inside it, and the window's
    samples that lie before the stream's end (the oracle's cap_len: past it the oracle reads zeros and reports oob)"""
    nfr = 320 + 80 * d
    lo = int(p) - 40
    cap = np.zeros(2 * nfr + 100, np.complex128)
    a, b = max(lo, 0), min(lo + len(cap), len(x))
    if b > a:
        cap[a - lo:b - lo] = x[a:b]
    return cap, 40, max(min(len(cap), len(x) - lo), 48)


def truth_axes(truth):
    """the truth's signs per subcarrier: re > 0 iff b0 == b1, im > 0 iff b0 == 0 (D10)"""
    t = np.asarray(truth).reshape(-1, 2)
    return t[:, 0] == t[:, 1], t[:, 0] == 0


def metrics(z, truth) -> dict:
    """bits, bit errors, slicer axis errors, sum |z - ref|^2 and EVM_dB of equalised subcarriers z [48 D] by the
    reference's rules (OFDM.c:852-908, 1104-1161) in fp64"""
    from ofdm_amd.stream import slice_bits
    z = np.asarray(z, np.complex128).reshape(-1)
    tr, ti = truth_axes(truth)
    bits = slice_bits(z)
    with np.errstate(invalid="ignore"):
        pr, pi = z.real > 0, z.imag > 0
    want = INV_SQRT2 * (np.where(tr, 1.0, -1.0) + 1j * np.where(ti, 1.0, -1.0))
    with np.errstate(all="ignore"):
        s = float((np.abs(z - want) ** 2).sum())
        db = max(10 * np.log10(s / len(z)), -400.0) if s > 0 else (-400.0 if s == s else s)
    return dict(bits=bits, bit_err=int((bits != np.asarray(truth)).sum()), axis=int((pr != tr).sum() + (pi != ti).sum()),
                evm_pre_sum=s, evm_db_pre=db)


def fp64_packet(oracle, x, p: int, truth) -> dict:
    """The oracle's decode of the packet at stream position p (Receiver() from the matched filter on, samples outside
    the stream zero) and the fp64 tracking rule on its H and Yf dumps: o (the oracle's answer), t (track_pilots'),
    plain and tracked (metrics of nopilot and of z')"""
    from ofdm_amd.stream import track_pilots
    d = len(truth) // 96
    cap, at, cap_len = window(x, p, d)
    o = oracle.decode_at(cap, truth, at, dumps=True, cap_len=cap_len)
    t = track_pilots(o["Yf"], o["H"])
    return dict(o=o, t=t, plain=metrics(o["nopilot"], truth), tracked=metrics(t["z"].reshape(-1), truth))


def axis_band(z) -> np.ndarray:
    """the subcarriers of one packet whose |Re z| or |Im z| is below AXIS_BAND of the packet's largest |z|: bool [48 D]"""
    z = np.asarray(z, np.complex128).reshape(-1)
    with np.errstate(invalid="ignore"):
        top = np.nanmax(np.abs(z)) if np.isfinite(z).any() else 0.0
        return (np.abs(z.real) < AXIS_BAND * top) | (np.abs(z.imag) < AXIS_BAND * top)


def pilot_floor(t, H) -> np.ndarray:
    """|P_d| is "not near 0" where it is at least a quarter of its noise-free value sum_pilots |H_k|^2: bool [D]"""
    from ofdm_amd.stream import PILOT_BINS
    full = float((np.abs(np.asarray(H)[list(PILOT_BINS)]) ** 2).sum())
    with np.errstate(invalid="ignore"):
        return np.abs(t["P"]) >= 0.25 * full


def wrap(a):
    """a phase difference into (-pi, pi]"""
    return np.angle(np.exp(1j * np.asarray(a, np.float64)))


def step_stream(oracle, d: int = 15, packets: int = 3, phi=PHI, gap: int = GAP):
    """Noise-free packets of d data symbols of blanks whose samples from the middle of data symbol s's cyclic prefix on
    -- 16 samples into it at 40 MS/s, so that the matched filter's 21 taps stay inside the prefix -- are multiplied by
    exp(j phi_s), up to the middle of the next symbol's prefix.  Frame sample k is waveform sample 2 k + 10 (the first
    long training symbol starts at 394 = 2 * 192 + 10), so symbol s's prefix starts at 650 + 160 s."""
    x, pos = ref.packet_stream(oracle, np.repeat(blank_words(d), packets, axis=0), gap=gap)
    for p in pos:
        for s in range(d):
            a = int(p) + 650 + 160 * s + 16
            x[a:a + 160] *= np.exp(1j * phi[s])
    return x.astype(np.complex64), pos
