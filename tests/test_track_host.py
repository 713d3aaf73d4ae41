"""Pilot phase tracking for the stream receiver (include/ofdm_mi355x_track.h), the checks that need no GPU: the
header, the binding and the build of the new translation unit; stream.track_pilots -- the executable specification of
OFDM_TRACK_PILOTS -- on synthetic spectra; what it is worth on this project's own chain (the oracle's decode of noisy
15-symbol and 2-symbol packets); and the seeds of the GPU parity streams.  Each test prints its figures before it
asserts.

Measured here (the oracle's chain at the true position, real noise at 10 dB, 64 packets each, seed 0x7AC): 15 data
symbols 3,446 bit errors without tracking and 4 with it, of 92,160 bits; 2 data symbols 0 without and 0 with, of
12,288 -- at this noise level a 2-symbol packet makes no error either way, so these counts do not show the small cost of
tracking on short packets; the link sweeps on the device do."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import detect_ref as ref
import track_ref as tk
from conftest import ROOT

BENEFIT_PACKETS, BENEFIT_SNR_DB, BENEFIT_SEED = 64, 10.0, 0x7AC


# ---------------------------------------------------------------- 1. the header, the binding, the build
def test_track_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.TRACK_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.TRACK_EXPORTS) == ["ofdm_receive_stream_tracked"]
    others = [v for k, v in vars(abi).items() if k.endswith("EXPORTS") and k != "TRACK_EXPORTS"]
    assert len(others) == 9
    for v in others:
        assert not set(names) & set(v)
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_timing.h"' in h
    for word in ("ofdm_receive_captures", "frame-mode", "smoothing"):     # what is out of scope is said
        assert word in h
    for other in ("ofdm_mi355x.h", "ofdm_mi355x_stream.h", "ofdm_mi355x_detect.h", "ofdm_mi355x_timing.h"):
        text = (ROOT / "include" / other).read_text()
        assert "ofdm_receive_stream_tracked" not in text and "OFDM_TRACK_PILOTS" not in text


def test_track_constants_match_the_header(pkg, tmp_path):
    abi = pkg.abi
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_track.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", OFDM_TRACK_NONE, OFDM_TRACK_PILOTS, '
                   "OFDM_K_STREAM_DECODE_TRACK, OFDM_K_STREAM_TIMING); return 0; }\n")
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [abi.TRACKING["none"], abi.TRACKING["pilots"], abi.K_STREAM_DECODE_TRACK, abi.K_STREAM_TIMING]
    assert got == [0, 1, 14, 13]
    from ofdm_amd import stream
    assert tuple(abi.TRACKING) == stream.TRACKINGS == ("none", "pilots")
    assert abi.tracking_code("none") == 0 and abi.tracking_code("pilots") == 1
    for bad in ("PILOTS", "pilot", "", None, 1, 0):
        with pytest.raises(ValueError):
            abi.tracking_code(bad)
    res, args = abi._TRACK_SIGS["ofdm_receive_stream_tracked"]
    tres, targs = abi._TIMING_SIGS["ofdm_receive_stream_timed"]
    # the timed call's arguments with `tracking` behind `timing` and d_phase at the end
    assert res is tres and args == targs[:6] + [C.c_int] + targs[6:] + [C.c_void_p]


def test_track_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    abi = pkg.abi
    opts = abi.make_rx_opts("c")
    fake = C.c_void_p(0x1000)                                         # never dereferenced: the call fails first
    call = lambda timing, tracking, so=None, d_timing=None, d_phase=None: lib.ofdm_receive_stream_tracked(
        None, None, 100, C.byref(opts), None if so is None else C.byref(so), timing, tracking, 1, 4, None, None, None, None,
        None, None, None, d_timing, d_phase)
    for tracking in (2, -1, 7):
        assert call(0, tracking) == -1 and b"tracking" in lib.ofdm_last_error(), tracking
        assert call(1, tracking, None, fake, fake) == -1 and b"tracking" in lib.ofdm_last_error(), tracking
    assert call(0, 0, None, None, fake) == -1 and b"d_phase" in lib.ofdm_last_error()
    for tracking in (0, 1):                                           # everything ofdm_receive_stream_timed refuses
        assert call(3, tracking) == -1 and b"timing" in lib.ofdm_last_error()
        assert call(0, tracking, None, fake) == -1 and b"d_timing" in lib.ofdm_last_error()
        assert call(0, tracking) == -1 and b"ctx" in lib.ofdm_last_error()
        assert call(1, tracking, abi.StreamOpts(2, 0.75)) == -1 and b"detector" in lib.ofdm_last_error()
        assert call(1, tracking, abi.StreamOpts(1, 1.0)) == -1 and b"threshold" in lib.ofdm_last_error()


def test_link_sweep_refuses_an_unknown_tracking_before_any_launch(pkg):
    from ofdm_amd import sweep

    class NoEngine:                                                   # any use of the engine would raise AttributeError
        pass
    for bad in ("pilot", "PILOTS", None, 1):
        with pytest.raises(ValueError, match="tracking"):
            sweep.link_sweep(NoEngine(), ref.rand_words(2, 4, 1), 2, 500, [20.0], tracking=bad)
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--tracking", "pilot"])
    from ofdm_amd import stream
    with pytest.raises(SystemExit):
        stream.main(["--frames", "2", "--tracking", "pilot"])


def test_track_kernel_is_built_spill_free_and_the_stream_kernels_did_not_move(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_stream_track.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_stream_track.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = [x for x in report if x["source"] == "ofdm_stream_track.hip"]
    assert {x["name"] for x in rows} == {"ofdm::stream_decode_track_kernel"}
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        assert x["VGPRs"] <= 256 and x["Occupancy [waves/SIMD]"] >= 2     # stream_decode_kernel's budget: 512 threads
        assert (x["VGPRs"], x["LDS Size [bytes/block]"]) == (214, 0)      # what the shared chain (ofdm_rxchain.h) builds to
    # the kernels whose translation units share ofdm_stream_decode.h and the decoder hook: the detect and select kernels'
    # rows are what they were, the decode kernels' what the shared chain (ofdm_rxchain.h) builds to
    want = {"ofdm::stream_detect_kernel<true>": (188, 64864), "ofdm::stream_detect_kernel<false>": (186, 64864),
            "ofdm::stream_select_kernel<0>": (42, 256), "ofdm::stream_select_kernel<1>": (74, 256),
            "ofdm::stream_select_kernel<2>": (22, 256), "ofdm::stream_decode_kernel<true>": (230, 0),
            "ofdm::stream_decode_kernel<false>": (189, 0), "ofdm::stream_detect_conj_kernel<true>": (193, 64992),
            "ofdm::stream_detect_conj_kernel<false>": (186, 64992), "ofdm::stream_detect_thr_kernel<true>": (152, 64864),
            "ofdm::stream_detect_thr_kernel<false>": (152, 64864), "ofdm::stream_timing_kernel": None}
    got = {x["name"]: (x["VGPRs"], x["LDS Size [bytes/block]"]) for x in report
           if x["source"] in ("ofdm_stream.hip", "ofdm_stream_conj.hip", "ofdm_stream_timing.hip")}
    assert set(got) == set(want)
    for k, v in want.items():
        assert v is None or got[k] == v, k


# ---------------------------------------------------------------- 2. the rule on synthetic spectra
def _synthetic(seed, d=7):
    """Y = H X u: a channel without a zero, QPSK data, the pilots {1, 1, 1, -1}, one rotation per symbol"""
    from ofdm_amd import stream
    rng = np.random.default_rng(seed)
    H = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    H[np.abs(H) < 0.1] = 0.5
    X = np.zeros((d, 64), np.complex128)
    q = (rng.integers(0, 2, (d, 48)) * 2 - 1 + 1j * (rng.integers(0, 2, (d, 48)) * 2 - 1)) / np.sqrt(2)
    X[:, list(stream.DATA_BINS)] = q
    X[:, list(stream.PILOT_BINS)] = stream.PILOT_VALUES
    phi = rng.uniform(-np.pi, np.pi, d)
    phi[0] = 0.0
    u = np.exp(1j * phi)
    return H, X, q, u, phi


def test_track_pilots_recovers_an_injected_rotation(pkg):
    from ofdm_amd import stream
    assert stream.PILOT_BINS == (11, 25, 39, 53) and stream.PILOT_VALUES == (1.0, 1.0, 1.0, -1.0)
    assert len(stream.DATA_BINS) == 48 and list(stream.DATA_BINS) == sorted(stream.DATA_BINS)
    assert not set(stream.DATA_BINS) & ({0, 1, 2, 3, 4, 5, 32, 59, 60, 61, 62, 63} | set(stream.PILOT_BINS))
    worst = 0.0
    for seed in (1, 2, 3):
        H, X, q, u, phi = _synthetic(seed)
        t = stream.track_pilots(H * X * u[:, None], H)
        dev = max(float(np.abs(t["u"] - u).max()), float(np.abs(tk.wrap(t["phase"] - phi)).max()), float(np.abs(t["z"] - q).max()))
        print(f"seed {seed}: |u - u_injected|, phase and z' deviate by at most {dev:.3g}")
        worst = max(worst, dev)
        assert t["u"].shape == (7,) and t["phase"].shape == (7,) and t["z"].shape == (7, 48) and not t["fallback"].any()
        assert t["u"].dtype == np.complex128 and t["z"].dtype == np.complex128 and t["phase"].dtype == np.float64
        # the oracle's flat dumps are taken as they come
        flat = stream.track_pilots((H * X * u[:, None]).reshape(-1), H)
        assert np.array_equal(flat["z"], t["z"])
    assert worst < 1e-12                                              # exact to fp64 rounding
    with pytest.raises(ValueError):
        stream.track_pilots(np.zeros(63), np.zeros(64))
    with pytest.raises(ValueError):
        stream.track_pilots(np.zeros(64), np.zeros(63))


def test_track_pilots_falls_back_to_one(pkg):
    from ofdm_amd import stream
    H, X, q, u, _ = _synthetic(4, d=5)
    Y = H * X * u[:, None]
    Y[1] = 0.0                                                        # a symbol wholly past the end: P = 0
    Y[2, 11] = np.nan                                                 # a NaN pilot
    Y[3, 25] = np.inf
    t = stream.track_pilots(Y, H)
    assert t["fallback"].tolist() == [False, True, True, True, False]
    assert np.array_equal(t["u"][1:4], np.ones(3)) and np.array_equal(t["phase"][1:4], np.zeros(3))
    assert np.array_equal(t["z"][1], np.zeros(48)) and np.array_equal(stream.slice_bits(t["z"][1]), np.tile([1, 0], 48))
    db = list(stream.DATA_BINS)
    assert np.allclose(t["z"][2], Y[2, db] / H[db]) and np.allclose(t["z"][0], q[0]) and np.allclose(t["z"][4], q[4])
    # S = 0 and Y = 0 (the stream ends before the training symbols): every z is 0 / 0, u = 1, the slicer decides "-"
    t0 = stream.track_pilots(np.zeros((5, 64)), np.zeros(64))
    assert t0["fallback"].all() and np.array_equal(t0["u"], np.ones(5)) and np.isnan(t0["z"][0]).all()
    assert np.array_equal(stream.slice_bits(t0["z"].reshape(-1)), np.tile([1, 0], 48 * 5))
    # four pilots that cancel exactly: |P| = 0 without a zero spectrum
    Yc = np.ones((1, 64), np.complex128)
    Yc[0, [11, 25, 39, 53]] = [1, -1, 1, 1]
    tc = stream.track_pilots(Yc, np.ones(64))
    assert tc["P"][0] == 0 and tc["fallback"][0] and tc["u"][0] == 1 and np.array_equal(tc["z"][0], np.ones(48))


def test_track_pilots_does_not_see_a_common_scale(pkg):
    from ofdm_amd import stream
    H, X, q, u, _ = _synthetic(5)
    Y = H * X * u[:, None]
    base = stream.track_pilots(Y, H)
    for s in (2.0 ** 12, 2.0 ** -12):                                 # powers of two: exact in fp64
        t = stream.track_pilots(s * Y, s * H)
        assert np.array_equal(t["u"], base["u"]) and np.array_equal(t["phase"], base["phase"]) and np.array_equal(t["z"], base["z"])
    t = stream.track_pilots(3.7 * Y, 3.7 * H)
    assert np.allclose(t["u"], base["u"], rtol=0, atol=1e-14) and np.allclose(t["z"], base["z"], rtol=0, atol=1e-13)
    # H alone scaled by a positive factor: u is unchanged, z' scales
    t = stream.track_pilots(Y, 0.5 * H)
    assert np.allclose(t["u"], base["u"], rtol=0, atol=1e-14) and np.allclose(t["z"], 2 * base["z"], rtol=0, atol=1e-13)


def test_rule_without_rotation_is_the_oracles_equaliser(pkg, oracle):
    """Y / H over stream.DATA_BINS is the oracle's own nopilot dump: the bin order of the rule is the reference's"""
    from ofdm_amd import stream
    truth = tk.blank_truth(3)
    w = oracle.frame_waveform(truth, "c", True, 1)
    x = np.concatenate([np.zeros(500), w, np.zeros(500)])
    r = tk.fp64_packet(oracle, x, 516, truth)
    db = list(stream.DATA_BINS)
    z0 = (r["o"]["Yf"].reshape(3, 64)[:, db] / r["o"]["H"][db]).reshape(-1)
    dev = float(np.abs(z0 - r["o"]["nopilot"]).max())
    print(f"Y / H against the oracle's nopilot: {dev:.3g}; phases {r['t']['phase'].round(5).tolist()}")
    assert dev < 1e-12 and r["plain"]["bit_err"] == 0 and r["tracked"]["bit_err"] == 0
    assert np.abs(r["t"]["phase"]).max() < 1e-3
    assert r["plain"]["bit_err"] == int((r["o"]["bits"] != truth).sum())
    assert abs(r["plain"]["evm_db_pre"] - float(r["o"]["res"][0])) < 1e-6


# ---------------------------------------------------------------- 3. what it is worth on the project's own chain
def _bit_errors(oracle, d):
    """BENEFIT_PACKETS C-convention packets of d data symbols with payloads of their own under real noise at
    BENEFIT_SNR_DB, each decoded by the oracle at its true position: total bit errors without and with tracking"""
    words = ref.rand_words(d, BENEFIT_PACKETS, BENEFIT_SEED + d)
    truth = ref.bits_of(words)
    rng = np.random.default_rng(BENEFIT_SEED + 100 + d)
    plain = tracked = 0
    for k in range(BENEFIT_PACKETS):
        w = oracle.frame_waveform(truth[k], "c", True, 1)
        x = np.concatenate([np.zeros(500), w, np.zeros(500)])
        sigma = np.sqrt(np.mean(np.abs(w) ** 2) / 10 ** (BENEFIT_SNR_DB / 10))
        x = x + sigma * rng.standard_normal(len(x))                   # real noise, as OFDM.c:651
        r = tk.fp64_packet(oracle, x, 516, truth[k])                 # first sample + 16: the position of a clean front
        plain += r["plain"]["bit_err"]
        tracked += r["tracked"]["bit_err"]
    return plain, tracked


def test_tracking_pays_on_long_packets(pkg, oracle):
    p15, t15 = _bit_errors(oracle, 15)
    p2, t2 = _bit_errors(oracle, 2)
    print(f"{BENEFIT_PACKETS} packets, real noise at {BENEFIT_SNR_DB:g} dB, the oracle's decode at the true position: 15 data "
          f"symbols {p15} bit errors without tracking, {t15} with ({96 * 15 * BENEFIT_PACKETS} bits); 2 data symbols {p2} "
          f"without, {t2} with ({96 * 2 * BENEFIT_PACKETS} bits)")
    assert BENEFIT_PACKETS >= 60
    assert t15 < p15                                                  # no assertion on the direction for 2 symbols


# ---------------------------------------------------------------- 4. the GPU parity streams' seeds
def test_parity_streams_keep_off_the_axes(pkg, oracle):
    """Under the fp64 rule alone, at the packets' true positions, at most 0.2 % of the subcarriers of the parity
    streams have an axis inside tk.AXIS_BAND of their packet's largest |z'|"""
    assert {k[0] for k in tk.PARITY_SEEDS} == {1, 2, 3, 4, 15} and {k[1] for k in tk.PARITY_SEEDS} == {8, 14}
    assert {k[2] for k in tk.PARITY_SEEDS} == {"real", "complex"} and {k[3] for k in tk.PARITY_SEEDS} == {0.0, 40e3, -90e3}
    assert sum(k[4] is not None for k in tk.PARITY_SEEDS) == 1
    band = total = 0
    for (d, snr, noise, cfo, taps), seed in tk.PARITY_SEEDS.items():
        x, pos = tk.noisy_stream(oracle, d, snr, noise, cfo, taps, seed)
        truth = tk.blank_truth(d)
        n = 0
        for p in pos:
            r = tk.fp64_packet(oracle, x, int(p) + 16, truth)
            n += int(tk.axis_band(r["t"]["z"]).sum())
        print(f"D={d:2d} {snr:2d} dB {noise:7s} {cfo:8.0f} Hz {'3 taps' if taps else '      '}: {n} of {48 * d * len(pos)} subcarriers in the band")
        band, total = band + n, total + 48 * d * len(pos)
    print(f"{band} of {total} subcarriers in the band ({100 * band / total:.3f} %)")
    assert band <= 0.002 * total
