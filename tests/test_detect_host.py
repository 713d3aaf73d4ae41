"""The optional detectors of the stream receiver (include/ofdm_mi355x_detect.h), the checks that need no GPU:
stream.detection_metric and stream.positions -- the executable specification of both detectors -- on noise-free streams
of the oracle's waveform, under carrier offsets and on the fading fixture, and the header, the binding and the resource
report of the new translation unit."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import detect_ref as ref
from conftest import ROOT


def _positions(x, detector, thr=0.75):
    from ofdm_amd.stream import detection_metric, select_packets
    return select_packets(detection_metric(x, detector), thr)["positions"]


# ---------------------------------------------------------------- 1, 2. unfaded noise-free streams
@pytest.mark.parametrize("d", [1, 2, 5, 15])
def test_both_detectors_place_unfaded_packets_alike(pkg, oracle, d):
    x, pos = ref.packet_stream(oracle, ref.rand_words(d, 4, 10 + d))
    got = {det: _positions(x, det) for det in ("reference", "conjugate")}
    print(f"D {d}: packet_pos - first sample {(got['conjugate'] - pos).tolist()}")
    assert len(got["reference"]) == 4
    assert np.array_equal(got["reference"], got["conjugate"])
    assert ((got["conjugate"] - pos) == 16).all()                    # packet offset 16: the front is 5 samples in


@pytest.mark.parametrize("d", [1, 2, 5, 15])
def test_conjugate_positions_do_not_move_with_the_carrier_offset(pkg, oracle, d):
    words = ref.rand_words(d, 4, 20 + d)
    want = _positions(ref.packet_stream(oracle, words)[0], "conjugate")
    assert len(want) == 4
    for cfo in (-90e3, 200e3):
        x = ref.packet_stream(oracle, words, cfo_hz=cfo)[0]
        assert np.array_equal(_positions(x, "conjugate"), want), cfo
        print(f"D {d} {cfo:9.0f} Hz: reference detector {(_positions(x, 'reference')).tolist()}, conjugate {want.tolist()}")


# ---------------------------------------------------------------- 3. positions
def test_positions_at_the_edges(pkg):
    from ofdm_amd.stream import detection_metric, positions
    lib = pkg.load_library()
    for det, halo in (("reference", 47), ("conjugate", 63)):
        code = pkg.abi.DETECTOR[det]
        for n in (0, 1, halo - 1, halo, halo + 1, 63, 64, 10000):
            want = max(n - halo, 0)
            assert positions(n, det) == pkg.abi.stream_positions(n, det) == lib.ofdm_stream_positions(n, code) == want
            assert len(detection_metric(np.ones(n, np.complex64), det)) == want
    assert positions(63, "conjugate") == 0 and positions(64, "conjugate") == 1
    assert positions(63, "reference") == 16 and positions(64, "reference") == 17
    assert lib.ofdm_stream_positions(-5, 1) == 0
    assert lib.ofdm_stream_positions(100, 2) == -1 and b"detector" in lib.ofdm_last_error()
    for bad in ("conj", None, 1):
        with pytest.raises(ValueError):
            positions(100, bad)
        with pytest.raises(ValueError):
            detection_metric(np.zeros(100, np.complex64), bad)
    # a single position is the direct quotient; zero power is NaN for both detectors
    rng = np.random.default_rng(3)
    x = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    c = (x[:32] * np.conj(x[32:])).sum()
    assert abs(detection_metric(x, "conjugate")[0] - abs(c) ** 2 / (np.abs(x[32:]) ** 2).sum() ** 2) < 1e-14
    c = (x[:32] * x[16:48]).sum()
    assert abs(detection_metric(x, "reference")[0] - abs(c) ** 2 / (np.abs(x[16:48]) ** 2).sum() ** 2) < 1e-14
    for det in ("reference", "conjugate"):
        assert np.isnan(detection_metric(np.zeros(200, np.complex64), det)).all()


def test_reference_metric_is_packet_detections(pkg, oracle):
    """detection_metric(x, "reference") is the metric the stream receiver's tests already hold the kernels to"""
    from ofdm_amd.stream import detection_metric
    from test_lazy_rule import corr_out
    x = ref.add_noise(ref.packet_stream(oracle, ref.rand_words(2, 3, 5))[0], 15.0, 3 * 980, 6)
    m, c = detection_metric(x), corr_out(x)
    assert len(m) == len(c) and np.abs(m - c).max() <= 1e-6 * np.abs(c).max()     # corr_out rounds to fp32


# ---------------------------------------------------------------- 4. the fading fixture
def test_fading_fixture(pkg, oracle):
    words, taps, x, pos = ref.fading_fixture(oracle)
    assert taps.shape == (60, 4) and len(x) == 60 * (983 + 500) + 500
    truth = ref.bits_of(words)
    conj, plain = _positions(x, "conjugate"), _positions(x, "reference")
    off = conj - pos[:len(conj)] if len(conj) == 60 else None
    print(f"fading fixture (seed {ref.FADE_SEED:#x}): conjugate {len(conj)} of 60, reference detector {len(plain)}; "
          f"conjugate packet_pos - first sample {None if off is None else (int(off.min()), int(off.max()))}")
    assert len(conj) == 60
    assert ((off >= 8) & (off <= 43)).all()                          # link_sweep's window for four taps
    errs = [ref.oracle_bit_errors(oracle, x, int(p), truth[k]) for k, p in enumerate(conj)]
    assert errs == [0] * 60
    assert len(plain) < 60


# ---------------------------------------------------------------- the GPU tests' streams
def test_gpu_streams_have_no_decision_on_the_threshold(pkg, oracle):
    """the condition on the streams of tests/test_gpu_detect.py (detect_ref.STREAM_SEEDS), and the band's share"""
    from ofdm_amd.stream import detection_metric, select_packets
    assert len(ref.STREAM_SEEDS) == 24
    for (d, snr, cfo, faded), seed in ref.STREAM_SEEDS.items():
        x, pos = ref.noisy_stream(oracle, d, snr, cfo, faded, seed)
        assert 2e4 <= len(x) <= 5e4 and len(x) > 3 * pkg.abi.STREAM_TILE
        m = detection_metric(x, "conjugate")
        assert ref.band_is_harmless(m, 0.75, 0.75e-3), (d, snr, cfo, faded)
        assert len(ref.band_positions(m, 0.75, 0.75e-3)) <= 0.01 * len(m)
        found = len(select_packets(m)["positions"])
        assert found == len(pos) or (faded and found >= 0.75 * len(pos)) or (snr == 14 and found >= len(pos) - 1)


# the largest share of positions inside the band on the six streams, either detector: 3.315e-4 (D = 2, 14 dB, -90 kHz,
# faded, the reference's metric), which is 3.3e-4 to the two figures it is stated with
MATLAB_BAND_SHARE = 3.3e-4


def test_matlab_streams_have_no_decision_on_the_threshold(pkg, oracle):
    """the conditions on the MATLAB-convention streams of tests/test_gpu_matlab_stream.py (detect_ref.MATLAB_SEEDS) that
    concern detection: no decision of either detector in the band, the band's share, what each detector finds.  A
    change of the generators fails here and not on the GPU."""
    from ofdm_amd.stream import detection_metric, select_packets
    assert len(ref.MATLAB_SEEDS) == 6 and set(ref.MATLAB_SEEDS) == set(ref.MATLAB_FOUND)
    for key, seed in ref.MATLAB_SEEDS.items():
        d, snr, cfo, faded = key
        assert seed % 1000 == (12000 + 100 * d + 10 * snr + faded) % 1000 and seed >= 12000       # the scheme
        x, pos = ref.matlab_stream(oracle, key)
        assert x.dtype == np.complex64 and 2e4 <= len(x) <= 5e4 and len(x) > 3 * pkg.abi.STREAM_TILE
        found = {}
        for det in ("reference", "conjugate"):
            m = detection_metric(x, det)
            share = len(ref.band_positions(m, 0.75, 0.75e-3)) / len(m)
            found[det] = len(select_packets(m)["positions"])
            print(f"matlab {key} seed {seed} {det}: {found[det]} of {len(pos)} packets, band share {share:.3g}")
            assert ref.band_is_harmless(m, 0.75, 0.75e-3), (key, det)
            assert round(share, 5) <= MATLAB_BAND_SHARE <= 0.01, (key, det)
        assert (found["conjugate"], len(pos)) == ref.MATLAB_FOUND[key]
        if cfo == 200e3:
            assert found["reference"] == 0
        elif faded:
            assert 4 <= found["reference"] <= 5
    # the default argument is the stream the builders made before they took one
    key = (2, 14, 40e3, False)
    a = ref.noisy_stream(oracle, *key, ref.STREAM_SEEDS[key])
    b = ref.noisy_stream(oracle, *key, ref.STREAM_SEEDS[key], conv="c")
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert a[0].tobytes() != ref.noisy_stream(oracle, *key, ref.STREAM_SEEDS[key], conv="matlab")[0].tobytes()


# ---------------------------------------------------------------- the header, the binding, the build
def test_detect_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.DETECT_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.DETECT_EXPORTS) == ["ofdm_receive_stream_ex", "ofdm_stream_positions"]
    others = (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS) | set(abi.STREAM_EXPORTS)
              | set(abi.TX_EXPORTS) | set(abi.CHANNEL_EXPORTS) | set(abi.FADING_EXPORTS))
    assert not set(names) & others
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    for other in ("ofdm_mi355x.h", "ofdm_mi355x_stream.h"):
        assert "ofdm_receive_stream_ex" not in (ROOT / "include" / other).read_text()


def test_stream_opts_layout_matches_the_header(pkg, tmp_path):
    abi = pkg.abi
    so = abi.StreamOpts
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_detect.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %g\\n", sizeof(ofdm_stream_opts), '
                   "offsetof(ofdm_stream_opts, detector), offsetof(ofdm_stream_opts, threshold), "
                   "offsetof(ofdm_stream_opts, reserved), OFDM_DETECT_REFERENCE, OFDM_DETECT_CONJUGATE, "
                   "OFDM_K_STREAM_DETECT_CONJ, (double)OFDM_DETECT_THRESHOLD); return 0; }\n")
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()
    assert [int(t) for t in got[:7]] == [32, so.detector.offset, so.threshold.offset, so.reserved.offset,
                                         abi.DETECTOR["reference"], abi.DETECTOR["conjugate"], abi.K_STREAM_DETECT_CONJ]
    assert float(got[7]) == abi.DETECT_THRESHOLD == 0.75
    assert C.sizeof(so) == 32 and abi.K_STREAM_DETECT_CONJ == abi.K_DRAW_TAPS + 1
    o = abi.make_stream_opts("conjugate", 0.6)
    assert o.detector == 1 and o.threshold == np.float32(0.6) and not any(o.reserved)
    for bad in (dict(detector="lag32"), dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")),
                dict(threshold=-0.5), dict(threshold="high")):
        with pytest.raises(ValueError):
            abi.make_stream_opts(**bad)
    from ofdm_amd import stream
    assert abi.DETECT_THRESHOLD == stream.THRESHOLD and set(abi.DETECTOR) == set(stream.DETECTORS)
    assert all(abi.DETECT_HALO[k] == 31 + stream.DETECTORS[k][0] for k in abi.DETECTOR)


def test_detect_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    abi = pkg.abi
    opts = abi.make_rx_opts("c")
    call = lambda so: lib.ofdm_receive_stream_ex(None, None, 100, C.byref(opts), None if so is None else C.byref(so), 1, 4,
                                                 None, None, None, None, None, None, None)
    assert call(None) == -1 and b"ctx" in lib.ofdm_last_error()
    assert call(abi.StreamOpts(2, 0.75)) == -1 and b"detector" in lib.ofdm_last_error()
    assert call(abi.StreamOpts(-1, 0.75)) == -1 and b"detector" in lib.ofdm_last_error()
    for thr in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert call(abi.StreamOpts(1, thr)) == -1 and b"threshold" in lib.ofdm_last_error(), thr
    so = abi.StreamOpts(1, 0.75)
    so.reserved[5] = 1
    assert call(so) == -1 and b"reserved" in lib.ofdm_last_error()


def test_detect_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_stream_conj.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_stream_conj.hip"] == []
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_stream_conj.hip"]
    assert {x["name"] for x in rows} == {"ofdm::stream_detect_conj_kernel<true>", "ofdm::stream_detect_conj_kernel<false>",
                                         "ofdm::stream_detect_thr_kernel<true>", "ofdm::stream_detect_thr_kernel<false>"}
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        assert x["VGPRs"] <= 256 and x["LDS Size [bytes/block]"] <= 64 * 1024          # two blocks per CU
        if "conj" in x["name"]:
            assert x["LDS Size [bytes/block]"] == 64992                # two planes of 8,000 floats, 248 bitmap words
