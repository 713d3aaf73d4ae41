"""Fine timing for the stream receiver (include/ofdm_mi355x_timing.h), the checks that need no GPU:
stream.ltf_template and stream.refine_timing -- the executable specification of OFDM_TIMING_LTF -- on noise-free
streams of the oracle's waveform, on the detector tests' noisy streams and fading fixture, at the stream's end, and
what the refined positions are worth to the decode; then the header, the binding and the resource report of the new
translation unit.  Each test prints its figures before it asserts."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import detect_ref as ref
import timing_ref as tr
from conftest import ROOT


@pytest.fixture(scope="module")
def tmpl(pkg, oracle):
    return tr.template(oracle)


# ---------------------------------------------------------------- 1. the template
def test_template_is_the_first_long_training_symbol(pkg, oracle, tmpl):
    from ofdm_amd import stream
    assert stream.LTF_START == 394 == 2 * 192 + 10 and stream.TIMING_FIRST == 322 and stream.TIMING_SPAN == tr.SPAN == 640
    assert tmpl.shape == (256,) and tmpl.dtype == np.complex128 and np.array_equal(tmpl[:128], tmpl[128:])
    for d in (1, 2, 5, 15):
        for seed in (100 + d, 200 + d):                               # two payloads
            w = oracle.frame_waveform(ref.bits_of(ref.rand_words(d, 1, seed))[0], "c", True, 1)
            assert len(w) == 2 * (320 + 80 * d) + 20
            t = stream.ltf_template(w)
            assert np.array_equal(t, tmpl), (d, seed)                # exactly 0.0 difference
            assert np.array_equal(w[522:640], t[:118]), (d, seed)    # cyclic: the second symbol repeats the first
    with pytest.raises(ValueError):
        stream.ltf_template(np.zeros(521, np.complex64))
    with pytest.raises(ValueError):
        stream.refine_timing(np.zeros(2000, np.complex64), [100], tmpl[:128])


# ---------------------------------------------------------------- 2. noise-free streams keep their positions
@pytest.mark.parametrize("d,cfo", tr.CLEAN_CASES)
def test_noise_free_positions_do_not_move(pkg, oracle, tmpl, d, cfo):
    from ofdm_amd.stream import refine_timing
    _, x, pos = tr.clean_stream(oracle, d, cfo)
    coarse = tr.coarse_positions(x)
    r = refine_timing(x, coarse, tmpl)
    print(f"D {d} {cfo:9.0f} Hz: coarse {(coarse - pos).tolist()}, refined {(r['positions'] - pos).tolist()}, quality "
          f"{r['quality'].round(4).tolist()}")
    assert len(coarse) == tr.CLEAN_PACKETS
    assert np.array_equal(coarse, pos + 16) and np.array_equal(r["positions"], coarse) and np.array_equal(r["coarse"], coarse)
    assert not r["shift"].any() and r["shift"].dtype == np.int32 and r["positions"].dtype == np.int64
    assert ((r["quality"] > 0.89) & (r["quality"] <= 1.0)).all()     # 200 kHz costs under 10 % of the peak


# ---------------------------------------------------------------- 3. the detector tests' noisy streams
def test_noisy_streams_are_placed_and_have_no_tie(pkg, oracle, tmpl):
    from ofdm_amd.stream import refine_timing
    assert len(ref.STREAM_SEEDS) == 24
    gaps, packets = [], 0
    for (d, snr, cfo, faded), seed in ref.STREAM_SEEDS.items():
        x, pos = ref.noisy_stream(oracle, d, snr, cfo, faded, seed)
        coarse = tr.coarse_positions(x)
        r = refine_timing(x, coarse, tmpl)
        off, _ = tr.offsets(r["positions"], pos)
        coff, _ = tr.offsets(coarse, pos)
        gap = tr.top_gap(r["metric"])
        print(f"D={d:2d} {snr} dB {cfo:7.0f} Hz {'faded  ' if faded else 'unfaded'}: {len(coarse)} packets, coarse "
              f"{int(coff.min())}..{int(coff.max())}, refined {int(off.min())}..{int(off.max())}, smallest gap {gap.min():.3g}, "
              f"quality {r['quality'].min():.3f}..{r['quality'].max():.3f}")
        assert len(coarse) > 0 and (r["quality"] > 0).all()           # every packet lies wholly inside: all are refined
        assert np.array_equal(r["positions"] - coarse, r["shift"]) and (np.diff(r["positions"]) > 0).all()
        assert ((r["shift"] >= -56) & (r["shift"] <= 7)).all()
        if faded:
            assert ((off >= 15) & (off <= 19)).all()
        else:
            assert (off == 16).all()
        assert (gap > 1e-4).all()
        gaps += gap.tolist()
        packets += len(coarse)
    print(f"{packets} packets, smallest relative gap between the two largest L {min(gaps):.4g}")
    assert packets == 290


# ---------------------------------------------------------------- 4. the fading fixture
def test_fading_fixture_refined(pkg, oracle, tmpl):
    from ofdm_amd.stream import refine_timing
    words, taps, x, pos = ref.fading_fixture(oracle)
    truth = ref.bits_of(words)
    coarse = tr.coarse_positions(x)
    r = refine_timing(x, coarse, tmpl)
    assert len(coarse) == 60 and (r["quality"] > 0).all()
    off, coff = r["positions"] - pos, coarse - pos
    print(f"fading fixture: coarse {int(coff.min())}..{int(coff.max())}, refined {int(off.min())}..{int(off.max())}")
    assert ((off >= 15) & (off <= 18)).all()
    errs = [ref.oracle_bit_errors(oracle, x, int(p), truth[k]) for k, p in enumerate(r["positions"])]
    assert errs == [0] * 60


# ---------------------------------------------------------------- 5. bounds
def test_bounds_zero_window_and_quality(pkg, oracle, tmpl):
    from ofdm_amd.stream import refine_timing
    d, snr, cfo, faded = 2, 14, 40e3, False
    x, pos = ref.noisy_stream(oracle, d, snr, cfo, faded, ref.STREAM_SEEDS[(d, snr, cfo, faded)])
    coarse = tr.coarse_positions(x)
    full = refine_timing(x, coarse, tmpl)
    assert full["shift"].any()                                        # the rule has something to do on this stream
    k = int(np.nonzero(full["shift"])[0][-1])
    p = int(coarse[k])
    # the whole search window [p + 322, p + 640] inside the stream, or the packet keeps its position
    inside = refine_timing(x[:p + 641], coarse[:k + 1], tmpl)
    cut = refine_timing(x[:p + 640], coarse[:k + 1], tmpl)
    print(f"packet {k} at {p}: shift {int(full['shift'][k])}; cut at p + 641 {int(inside['shift'][k])}, at p + 640 {int(cut['shift'][k])}")
    assert inside["shift"][k] == full["shift"][k] and inside["quality"][k] == full["quality"][k]
    assert cut["shift"][k] == 0 and cut["quality"][k] == 0.0 and cut["positions"][k] == p and not cut["metric"][k].any()
    assert np.array_equal(cut["positions"][:k], full["positions"][:k])
    # an all-zero window keeps p
    z = x.copy()
    z[p + 322:p + 641] = 0
    zr = refine_timing(z, coarse, tmpl)
    assert zr["positions"][k] == p and zr["shift"][k] == 0 and zr["quality"][k] == 0.0
    assert np.array_equal(np.delete(zr["positions"], k), np.delete(full["positions"], k))
    # quality lies in [0, 1] and does not see the scale of the stream or of the template
    assert ((full["quality"] >= 0) & (full["quality"] <= 1)).all()
    for scale in (2.0 ** 12, 2.0 ** -12):
        s = refine_timing(x.astype(np.complex128) * scale, coarse, tmpl)
        assert np.array_equal(s["positions"], full["positions"]) and np.array_equal(s["quality"], full["quality"])
        s = refine_timing(x, coarse, tmpl * scale)
        assert np.array_equal(s["positions"], full["positions"]) and np.array_equal(s["quality"], full["quality"])
    rng = np.random.default_rng(5)
    noise = rng.standard_normal(3000) + 1j * rng.standard_normal(3000)
    q = refine_timing(noise, [100, 900, 2359, 2360], tmpl)
    print(f"noise alone: quality {q['quality'].round(3).tolist()}")
    assert ((q["quality"][:3] > 0) & (q["quality"][:3] < 0.5)).all() and q["quality"][3] == 0 and q["shift"][3] == 0


# ---------------------------------------------------------------- 6. what it is worth
def test_refined_positions_decode_better(pkg, oracle, tmpl):
    """216 unfaded packets of 2 data symbols at 10 dB and 40 kHz (timing_ref.BENEFIT holds the seeds and the conditions
    on them): the oracle's decode_at makes under a tenth of the bit errors at the refined positions that it makes at
    the coarse ones."""
    from ofdm_amd.stream import refine_timing
    words, x, pos = tr.benefit_stream(oracle)
    truth = ref.bits_of(words)
    coarse = tr.coarse_positions(x)
    r = refine_timing(x, coarse, tmpl)
    coff, idx = tr.offsets(coarse, pos)
    real = (coff >= 0) & (coff < 100)                                 # records that belong to a packet
    off = (r["positions"] - pos[idx])[real]
    x64 = x.astype(np.complex128)
    err = lambda ps: sum(ref.oracle_bit_errors(oracle, x64, int(p), truth[k]) for p, k in zip(ps[real], idx[real]))
    ec, er = err(coarse), err(r["positions"])
    bits = 192 * int(real.sum())
    print(f"{int(real.sum())} of {len(pos)} packets found ({len(coarse)} records); coarse positions {int(coff[real].min())} / "
          f"{np.median(coff[real]):g} / {int(coff[real].max())}, refined {int(off.min())}..{int(off.max())}; bit errors coarse {ec} "
          f"(BER {ec / bits:.3g}), refined {er} (BER {er / bits:.3g})")
    assert real.sum() >= 150
    assert (off == 16).all()
    assert ec >= 10                                                   # the condition on the seeds
    assert er < ec / 10


# ---------------------------------------------------------------- 6b. MATLAB-convention recordings
@pytest.fixture(scope="module")
def tmpl_m(pkg, oracle):
    return tr.template(oracle, "matlab")


def test_matlab_template_is_the_c_template_rotated_by_half_a_period(pkg, oracle, tmpl, tmpl_m):
    from ofdm_amd import stream
    assert np.array_equal(tmpl_m, np.roll(tmpl, -64)) and not np.array_equal(tmpl_m, tmpl)
    for d in (1, 2, 5, 15):
        for seed in (100 + d, 200 + d):                               # two payloads
            bits = ref.bits_of(ref.rand_words(d, 1, seed))[0]
            wm, wc = (oracle.frame_waveform(bits, conv, True, 1) for conv in ("matlab", "c"))
            assert np.array_equal(stream.ltf_template(wm), np.roll(tmpl, -64)), (d, seed)     # exactly 0.0 difference
            k = np.arange(128)
            assert np.array_equal(wm[394 + k], wc[394 + (k + 64) % 128]), (d, seed)
            # the short training field is the same up to rounding (an fp32 step of the peak): detection does not see
            # the convention
            assert np.abs(wm[:320] - wc[:320]).max() <= 2.0 ** -23 * np.abs(wc).max(), (d, seed)


@pytest.mark.parametrize("d,cfo", tr.CLEAN_CASES)
def test_noise_free_matlab_positions_do_not_move(pkg, oracle, tmpl, tmpl_m, d, cfo):
    """under the MATLAB template; and the signature of the defect this value exists for: at 200 kHz the C template
    does not leave a MATLAB-convention packet at its first sample + 16"""
    from ofdm_amd.stream import refine_timing
    words, x, pos = tr.clean_stream(oracle, d, cfo, conv="matlab")
    coarse = tr.coarse_positions(x)
    r, wrong = refine_timing(x, coarse, tmpl_m), refine_timing(x, coarse, tmpl)
    print(f"matlab D {d} {cfo:9.0f} Hz: coarse {(coarse - pos).tolist()}, MATLAB template {(r['positions'] - pos).tolist()} quality "
          f"{r['quality'].round(4).tolist()}; C template {(wrong['positions'] - pos).tolist()} quality {wrong['quality'].round(3).tolist()}")
    assert len(coarse) == tr.CLEAN_PACKETS and np.array_equal(coarse, pos + 16)
    assert np.array_equal(r["positions"], pos + 16) and not r["shift"].any()
    assert ((r["quality"] > 0.89) & (r["quality"] <= 1.0)).all()
    if cfo == 200e3:
        assert not np.array_equal(wrong["positions"], pos + 16)
        assert (wrong["quality"] < r["quality"]).all()
        # what it costs: the oracle's decode has no bit error at the MATLAB template's positions (nor at the coarse ones)
        truth = ref.bits_of(words)
        err = lambda ps: sum(ref.oracle_bit_errors(oracle, x, int(p), truth[k]) for k, p in enumerate(ps))
        ec, er, ew = err(coarse), err(r["positions"]), err(wrong["positions"])
        print(f"matlab D {d} 200 kHz: bit errors coarse {ec}, MATLAB template {er}, C template {ew}")
        assert ec == 0 and er == 0


def test_timing_ltf_matlab_passes_the_argument_check(pkg):
    """2 is a timing now: the call gets as far as everything ofdm_receive_stream_ex refuses, d_timing allowed"""
    lib = pkg.load_library()
    abi = pkg.abi
    opts = abi.make_rx_opts("c")
    fake = C.c_void_p(0x1000)                                         # never dereferenced: the call fails first
    call = lambda so, d_timing: lib.ofdm_receive_stream_timed(
        None, None, 100, C.byref(opts), None if so is None else C.byref(so), abi.TIMING["ltf-matlab"], 1, 4, None, None, None,
        None, None, None, None, d_timing)
    for d_timing in (None, fake):
        assert call(None, d_timing) == -1 and b"ctx" in lib.ofdm_last_error()
        assert call(abi.StreamOpts(2, 0.75), d_timing) == -1 and b"detector" in lib.ofdm_last_error()
        assert call(abi.StreamOpts(1, 1.0), d_timing) == -1 and b"threshold" in lib.ofdm_last_error()


def test_matlab_noisy_streams_are_placed_and_have_no_tie(pkg, oracle, tmpl_m):
    """the conditions on detect_ref.MATLAB_SEEDS that concern the timing (conjugate detector)"""
    from ofdm_amd.stream import refine_timing
    gaps = []
    for key in ref.MATLAB_SEEDS:
        d, snr, cfo, faded = key
        x, pos = ref.matlab_stream(oracle, key)
        coarse = tr.coarse_positions(x)
        r = refine_timing(x, coarse, tmpl_m)
        off, _ = tr.offsets(r["positions"], pos)
        gap = tr.top_gap(r["metric"])
        print(f"matlab D={d:2d} {snr} dB {cfo:7.0f} Hz {'faded  ' if faded else 'unfaded'}: {len(coarse)} packets, refined "
              f"{int(off.min())}..{int(off.max())}, smallest gap {gap.min():.3g}, quality {r['quality'].min():.3f}..{r['quality'].max():.3f}")
        assert len(coarse) == ref.MATLAB_FOUND[key][0] and (r["quality"] > 0).all()
        assert (gap > 1e-4).all()
        assert ((off >= 16) & (off <= 18)).all() if faded else (off == 16).all()
        gaps.append(float(gap.min()))
    print(f"smallest relative gap between the two largest L on the six streams {min(gaps):.4g}")
    assert min(gaps) > 2 * 0.034                                      # the GPU tests' hard bound is half the smallest gap


# ---------------------------------------------------------------- 7. the header, the binding, the build
def test_timing_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.TIMING_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.TIMING_EXPORTS) == ["ofdm_receive_stream_timed"]
    others = (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS) | set(abi.STREAM_EXPORTS)
              | set(abi.TX_EXPORTS) | set(abi.CHANNEL_EXPORTS) | set(abi.FADING_EXPORTS) | set(abi.DETECT_EXPORTS))
    assert not set(names) & others
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_detect.h"' in h
    for other in ("ofdm_mi355x.h", "ofdm_mi355x_stream.h", "ofdm_mi355x_detect.h"):
        text = (ROOT / "include" / other).read_text()
        assert "ofdm_receive_stream_timed" not in text and "OFDM_TIMING_LTF" not in text


def test_stream_timing_layout_matches_the_header(pkg, tmp_path):
    abi = pkg.abi
    st = abi.StreamTiming
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_timing.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(ofdm_stream_timing), '
                   "offsetof(ofdm_stream_timing, coarse_pos), offsetof(ofdm_stream_timing, quality), "
                   "offsetof(ofdm_stream_timing, shift), OFDM_TIMING_NONE, OFDM_TIMING_LTF, OFDM_TIMING_BACK, "
                   "OFDM_TIMING_FWD, OFDM_K_STREAM_TIMING, OFDM_TIMING_LTF_MATLAB); return 0; }\n")
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [16, st.coarse_pos.offset, st.quality.offset, st.shift.offset, abi.TIMING["none"], abi.TIMING["ltf"],
                   abi.TIMING_BACK, abi.TIMING_FWD, abi.K_STREAM_TIMING, abi.TIMING["ltf-matlab"]]
    assert got == [16, 0, 8, 12, 0, 1, 56, 8, 13, 2]
    assert C.sizeof(st) == 16 and abi.K_STREAM_TIMING == abi.K_STREAM_DETECT_CONJ + 1
    dt = abi.stream_timing_dtype()
    assert dt.itemsize == 16 and [dt.fields[n][1] for n in ("coarse_pos", "quality", "shift")] == [0, 8, 12]
    from ofdm_amd import stream
    assert set(abi.TIMING) == set(stream.TIMINGS) and (abi.TIMING_BACK, abi.TIMING_FWD) == (stream.TIMING_BACK, stream.TIMING_FWD)
    assert stream.TIMING_CANDIDATES == 64
    assert abi.timing_code("none") == 0 and abi.timing_code("ltf") == 1 and abi.timing_code("ltf-matlab") == 2
    assert tuple(abi.TIMING) == stream.TIMINGS == ("none", "ltf", "ltf-matlab")
    for bad in ("LTF", "fine", None, 1):
        with pytest.raises(ValueError):
            abi.timing_code(bad)


def test_timing_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    abi = pkg.abi
    opts = abi.make_rx_opts("c")
    conj = abi.StreamOpts(1, 0.75)
    fake = C.c_void_p(0x1000)                                         # never dereferenced: the call fails first
    call = lambda timing, so=None, d_timing=None: lib.ofdm_receive_stream_timed(
        None, None, 100, C.byref(opts), None if so is None else C.byref(so), timing, 1, 4, None, None, None, None, None,
        None, None, d_timing)
    for timing in (3, -1, 7):
        assert call(timing) == -1 and b"timing" in lib.ofdm_last_error(), timing
        assert call(timing, conj, fake) == -1 and b"timing" in lib.ofdm_last_error(), timing
    assert call(0, None, fake) == -1 and b"d_timing" in lib.ofdm_last_error()
    for timing in (0, 1):                                             # everything ofdm_receive_stream_ex refuses
        assert call(timing) == -1 and b"ctx" in lib.ofdm_last_error()
        assert call(timing, abi.StreamOpts(2, 0.75)) == -1 and b"detector" in lib.ofdm_last_error()
        assert call(timing, abi.StreamOpts(1, 1.0)) == -1 and b"threshold" in lib.ofdm_last_error()


def test_timing_kernel_is_built_spill_free_and_the_stream_kernels_did_not_move(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_stream_timing.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_stream_timing.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = [x for x in report if x["source"] == "ofdm_stream_timing.hip"]
    assert {x["name"] for x in rows} == {"ofdm::stream_timing_kernel"}
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        assert x["VGPRs"] <= 128 and x["LDS Size [bytes/block]"] <= 16 * 1024          # four waves per SIMD at least
    # the translation units whose host code takes the hook: their kernels' rows are what they were before it (the decode
    # kernels' rows are what the shared chain, ofdm_rxchain.h, builds to)
    want = {"ofdm::stream_detect_kernel<true>": (188, 64864), "ofdm::stream_detect_kernel<false>": (186, 64864),
            "ofdm::stream_select_kernel<0>": (42, 256), "ofdm::stream_select_kernel<1>": (74, 256),
            "ofdm::stream_select_kernel<2>": (22, 256), "ofdm::stream_decode_kernel<true>": (230, 0),
            "ofdm::stream_decode_kernel<false>": (189, 0), "ofdm::stream_detect_conj_kernel<true>": (193, 64992),
            "ofdm::stream_detect_conj_kernel<false>": (186, 64992), "ofdm::stream_detect_thr_kernel<true>": (152, 64864),
            "ofdm::stream_detect_thr_kernel<false>": (152, 64864)}
    got = {x["name"]: (x["VGPRs"], x["LDS Size [bytes/block]"]) for x in report
           if x["source"] in ("ofdm_stream.hip", "ofdm_stream_conj.hip")}
    assert got == want
