"""Receive diversity for the stream receiver (include/ofdm_mi355x_diversity.h), the checks that need no GPU: the header,
the binding and the build of the new translation unit; the argument checks; stream.diversity_metric,
stream.refine_timing_branches and stream.combine_branches -- the executable specification of the B >= 2 path -- against
the oracle; what diversity is worth under flat Rayleigh fading; the cross-faded stream; and the seeds of the GPU parity
streams.  Each test prints its figures before it asserts.

Measured here (fp64, the rules on the oracle's rxframe dumps at first sample + 16, seed 0xD17): 300 flat-Rayleigh
2-symbol packets at 10 dB, complex noise, 40 kHz offset, bit errors of 57,600: B = 1 2,376, B = 2 192, B = 4 3.
The cross-faded stream (8 packets, D = 2, 20 dB, 40 kHz, weak gain 0.05): either branch alone finds 4, the combined rule 8,
all at + 16 with no bit error; at D = 15 and 14 dB the combined rule finds 6 of 6 at + 16 and makes 10 bit errors
untracked, 0 tracked.  combine_branches with one branch reproduces the oracle's H, Yf and nopilot dumps to 8.2e-16
normwise on a clean and on a noisy packet of 3 data symbols."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import detect_ref as ref
import div_ref as dv
import track_ref as tk
from conftest import ROOT

PAYS_PACKETS, PAYS_SNR_DB, PAYS_CFO, PAYS_SEED = 300, 10.0, 40e3, 0xD17


# ---------------------------------------------------------------- 1. the header, the binding, the build
def test_diversity_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.DIVERSITY_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.DIVERSITY_FUNCTIONS) == ["ofdm_receive_stream_diversity"]
    for k, v in vars(abi).items():
        if k.endswith("EXPORTS"):
            assert not set(names) & set(v), k
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_track.h"' in h
    for word in ("ofdm_receive_captures", "frame-mode", "equal-gain", "noise floors", "would cancel"):
        assert word in h, word
    new = ("ofdm_receive_stream_diversity", "OFDM_DIVERSITY_MAX_BRANCHES", "OFDM_K_STREAM_DETECT_DIV",
           "OFDM_K_STREAM_TIMING_DIV", "OFDM_K_STREAM_DECODE_DIV")
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != abi.DIVERSITY_HEADER.name:
            text = other.read_text()
            for word in new:
                assert word not in text, (other.name, word)


def test_diversity_constants_match_the_header(pkg, tmp_path):
    abi = pkg.abi
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_diversity.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", OFDM_DIVERSITY_MAX_BRANCHES, OFDM_K_STREAM_DETECT_DIV, '
                   "OFDM_K_STREAM_TIMING_DIV, OFDM_K_STREAM_DECODE_DIV, OFDM_K_STREAM_DECODE_TRACK); return 0; }\n")
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [abi.DIVERSITY_MAX_BRANCHES, abi.K_STREAM_DETECT_DIV, abi.K_STREAM_TIMING_DIV, abi.K_STREAM_DECODE_DIV,
                   abi.K_STREAM_DECODE_TRACK]
    assert got == [4, 15, 16, 17, 14]
    from ofdm_amd import stream
    assert stream.MAX_BRANCHES == 4
    res, args = abi._DIVERSITY_SIGS["ofdm_receive_stream_diversity"]
    tres, targs = abi._TRACK_SIGS["ofdm_receive_stream_tracked"]
    # the tracked call's arguments with the branch table and its length in place of d_samples, and d_gain at the end
    assert res is tres and args == targs[:1] + [C.POINTER(C.c_void_p), C.c_int32] + targs[2:] + [C.c_void_p]


def test_diversity_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_stream_div.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_stream_div.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = {x["name"]: x for x in report if x["source"] == "ofdm_stream_div.hip"}
    assert set(rows) == {"ofdm::stream_detect_div_kernel<true>", "ofdm::stream_detect_div_kernel<false>",
                         "ofdm::stream_timing_div_kernel", "ofdm::stream_decode_div_kernel"}
    for name, x in rows.items():
        print(f"{name}: {x['VGPRs']} VGPRs, {x['LDS Size [bytes/block]']} B of static LDS, {x['Occupancy [waves/SIMD]']} waves per SIMD")
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), name
        assert x["VGPRs"] <= 256
    assert rows["ofdm::stream_decode_div_kernel"]["Occupancy [waves/SIMD]"] >= 2      # 512 threads: two waves per SIMD
    # the detector keeps stream_detect_conj_kernel's LDS and two blocks per CU
    for m in ("true", "false"):
        x = rows[f"ofdm::stream_detect_div_kernel<{m}>"]
        assert x["LDS Size [bytes/block]"] == 64992 and x["Occupancy [waves/SIMD]"] >= 2


# ---------------------------------------------------------------- 2. argument errors come before any device work
def test_diversity_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    abi = pkg.abi
    opts = abi.make_rx_opts("c")
    conj, refd = abi.StreamOpts(1, 0.75), abi.StreamOpts(0, 0.75)
    fake = 0x1000                                                     # never dereferenced: the call fails first

    def call(ptrs, nb, n=100, so=conj, timing=0, tracking=0, d_timing=None, d_phase=None, d_gain=None, table=True):
        tab = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if table else None
        return lib.ofdm_receive_stream_diversity(None, tab, nb, n, C.byref(opts), None if so is None else C.byref(so), timing,
                                                 tracking, 1, 4, None, None, None, None, None, None, None, d_timing, d_phase, d_gain)
    err = lib.ofdm_last_error
    for nb in (0, -1, 5, 64):
        assert call([fake] * 4, nb) == -1 and b"n_branches" in err(), nb
    assert call([], 2, table=False) == -1 and b"d_branches is NULL" in err()
    assert call([fake, None], 2) == -1 and b"d_branches[1] is NULL" in err()
    assert call([fake, fake + 4], 2) == -1 and b"d_branches[1] must be 8-byte aligned" in err()
    assert call([None], 1) == -1 and b"d_branches[0] is NULL" in err()
    # with no samples the entries are not looked at: the call goes on to the next check
    assert call([None, None], 2, n=0) == -1 and b"ctx" in err()
    for so in (None, refd):
        for nb in (2, 3, 4):
            assert call([fake] * nb, nb, so=so) == -1 and b"OFDM_DETECT_CONJUGATE" in err() and b"cancel" in err()
    assert call([fake], 1, d_gain=fake) == -1 and b"d_gain" in err()
    # everything ofdm_receive_stream_tracked refuses, for one branch and for more
    for nb in (1, 2, 4):
        p = [fake + 8 * b for b in range(nb)]                         # different 16-byte alignments are fine
        for tracking in (2, -1):
            assert call(p, nb, tracking=tracking) == -1 and b"tracking" in err()
        assert call(p, nb, d_phase=fake) == -1 and b"d_phase" in err()
        assert call(p, nb, timing=3) == -1 and b"timing" in err()
        assert call(p, nb, d_timing=fake) == -1 and b"d_timing" in err()
        assert call(p, nb, so=abi.StreamOpts(2, 0.75)) == -1 and b"detector" in err()
        assert call(p, nb, so=abi.StreamOpts(1, 1.0)) == -1 and b"threshold" in err()
        assert call(p, nb, so=abi.StreamOpts(1, float("nan"))) == -1 and b"threshold" in err()
        bad = abi.StreamOpts(1, 0.75)
        bad.reserved[3] = 1
        assert call(p, nb, so=bad) == -1 and b"reserved" in err()
        assert call(p, nb, timing=1, tracking=1, d_timing=fake, d_phase=fake) == -1 and b"ctx" in err()


def test_link_sweep_refuses_bad_branches_before_any_launch(pkg):
    from ofdm_amd import sweep

    class NoEngine:                                                   # any use of the engine would raise AttributeError
        pass
    words = ref.rand_words(2, 4, 1)
    for bad in (0, 5, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="branches"):
            sweep.link_sweep(NoEngine(), words, 2, 500, [20.0], detector="conjugate", branches=bad)
    for det in ("reference",):
        with pytest.raises(ValueError, match="conjugate"):
            sweep.link_sweep(NoEngine(), words, 2, 500, [20.0], detector=det, branches=2)
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--branches", "2"])
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--branches", "5", "--detector", "conjugate"])


# ---------------------------------------------------------------- 3. the rules against the oracle
def normwise(a, b):
    return float(np.linalg.norm(np.asarray(a).reshape(-1) - np.asarray(b).reshape(-1)) / np.linalg.norm(np.asarray(b).reshape(-1)))


def _d3_packet(oracle, noisy):
    truth = ref.bits_of(ref.rand_words(3, 1, 31))[0]
    w = oracle.frame_waveform(truth, "c", True, 1)
    x = np.concatenate([np.zeros(500), w, np.zeros(500)]) * np.exp(2j * np.pi * 40e3 * ref.TS * np.arange(len(w) + 1000))
    if noisy:
        rng = np.random.default_rng(32)
        sigma = np.sqrt(np.mean(np.abs(w) ** 2) / 10 ** 1.5 / 2)         # 15 dB
        x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    cap, at, cap_len = tk.window(x, 516, 3)
    return truth, oracle.decode_at(cap, truth, at, dumps=True, cap_len=cap_len)


@pytest.mark.parametrize("noisy", [False, True])
def test_one_branch_is_the_oracles_chain(pkg, oracle, noisy):
    from ofdm_amd import stream
    truth, o = _d3_packet(oracle, noisy)
    c = stream.combine_branches(o["rxframe"])
    dev = dict(H=normwise(c["H"][0], o["H"]), Yf=normwise(c["Y"][0], o["Yf"]), nopilot=normwise(c["z"], o["nopilot"]),
               cfo=float(np.abs(np.asarray(c["cfo"]) - o["cfo"]).max() / max(np.abs(o["cfo"]).max(), 1.0)))
    print(f"{'noisy' if noisy else 'clean'} D = 3 packet, combine_branches with one branch against the oracle's dumps: {dev}; "
          f"cfo {c['cfo']} Hz")
    assert c["z"].shape == (3, 48) and c["N"].shape == (3, 64) and c["H"].shape == (1, 64) and c["gain"].shape == (1,)
    assert max(dev.values()) <= 1e-9
    assert abs(sum(c["cfo"]) - 40e3) < (2e3 if noisy else 50)
    assert np.array_equal(stream.slice_bits(c["z"].reshape(-1)), o["bits"])
    # one-dimensional input is one branch; the double-precision CFO is the other option
    assert np.array_equal(stream.combine_branches(o["rxframe"].reshape(-1))["z"], c["z"])
    c64 = stream.combine_branches(o["rxframe"], float_cfo=False)
    assert normwise(c64["z"], c["z"]) < 1e-6 and c64["cfo"] != c["cfo"]
    # tracking on one branch is track_pilots on the oracle's dumps
    t, ct = stream.track_pilots(o["Yf"], o["H"]), stream.combine_branches(o["rxframe"], "pilots")
    assert normwise(ct["z"], t["z"]) <= 1e-9 and np.abs(tk.wrap(ct["phase"] - t["phase"])).max() <= 1e-9
    assert not ct["fallback"].any() and c["u"] is None and c["phase"] is None
    for bad in (np.zeros(399), np.zeros((5, 480)), np.zeros((2, 481))):
        with pytest.raises(ValueError):
            stream.combine_branches(bad)
    with pytest.raises(ValueError):
        stream.combine_branches(o["rxframe"], "pilot")


def test_ltf_signs_and_the_transform_are_the_oracles(pkg, oracle):
    from ofdm_amd import stream
    _, _, lf = oracle.preambles("c")
    assert lf.shape == (64,) and not lf.imag.any()
    assert np.array_equal(stream.LTF_SIGNS, lf.real)
    assert stream.USED_BINS == tuple(sorted(stream.DATA_BINS + stream.PILOT_BINS)) and len(stream.USED_BINS) == 52
    rng = np.random.default_rng(33)
    worst = 0.0
    for _ in range(4):
        v = rng.standard_normal(64) + 1j * rng.standard_normal(64)
        worst = max(worst, normwise(stream.fft64(v), oracle.fft64(v)))
    print(f"stream.fft64 against the oracle's fft: {worst:.3g} normwise")
    assert worst < 1e-13
    assert stream.fft64(np.zeros((2, 3, 64))).shape == (2, 3, 64)
    with pytest.raises(ValueError):
        stream.fft64(np.zeros(63))


def test_identical_branches_and_a_common_scale(pkg, oracle):
    from ofdm_amd import stream
    _, o = _d3_packet(oracle, True)
    f = o["rxframe"]
    one = stream.combine_branches(f, "pilots")
    for nb in (2, 4):
        c = stream.combine_branches(np.stack([f] * nb), "pilots")
        dev = float(np.abs(c["z"] - one["z"]).max())
        print(f"{nb} identical branches against one: |z - z1| at most {dev:.3g}, gains {c['gain'].tolist()}")
        assert dev <= 1e-12 and c["cfo"] == one["cfo"] and np.array_equal(c["gain"], np.repeat(one["gain"], nb))
    rng = np.random.default_rng(34)
    rms = np.sqrt(np.mean(np.abs(f[192:]) ** 2))
    fr = np.stack([f, (0.3 - 0.8j) * f + 0.05 * rms * (rng.standard_normal(len(f)) + 1j * rng.standard_normal(len(f)))])
    base = stream.combine_branches(fr, "pilots")
    for s in (2.0 ** 12, 2.0 ** -12):                                 # powers of two: exact in fp64
        c = stream.combine_branches(s * fr, "pilots")
        assert np.array_equal(c["z"], base["z"]) and np.array_equal(c["phase"], base["phase"]) and c["cfo"] == base["cfo"]
        assert np.array_equal(c["gain"], s * s * base["gain"])
    assert base["gain"][1] == pytest.approx(0.73 * base["gain"][0], rel=0.05)
    # all-zero branches: G = 0, z = 0 / 0, the slicer decides "-"
    z0 = stream.combine_branches(np.zeros((2, 560)), "pilots")
    assert np.isnan(z0["z"]).all() and z0["fallback"].all() and not z0["gain"].any()
    assert np.array_equal(stream.slice_bits(z0["z"].reshape(-1)), np.tile([1, 0], 48 * 3))


def test_diversity_metric_of_one_branch_and_of_a_gap(pkg, oracle):
    from ofdm_amd import stream
    x, pos = ref.packet_stream(oracle, ref.rand_words(2, 3, 35), cfo_hz=40e3)
    m1 = stream.detection_metric(x, "conjugate")
    assert np.array_equal(stream.diversity_metric([x]), m1, equal_nan=True)
    assert np.isnan(m1[:400]).all() and np.isnan(stream.diversity_metric([x, 2 * x, x])[:400]).all()      # an all-zero gap
    # branches of any phase add coherently: the combined metric of rotated copies is one branch's
    m3 = stream.diversity_metric([x, np.exp(2.1j) * x, -0.5j * x])
    ok = np.isfinite(m1)
    dev = float((np.abs(m3[ok] - m1[ok]) / np.maximum(m1[ok], 1.0)).max())      # M is large where the power window is nearly empty
    print(f"three rotated and scaled copies against one branch: |M3 - M1| / max(M1, 1) at most {dev:.3g}")
    assert dev < 1e-12 and np.array_equal(np.isnan(m3), np.isnan(m1))
    assert len(stream.diversity_metric([np.ones(63), np.ones(63)])) == 0 and len(stream.diversity_metric([np.ones(64)] * 2)) == 1
    for bad in ([], [x] * 5, [x, x[:-1]]):
        with pytest.raises(ValueError):
            stream.diversity_metric(bad)
    # one branch through the timing rule is refine_timing
    tpl = dv.c_template(oracle)
    a, b = stream.refine_timing(x, pos + 16, tpl), stream.refine_timing_branches([x], pos + 16, tpl)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    two = stream.refine_timing_branches([x, np.exp(1j) * x], pos + 20, tpl)
    assert np.array_equal(two["positions"], pos + 16) and np.allclose(two["quality"], a["quality"], rtol=1e-12)


# ---------------------------------------------------------------- 4. diversity pays
def _rayleigh_errors(oracle):
    """PAYS_PACKETS 2-symbol packets with payloads of their own, an independent flat Rayleigh gain per packet and branch,
    complex noise at PAYS_SNR_DB against a gain-1 packet and a carrier offset; each decoded by the fp64 rule on the
    oracle's frames at first sample + 16, over the first B of four branches: bit errors for B = 1, 2, 4"""
    from ofdm_amd import stream
    truth = ref.bits_of(ref.rand_words(2, PAYS_PACKETS, PAYS_SEED))
    rng = np.random.default_rng(PAYS_SEED + 1)
    errors = {1: 0, 2: 0, 4: 0}
    for k in range(PAYS_PACKETS):
        w = oracle.frame_waveform(truth[k], "c", True, 1)
        clean = np.concatenate([np.zeros(500), w, np.zeros(500)]) * np.exp(2j * np.pi * PAYS_CFO * ref.TS * np.arange(len(w) + 1000))
        sigma = np.sqrt(np.mean(np.abs(w) ** 2) / 10 ** (PAYS_SNR_DB / 10) / 2)
        g = (rng.standard_normal(4) + 1j * rng.standard_normal(4)) / np.sqrt(2)
        xs = [gb * clean + sigma * (rng.standard_normal(len(clean)) + 1j * rng.standard_normal(len(clean))) for gb in g]
        fr, _ = dv.frames_at(oracle, xs, 516, truth[k])
        for nb in errors:
            z = stream.combine_branches(fr[:nb])["z"]
            errors[nb] += int((stream.slice_bits(z.reshape(-1)) != truth[k]).sum())
    return errors


def test_diversity_pays_under_flat_rayleigh_fading(pkg, oracle):
    e = _rayleigh_errors(oracle)
    print(f"{PAYS_PACKETS} flat-Rayleigh 2-symbol packets at {PAYS_SNR_DB:g} dB, {PAYS_CFO / 1e3:g} kHz, the fp64 rule at first sample + "
          f"16: bit errors of {192 * PAYS_PACKETS}: B = 1 {e[1]}, B = 2 {e[2]}, B = 4 {e[4]}")
    assert PAYS_PACKETS == 300 and e[1] > 0
    assert 2 * e[2] <= e[1]
    assert e[4] <= e[2]


# ---------------------------------------------------------------- 5. the cross-faded stream
def test_cross_faded_stream_needs_both_branches(pkg, oracle):
    from ofdm_amd import stream
    words, xs, pos = dv.cross_faded(oracle)
    truth = tk.blank_truth(2)
    assert xs.shape[0] == 2 and len(pos) == 8 and xs.dtype == np.complex64
    alone = [stream.select_packets(stream.detection_metric(x.astype(np.complex128), "conjugate"))["positions"] for x in xs]
    r = dv.fp64_receive(oracle, xs, dv.c_template(oracle))
    errs = [dv.fp64_packet(oracle, xs, int(p), truth)["m"]["bit_err"] for p in r["tim"]["positions"]]
    print(f"cross-faded stream: branch 0 alone finds {len(alone[0])}, branch 1 alone {len(alone[1])}, the combined rule "
          f"{len(r['sel']['positions'])} of {len(pos)}; refined - first sample {(r['tim']['positions'] - pos).tolist()}, bit errors {errs}")
    assert len(alone[0]) == 4 and len(alone[1]) == 4
    assert set((alone[0] - 16) // (pos[1] - pos[0])) == {0, 2, 4, 6} and set((alone[1] - 16) // (pos[1] - pos[0])) == {1, 3, 5, 7}
    assert len(r["sel"]["positions"]) == 8 and np.array_equal(r["tim"]["positions"], pos + 16)
    assert errs == [0] * 8


def test_cross_faded_long_packets_need_tracking(pkg, oracle):
    words, xs, pos = dv.cross_faded(oracle, d=15, packets=6, snr_db=14.0)
    truth = tk.blank_truth(15)
    r = dv.fp64_receive(oracle, xs, dv.c_template(oracle))
    assert len(r["sel"]["positions"]) == 6 and np.array_equal(r["tim"]["positions"], pos + 16)
    plain = sum(dv.fp64_packet(oracle, xs, int(p), truth)["m"]["bit_err"] for p in r["tim"]["positions"])
    tracked = sum(dv.fp64_packet(oracle, xs, int(p), truth, "pilots")["m"]["bit_err"] for p in r["tim"]["positions"])
    print(f"cross-faded D = 15 at 14 dB: 6 of 6 found at + 16; bit errors {plain} untracked, {tracked} with the pilot step on the "
          f"combined numerators")
    assert tracked < plain


# ---------------------------------------------------------------- 6. the GPU parity streams' seeds
def test_parity_streams_meet_their_conditions(pkg, oracle):
    assert {k[0] for k in dv.PARITY_SEEDS} == {1, 2, 4, 15} and {k[1] for k in dv.PARITY_SEEDS} == {2, 3, 4}
    assert {k[3] for k in dv.PARITY_SEEDS} == {0.0, 40e3, -90e3}
    tpl = dv.c_template(oracle)
    band = total = 0
    for key in dv.PARITY_SEEDS:
        d, nb, snr, cfo = key
        words, xs, pos = dv.parity_stream(oracle, key)
        assert xs.shape[0] == nb and xs.shape[1] > 3 * 7936 and xs.dtype == np.complex64
        r = dv.fp64_receive(oracle, xs, tpl)
        m = r["metric"]
        share = len(ref.band_positions(m, 0.75, 0.75e-3)) / len(m)
        apart = dv.two_largest_apart(r["tim"]["metric"])
        truth = tk.blank_truth(d)
        n = sum(int(tk.axis_band(dv.fp64_packet(oracle, xs, int(p), truth, "pilots")["c"]["z"]).sum()) for p in r["tim"]["positions"])
        found = len(r["sel"]["positions"])
        print(f"D={d:2d} B={nb} {snr:2d} dB {cfo:8.0f} Hz seed {dv.PARITY_SEEDS[key]}: {found} of {len(pos)} packets, {100 * share:.3f} % of "
              f"the positions in the band, two largest L {apart:.3g} apart, {n} of {48 * d * found} subcarriers in the axis band")
        assert found >= 5
        assert ref.band_is_harmless(m, 0.75, 0.75e-3) and share <= 0.01
        assert apart > 1e-4
        band, total = band + n, total + 48 * d * found
    print(f"{band} of {total} subcarriers in the axis band ({100 * band / total:.3f} %)")
    assert band <= 0.002 * total
