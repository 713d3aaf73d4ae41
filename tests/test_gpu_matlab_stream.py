"""GPU tests of the stream receiver on MATLAB-convention recordings (OFDM_CONV_MATLAB: detect_ref.noisy_stream with
conv="matlab", Engine.transmit_packets(conv="matlab"), Engine.transmitter("matlab", "tester")) and of the timing value
made for them, OFDM_TIMING_LTF_MATLAB / timing="ltf-matlab" (include/ofdm_mi355x_timing.h).

Streams: detect_ref.MATLAB_SEEDS, six streams of 25,420 to 28,220 samples (89 packets sent, of which the conjugate
detector finds 84: detect_ref.MATLAB_FOUND).  tests/test_detect_host.py and tests/test_timing_host.py check on the CPU the conditions
that let these tests demand exact positions: no front or confirmation decision of either detector inside
|M - 0.75| <= 0.75e-3, and under the conjugate detector every record's two largest L more than 1e-4 apart -- the
smallest relative gap of the six streams is 0.069, so the kernel's L may deviate by 0.034 before a position could
differ.  The tests keep the requirement of tests/test_gpu_timing.py, 6e-5, and its measured bound.

Every tolerance is imported from the module that states it: METRIC_TOL and BAND (test_gpu_stream), CONJ_DEV_MEASURED,
METRIC_FLOOR (test_gpu_detect), TIMING_DEV_MEASURED (test_gpu_timing), CFO_TOL_HZ (test_gpu_captures).
Each test prints its figures before it asserts.

Measured on an MI355X (2026-10-20).  Metric deviations on the six streams: 3.08e-4 for the reference's metric (D = 2,
25 dB, unfaded, at M = 4.9; 2.5e-5 to 1.2e-4 on the others; METRIC_TOL 4.74e-4), 2.10e-6 for the conjugate one (D = 15,
25 dB, 200 kHz; 1.1e-6 to 1.4e-6 on the others; 4 x CONJ_DEV_MEASURED 1.44e-5); no crossing differs off the band, at most
0.033 % of the positions lie in it; the selection is exact.  The reference detector finds 18, 5, 18, 4, 0 and 21 packets,
the conjugate one 18, 15, 18, 5, 7 and 21.  Decode without timing: 150 records equal the oracle's, CFO within 0.016 Hz.
timing="ltf-matlab": positions exactly the fp64 rule's on all 84 packets, unfaded at first sample + 16 with quality 0.90
to 0.997, faded at + 16 to + 18 with quality 0.47 to 0.93; largest |quality - quality_fp64| 2.88e-7 (D = 1, 14 dB),
under TIMING_DEV_MEASURED; CFO at the refined positions within 0.033 Hz.  Loopback: 67 of 67 packets at + 16 for both
detectors and D = 2 and 15, shift 0, quality 0.987 to 1.000.  Noise-free 200 kHz: + 16, quality 0.907 to 0.914, 0 bit
errors; with the C template positions -38 and + 20, quality 0.25 to 0.26, 51 (D = 2) and 394 (D = 15) bit errors.  Tester
payload: 4 of 4 packets at + 16 or + 17 without timing, + 16 with it (quality 0.997), no bit error; eq bit-identical to
receive_captures on 3 windows.  Wall time (pytest --durations): the module 2.9 s, of which 2.1 s set up the six streams'
runs (the context, the first launches and the fp64 references); the loopback 0.11 s for D = 2 and 0.01 s for D = 15;
every other test 0.01 s or less."""
import numpy as np
import pytest

import detect_ref as ref
import timing_ref as tr
from conftest import normwise
from test_gpu_captures import CFO_TOL_HZ, check_against_oracle, check_against_receiver
from test_gpu_detect import CONJ_DEV_MEASURED, METRIC_FLOOR, assert_selection_exact
from test_gpu_detect import run as det_run
from test_gpu_stream import BAND, METRIC_TOL
from test_gpu_timing import TIMING_DEV_MEASURED, blank_truth, quality_dev, rx, same_bits
from test_stream_host import base_stream

pytestmark = pytest.mark.gpu

DETECTORS = ("reference", "conjugate")
HARD_QUALITY_BOUND = 0.034      # half the smallest relative gap between the two largest L on the six streams (0.069)
MSG2 = " " * 24


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tmpl_m(pkg, oracle):
    return tr.template(oracle, "matlab")


@pytest.fixture(scope="module")
def runs(eng, oracle, tmpl_m):
    """The six MATLAB-convention streams through both detectors with every detection output, through the conjugate
    detector with timing "ltf-matlab", their fp64 metrics and the fp64 timing rule on the coarse positions (shared,
    left unchanged by the tests)."""
    from ofdm_amd.stream import detection_metric, refine_timing
    out = []
    for key, seed in ref.MATLAB_SEEDS.items():
        d, snr, cfo, faded = key
        assert eng.set_long_message(" " * (12 * d)) == d
        x, pos = ref.matlab_stream(oracle, key)
        det = {name: det_run(eng, x, name, want_eq=True) for name in DETECTORS}
        ltf = rx(eng, x, "ltf-matlab")
        out.append(dict(key=key, d=d, snr=snr, cfo=cfo, faded=faded, x=x, pos=pos, words=ref.rand_words(d, len(pos), seed),
                        det=det, ltf=ltf, ref={name: detection_metric(x, name) for name in DETECTORS},
                        want=refine_timing(x, det["conjugate"]["positions"], tmpl_m)))
    _torch().cuda.synchronize()
    return out


def tag(r):
    return f"matlab D={r['d']:2d} {r['snr']} dB {r['cfo']:7.0f} Hz {'faded  ' if r['faded'] else 'unfaded'}"


# ---------------------------------------------------------------- 1. detection and selection
def test_detection_and_selection_against_double(runs):
    from ofdm_amd.stream import select_packets
    worst = dict.fromkeys(DETECTORS, 0.0)
    tol = {"reference": METRIC_TOL, "conjugate": 4 * CONJ_DEV_MEASURED}
    for r in runs:
        for det in DETECTORS:
            o, want_m = r["det"][det], r["ref"][det]
            g = o["metric"].astype(np.float64)
            ok = np.isfinite(want_m)
            assert len(g) == len(want_m) and ok.sum() > 0.99 * len(want_m) and np.isfinite(g[ok]).all()
            dev = np.abs(g[ok] - want_m[ok]) / np.maximum(want_m[ok], METRIC_FLOOR)
            with np.errstate(invalid="ignore"):
                want = want_m > 0.75
                band = np.abs(want_m - 0.75) <= BAND                 # False where the reference is NaN
            got = o["bitmap"]
            diff = int((got != want)[~band & ok].sum())
            sel = select_packets(want_m)
            off, _ = tr.offsets(o["positions"], r["pos"])
            print(f"{tag(r)} {det}: metric deviation {dev.max():.3g} (bound {tol[det]:.3g}, at M = {want_m[ok][dev.argmax()]:.3g}); "
                  f"{int(got.sum())} crossings, {diff} differ off the band, {int(band.sum())} positions ({100 * band.mean():.3f} %) "
                  f"in it, {int((got != want)[band].sum())} differ there; packets {o['found']} of {len(r['pos'])} sent, packet_pos - "
                  f"first sample {(int(off.min()), int(off.max())) if len(off) else None}")
            worst[det] = max(worst[det], float(dev.max()))
            assert diff == 0
            assert not got[~ok].any()
            assert band.mean() <= 0.01
            assert_selection_exact(o)
            assert np.array_equal(o["positions"], sel["positions"]) and np.array_equal(o["records"]["flags"] & 4, sel["flags"])
        assert (r["det"]["conjugate"]["found"], len(r["pos"])) == ref.MATLAB_FOUND[r["key"]]
    print(f"matlab streams: largest metric deviation reference {worst['reference']:.4g} (METRIC_TOL {METRIC_TOL:.4g}), conjugate "
          f"{worst['conjugate']:.4g} (4 x CONJ_DEV_MEASURED {4 * CONJ_DEV_MEASURED:.4g})")
    assert METRIC_TOL < 1e-3 and 4 * CONJ_DEV_MEASURED < 1e-3
    assert worst["reference"] <= tol["reference"]
    assert worst["conjugate"] <= tol["conjugate"]


# ---------------------------------------------------------------- 2. the decode against the oracle
def decode_against_the_oracle(oracle, x, out, truth, mode="c", keep=None):
    """Every record of `out` (or those of `keep`) against oracle.decode_at on [p - 40, p + 2 nfr + 60), by
    test_gpu_captures' rule with no position on the threshold allowed: the records checked and the largest deviation of
    the two CFO estimates in Hz"""
    x = np.asarray(x).astype(np.complex128)
    nfr = 320 + 80 * (len(truth) // 96)
    idx = np.arange(out["count"]) if keep is None else np.asarray(keep)
    caps, ora = [], []
    for p in out["positions"][idx]:
        lo = int(p) - 40
        assert lo >= 0 and lo + 2 * nfr + 100 <= len(x)
        caps.append(x[lo:lo + 2 * nfr + 100])
        ora.append(oracle.decode_at(caps[-1], truth, 40, mode, dumps=True, cap_len=len(caps[-1])))
    rec = out["records"][idx].copy()
    rec["packet_idx"] = 40
    rec["flags"] &= 3
    same = check_against_oracle(rec, np.asarray(out["bits"])[idx], np.asarray(out["eq"])[idx], ora, caps, truth, 0)
    assert len(same) == len(idx)
    cfo_dev = 0.0
    for k in same:
        cfo_dev = max(cfo_dev, abs(float(rec["cfo_coarse_hz"][k]) - float(ora[k]["cfo"][0])),
                      abs(float(rec["cfo_fine_hz"][k]) - float(ora[k]["cfo"][1])))
    return len(same), cfo_dev


def assert_payload_rows(r, out):
    """every packet found, and every record's payload words the transmitted row's"""
    off, k = tr.offsets(out["positions"], r["pos"])
    assert out["count"] == len(r["pos"]) and np.array_equal(k, np.arange(len(r["pos"])))
    assert np.array_equal(out["bits"], ref.bits_of(r["words"]))


def test_decode_against_the_oracle(runs, oracle):
    total, cfo_dev, exact = 0, 0.0, 0
    for r in runs:
        for det in DETECTORS:
            o = r["det"][det]
            n, dev = decode_against_the_oracle(oracle, r["x"], o, blank_truth(r["d"]))
            print(f"{tag(r)} {det}: {n} records against the oracle, CFO within {dev:.4g} Hz")
            total, cfo_dev = total + n, max(cfo_dev, dev)
            if not r["faded"] and r["snr"] == 25 and o["count"]:      # the reference's metric finds nothing at 200 kHz
                assert_payload_rows(r, o)
                exact += o["count"]
    print(f"matlab streams, no timing: {total} records, CFO within {cfo_dev:.4g} Hz (CFO_TOL_HZ {CFO_TOL_HZ}); {exact} records of "
          f"the unfaded 25 dB streams carry their transmitted rows")
    assert total >= 84 and exact == 18 + 18 + 7 and cfo_dev <= CFO_TOL_HZ


# ---------------------------------------------------------------- 3. transmit_packets(conv="matlab") loopback
@pytest.mark.parametrize("d", [2, 15])
def test_transmit_packets_matlab_loopback(eng, pkg, d):
    torch = _torch()
    n = 67
    words = ref.rand_words(d, n, 0x3A7 + d)
    stride = pkg.abi.packet_len(d) + ref.GAP
    pos = ref.GAP + stride * np.arange(n)
    rec = eng.transmit_packets(words, d, pos0=ref.GAP, stride=stride, n_out=n * stride + ref.GAP, conv="matlab")
    assert eng.set_long_message(" " * (12 * d)) == d
    for det in DETECTORS:
        none = eng.receive_stream(rec, detector=det, want_eq=True)
        ltf = eng.receive_stream(rec, detector=det, want_eq=True, timing="ltf-matlab")
        print(f"matlab loopback D {d} {det}: {none['count']} of {n} packets, packet_pos - first sample "
              f"{sorted(set((none['positions'] - pos[:none['count']]).tolist())) if none['count'] == n else '?'}; ltf-matlab shifts "
              f"{sorted(set(ltf['shift'].tolist()))}, quality {ltf['quality'].min():.4f}..{ltf['quality'].max():.4f}")
        assert none["count"] == none["found"] == n and np.array_equal(none["positions"], pos + 16)
        assert np.array_equal(none["bits"].cpu().numpy(), ref.bits_of(words))
        assert ltf["count"] == ltf["found"] == n and not ltf["shift"].any()
        assert np.array_equal(ltf["coarse_pos"], none["positions"]) and np.array_equal(ltf["positions"], none["positions"])
        assert ltf["records"].tobytes() == none["records"].tobytes()
        assert torch.equal(ltf["bits"], none["bits"])
        assert torch.equal(torch.view_as_real(ltf["eq"]).view(torch.int32), torch.view_as_real(none["eq"]).view(torch.int32))
        assert (ltf["quality"] > 0.9).all() and (ltf["quality"] <= 1).all()


# ---------------------------------------------------------------- 4. timing="ltf-matlab" on the noisy streams
def test_ltf_matlab_positions_are_the_fp64_rule(runs, oracle):
    """The largest |quality_gpu - quality_fp64| of the six streams on an MI355X, 2026-10-20: 2.88e-7 (D = 1, 14 dB, 0 Hz,
    unfaded; 1.3e-7 to 2.3e-7 on the others), under TIMING_DEV_MEASURED = 3.29e-7, so 4 x that figure is asserted as
    tests/test_gpu_timing.py asserts it and no figure of this module's own is needed."""
    worst, total, cfo_dev = 0.0, 0, 0.0
    for r in runs:
        none, ltf, want = r["det"]["conjugate"], r["ltf"], r["want"]
        dev = quality_dev(ltf, want)
        off, _ = tr.offsets(ltf["positions"], r["pos"])
        gap = tr.top_gap(want["metric"]).min()
        print(f"{tag(r)}: {ltf['count']} packets, refined packet_pos - first sample {int(off.min())}..{int(off.max())}, quality "
              f"{ltf['quality'].min():.3f}..{ltf['quality'].max():.3f}, deviation from fp64 {dev:.3g} (4 x TIMING_DEV_MEASURED "
              f"{4 * TIMING_DEV_MEASURED:.3g}, hard bound {HARD_QUALITY_BOUND}), smallest gap {gap:.3g}")
        worst = max(worst, dev)
        assert ltf["count"] == ltf["found"] == none["count"] > 0
        assert gap > 2 * HARD_QUALITY_BOUND
        assert np.array_equal(ltf["coarse_pos"], none["positions"]) and np.array_equal(ltf["coarse_pos"], want["coarse"])
        assert np.array_equal(ltf["positions"], want["positions"]) and np.array_equal(ltf["shift"], want["shift"])
        assert np.array_equal(ltf["positions"] - ltf["coarse_pos"], ltf["shift"]) and (np.diff(ltf["positions"]) > 0).all()
        assert np.array_equal(ltf["records"]["packet_idx"], ltf["positions"].astype(np.int32))
        assert np.array_equal(ltf["records"]["flags"], none["records"]["flags"]) and not ltf["records"]["reserved8"].any()
        assert (ltf["quality"] > 0).all() and (ltf["quality"] <= 1).all()
        assert ((off >= 16) & (off <= 18)).all() if r["faded"] else (off == 16).all()
        if not r["faded"]:
            assert (ltf["quality"] > 0.9).all()
        keep = np.nonzero(ltf["shift"] == 0)[0]
        assert ltf["records"][keep].tobytes() == none["records"][keep].tobytes()
        assert same_bits(ltf["eq"][keep], none["eq"][keep])
        # the decode at the refined positions
        n, cdev = decode_against_the_oracle(oracle, r["x"], ltf, blank_truth(r["d"]))
        total, cfo_dev = total + n, max(cfo_dev, cdev)
        if not r["faded"] and r["snr"] == 25:
            assert_payload_rows(r, ltf)
    bound = 4 * TIMING_DEV_MEASURED
    print(f"ltf-matlab: {total} packets, largest quality deviation {worst:.4g} (asserted {bound:.4g}; TIMING_DEV_MEASURED "
          f"{TIMING_DEV_MEASURED}), decode at the refined positions: CFO within {cfo_dev:.4g} Hz")
    assert total == sum(v[0] for v in ref.MATLAB_FOUND.values())
    assert worst <= HARD_QUALITY_BOUND
    assert bound < 6e-5 and worst <= 6e-5
    assert worst <= bound
    assert cfo_dev <= CFO_TOL_HZ


# ---------------------------------------------------------------- 5. the defect the value exists for
@pytest.mark.parametrize("d", [2, 15])
def test_noise_free_200_khz_matlab_stream_decodes_at_plus_16(eng, oracle, tmpl_m, d):
    """With timing="ltf-matlab" every packet of the noise-free 200 kHz MATLAB-convention stream stays at its first
    sample + 16 and decodes without a bit error; with the C template ("ltf") the same recording does not stay there."""
    from ofdm_amd.stream import refine_timing
    assert eng.set_long_message(" " * (12 * d)) == d
    words, x, pos = tr.clean_stream(oracle, d, 200e3, conv="matlab")
    x = x.astype(np.complex64)
    none, good, wrong = rx(eng, x, "none"), rx(eng, x, "ltf-matlab"), rx(eng, x, "ltf")
    want = refine_timing(x, none["positions"], tmpl_m)
    truth = ref.bits_of(words)
    err = lambda o: int((o["bits"] != truth).sum())
    print(f"matlab D {d} 200 kHz noise-free: coarse {(none['positions'] - pos).tolist()}; ltf-matlab {(good['positions'] - pos).tolist()} "
          f"quality {good['quality'].round(4).tolist()} (deviation from fp64 {quality_dev(good, want):.3g}), bit errors {err(good)}; "
          f"ltf (the C template) {(wrong['positions'] - pos).tolist()} quality {wrong['quality'].round(3).tolist()}, bit errors {err(wrong)}")
    assert none["count"] == good["count"] == wrong["count"] == tr.CLEAN_PACKETS
    assert np.array_equal(none["positions"], pos + 16) and err(none) == 0
    assert np.array_equal(good["positions"], pos + 16) and not good["shift"].any() and err(good) == 0
    assert np.array_equal(good["positions"], want["positions"])
    assert (good["quality"] > 0.89).all() and quality_dev(good, want) <= 4 * TIMING_DEV_MEASURED
    assert good["records"].tobytes() == none["records"].tobytes() and same_bits(good["eq"], none["eq"])
    assert not np.array_equal(wrong["positions"], pos + 16) and (wrong["quality"] < good["quality"]).all()


# ---------------------------------------------------------------- 6. payload="tester"
TESTER_SEED = 0x7E57


def _tester_records_against_the_receivers(eng, x, out, cap_len=3000):
    """the records whose window [p - 411, p - 411 + cap_len) fits against receive_captures and the single-capture
    receiver on it: the comparison of test_gpu_stream.test_decode_against_the_oracle_and_receive_captures"""
    fit = [k for k, p in enumerate(out["positions"]) if p - 411 >= 0 and p - 411 + cap_len <= len(x)]
    assert len(fit) >= 3
    starts = np.array([int(out["positions"][k]) - 411 for k in fit])
    windows = np.stack([x[s:s + cap_len] for s in starts])
    cap = eng.receive_captures(windows, mode="matlab", payload="tester", want_bits=True, want_eq=True)
    assert cap["cap_len"] == cap_len
    rec = out["records"][fit].copy()
    rec["packet_idx"] = 411
    rec["flags"] &= 3
    crec = cap["records"]
    assert np.array_equal(crec["packet_idx"].astype(np.int64) + starts, out["positions"][fit])
    assert np.array_equal(cap["bits"], out["bits"][fit])
    assert np.array_equal(crec["flags"], rec["flags"]) and np.array_equal(crec["bit_err"], rec["bit_err"])
    dev_eq = normwise(out["eq"][fit], cap["eq"])
    print(f"tester payload: {len(fit)} windows, eq against receive_captures within {dev_eq:.3g}")
    assert dev_eq < 1e-6
    for k, wdw in enumerate(windows):
        o = check_against_receiver(eng, wdw, rec[k], out["eq"][fit][k], "matlab", "tester")
        assert np.array_equal(o["bits"], out["bits"][fit][k])


def test_tester_payload_through_the_stream_receiver(eng, oracle):
    """Four periods of Transmitter("matlab", "tester") behind 500-sample gaps under real noise at 25 dB.  Under the
    reference detector -- receive_captures' own rule -- the records against receive_captures(mode="matlab",
    payload="tester") and the single-capture receiver on windows cut at position - 411, as tests/test_gpu_stream.py holds
    the message payload; under the conjugate detector, whose positions receive_captures does not reproduce, against the
    oracle's decode at each position.  With timing="ltf-matlab" a record that did not move is the untimed one byte for
    byte, and every record is held to the oracle's decode at its refined position."""
    from ofdm_amd.stream import synthetic_segments
    w = eng.transmitter("matlab", "tester")
    period = len(w) // 10
    assert period == 980 and eng.payload_frames("tester") == 2
    x = base_stream(w, 25.0, 0.0, TESTER_SEED, segments=synthetic_segments(period, 4, 500))
    pos = 500 + (period + 500) * np.arange(4)
    assert len(x) == 4 * (period + 500) + 500
    truth = oracle.tester_bits()
    for det in DETECTORS:
        kw = dict(mode="matlab", payload="tester", detector=det, want_eq=True)
        none = eng.receive_stream(x, **kw)
        ltf = eng.receive_stream(x, timing="ltf-matlab", **kw)
        print(f"tester payload {det}: {none['count']} packets, packet_pos - first sample {(none['positions'] - pos[:none['count']]).tolist()}, "
              f"bit_err {none['records']['bit_err'].tolist()}; ltf-matlab shifts {ltf['shift'].tolist()}, quality "
              f"{ltf['quality'].round(4).tolist()}")
        assert none["count"] == none["found"] == ltf["count"] == 4
        assert all(np.array_equal(b, truth) for b in none["bits"]) and not none["records"]["bit_err"].any()
        n_ora, cdev = decode_against_the_oracle(oracle, x, none, truth, "matlab")
        print(f"tester payload {det}: {n_ora} records against the oracle, CFO within {cdev:.4g} Hz")
        assert n_ora == 4 and cdev <= CFO_TOL_HZ
        if det == "reference":
            _tester_records_against_the_receivers(eng, x, none)
        # ---- with timing
        off = ltf["positions"] - pos
        assert np.array_equal(ltf["coarse_pos"], none["positions"]) and (off == 16).all() and (ltf["quality"] > 0.9).all()
        keep = np.nonzero(ltf["shift"] == 0)[0]
        assert ltf["records"][keep].tobytes() == none["records"][keep].tobytes() and same_bits(ltf["eq"][keep], none["eq"][keep])
        assert all(np.array_equal(b, truth) for b in ltf["bits"])
        n_ora, cdev = decode_against_the_oracle(oracle, x, ltf, truth, "matlab")
        print(f"tester payload {det}, ltf-matlab: {n_ora} records against the oracle, CFO within {cdev:.4g} Hz")
        assert n_ora == 4 and cdev <= CFO_TOL_HZ


# ---------------------------------------------------------------- 7. the two cached templates
def test_the_two_cached_templates_do_not_disturb_each_other(pkg, oracle):
    """OFDM_TIMING_LTF on a C-convention stream before and after the context's first OFDM_TIMING_LTF_MATLAB call: byte
    for byte the same; then the other order on a fresh context; and each value gives the same bytes in both contexts."""
    key = (2, 14, 40e3, False)
    streams = {"ltf": ref.noisy_stream(oracle, *key, ref.STREAM_SEEDS[key])[0], "ltf-matlab": ref.matlab_stream(oracle, key)[0]}
    image = lambda o: (o["records"].tobytes(), np.ascontiguousarray(o["bits"]).tobytes(), np.ascontiguousarray(o["eq"]).tobytes(),
                       o["coarse_pos"].tobytes(), o["shift"].tobytes(), o["quality"].tobytes())
    seen = {}
    for first, second in (("ltf", "ltf-matlab"), ("ltf-matlab", "ltf")):
        with pkg.Engine(0) as e:
            assert e.set_long_message(MSG2) == 2
            a = rx(e, streams[first], first)
            b = rx(e, streams[second], second)
            c = rx(e, streams[first], first)
            d = rx(e, streams[second], second)
            print(f"templates, {first} first: {a['count']} and {b['count']} packets, shifts {sorted(set(a['shift'].tolist()))} and "
                  f"{sorted(set(b['shift'].tolist()))}")
            assert a["count"] > 0 and b["count"] > 0 and (a if first == "ltf" else b)["shift"].any()
            assert image(a) == image(c) and image(b) == image(d)
            seen[first, first], seen[first, second] = image(a), image(b)
    assert seen["ltf", "ltf"] == seen["ltf-matlab", "ltf"] and seen["ltf", "ltf-matlab"] == seen["ltf-matlab", "ltf-matlab"]
