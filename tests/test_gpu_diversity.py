"""GPU tests of the stream receiver's receive diversity (include/ofdm_mi355x_diversity.h, ofdm_receive_stream_diversity,
Engine.receive_diversity, csrc/ofdm_stream_div.hip): one branch byte for byte against ofdm_receive_stream_tracked, the
cross-faded stream that only the combined receiver decodes, parity with the fp64 rules (stream.diversity_metric,
stream.refine_timing_branches, stream.combine_branches on the oracle's frames) over D = 1, 2, 4, 15 and B = 2, 3, 4,
identical branches, the branches' alignments, the recordings' scale, the stream's end, max_packets, looping waves, the
argument checks and the link sweep.

Streams (div_ref.PARITY_SEEDS): about 3e4 samples per branch, more than three detection tiles, flat Rayleigh gains per
packet and branch, complex noise of one power on every branch; tests/test_diversity_host.py checks their seeds'
conditions on the CPU.  Tolerances: eq normwise 1e-4, evm_db_pre 2e-3 dB and post_axis_err 2 are tests/test_gpu_track.py's
(EQ_TOL, EVM_TOL_DB, AXIS_TOL); bits are compared except where the fp64 |Re z| or |Im z| is below track_ref.AXIS_BAND of
the packet's largest |z|; crossings except where |M - 0.75| <= 0.75e-3.  The common carrier offset fc + ff is compared
within 1 Hz: an fp32 angle is good to about 1e-6 rad, 0.05 Hz across the fine estimate's lag of 64 samples.

The deviations of the fp32 kernels from the fp64 rules that the issue leaves open, the largest over the parity streams
on an MI355X (each asserted at 4 x, the margin tests/test_gpu_track.py and tests/test_gpu_timing.py give):
  PHASE_DEV_MEASURED    |phase - phase_fp64| on symbols whose |P_d| is at least a quarter of its noise-free value:
                        4.79e-7 rad (D = 15, B = 2, 16 dB, 40 kHz; 1.3e-7 to 4.4e-7 on the other streams, 325 symbols)
  QUALITY_DEV_MEASURED  |quality - quality_fp64|: 2.42e-7 (D = 2, B = 4, 14 dB, -90 kHz; 9.6e-8 to 2.1e-7 elsewhere)
  METRIC_DEV_MEASURED   |M - M_fp64| / max(M_fp64, 0.075), as tests/test_gpu_detect.py takes it: 1.30e-6 (D = 15, B = 2,
                        16 dB, 40 kHz, at M = 0.088; 7.9e-7 to 1.2e-6 elsewhere)
  GAIN_DEV_MEASURED     |gain - gain_fp64| / gain_fp64: 2.34e-7 (D = 1, B = 2, 14 dB; 1.5e-7 to 2.3e-7 elsewhere)
There eq stays within 6.1e-7 of the packet's largest |z|, evm_db_pre within 1.4e-5 dB, post_axis_err exact, fc + ff
within 0.004 Hz, and no subcarrier of the 31,200 compared lies in the excluded band.
Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import detect_ref as ref
import div_ref as dv
import track_ref as tk

pytestmark = pytest.mark.gpu

EQ_TOL, EVM_TOL_DB, AXIS_TOL = 1e-4, 2e-3, 2          # tests/test_gpu_track.py's
CFO_TOL_HZ = 1.0
METRIC_FLOOR, BAND = 0.075, 0.75e-3
# measured on an MI355X over div_ref.PARITY_SEEDS, see the module docstring
PHASE_DEV_MEASURED = 4.80e-7      # rad
QUALITY_DEV_MEASURED = 2.43e-7
METRIC_DEV_MEASURED = 1.30e-6
GAIN_DEV_MEASURED = 2.34e-7


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


def rx(eng, xs, tracking="pilots", timing="ltf", **kw):
    kw = dict(dict(want_bits=True, want_eq=True, detector="conjugate"), **kw)
    if isinstance(xs, np.ndarray):
        xs = np.ascontiguousarray(xs, np.complex64)
    return eng.receive_diversity(xs, timing=timing, tracking=tracking, **kw)


def rx1(eng, x, tracking="pilots", timing="ltf", **kw):
    kw = dict(dict(want_bits=True, want_eq=True, detector="conjugate"), **kw)
    return eng.receive_stream(x if _torch().is_tensor(x) else np.ascontiguousarray(x, np.complex64), timing=timing,
                              tracking=tracking, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def host(t):
    return t.cpu().numpy() if _torch().is_tensor(t) else np.asarray(t)


IDS = ("K_STREAM_DETECT", "K_STREAM_DETECT_CONJ", "K_STREAM_SELECT", "K_STREAM_TIMING", "K_STREAM_DECODE", "K_STREAM_DECODE_TRACK",
       "K_STREAM_DETECT_DIV", "K_STREAM_TIMING_DIV", "K_STREAM_DECODE_DIV")


def launches(eng, abi):
    return {k: eng.timing_query(getattr(abi, k))[1] for k in IDS}


def raw_call(eng, pkg, branches, nd, sopts, timing, tracking, max_packets=64, want_timing=False, want_phase=False,
             want_gain=False, tracked=False):
    """ofdm_receive_stream_diversity (or, tracked=True, ofdm_receive_stream_tracked on the one branch) through ctypes on
    outputs prefilled with a sentinel: the return code, every output as host bytes, and d_count"""
    torch = _torch()
    abi, lib = pkg.abi, eng.lib
    n, nb = len(branches[0]), len(branches)
    lc = n - 47 if sopts is None or sopts.detector == 0 else n - 63
    pk = torch.full((max_packets, 64), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    words = torch.full((max_packets, 3 * nd), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    eq = torch.full((max_packets, 96 * nd), 7.5, dtype=torch.float32, device="cuda")
    row = torch.zeros(abi.NCOUNTERS, dtype=torch.int64, device="cuda")
    metric = torch.full((lc,), -3.0, dtype=torch.float32, device="cuda")
    cross = torch.full(((lc + 31) // 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tim = torch.full((max_packets, 16), 0x5A, dtype=torch.uint8, device="cuda")
    phase = torch.full((max_packets, nd), 7.5, dtype=torch.float32, device="cuda")
    gain = torch.full((max_packets, nb), 7.5, dtype=torch.float32, device="cuda")
    opts = abi.make_rx_opts("c")
    p = lambda t: C.c_void_p(t.data_ptr())
    so = None if sopts is None else C.byref(sopts)
    tail = (abi.PAYLOAD["message"], max_packets, p(pk), p(cnt), p(words), p(eq), p(row), p(metric), p(cross),
            p(tim) if want_timing else None, p(phase) if want_phase else None)
    if tracked:
        rc = lib.ofdm_receive_stream_tracked(eng.ctx, p(branches[0]), n, C.byref(opts), so, timing, tracking, *tail)
    else:
        table = (C.c_void_p * nb)(*[b.data_ptr() for b in branches])
        rc = lib.ofdm_receive_stream_diversity(eng.ctx, table, nb, n, C.byref(opts), so, timing, tracking, *tail,
                                               p(gain) if want_gain else None)
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy().tobytes() for k, t in dict(pk=pk, cnt=cnt, words=words, eq=eq, row=row, metric=metric, cross=cross,
                                                         tim=tim, phase=phase, gain=gain).items()}
    return rc, out, [int(v) for v in cnt.cpu()]


FILL = dict(pk=(np.uint8, 0x5A), cnt=(np.int64, -7), words=(np.int32, 0x5A5A5A5A), eq=(np.float32, 7.5), row=(np.int64, 0),
            metric=(np.float32, -3.0), cross=(np.int32, 0x5A5A5A5A), tim=(np.uint8, 0x5A), phase=(np.float32, 7.5),
            gain=(np.float32, 7.5))


def untouched(out, k) -> bool:
    """output k of raw_call still holds nothing but its sentinel"""
    dt, v = FILL[k]
    return bool((np.frombuffer(out[k], dt) == v).all())


# ---------------------------------------------------------------- 1. one branch is ofdm_receive_stream_tracked
def test_one_branch_is_ofdm_receive_stream_tracked(eng, pkg, oracle):
    torch = _torch()
    abi = pkg.abi
    assert eng.set_long_message(" " * 24) == 2
    x, pos = ref.noisy_stream(oracle, 2, 20.0, 40e3, False, 502)
    x_dev = torch.from_numpy(x).cuda()
    eng.timing(True)
    try:
        for det in ("reference", "conjugate"):
            sopts = abi.StreamOpts(abi.DETECTOR[det], 0.75)
            for timing in ("none", "ltf"):
                for tracking in ("none", "pilots"):
                    kw = dict(want_timing=timing != "none", want_phase=tracking != "none")
                    eng.timing_reset()
                    rc, base, cnt = raw_call(eng, pkg, [x_dev], 2, sopts, abi.TIMING[timing], abi.TRACKING[tracking], tracked=True, **kw)
                    want = launches(eng, abi)
                    eng.timing_reset()
                    rc1, one, cnt1 = raw_call(eng, pkg, [x_dev], 2, sopts, abi.TIMING[timing], abi.TRACKING[tracking], **kw)
                    got = launches(eng, abi)
                    print(f"detector {det}, timing {timing}, tracking {tracking}: {cnt1[0]} packets of {len(pos)} sent; launches {got}")
                    assert rc == rc1 == 0 and cnt == cnt1 and cnt[0] == cnt[1] == len(pos)
                    assert got == want and not any(got[k] for k in IDS if k.endswith("_DIV"))
                    for k in base:
                        assert one[k] == base[k], k                  # d_gain among them: never written
    finally:
        eng.timing(False)
    # the Engine takes the same route
    a, b = eng.receive_stream(x_dev, want_eq=True), eng.receive_diversity([x_dev], want_eq=True)
    assert a["records"].tobytes() == b["records"].tobytes() and b["gain"] is None and b["branches"] == 1
    assert same_bits(host(a["eq"]), host(b["eq"])) and same_bits(host(a["bits"]), host(b["bits"]))
    c = eng.receive_diversity(x_dev.reshape(1, -1), detector="conjugate", timing="ltf", tracking="pilots", keep_device=True)
    d = rx1(eng, x_dev, want_eq=False)
    assert c["records"].tobytes() == d["records"].tobytes() and same_bits(c["phase"], d["phase"]) and c["d_gain"] is None


# ---------------------------------------------------------------- 2. the cross-faded stream: fails without the feature
def test_cross_faded_stream_needs_both_branches(eng, oracle):
    assert eng.set_long_message(" " * 24) == 2
    words, xs, pos = dv.cross_faded(oracle)
    alone = [rx1(eng, x) for x in xs]
    both = rx(eng, xs)
    share = both["gain"] / both["gain"].sum(axis=1, keepdims=True)
    print(f"cross-faded stream: branch 0 alone finds {alone[0]['count']}, branch 1 alone {alone[1]['count']}, both {both['count']} of "
          f"{len(pos)}; positions - first sample {(both['positions'] - pos).tolist()}, bit errors {both['records']['bit_err'].tolist()}, "
          f"strong branch's share of the gain {share.max(axis=1).round(4).tolist()}")
    assert alone[0]["count"] == 4 and alone[1]["count"] == 4
    assert both["count"] == both["found"] == 8 and np.array_equal(both["positions"], pos + 16)
    assert not both["records"]["bit_err"].any() and np.array_equal(both["bits"], np.tile(tk.blank_truth(2), (8, 1)))
    assert both["gain"].shape == (8, 2) and both["gain"].dtype == np.float32
    assert np.array_equal(share.argmax(axis=1), np.arange(8) % 2) and (share.max(axis=1) > 0.99).all()


def test_cross_faded_long_packets_need_tracking(eng, oracle):
    d = 15
    assert eng.set_long_message(" " * (12 * d)) == d
    words, xs, pos = dv.cross_faded(oracle, d=d, packets=6, snr_db=14.0)
    plain, trk = rx(eng, xs, "none"), rx(eng, xs, "pilots")
    e0, e1 = int(plain["records"]["bit_err"].sum()), int(trk["records"]["bit_err"].sum())
    print(f"cross-faded D = 15 at 14 dB: {trk['count']} of {len(pos)} found, positions - first sample "
          f"{(trk['positions'] - pos).tolist()}; bit errors {e0} untracked, {e1} tracked")
    assert plain["count"] == trk["count"] == len(pos) and np.array_equal(trk["positions"], pos + 16)
    assert e1 < e0


# ---------------------------------------------------------------- 3. parity with the fp64 rules
@pytest.fixture(scope="module")
def parity_runs(eng, oracle):
    """The parity streams untracked and tracked, and the fp64 detection and timing rules on them (shared, left
    unchanged by the tests)"""
    tpl = dv.c_template(oracle)
    out = []
    for key in dv.PARITY_SEEDS:
        d, nb, snr, cfo = key
        assert eng.set_long_message(" " * (12 * d)) == d
        words, xs, pos = dv.parity_stream(oracle, key)
        out.append(dict(key=key, d=d, nb=nb, xs=xs, pos=pos, want=dv.fp64_receive(oracle, xs, tpl),
                        none=rx(eng, xs, "none", want_metric=True, want_cross=True),
                        trk=rx(eng, xs, "pilots", want_metric=True, want_cross=True)))
    _torch().cuda.synchronize()
    return out


def tag(r):
    d, nb, snr, cfo = r["key"]
    return f"D={d:2d} B={nb} {snr:2d} dB {cfo:8.0f} Hz"


def test_detection_and_timing_against_the_fp64_rules(parity_runs):
    from ofdm_amd.stream import unpack_cross
    worst_m = worst_q = 0.0
    for r in parity_runs:
        o, want = r["trk"], r["want"]
        m64, sel, tim = want["metric"], want["sel"], want["tim"]
        g = o["metric"].astype(np.float64)
        assert len(g) == len(m64) == r["xs"].shape[1] - 63 and np.isfinite(m64).all() and np.isfinite(g).all()
        dev = np.abs(g - m64) / np.maximum(m64, METRIC_FLOOR)
        band = np.abs(m64 - 0.75) <= BAND
        got = unpack_cross(o["cross"], len(m64))
        diff = int((got != (m64 > 0.75))[~band].sum())
        qdev = float(np.abs(o["quality"].astype(np.float64) - tim["quality"]).max())
        print(f"{tag(r)}: metric deviation {dev.max():.3g} (at M = {m64[dev.argmax()]:.3g}), {int(got.sum())} crossings, {diff} differ "
              f"off the band, {int(band.sum())} positions in it; {o['found']} packets of {len(r['pos'])}, shifts "
              f"{sorted(set(o['shift'].tolist()))}, quality deviation {qdev:.3g}")
        worst_m, worst_q = max(worst_m, float(dev.max())), max(worst_q, qdev)
        assert diff == 0 and band.sum() <= 0.01 * len(m64)
        assert o["found"] == o["count"] == len(sel["positions"]) > 0
        assert np.array_equal(o["coarse_pos"], sel["positions"]) and np.array_equal(o["positions"], tim["positions"])
        assert np.array_equal(o["shift"], tim["shift"])
        assert np.array_equal(o["records"]["flags"] & 4, sel["flags"])
        # the option leaves detection and timing alone
        n = r["none"]
        assert same_bits(n["metric"], o["metric"]) and same_bits(n["cross"], o["cross"]) and same_bits(n["quality"], o["quality"])
        assert np.array_equal(n["positions"], o["positions"])
    print(f"largest metric deviation {worst_m:.4g} (METRIC_DEV_MEASURED {METRIC_DEV_MEASURED}), largest quality deviation "
          f"{worst_q:.4g} (QUALITY_DEV_MEASURED {QUALITY_DEV_MEASURED})")
    assert 4 * METRIC_DEV_MEASURED < 1e-3 and worst_m <= 4 * METRIC_DEV_MEASURED
    assert worst_q <= 4 * QUALITY_DEV_MEASURED


def check_decode(oracle, r, out, tracking, worst, packets=None):
    """every record of a run against the fp64 decode rule at the record's position; returns (compared, excluded)"""
    from ofdm_amd.stream import PILOT_BINS
    d, nb = r["d"], r["nb"]
    truth = tk.blank_truth(d)
    rec, bits, eq, gain = out["records"], host(out["bits"]), host(out["eq"]), out["gain"]
    xs = out.get("xs64")
    if xs is None:
        xs = out["xs64"] = [x.astype(np.complex128) for x in r["xs"][:, :out.get("n", r["xs"].shape[1])]]
    compared = excluded = 0
    for k in (range(out["count"]) if packets is None else packets):
        q = dv.fp64_packet(oracle, xs, int(rec["packet_pos"][k]), truth, tracking)
        c, want = q["c"], q["m"]
        z = c["z"].reshape(-1)
        with np.errstate(invalid="ignore"):
            e = float(np.nanmax(np.abs(eq[k] - z)) / max(np.nanmax(np.abs(z)), 1e-30)) if np.isfinite(z).any() else 0.0
        dvm = abs(float(rec["evm_db_pre"][k]) - want["evm_db_pre"]) if np.isfinite(want["evm_db_pre"]) else 0.0
        ax = abs(int(rec["post_axis_err"][k]) - want["axis"])
        band = tk.axis_band(z)
        gd = float((np.abs(gain[k].astype(np.float64) - c["gain"]) / np.maximum(c["gain"], 1e-300)).max()) if c["gain"].all() else 0.0
        cfo = abs(float(rec["cfo_coarse_hz"][k]) + float(rec["cfo_fine_hz"][k]) - sum(c["cfo"]))
        ph = 0.0
        if tracking == "pilots":
            ok = (np.abs(c["P"]) >= 0.25 * float(c["G"][list(PILOT_BINS)].sum())) & ~c["fallback"]
            if ok.any():
                ph = float(np.abs(tk.wrap(out["phase"][k].astype(np.float64) - c["phase"]))[ok].max())
            worst["phase_symbols"] += int(ok.sum())
        for name, v in (("eq", e), ("evm", dvm), ("axis", ax), ("gain", gd), ("cfo", cfo), ("phase", ph)):
            worst[name] = max(worst[name], v)
        assert e < EQ_TOL, (k, e)
        assert dvm <= EVM_TOL_DB, (k, dvm)
        assert ax <= AXIS_TOL, (k, ax)
        assert cfo <= CFO_TOL_HZ, (k, cfo)
        assert np.array_equal(bits[k][~np.repeat(band, 2)], want["bits"][~np.repeat(band, 2)]), k
        assert int(rec["bit_err"][k]) == int((bits[k] != truth).sum()), k
        assert float(rec["ber"][k]) == pytest.approx(int(rec["bit_err"][k]) / (96.0 * d), abs=1e-6)
        assert int(rec["flags"][k]) & 2 == 2 * int(q["oob"]), k
        compared, excluded = compared + 48 * d, excluded + int(band.sum())
    return compared, excluded


def new_worst():
    return dict(eq=0.0, evm=0.0, axis=0, gain=0.0, cfo=0.0, phase=0.0, phase_symbols=0)


def test_decode_against_the_fp64_rule(parity_runs, oracle):
    worst, compared, excluded, packets = new_worst(), 0, 0, 0
    for r in parity_runs:
        for tracking, key in (("none", "none"), ("pilots", "trk")):
            o, w = r[key], new_worst()
            c, e = check_decode(oracle, r, o, tracking, w)
            print(f"{tag(r)} tracking {tracking:6s}: {o['count']} packets, bit errors {int(o['records']['bit_err'].sum())}, eq {w['eq']:.3g}, "
                  f"evm_db_pre {w['evm']:.3g} dB, post_axis {w['axis']}, gain {w['gain']:.3g}, cfo {w['cfo']:.3g} Hz, phase {w['phase']:.3g} "
                  f"rad on {w['phase_symbols']} symbols, {e} of {c} subcarriers excluded")
            for k in ("eq", "evm", "axis", "gain", "cfo", "phase"):
                worst[k] = max(worst[k], w[k])
            worst["phase_symbols"] += w["phase_symbols"]
            compared, excluded, packets = compared + c, excluded + e, packets + o["count"]
        # what the option leaves alone is byte-equal to the untracked run on the same recordings
        n, t = r["none"], r["trk"]
        for name in ("packet_pos", "reserved8", "packet_idx", "flags", "cfo_coarse_hz", "cfo_fine_hz", "reserved"):
            assert same_bits(t["records"][name], n["records"][name]), name
        assert same_bits(t["gain"], n["gain"]) and n["phase"] is None and t["phase"].shape == (t["count"], r["d"])
    print(f"decode parity: {packets} records, eq {worst['eq']:.4g}, evm_db_pre {worst['evm']:.4g} dB, post_axis {worst['axis']}, cfo "
          f"{worst['cfo']:.4g} Hz, largest gain deviation {worst['gain']:.4g} (GAIN_DEV_MEASURED {GAIN_DEV_MEASURED}), largest phase "
          f"deviation {worst['phase']:.4g} rad on {worst['phase_symbols']} symbols (PHASE_DEV_MEASURED {PHASE_DEV_MEASURED}), {excluded} of "
          f"{compared} subcarriers excluded")
    assert packets >= 100 and worst["phase_symbols"] > 0
    assert excluded <= 0.002 * compared
    assert worst["phase"] <= 4 * PHASE_DEV_MEASURED
    assert worst["gain"] <= 4 * GAIN_DEV_MEASURED


# ---------------------------------------------------------------- 4. identical branches
@pytest.mark.parametrize("nb", [2, 4])
def test_identical_branches_are_one_branch(eng, parity_runs, nb):
    torch = _torch()
    r = next(q for q in parity_runs if q["key"] == (2, 3, 12, 40e3))
    assert eng.set_long_message(" " * 24) == 2
    x = torch.from_numpy(r["xs"][0]).cuda()
    one = rx1(eng, x)
    o = rx(eng, [x.clone() for _ in range(nb)])
    z1, z = host(one["eq"]), host(o["eq"])
    dev = max(float(np.abs(z[k] - z1[k]).max() / np.abs(z1[k]).max()) for k in range(one["count"]))
    band = np.stack([np.repeat(tk.axis_band(z1[k]), 2) for k in range(one["count"])])
    print(f"{nb} copies of one recording: {o['count']} packets (one copy {one['count']}), eq deviates by at most {dev:.3g} of the "
          f"packet's largest, {int(band.sum()) // 2} subcarriers in the axis band")
    assert o["count"] == one["count"] > 0 and np.array_equal(o["positions"], one["positions"]) and np.array_equal(o["shift"], one["shift"])
    assert dev < EQ_TOL
    assert np.array_equal(host(o["bits"])[~band], host(one["bits"])[~band])
    for b in range(1, nb):
        assert same_bits(o["gain"][:, b], o["gain"][:, 0])


# ---------------------------------------------------------------- 5. alignments
def test_branches_at_different_alignments(eng, parity_runs):
    torch = _torch()
    r = next(q for q in parity_runs if q["key"] == (1, 2, 14, 0.0))
    assert eng.set_long_message(" " * 12) == 1
    base = r["trk"]
    n = r["xs"].shape[1]
    for off in ((0, 1), (1, 0), (1, 1)):
        rows = []
        for b, k in enumerate(off):
            buf = torch.zeros(n + 2, dtype=torch.complex64, device="cuda")
            buf[k:k + n] = torch.from_numpy(r["xs"][b]).cuda()
            rows.append(buf[k:k + n])
            assert rows[-1].data_ptr() % 16 == 8 * k
        o = rx(eng, rows, want_metric=True, want_cross=True)
        print(f"branches {8 * off[0]} and {8 * off[1]} bytes off a 16-byte boundary: {o['count']} packets, every output compared byte for byte")
        assert o["count"] == base["count"] and o["records"].tobytes() == base["records"].tobytes()
        for k in ("bits", "eq", "metric", "cross", "quality", "phase", "gain"):
            assert same_bits(host(o[k]), host(base[k])), k


# ---------------------------------------------------------------- 6. scale, stream end, prefixes, looping waves
def test_scale_of_the_recordings(eng, parity_runs):
    torch = _torch()
    r = next(q for q in parity_runs if q["key"] == (15, 4, 12, 0.0))
    assert eng.set_long_message(" " * 180) == 15
    base = r["trk"]
    x = torch.from_numpy(r["xs"]).cuda()
    for s in (2.0 ** 12, 2.0 ** -12):
        o = rx(eng, x * s)
        same_eq = same_bits(host(o["eq"]), base["eq"])
        print(f"recordings x {s:g}: {o['count']} packets, bits, positions and phases compared byte for byte; eq byte-identical too: {same_eq}")
        assert o["count"] == base["count"] > 0 and np.array_equal(o["positions"], base["positions"])
        assert same_bits(host(o["bits"]), base["bits"]) and same_bits(o["phase"], base["phase"])
        assert same_bits(o["records"]["bit_err"], base["records"]["bit_err"]) and same_bits(o["quality"], base["quality"])
        assert np.allclose(o["gain"], base["gain"] * np.float32(s * s), rtol=1e-6)


def test_stream_end(eng, oracle, parity_runs):
    r = next(q for q in parity_runs if q["key"] == (15, 2, 16, 40e3))
    d = 15
    assert eng.set_long_message(" " * 180) == d
    truth = tk.blank_truth(d)
    full = r["trk"]
    k = full["count"] - 1
    p = int(full["positions"][k])
    # cut inside data symbol 9 of the last packet: frame sample 336 + 80 s is stream sample p + 2 (336 + 80 s) - 20
    n = p + 2 * (336 + 80 * 9) - 20 + 70
    zfirst = min(s for s in range(d + 1) if s == d or p + 2 * (336 + 80 * s) >= n + 20)
    assert zfirst == 10
    xs = np.ascontiguousarray(r["xs"][:, :n])
    for tracking in ("none", "pilots"):
        o = rx(eng, xs, tracking)
        assert o["count"] == k + 1 and o["positions"][k] == p and int(o["records"]["flags"][k]) & 2
        assert o["records"][:k].tobytes() == r["trk" if tracking == "pilots" else "none"]["records"][:k].tobytes()
        eq, bits = o["eq"][k].reshape(d, 48), o["bits"][k].reshape(d, 96)
        print(f"cut inside symbol 9, tracking {tracking}: bit errors {int(o['records']['bit_err'][k])}, flags {int(o['records']['flags'][k])}")
        assert not eq[zfirst:].real.any() and not eq[zfirst:].imag.any()
        assert np.array_equal(bits[zfirst:], np.tile([1, 0], (d - zfirst, 48)))
        if tracking == "pilots":
            assert not o["phase"][k][zfirst:].any()
        # their share of the counts is the payload's own
        share_be = int((np.tile([1, 0], 48 * (d - zfirst)) != truth[96 * zfirst:]).sum())
        assert int(o["records"]["bit_err"][k]) - int((o["bits"][k][:96 * zfirst] != truth[:96 * zfirst]).sum()) == share_be
        # the partly cut symbol, and the whole record, against the fp64 rule on the zero-padded windows
        worst = new_worst()
        check_decode(oracle, r, dict(o, n=n), tracking, worst, packets=[k])
        print(f"cut packet against the fp64 rule: {worst}")
    # a stream that ends before the long training symbols: S = 0 on every branch, z = 0 / 0
    n0 = p + 300                                                      # the front is still confirmed: n > front + 277 = p + 266
    o = rx(eng, np.ascontiguousarray(r["xs"][:, :n0]), "pilots", timing="none")
    rec = o["records"][o["count"] - 1]
    print(f"cut before the training symbols: evm_pre_sum {rec['evm_pre_sum']}, evm_db_pre {rec['evm_db_pre']}, bit_err {rec['bit_err']}, "
          f"gain {o['gain'][-1].tolist()}, phases {o['phase'][-1].tolist()}")
    assert o["count"] == k + 1 and np.isnan(rec["evm_pre_sum"]) and np.isnan(rec["evm_db_pre"])
    assert np.array_equal(o["bits"][-1], np.tile([1, 0], 48 * d)) and not o["phase"][-1].any() and not o["gain"][-1].any()
    assert int(rec["bit_err"]) == int((np.tile([1, 0], 48 * d) != truth).sum())


def test_max_packets_gives_prefixes(eng, parity_runs):
    r = next(q for q in parity_runs if q["key"] == (4, 4, 10, -90e3))
    assert eng.set_long_message(" " * 48) == 4
    base = r["trk"]
    assert base["found"] > 3
    for m in (1, 3):
        o = rx(eng, r["xs"], max_packets=m)
        assert o["found"] == base["found"] and o["count"] == m
        assert o["records"].tobytes() == base["records"][:m].tobytes()
        for k in ("bits", "eq", "phase", "gain", "quality"):
            assert same_bits(o[k], base[k][:m]), k
    o = rx(eng, r["xs"], max_packets=0, want_bits=False, want_eq=False)
    assert o["found"] == base["found"] and o["count"] == 0 and o["phase"].shape == (0, 4) and o["gain"].shape == (0, 4)


def test_looping_waves(eng, oracle):
    """One noisy three-packet segment on two branches tiled until the recordings hold more packets than 2 x CUs x 8
    waves: the timing and decode waves loop, and every repeat gives the first one's records"""
    torch = _torch()
    d, per = 4, 3
    assert eng.set_long_message(" " * (12 * d)) == d
    words = np.repeat(tk.blank_words(d), per, axis=0)
    gains = np.array([[1.0, 0.6j, -0.8], [0.5 - 0.5j, 1.0, 0.7j]])
    seg, pos = dv.branch_stream(oracle, words, gains, 16.0, 40e3, 6402)
    period = seg.shape[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    repeats = (2 * cus * 8) // per + 2
    x = torch.from_numpy(seg).cuda().repeat(1, repeats + 1)            # the closing repeat is not compared: it holds the last front
    # fine timing on: a coarse front may move by a sample with the detection runs' absolute boundaries
    o = rx(eng, x)
    c = per * repeats
    print(f"{o['count']} packets of {d} data symbols on 2 branches, {cus} CUs, period {period}: bit errors per repeat "
          f"{int(o['records']['bit_err'][:per].sum())}")
    assert o["found"] == o["count"] == per * (repeats + 1) > 2 * cus * 8
    rec, bits, eq = o["records"][:c], host(o["bits"])[:c], host(o["eq"])[:c]
    assert np.array_equal(rec["packet_pos"].reshape(repeats, per), rec["packet_pos"][:per] + period * np.arange(repeats)[:, None])
    for name in rec.dtype.names:
        if name not in ("packet_pos", "packet_idx"):
            assert same_bits(rec[name].reshape(repeats, -1), np.tile(rec[name][:per].reshape(1, -1), (repeats, 1))), name
    for a in (bits, eq, o["phase"][:c], o["gain"][:c], o["quality"][:c]):
        assert same_bits(a.reshape(repeats, -1), np.tile(a[:per].reshape(1, -1), (repeats, 1)))
    alone = rx(eng, seg)
    assert alone["count"] == per and same_bits(alone["eq"], eq[:per]) and same_bits(alone["gain"], o["gain"][:per])


# ---------------------------------------------------------------- 7. arguments on the device
def test_arguments(eng, pkg, oracle):
    torch = _torch()
    abi, lib = pkg.abi, eng.lib
    assert eng.set_long_message(" " * 24) == 2
    words, xs, pos = dv.cross_faded(oracle)
    x = [torch.from_numpy(v).cuda() for v in xs]
    odd = torch.zeros(len(xs[0]) * 2 + 1, dtype=torch.float32, device="cuda")[1:]      # 4 bytes off: not a sample boundary
    conj, refd = abi.StreamOpts(1, 0.75), abi.StreamOpts(0, 0.75)
    eng.timing(True)
    try:
        eng.timing_reset()
        cases = [dict(branches=x * 3, sopts=conj), dict(branches=[x[0], odd], sopts=conj), dict(branches=x, sopts=refd),
                 dict(branches=x, sopts=None), dict(branches=x[:1], sopts=conj, want_gain=True),
                 dict(branches=x, sopts=conj, tracking=2), dict(branches=x, sopts=conj, want_phase=True),
                 dict(branches=x, sopts=conj, timing=3), dict(branches=x, sopts=conj, want_timing=True),
                 dict(branches=x, sopts=abi.StreamOpts(1, 1.5))]
        for kw in cases:
            kw = dict(dict(timing=0, tracking=0), **kw)
            rc, out, cnt = raw_call(eng, pkg, kw.pop("branches"), 2, kw.pop("sopts"), kw.pop("timing"), kw.pop("tracking"), **kw)
            assert rc == -1 and lib.ofdm_last_error(), kw
            for k in FILL:
                assert untouched(out, k), (kw, k)
            assert cnt == [-7, -7]
        assert sum(launches(eng, abi).values()) == 0
        # d_gain = NULL and d_phase = NULL are accepted and change nothing else
        rc, full, cnt = raw_call(eng, pkg, x, 2, conj, 1, 1, want_timing=True, want_phase=True, want_gain=True)
        rc0, bare, cnt0 = raw_call(eng, pkg, x, 2, conj, 1, 1, want_timing=True)
        assert rc == rc0 == 0 and cnt == cnt0 == [8, 8]
        for k in ("pk", "cnt", "words", "eq", "row", "metric", "cross", "tim"):
            assert bare[k] == full[k], k
        assert untouched(bare, "phase") and untouched(bare, "gain") and not untouched(full, "phase")
        g = np.frombuffer(full["gain"], np.float32).reshape(64, 2)
        assert (g[8:] == 7.5).all() and not (g[:8] == 7.5).any()     # rows past d_count[1] are never written
        got = launches(eng, abi)
        assert got == dict({k: 0 for k in IDS}, K_STREAM_DETECT_DIV=2, K_STREAM_SELECT=2, K_STREAM_TIMING_DIV=2, K_STREAM_DECODE_DIV=2)
    finally:
        eng.timing(False)
    # what the Engine refuses before any launch
    t = torch.stack(x)
    for bad in (t[:, ::2], t.real, torch.stack(x * 3)[:5], [x[0], x[1][:-1]], [x[0], x[1].cpu()], "x", xs.astype(np.complex128), xs[0]):
        with pytest.raises(ValueError):
            eng.receive_diversity(bad, detector="conjugate")
    for fn in (eng.receive_diversity, eng.receive_diversity_device):
        with pytest.raises(ValueError, match="conjugate"):
            fn(t)                                                    # two branches under the default detector
    dvc = eng.receive_diversity_device(t, detector="conjugate", timing="ltf", tracking="pilots")
    assert [int(v) for v in dvc["d_count"].cpu()] == [8, 8] and dvc["d_gain"].shape[1] == 2 and dvc["d_phase"].shape[1] == 2
    assert same_bits(dvc["d_gain"][:8].cpu().numpy(), g[:8])


# ---------------------------------------------------------------- 8. the link sweep
def test_link_sweep_with_branches(pkg):
    from ofdm_amd import sweep
    abi = pkg.abi
    words = ref.rand_words(2, 256, 0xD1F)
    snrs = (10.0, 20.0)
    kw = dict(noise="complex", fading=dict(pdp=[1.0]), detector="conjugate", timing="ltf")
    with pkg.Engine(0) as e:
        plain = sweep.link_sweep(e, words, 2, 500, snrs, **kw)
        res = {b: sweep.link_sweep(e, words, 2, 500, snrs, branches=b, **kw) for b in (1, 2)}
    ber = {}
    for b, r in res.items():
        for s, row in zip(snrs, r["totals"]):
            print(f"link branches {b} {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, received {row[abi.S_RECEIVED]}, "
                  f"bit errors {row[abi.S_BIT_ERR]} of {row[abi.S_BITS]}")
        ber[b] = r["totals"][:, abi.S_BIT_ERR] / np.maximum(r["totals"][:, abi.S_BITS], 1)
    assert np.array_equal(res[1]["totals"], plain["totals"]) and res[1]["power"] == plain["power"]
    assert (res[2]["totals"][:, abi.S_MATCHED] >= res[1]["totals"][:, abi.S_MATCHED]).all()
    assert res[1]["totals"][0, abi.S_BIT_ERR] > 0 and ber[2][0] < ber[1][0]
