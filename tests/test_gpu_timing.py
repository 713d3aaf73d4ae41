"""GPU tests of the stream receiver's fine timing (include/ofdm_mi355x_timing.h, ofdm_receive_stream_timed,
Engine.receive_stream(timing=), csrc/ofdm_stream_timing.hip): OFDM_TIMING_NONE byte for byte against
ofdm_receive_stream_ex, noise-free streams that keep their positions, the refined positions of noisy and faded streams
against stream.refine_timing in fp64 -- exactly -- with the decode at the refined position against the oracle, the
stream's end, a tie of all candidates, an all-zero search window, the reference detector's coarse positions,
launch-shape independence, the link sweep and the stream command.  tests/test_gpu_matlab_stream.py holds
OFDM_TIMING_LTF_MATLAB, the same kernel with the other convention's template.

Streams: detect_ref.noisy_stream under detect_ref.STREAM_SEEDS (25,420 to 27,194 samples, 290 packets in all) and
timing_ref.clean_stream.  tests/test_timing_host.py checks on the CPU that on every one of the 290 packets the two
largest L differ by more than 1e-4 of the larger (the smallest gap is 1.23e-4), which is what lets these tests demand
the fp64 rule's position exactly: the kernel's L must then be within 6e-5, half that gap.

The quality's deviation is |quality_gpu - quality_ref| against the fp64 rule with the oracle's template (quality lies in
[0, 1]; its numerator is L of the chosen candidate, so the relative deviation of L is that of the quality up to the
rounding of the power sums).  TIMING_DEV_MEASURED is its largest value over the 290 packets and the noise-free streams
on an MI355X, 3.29e-7 (D = 2, 14 dB, faded, relative 3.9e-7; 7e-8 to 2.9e-7 on the other streams, 7e-8 to 2.3e-7 on the
noise-free ones): a few fp32 steps, as 32-term chains of fused multiply-adds give.  The tests assert 4 x that, which
must stay under 6e-5 -- it does by a factor of 45.  The device's template differs from the oracle's by 1.7e-7 of its
peak (fp32 Transmitter() against fp64), which the figure includes.
Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import detect_ref as ref
import timing_ref as tr
from test_gpu_captures import CFO_TOL_HZ, check_against_oracle

pytestmark = pytest.mark.gpu

TIMING_DEV_MEASURED = 3.29e-7   # measured on an MI355X, see the module docstring
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
def tmpl(pkg, oracle):
    return tr.template(oracle)


def blank_truth(d):
    from ofdm_amd.stream import pack_messages
    return ref.bits_of(pack_messages([" " * (12 * d)], d)[0])[0]


def rx(eng, x, timing, detector="conjugate", **kw):
    kw = dict(dict(want_bits=True, want_eq=True), **kw)
    return eng.receive_stream(x if _torch().is_tensor(x) else np.ascontiguousarray(x, np.complex64), detector=detector,
                              timing=timing, **kw)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def quality_dev(out, want):
    return float(np.abs(out["quality"].astype(np.float64) - want["quality"]).max()) if len(want["quality"]) else 0.0


@pytest.fixture(scope="module")
def runs(eng, oracle, tmpl):
    """The 24 streams through the conjugate detector without and with timing, and the fp64 rule on the coarse positions
    (shared, left unchanged by the tests)."""
    from ofdm_amd.stream import refine_timing
    out = []
    for (d, snr, cfo, faded), seed in ref.STREAM_SEEDS.items():
        assert eng.set_long_message(" " * (12 * d)) == d
        x, pos = ref.noisy_stream(oracle, d, snr, cfo, faded, seed)
        none, ltf = rx(eng, x, "none"), rx(eng, x, "ltf")
        out.append(dict(d=d, snr=snr, cfo=cfo, faded=faded, x=x, pos=pos, none=none, ltf=ltf,
                        want=refine_timing(x, none["positions"], tmpl)))
    _torch().cuda.synchronize()
    return out


def tag(r):
    return f"D={r['d']:2d} {r['snr']} dB {r['cfo']:7.0f} Hz {'faded  ' if r['faded'] else 'unfaded'}"


# ---------------------------------------------------------------- 1. timing off is today's receiver
def raw_call(eng, pkg, x_dev, nd, sopts, timing=None, max_packets=64, want_timing=False):
    """ofdm_receive_stream_ex (timing None) or ofdm_receive_stream_timed through ctypes on outputs prefilled with a
    sentinel: every output as host bytes"""
    torch = _torch()
    abi, lib = pkg.abi, eng.lib
    n = len(x_dev)
    lc = n - 47 if sopts is None or sopts.detector == 0 else n - 63
    pk = torch.full((max_packets, 64), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    words = torch.full((max_packets, 3 * nd), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    eq = torch.full((max_packets, 96 * nd), 7.5, dtype=torch.float32, device="cuda")
    row = torch.zeros(abi.NCOUNTERS, dtype=torch.int64, device="cuda")
    metric = torch.full((lc,), -3.0, dtype=torch.float32, device="cuda")
    cross = torch.full(((lc + 31) // 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tim = torch.full((max_packets, 16), 0x5A, dtype=torch.uint8, device="cuda")
    opts = abi.make_rx_opts("c")
    p = lambda t: C.c_void_p(t.data_ptr())
    so = None if sopts is None else C.byref(sopts)
    tail = (abi.PAYLOAD["message"], max_packets, p(pk), p(cnt), p(words), p(eq), p(row), p(metric), p(cross))
    if timing is None:
        rc = lib.ofdm_receive_stream_ex(eng.ctx, p(x_dev), n, C.byref(opts), so, *tail)
    else:
        rc = lib.ofdm_receive_stream_timed(eng.ctx, p(x_dev), n, C.byref(opts), so, timing, *tail,
                                           p(tim) if want_timing else None)
    assert rc == 0, lib.ofdm_last_error()
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().tobytes() for k, t in dict(pk=pk, cnt=cnt, words=words, eq=eq, row=row, metric=metric,
                                                          cross=cross, tim=tim).items()}, [int(v) for v in cnt.cpu()]


def test_timing_none_is_ofdm_receive_stream_ex(eng, pkg, oracle):
    torch = _torch()
    abi = pkg.abi
    assert eng.set_long_message(MSG2) == 2
    x, pos = ref.noisy_stream(oracle, 2, 20.0, 40e3, False, 502)
    x_dev = torch.from_numpy(x).cuda()
    eng.timing(True)
    try:
        eng.timing_reset()
        for sopts in (None, abi.StreamOpts(abi.DETECTOR["reference"], 0.75), abi.StreamOpts(abi.DETECTOR["conjugate"], 0.75)):
            base, cnt = raw_call(eng, pkg, x_dev, 2, sopts)
            none, _ = raw_call(eng, pkg, x_dev, 2, sopts, timing=abi.TIMING["none"])
            print(f"detector {None if sopts is None else sopts.detector}: {cnt[0]} packets of {len(pos)} sent")
            assert cnt[0] == cnt[1] == len(pos)
            for k in base:
                assert none[k] == base[k], k                         # d_timing among them: never written
        launches = {k: eng.timing_query(k)[1] for k in (abi.K_STREAM_DETECT, abi.K_STREAM_DETECT_CONJ, abi.K_STREAM_SELECT,
                                                        abi.K_STREAM_DECODE, abi.K_STREAM_TIMING)}
        # a non-NULL d_timing without timing, and an unknown timing, are refused before any launch
        lib, p = eng.lib, lambda t: C.c_void_p(t.data_ptr())
        pk = torch.full((8, 64), 0x5A, dtype=torch.uint8, device="cuda")
        cnt8 = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        tim = torch.full((8, 16), 0x5A, dtype=torch.uint8, device="cuda")
        opts = abi.make_rx_opts("c")
        for timing, d_timing in ((0, p(tim)), (3, None), (-1, p(tim))):
            rc = lib.ofdm_receive_stream_timed(eng.ctx, p(x_dev), len(x_dev), C.byref(opts), None, timing, 1, 8, p(pk), p(cnt8),
                                               None, None, None, None, None, d_timing)
            assert rc == -1 and lib.ofdm_last_error(), timing
        after = {k: eng.timing_query(k)[1] for k in launches}
    finally:
        eng.timing(False)
    torch.cuda.synchronize()
    assert launches == {abi.K_STREAM_DETECT: 4, abi.K_STREAM_DETECT_CONJ: 2, abi.K_STREAM_SELECT: 6, abi.K_STREAM_DECODE: 6,
                        abi.K_STREAM_TIMING: 0}
    assert after == launches
    assert (pk == 0x5A).all() and (cnt8 == -7).all() and (tim == 0x5A).all()
    # the Engine's default takes the same route, and refuses an unknown timing before any launch
    a, b = eng.receive_stream(x_dev, want_eq=True), eng.receive_stream(x_dev, want_eq=True, timing="none")
    assert a["records"].tobytes() == b["records"].tobytes() and a["coarse_pos"] is None and b["quality"] is None
    for bad in ("LTF", None, 1):
        with pytest.raises(ValueError):
            eng.receive_stream(x_dev, timing=bad)
        with pytest.raises(ValueError):
            eng.receive_stream_device(x_dev, timing=bad)


def test_d_timing_is_optional_and_only_its_first_rows_are_written(eng, pkg, oracle):
    torch = _torch()
    abi = pkg.abi
    assert eng.set_long_message(MSG2) == 2
    x, pos = ref.noisy_stream(oracle, 2, 14.0, 40e3, False, ref.STREAM_SEEDS[(2, 14, 40e3, False)])
    x_dev = torch.from_numpy(x).cuda()
    conj = abi.StreamOpts(abi.DETECTOR["conjugate"], 0.75)
    eng.timing(True)
    try:
        eng.timing_reset()
        without, cnt = raw_call(eng, pkg, x_dev, 2, conj, timing=abi.TIMING["ltf"])
        with_rows, _ = raw_call(eng, pkg, x_dev, 2, conj, timing=abi.TIMING["ltf"], want_timing=True)
        few, cnt5 = raw_call(eng, pkg, x_dev, 2, conj, timing=abi.TIMING["ltf"], max_packets=5, want_timing=True)
        launches = eng.timing_query(abi.K_STREAM_TIMING)
    finally:
        eng.timing(False)
    assert cnt == [len(pos), len(pos)] and cnt5 == [len(pos), 5] and launches[1] == 3 and launches[0] > 0
    for k in ("pk", "cnt", "words", "eq", "row", "metric", "cross"):
        assert without[k] == with_rows[k], k
    assert without["tim"] == bytes([0x5A]) * len(without["tim"])
    rows = np.frombuffer(with_rows["tim"], abi.stream_timing_dtype())
    tail = with_rows["tim"][16 * cnt[1]:]
    assert tail == bytes([0x5A]) * len(tail)                          # rows past d_count[1] are never written
    rec = np.frombuffer(with_rows["pk"], abi.stream_packet_dtype())[:cnt[1]]
    assert np.array_equal(rec["packet_pos"], rows["coarse_pos"][:cnt[1]] + rows["shift"][:cnt[1]]) and rows["shift"][:cnt[1]].any()
    assert few["tim"][:80] == with_rows["tim"][:80] and few["tim"][80:] == bytes([0x5A]) * (len(few["tim"]) - 80)
    assert few["pk"][:320] == with_rows["pk"][:320]


# ---------------------------------------------------------------- 2. clean streams keep their positions
@pytest.mark.parametrize("d,cfo", tr.CLEAN_CASES)
def test_clean_streams_keep_their_positions(eng, oracle, tmpl, d, cfo):
    from ofdm_amd.stream import refine_timing
    assert eng.set_long_message(" " * (12 * d)) == d
    words, x, pos = tr.clean_stream(oracle, d, cfo)
    x = x.astype(np.complex64)
    none, ltf = rx(eng, x, "none"), rx(eng, x, "ltf")
    want = refine_timing(x, none["positions"], tmpl)
    dev = quality_dev(ltf, want)
    print(f"D {d} {cfo:9.0f} Hz: positions {(ltf['positions'] - pos).tolist()}, quality {ltf['quality'].round(4).tolist()}, "
          f"deviation from fp64 {dev:.3g}")
    assert none["count"] == ltf["count"] == tr.CLEAN_PACKETS and np.array_equal(none["positions"], pos + 16)
    assert ltf["records"].tobytes() == none["records"].tobytes()
    assert same_bits(ltf["bits"], none["bits"]) and same_bits(ltf["eq"], none["eq"])
    assert np.array_equal(ltf["coarse_pos"], ltf["positions"]) and not ltf["shift"].any()
    assert np.array_equal(want["positions"], none["positions"])
    assert np.array_equal(ltf["bits"], ref.bits_of(words))
    assert 4 * TIMING_DEV_MEASURED < 6e-5 and dev <= 4 * TIMING_DEV_MEASURED


# ---------------------------------------------------------------- 3. noisy streams
def test_refined_positions_are_the_fp64_rule(runs):
    worst, packets = 0.0, 0
    for r in runs:
        none, ltf, want = r["none"], r["ltf"], r["want"]
        dev = quality_dev(ltf, want)
        off, _ = tr.offsets(ltf["positions"], r["pos"])
        coff, _ = tr.offsets(none["positions"], r["pos"])
        print(f"{tag(r)}: {ltf['count']} packets, coarse {int(coff.min())}..{int(coff.max())}, refined {int(off.min())}.."
              f"{int(off.max())}, quality deviation {dev:.3g}, smallest gap {tr.top_gap(want['metric']).min():.3g}")
        worst, packets = max(worst, dev), packets + ltf["count"]
        assert ltf["count"] == ltf["found"] == none["count"] == none["found"] > 0
        assert np.array_equal(ltf["coarse_pos"], none["positions"])
        assert np.array_equal(ltf["positions"], want["positions"])
        assert np.array_equal(ltf["shift"], want["shift"]) and np.array_equal(ltf["positions"] - ltf["coarse_pos"], ltf["shift"])
        assert np.array_equal(ltf["records"]["packet_idx"], ltf["positions"].astype(np.int32))
        assert np.array_equal(ltf["records"]["flags"], none["records"]["flags"]) and not ltf["records"]["reserved8"].any()
        assert (ltf["quality"] > 0).all() and (ltf["quality"] <= 1).all()
        if r["faded"]:
            assert ((off >= 15) & (off <= 19)).all()
        else:
            assert (off == 16).all()
        # a record whose position did not move is the record without timing, bit for bit
        keep = np.nonzero(ltf["shift"] == 0)[0]
        assert ltf["records"][keep].tobytes() == none["records"][keep].tobytes()
        assert same_bits(ltf["eq"][keep], none["eq"][keep])
    print(f"timing: {packets} packets, largest quality deviation {worst:.4g} (TIMING_DEV_MEASURED {TIMING_DEV_MEASURED})")
    assert packets == 290
    assert 4 * TIMING_DEV_MEASURED < 6e-5
    assert worst <= 4 * TIMING_DEV_MEASURED


def test_decode_at_the_refined_position_against_the_oracle(runs, oracle):
    total, cfo_dev = 0, 0.0
    for r in runs:
        d, ltf, x = r["d"], r["ltf"], r["x"].astype(np.complex128)
        truth = blank_truth(d)                                        # the receiver counts errors against the context's message
        nfr = 320 + 80 * d
        caps, ora = [], []
        for p in ltf["positions"]:
            lo = int(p) - 40
            assert lo >= 0 and lo + 2 * nfr + 100 <= len(x)
            caps.append(x[lo:lo + 2 * nfr + 100])
            ora.append(oracle.decode_at(caps[-1], truth, 40, dumps=True, cap_len=len(caps[-1])))
        rec = ltf["records"].copy()
        rec["packet_idx"] = 40
        rec["flags"] &= 3
        same = check_against_oracle(rec, ltf["bits"], ltf["eq"], ora, caps, truth, 0)
        assert len(same) == ltf["count"]
        for k in same:
            cfo_dev = max(cfo_dev, abs(float(rec["cfo_coarse_hz"][k]) - float(ora[k]["cfo"][0])),
                          abs(float(rec["cfo_fine_hz"][k]) - float(ora[k]["cfo"][1])))
        total += len(same)
    print(f"decode at the refined positions: {total} packets, CFO within {cfo_dev:.4g} Hz")
    assert total == 290 and cfo_dev <= CFO_TOL_HZ


# ---------------------------------------------------------------- 4. the stream's end
def test_stream_end(eng, runs, tmpl):
    from ofdm_amd.stream import refine_timing
    r = next(q for q in runs if (q["d"], q["snr"], q["cfo"], q["faded"]) == (2, 14, 40e3, False))
    assert eng.set_long_message(MSG2) == 2
    full = r["ltf"]
    k = int(np.nonzero(full["shift"])[0][-1])
    p = int(full["coarse_pos"][k])
    for n, refined in ((p + 641, True), (p + 640, False)):
        cut, none = rx(eng, r["x"][:n], "ltf"), rx(eng, r["x"][:n], "none")
        want = refine_timing(r["x"][:n], none["positions"], tmpl)
        print(f"cut at p + {n - p}: positions {cut['positions'][-2:].tolist()}, shift {cut['shift'][-2:].tolist()}, flags "
              f"{cut['records']['flags'][-2:].tolist()}, quality {cut['quality'][-2:].round(4).tolist()}")
        assert cut["count"] == k + 1 and np.array_equal(none["positions"], full["coarse_pos"][:k + 1])
        assert np.array_equal(cut["positions"], want["positions"]) and np.array_equal(cut["shift"], want["shift"])
        assert (cut["shift"][k] != 0) == refined and (cut["quality"][k] > 0) == refined
        assert cut["positions"][k] == (full["positions"][k] if refined else p)
        if not refined:
            assert cut["quality"][k] == 0.0 and cut["records"][k].tobytes() == none["records"][k].tobytes()
        # OFDM_CAPTURE_OOB by the existing rule at the final position, OFDM_STREAM_LAST_FRONT from the front
        oob = cut["positions"] + 2 * (480 - 1) >= n + 20
        assert oob.tolist() == [False] * k + [True]
        assert np.array_equal(cut["records"]["flags"], 2 * oob + 4 * (np.arange(k + 1) == k))
        assert cut["records"][:k].tobytes() == full["records"][:k].tobytes()


# ---------------------------------------------------------------- 4b. ties, an all-zero window, the other detector
TIE_VALUE = 0.25 + 0.125j


def _two_packets_with_a_flat_window(oracle, value):
    """Two noise-free packets of 2 data symbols; the second one's search window [p + 322, p + 640] (p its coarse
    position, first sample + 16: behind the short training field, so the detection does not see it) holds one value"""
    x, pos = ref.packet_stream(oracle, ref.rand_words(2, 2, 0x71E))
    p = int(pos[1]) + 16
    x[p + 322:p + tr.SPAN + 1] = value
    return x.astype(np.complex64), pos, p


def test_equal_candidates_take_the_smallest_shift(eng, oracle, tmpl):
    """All 64 candidates of the second packet run the same chain on the same values, so their L are bit-equal on the
    device and equal in fp64: the rule's tie-break (the butterfly's `ov == best && oj < bj`) must choose candidate 0."""
    from ofdm_amd.stream import refine_timing
    assert eng.set_long_message(MSG2) == 2
    x, pos, p = _two_packets_with_a_flat_window(oracle, TIE_VALUE)
    none, ltf = rx(eng, x, "none"), rx(eng, x, "ltf")
    want = refine_timing(x, none["positions"], tmpl)
    dev = quality_dev(ltf, want)
    print(f"tie: coarse {(none['positions'] - pos).tolist()}, shifts {ltf['shift'].tolist()} (fp64 {want['shift'].tolist()}), quality "
          f"{ltf['quality'].tolist()} (fp64 {want['quality'].tolist()}, deviation {dev:.3g}), spread of the fp64 L {np.ptp(want['metric'][1]):.3g}")
    assert none["count"] == ltf["count"] == 2 and np.array_equal(none["positions"], pos + 16) and none["positions"][1] == p
    assert np.ptp(want["metric"][1]) == 0.0 and want["metric"][1][0] > 0            # a tie of all 64 in fp64 as well
    assert ltf["shift"].tolist() == want["shift"].tolist() == [0, -56]
    assert np.array_equal(ltf["positions"], want["positions"]) and ltf["positions"][1] == p - 56
    assert np.array_equal(ltf["coarse_pos"], none["positions"])
    assert 0 < ltf["quality"][1] < 1 and dev <= 4 * TIMING_DEV_MEASURED
    assert ltf["records"][:1].tobytes() == none["records"][:1].tobytes()


def test_an_all_zero_window_keeps_the_position(eng, oracle, tmpl):
    """every L is 0: the kernel's `lbest > 0` branch -- shift 0, quality exactly 0 and no NaN, the record untouched"""
    from ofdm_amd.stream import refine_timing
    assert eng.set_long_message(MSG2) == 2
    x, pos, p = _two_packets_with_a_flat_window(oracle, 0.0)
    assert not x[p + 322:p + 641].any() and x[p + 321] != 0
    none, ltf = rx(eng, x, "none"), rx(eng, x, "ltf")
    want = refine_timing(x, none["positions"], tmpl)
    print(f"zero window: shifts {ltf['shift'].tolist()}, quality {ltf['quality'].tolist()} (fp64 {want['quality'].tolist()})")
    assert none["count"] == ltf["count"] == 2 and none["positions"][1] == p
    assert want["shift"].tolist() == [0, 0] and want["quality"][1] == 0.0
    assert ltf["shift"].tolist() == [0, 0] and ltf["quality"][1] == 0.0 and np.isfinite(ltf["quality"]).all()
    assert ltf["quality"][0] > 0.89 and quality_dev(ltf, want) <= 4 * TIMING_DEV_MEASURED
    assert np.array_equal(ltf["coarse_pos"], none["positions"]) and np.array_equal(ltf["positions"], none["positions"])
    assert ltf["records"].tobytes() == none["records"].tobytes()
    assert same_bits(ltf["bits"], none["bits"]) and same_bits(ltf["eq"], none["eq"])


@pytest.mark.parametrize("key", [(2, 25, 0.0, False), (15, 14, 40e3, False)])
def test_timing_under_the_reference_detector(eng, oracle, tmpl, key):
    """detector="reference" with timing="ltf": the positions are the fp64 rule on that detector's coarse positions"""
    from ofdm_amd.stream import refine_timing
    d = key[0]
    assert eng.set_long_message(" " * (12 * d)) == d
    x, pos = ref.noisy_stream(oracle, *key, ref.STREAM_SEEDS[key])
    none, ltf = rx(eng, x, "none", detector="reference"), rx(eng, x, "ltf", detector="reference")
    want = refine_timing(x, none["positions"], tmpl)
    dev, gap = quality_dev(ltf, want), tr.top_gap(want["metric"]).min()
    off, _ = tr.offsets(ltf["positions"], pos)
    print(f"reference detector {key}: {ltf['count']} packets of {len(pos)}, shifts {sorted(set(ltf['shift'].tolist()))}, refined "
          f"{int(off.min())}..{int(off.max())}, quality deviation {dev:.3g}, smallest gap {gap:.3g}")
    assert ltf["count"] == ltf["found"] == none["count"] == len(pos) and ltf["shift"].any()
    assert gap > 1e-4                                                 # what lets the positions be demanded exactly
    assert np.array_equal(ltf["coarse_pos"], none["positions"])
    assert np.array_equal(ltf["positions"], want["positions"]) and np.array_equal(ltf["shift"], want["shift"])
    assert (off == 16).all() and dev <= 4 * TIMING_DEV_MEASURED
    keep = np.nonzero(ltf["shift"] == 0)[0]
    assert ltf["records"][keep].tobytes() == none["records"][keep].tobytes() and same_bits(ltf["eq"][keep], none["eq"][keep])


# ---------------------------------------------------------------- 5. launch shapes
def test_launch_shape_independence(eng, runs):
    torch = _torch()
    r = next(q for q in runs if (q["d"], q["snr"], q["cfo"], q["faded"]) == (2, 14, 40e3, True))
    assert eng.set_long_message(MSG2) == 2
    base = r["ltf"]
    x = torch.from_numpy(r["x"]).cuda()
    n = len(x)
    timing_rows = lambda o: np.stack([o["coarse_pos"], o["shift"].astype(np.int64), o["quality"].view(np.int32).astype(np.int64)])
    buf = torch.zeros(n + 4, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for off in (1, 2):                                                # 8 bytes off a 16-byte line, and on one
        view = buf[off:off + n]
        view.copy_(x)
        assert view.data_ptr() % 16 == 8 * (off & 1)
        o = rx(eng, view, "ltf")
        assert o["records"].tobytes() == base["records"].tobytes() and np.array_equal(timing_rows(o), timing_rows(base))
        assert same_bits(o["eq"].cpu().numpy(), base["eq"]) and same_bits(o["bits"].cpu().numpy(), base["bits"])
    assert torch.equal(torch.view_as_real(buf[2:2 + n]), torch.view_as_real(x))          # the input is never written
    # max_packets below the number found: the first rows
    for k in (1, 5):
        o = rx(eng, r["x"], "ltf", max_packets=k)
        assert o["found"] == base["found"] > 5 and o["count"] == k
        assert o["records"].tobytes() == base["records"][:k].tobytes()
        assert np.array_equal(timing_rows(o), timing_rows(base)[:, :k]) and same_bits(o["eq"], base["eq"][:k])
    o = rx(eng, r["x"], "ltf", max_packets=0, want_bits=False, want_eq=False)
    assert o["found"] == base["found"] and o["count"] == 0 and len(o["quality"]) == 0
    # the same samples 260 detection runs further into a longer recording
    shift = 31 * 260
    long = torch.zeros(shift + n + 1000, dtype=torch.complex64, device="cuda")
    long[shift:shift + n] = x
    o = rx(eng, long, "ltf")
    c = base["count"]
    assert o["count"] == c
    assert np.array_equal(o["positions"], base["positions"] + shift) and np.array_equal(o["coarse_pos"], base["coarse_pos"] + shift)
    assert np.array_equal(o["shift"], base["shift"]) and np.array_equal(o["quality"].view(np.int32), base["quality"].view(np.int32))
    assert same_bits(o["eq"].cpu().numpy(), base["eq"]) and same_bits(o["bits"].cpu().numpy(), base["bits"])
    for name in ("flags", "bit_err", "cfo_coarse_hz", "cfo_fine_hz", "evm_pre_sum"):
        assert same_bits(o["records"][name], base["records"][name]), name


# ---------------------------------------------------------------- 6. the link sweep
LINK_GOLDEN = "link_default_256.csv"     # `link --packets 256 --snr 10:30:20 --noise complex` before the timing option existed


def test_link_sweep_with_timing(pkg, tmp_path):
    from conftest import GOLDEN
    from ofdm_amd import sweep
    from ofdm_amd.stream import score_packets
    abi = pkg.abi
    words = ref.rand_words(2, 256, 0x11B)
    gap, snrs = 500, (30.0, 10.0)
    stride = abi.packet_len(2) + gap
    tx_pos = gap + stride * np.arange(256)
    with pkg.Engine(0) as e:
        res = {t: sweep.link_sweep(e, words, 2, gap, snrs, cfo_hz=40e3, noise="complex", detector="conjugate", timing=t)
               for t in ("none", "ltf")}
        exact = sweep.link_sweep(e, words, 2, gap, snrs, cfo_hz=40e3, noise="complex", detector="conjugate", timing="ltf",
                                 window=(16, 16))
        for t, r in res.items():
            for s, row in zip(snrs, r["totals"]):
                print(f"link timing {t} {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, received "
                      f"{row[abi.S_RECEIVED]}, bit errors {row[abi.S_BIT_ERR]} of {row[abi.S_BITS]}")
        # every matched record lies at tx_pos + 16: the window (16, 16) matches what (8, 40) matches
        assert np.array_equal(exact["totals"], res["ltf"]["totals"])
        assert (res["ltf"]["totals"][:, abi.S_MATCHED] >= res["none"]["totals"][:, abi.S_MATCHED]).all()
        assert res["ltf"]["totals"][0, abi.S_MATCHED] == 256
        assert res["ltf"]["totals"][1, abi.S_BIT_ERR] <= res["none"]["totals"][1, abi.S_BIT_ERR]
        # the same sweep through the library calls, scored on the host, packet by packet
        rec = e.transmit_packets(words, 2, pos0=gap, stride=stride, n_out=256 * stride + gap)
        for q, s in enumerate(snrs):
            y = e.impair_stream(rec, res["ltf"]["power"], s, 40e3, noise="complex", snr_index=q)
            got = {}
            for t in ("none", "ltf"):
                o = e.receive_stream(y, detector="conjugate", timing=t, keep_device=True)
                w = o["d_words"][:o["count"]].cpu().numpy().view(np.uint32)
                got[t] = (o, score_packets(tx_pos, words, o["positions"], w, window=(8, 40)))
                assert np.array_equal(res[t]["totals"][q], got[t][1]["totals"])
            (on, sn), (ol, sl) = got["none"], got["ltf"]
            hit = sl["rx_index"] >= 0
            assert np.array_equal(ol["positions"][sl["rx_index"][hit]], tx_pos[hit] + 16)
            assert not ((sn["rx_index"] >= 0) & ~hit).any()           # no record that timing "none" matched is lost
            assert np.array_equal(ol["coarse_pos"], on["positions"])
    # the default arguments are the command as it was: link.csv byte for byte
    out = tmp_path / "link"
    assert sweep.link_main(["--packets", "256", "--snr", "10:30:20", "--noise", "complex", "--out", str(out)]) == 0
    assert (out / "link.csv").read_bytes() == (GOLDEN / LINK_GOLDEN).read_bytes()


# ---------------------------------------------------------------- 7. the stream command
def test_stream_command_writes_coarse_pos(pkg, tmp_path):
    import csv
    from ofdm_amd import stream, sweep
    base = ["--frames", "6", "--snr", "12", "--noise", "complex", "--detector", "conjugate"]
    assert stream.main(base + ["--out", str(tmp_path / "none")]) == 0
    assert stream.main(base + ["--timing", "ltf", "--out", str(tmp_path / "ltf")]) == 0
    none = list(csv.reader(open(tmp_path / "none" / "packets.csv")))
    ltf = list(csv.reader(open(tmp_path / "ltf" / "packets.csv")))
    cols = ["packet_pos", "flags", "cfo_coarse_hz", "cfo_fine_hz", "bit_err", "evm_db_pre", "message"]
    assert none[0] == cols and ltf[0] == cols + ["coarse_pos"]        # the column only when timing is on
    assert len(none) == len(ltf) == 7
    coarse = [int(r[0]) for r in none[1:]]
    print(f"stream command: coarse {coarse}, refined {[int(r[0]) for r in ltf[1:]]}")
    assert [int(r[7]) for r in ltf[1:]] == coarse
    # 980 samples per packet and 500 per gap: the refined positions sit on the grid, first sample + 16
    assert [int(r[0]) for r in ltf[1:]] == [500 + 16 + 1480 * k for k in range(6)]
    with pytest.raises(SystemExit):
        stream.main(base + ["--timing", "fine"])
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--timing", "fine"])
    with pytest.raises(ValueError):
        with pkg.Engine(0) as e:
            sweep.link_sweep(e, ref.rand_words(2, 4, 1), 2, 500, [20.0], timing="fine")
