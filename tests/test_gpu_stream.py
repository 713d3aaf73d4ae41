"""GPU tests of the stream receiver (include/ofdm_mi355x_stream.h, Engine.receive_stream): the detection metric and the
crossings against the double-precision metric, the selection bit for bit against stream.select_packets, tile edges, the
decoded packets against the windowed oracle and against Engine.receive_captures on the same windows, launch-shape
independence, the edges of the rule and the argument checks.

Streams are the base stream zeros(700) | wave | zeros(1500) | wave[:3 period] | zeros(400) with real-only noise over all
of it (15,340 samples for the 2-symbol message, 21,580 for the 5-symbol one; 13 transmitted packets each).

The metric's deviation.  M = |c|^2 / p^2 with c a sum of 32 products that cancel when M is small: the fp32 error of c
is relative to p, not to |c|, so the relative error of M grows without bound as M -> 0 (an fp32 restatement of the
kernel's sums on the CPU gives 2e-3 at M ~ 1e-10) although no decision depends on M there.  The deviation is therefore
taken as |M_gpu - M_ref| / max(M_ref, 0.075): relative from one decade below the 0.75 threshold upwards, and against
that floor below it.  The plain relative figure is printed beside it (6.2e-3 on an MI355X, at M = 1.2e-7).  Measured
on an MI355X over the 18 base streams: 1.184e-4, METRIC_MEASURED below (at 25 dB, where the power window leaves a
packet for a gap 25 dB down and p cancels); the test asserts 4 x that, which must stay under 1e-3, the threshold jitter
the parity rule of test_gpu_captures.py treats as "on the threshold".  On the same run: no crossing differs from the
double-precision one outside |M - 0.75| <= 0.75e-3 (at most 0.28 % of the positions lie inside), the selection equals
stream.select_packets everywhere, and of 186 packets with a fitting window the oracle places none elsewhere (eq within
6.2e-7, evm_db_pre within 8.4e-6 dB, CFO estimates within 0.0234 Hz; eq bit-identical to receive_captures).
Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from conftest import normwise
from test_gpu_captures import CFO_TOL_HZ, check_against_oracle
from test_stream_host import CFOS, MSG, MSG5, base_stream

pytestmark = pytest.mark.gpu

SNRS = (10, 14, 25)
METRIC_FLOOR = 0.075
METRIC_MEASURED = 1.184e-4
METRIC_TOL = 4 * METRIC_MEASURED
BAND = 0.75e-3


def _torch():
    import torch
    return torch


def metric64(x):
    """Packet_Detection's M in double precision (test_lazy_rule.corr_out without its cast to float)"""
    x = np.asarray(x).astype(np.complex128)
    lc = len(x) - 47
    cs = np.concatenate([[0], np.cumsum(x[:-16] * x[16:])])
    cp = np.concatenate([[0], np.cumsum(np.abs(x[16:]) ** 2)])
    n = np.arange(lc)
    with np.errstate(all="ignore"):
        return np.abs(cs[n + 32] - cs[n]) ** 2 / (cp[n + 32] - cp[n]) ** 2


def run(engine, x, **kw):
    """receive_stream on a host array with every output, and the rule on the crossings it returned"""
    from ofdm_amd.stream import select_packets, unpack_cross
    kw = dict(dict(want_bits=True, want_eq=True, want_metric=True, want_cross=True), **kw)
    out = engine.receive_stream(np.ascontiguousarray(x, np.complex64), **kw)
    if out["cross"] is not None:
        out["bitmap"] = unpack_cross(out["cross"], max(len(x) - 47, 0))
        out["sel"] = select_packets(out["bitmap"])
    return out


def assert_selection_exact(out, max_packets=None):
    sel = out["sel"]
    assert out["found"] == len(sel["positions"])
    k = out["found"] if max_packets is None else min(out["found"], max_packets)
    assert out["count"] == k == len(out["records"])
    assert np.array_equal(out["positions"], sel["positions"][:k])
    assert np.array_equal(out["records"]["flags"] & 4, sel["flags"][:k])
    assert not (out["records"]["flags"] & 1).any() and not out["records"]["reserved8"].any()
    assert np.array_equal(out["records"]["packet_idx"], out["positions"].astype(np.int32))


@pytest.fixture(scope="module")
def runs(engine, oracle):
    """The 18 base streams (D = 2 and 5; 10, 14, 25 dB; three CFOs) through receive_stream with a counters row, the
    windowed oracle and receive_captures on every packet whose window [f - 400, f - 400 + cap_len) fits (shared, left
    unchanged by the tests)."""
    torch = _torch()
    all_runs = []
    try:
        for nd, msg in ((2, MSG), (5, MSG5)):
            assert engine.set_message(msg) == nd
            truth = oracle.message_bits(msg)
            wave = oracle.frame_waveform(truth)
            cap_len = int(len(wave) * 0.307)
            for snr in SNRS:
                for q, cfo in enumerate(CFOS):
                    x = base_stream(wave, snr, cfo, 1000 * nd + 10 * snr + q)
                    row = engine.new_counters(1)[0]
                    out = run(engine, x, counters=row)
                    r = dict(nd=nd, snr=snr, cfo=cfo, x=x, out=out, row=row.cpu().numpy().copy(), truth=truth,
                             cap_len=cap_len, ref=metric64(x))
                    fit = [k for k, p in enumerate(out["positions"])
                           if p - 411 >= 0 and p - 411 + cap_len <= len(x)]
                    r["fit"] = fit
                    r["starts"] = [int(out["positions"][k]) - 411 for k in fit]
                    r["windows"] = np.stack([x[s:s + cap_len] for s in r["starts"]]) if fit else np.zeros((0, cap_len), np.complex64)
                    r["ora"] = [oracle.receiver_frame(w.astype(np.complex128), truth, "c", dumps=True) for w in r["windows"]]
                    r["cap"] = engine.receive_captures(r["windows"], want_bits=True, want_eq=True)
                    all_runs.append(r)
    finally:
        engine.set_message(MSG)
    torch.cuda.synchronize()
    return all_runs


# ---------------------------------------------------------------- 1. the metric
def test_metric_against_double(runs):
    worst, plain = 0.0, 0.0
    for r in runs:
        g, ref = r["out"]["metric"].astype(np.float64), r["ref"]
        assert len(g) == len(ref) == len(r["x"]) - 47
        ok = np.isfinite(ref)
        assert ok.sum() > 0.99 * len(ref) and np.isfinite(g[ok]).all()
        dev = np.abs(g[ok] - ref[ok]) / np.maximum(ref[ok], METRIC_FLOOR)
        rel = np.abs(g[ok] - ref[ok]) / np.maximum(ref[ok], 1e-300)
        print(f"D={r['nd']} {r['snr']:2d} dB {r['cfo']:9.0f} Hz: deviation {dev.max():.3g} (at M = {ref[ok][dev.argmax()]:.3g}), "
              f"plain relative {rel.max():.3g} (at M = {ref[ok][rel.argmax()]:.3g})")
        worst, plain = max(worst, float(dev.max())), max(plain, float(rel.max()))
    print(f"metric: largest deviation {worst:.4g} (tolerance {METRIC_TOL:.4g}), largest plain relative deviation {plain:.4g}")
    assert METRIC_TOL < 1e-3
    assert worst <= METRIC_TOL


# ---------------------------------------------------------------- 2. the crossings
def test_crossings_against_double(runs):
    for r in runs:
        ref, got = r["ref"], r["out"]["bitmap"]
        with np.errstate(invalid="ignore"):
            want = ref > 0.75
            off = np.abs(ref - 0.75) > BAND                      # False where the reference is NaN
            band = np.abs(ref - 0.75) <= BAND
        diff = int((got != want)[off].sum())
        share = band.sum() / len(ref)
        print(f"D={r['nd']} {r['snr']:2d} dB {r['cfo']:9.0f} Hz: {int(got.sum())} crossings, {diff} differ off the band, "
              f"{int(band.sum())} positions ({100 * share:.2f} %) in it, {int((got != want)[band].sum())} differ there")
        assert diff == 0
        assert share <= 0.01
        assert not got[~np.isfinite(ref)].any()


# ---------------------------------------------------------------- 3. the selection is exact
def test_selection_is_exact(runs):
    for r in runs:
        assert_selection_exact(r["out"])
        n = len(r["x"])
        assert 8 <= r["out"]["found"] <= 13 <= n // 301 + 1
        if r["snr"] >= 14:
            assert r["out"]["found"] == 13


# ---------------------------------------------------------------- 4. tile edges
def _shifted(wave, x0, shift, seed):
    """x0 behind `shift` more samples of idle channel at the stream's noise level"""
    return np.concatenate([base_stream(wave, 25.0, 0.0, seed, segments=[("gap", shift)]), x0])


def test_tile_edges(engine, oracle, pkg):
    T = pkg.abi.STREAM_TILE
    wave = oracle.frame_waveform(oracle.message_bits(MSG))
    P = len(wave) // 10
    plain = [("gap", 700), ("wave", 0, 4 * P), ("gap", 400)]
    x0 = base_stream(wave, 25.0, 0.0, 41, segments=plain)
    o0 = run(engine, x0)
    assert_selection_exact(o0)
    assert o0["count"] == 4
    f0 = int(o0["positions"][0]) - 11
    cases = [("front at TILE - 1", x0, o0, T - 1 - f0), ("front at TILE", x0, o0, T - f0), ("front at TILE + 1", x0, o0, T + 1 - f0),
             ("front + 230 at TILE", x0, o0, T - 230 - f0), ("front + 230 at TILE - 1", x0, o0, T - 231 - f0)]
    # a stray crossing -- 48 samples of the STF plateau -- 250 positions (inside the look-back: the packet's front is
    # none) or 360 positions (outside it) ahead of the first packet's front, with front - 300 on a tile edge
    r0 = f0 - 700
    for name, dist in (("stray inside", 250), ("stray outside", 360)):
        seg = [("gap", 700), ("wave", r0 + 60, r0 + 108), ("gap", dist - 48 - r0), ("wave", 0, 4 * P), ("gap", 400)]
        xs = base_stream(wave, 25.0, 0.0, 42, segments=seg)
        os_ = run(engine, xs)
        assert_selection_exact(os_)
        stray = np.nonzero(os_["bitmap"][690:712])[0] + 690
        fs = 700 + dist
        near = os_["sel"]["fronts"][np.abs(os_["sel"]["fronts"] - fs) <= 8]
        print(f"{name}: stray crossings {stray.tolist()}, fronts {os_['sel']['fronts'].tolist()}, packets {os_['positions'].tolist()}")
        assert len(stray) and stray.min() in os_["sel"]["fronts"]      # the stray crossing is a front of its own
        assert len(near) == (0 if dist == 250 else 1) and os_["count"] == (3 if dist == 250 else 4)
        for edge in (T, T - 1):
            cases.append((f"{name}, front - 300 at {edge - T:+d}", xs, os_, edge + 300 - fs))
    for k, (name, x, o, shift) in enumerate(cases):
        o1 = run(engine, _shifted(wave, x, shift, 100 + k))
        assert_selection_exact(o1)
        print(f"{name}: shift {shift}, packets {o1['positions'].tolist()}")
        assert np.array_equal(o1["positions"], o["positions"] + shift), name
        assert np.array_equal(o1["bits"], o["bits"]) and np.array_equal(o1["records"]["bit_err"], o["records"]["bit_err"]), name


# ---------------------------------------------------------------- 5. the decoded packets
def _window_records(r):
    """the fitting packets' records in window coordinates, as test_gpu_captures.check_against_oracle reads them"""
    rec = r["out"]["records"][r["fit"]].copy()
    rec["packet_idx"] = (r["out"]["positions"][r["fit"]] - np.asarray(r["starts"], np.int64)).astype(np.int32)
    rec["flags"] &= 3
    return rec


def test_decode_against_the_oracle_and_receive_captures(runs):
    total = moved = 0
    cfo_dev = 0.0
    for r in runs:
        out, fit = r["out"], r["fit"]
        assert len(fit) >= 5
        rec = _window_records(r)
        assert (rec["packet_idx"] == 411).all()
        budget = len(fit)                                            # the 2 % bound is over all packets, below
        same = check_against_oracle(rec, out["bits"][fit], out["eq"][fit], r["ora"], r["windows"], r["truth"], budget)
        total += len(fit)
        moved += len(fit) - len(same)
        for k in same:
            o = r["ora"][k]
            cfo_dev = max(cfo_dev, abs(float(rec["cfo_coarse_hz"][k]) - float(o["cfo"][0])),
                          abs(float(rec["cfo_fine_hz"][k]) - float(o["cfo"][1])))
        # the same windows through the batched receiver: position, bits and flags are equal
        cap = r["cap"]["records"]
        assert np.array_equal(cap["packet_idx"].astype(np.int64) - 11 + np.asarray(r["starts"]), out["positions"][fit] - 11)
        assert np.array_equal(r["cap"]["bits"], out["bits"][fit])
        assert np.array_equal(cap["flags"], rec["flags"])
        assert np.array_equal(cap["bit_err"], rec["bit_err"])
        ident = np.array_equal(r["cap"]["eq"].view(np.float32), out["eq"][fit].view(np.float32))
        print(f"D={r['nd']} {r['snr']:2d} dB {r['cfo']:9.0f} Hz: {len(fit)} windows, eq vs receive_captures "
              f"{'bit-identical' if ident else 'within %.3g' % normwise(out['eq'][fit], r['cap']['eq'])}")
        assert normwise(out["eq"][fit], r["cap"]["eq"]) < 1e-6
    print(f"decode: {total} packets, {moved} placed elsewhere by the oracle window (threshold), CFO within {cfo_dev:.4g} Hz")
    assert total >= 150 and moved <= 0.02 * total
    assert cfo_dev <= CFO_TOL_HZ


def test_decode_multipath_cfo_complex_noise(engine, oracle):
    truth = oracle.message_bits(MSG)
    wave = oracle.frame_waveform(truth)
    x = base_stream(wave, 25.0, 40e3, 77, taps=[1, 0, 0.4 + 0.3j], noise="complex")
    out = run(engine, x)
    assert_selection_exact(out)
    assert out["found"] == 13
    r = dict(out=out, fit=[k for k, p in enumerate(out["positions"]) if p - 411 >= 0 and p - 411 + 3008 <= len(x)])
    r["starts"] = [int(out["positions"][k]) - 411 for k in r["fit"]]
    windows = np.stack([x[s:s + 3008] for s in r["starts"]])
    ora = [oracle.receiver_frame(w.astype(np.complex128), truth, "c", dumps=True) for w in windows]
    rec = _window_records(r)
    same = check_against_oracle(rec, out["bits"][r["fit"]], out["eq"][r["fit"]], ora, windows, truth, 0)
    assert len(same) == len(r["fit"]) >= 9
    assert not out["records"]["bit_err"].any() and all(m.startswith(MSG.decode()) for m in out["messages"])
    for k in same:
        assert abs(float(rec["cfo_coarse_hz"][k]) - float(ora[k]["cfo"][0])) <= CFO_TOL_HZ
        assert abs(float(rec["cfo_fine_hz"][k]) - float(ora[k]["cfo"][1])) <= CFO_TOL_HZ
    est = rec["cfo_coarse_hz"] + rec["cfo_fine_hz"]
    print(f"multipath stream: {out['found']} packets, coarse + fine {est.min():.0f} .. {est.max():.0f} Hz")
    assert abs(float(np.mean(est)) - 40e3) < 1e3


# ---------------------------------------------------------------- 6. launch shapes
def test_launch_shape_independence(engine, pkg, runs):
    torch = _torch()
    abi = pkg.abi
    r = next(q for q in runs if q["nd"] == 2 and q["snr"] == 14 and q["cfo"] == 40e3)
    x = torch.from_numpy(r["x"]).cuda()
    n = len(x)
    buf = torch.zeros(n + 4, dtype=torch.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    outs = []
    for off in (1, 2):                                                # 8 bytes off a 16-byte line, and on one
        view = buf[off:off + n]
        view.copy_(x)
        assert view.data_ptr() % 16 == 8 * (off & 1)
        row = engine.new_counters(1)[0]
        o = engine.receive_stream(view, want_bits=True, want_eq=True, want_metric=True, want_cross=True, counters=row)
        outs.append((o, row.cpu().numpy()))
    a, b = outs[0][0], outs[1][0]
    ref = r["out"]
    for o, row in outs:
        assert torch.equal(o["cross"], a["cross"]) and np.array_equal(o["cross"].cpu().numpy().view(np.uint32), ref["cross"])
        assert torch.equal(o["metric"].view(torch.int32), a["metric"].view(torch.int32))
        assert np.array_equal(o["positions"], ref["positions"]) and o["found"] == ref["found"] == o["count"]
        assert o["records"].tobytes() == ref["records"].tobytes()
        assert np.array_equal(o["bits"].cpu().numpy(), ref["bits"])
        assert np.array_equal(o["eq"].cpu().numpy().view(np.float32), ref["eq"].view(np.float32))
        # the counters row is the host reduction of the written records
        assert np.array_equal(row, abi.reduce_capture_records(o["records"], 2))
        assert np.array_equal(row, r["row"]) and row[abi.C_FRAMES] == o["count"] and row[abi.C_SYNC_FAIL] == 0
    assert torch.equal(torch.view_as_real(buf[2:2 + n]), torch.view_as_real(x))          # the input is never written
    for k in (1, 3):
        row = engine.new_counters(1)[0]
        o = engine.receive_stream(x, max_packets=k, want_bits=True, want_eq=True, want_cross=True, counters=row)
        assert o["found"] == ref["found"] and o["count"] == k
        assert o["records"].tobytes() == ref["records"][:k].tobytes()
        assert np.array_equal(o["bits"].cpu().numpy(), ref["bits"][:k])
        assert np.array_equal(o["eq"].cpu().numpy().view(np.float32), ref["eq"][:k].view(np.float32))
        assert np.array_equal(row.cpu().numpy(), abi.reduce_capture_records(ref["records"][:k], 2))
    o = engine.receive_stream(x, max_packets=0, want_bits=False)
    assert o["found"] == ref["found"] and o["count"] == 0 and len(o["records"]) == 0
    # records only (the kernel variant without outputs) gives the same records
    o = engine.receive_stream(x, want_bits=False)
    assert o["records"].tobytes() == ref["records"].tobytes() and o["bits"] is None and o["messages"] is None


# ---------------------------------------------------------------- 7. edges
def test_short_streams_have_no_packets(engine):
    rng = np.random.default_rng(7)
    for n in (0, 47, 48, 347):
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        o = run(engine, x)
        assert o["found"] == 0 and o["count"] == 0 and len(o["records"]) == 0 and o["messages"] == []
        assert len(o["metric"]) == max(n - 47, 0) and len(o["bitmap"]) == max(n - 47, 0)
        if n >= 48:
            assert np.allclose(o["metric"], metric64(x), rtol=1e-4)


def test_truncated_last_packet_and_start_inside_a_plateau(engine, oracle):
    wave = oracle.frame_waveform(oracle.message_bits(MSG))
    P = len(wave) // 10
    x = base_stream(wave, 25.0, 0.0, 51, segments=[("gap", 700), ("wave", 0, 3 * P), ("gap", 400)])
    full = run(engine, x)
    assert_selection_exact(full)
    assert full["count"] == 3 and not (full["records"]["flags"] & 2).any()
    # the stream ends 100 samples into the last packet's data (the data starts 2 x 320 samples past packet_pos)
    p = int(full["positions"][-1])
    cut = run(engine, x[:p + 640 + 100])
    assert_selection_exact(cut)
    assert np.array_equal(cut["positions"], full["positions"])
    assert cut["records"]["flags"].tolist() == [0, 0, 2 | 4]
    assert cut["records"][:2].tobytes() == full["records"][:2].tobytes()
    assert abs(float(cut["records"]["cfo_coarse_hz"][2]) - float(full["records"]["cfo_coarse_hz"][2])) < 1.0
    # the stream starts 40 samples into the first packet's plateau: no front there, the later packets stay
    f0 = int(full["positions"][0]) - 11
    mid = run(engine, x[f0 + 40:])
    assert_selection_exact(mid)
    assert mid["bitmap"][:100].any()
    assert np.array_equal(mid["positions"], full["positions"][1:] - (f0 + 40))
    assert np.array_equal(mid["bits"], full["bits"][1:])


def test_zero_power_gives_no_crossing(engine, oracle):
    z = run(engine, np.zeros(9000, np.complex64))
    assert z["found"] == 0 and not z["bitmap"].any() and np.isnan(z["metric"]).all()
    wave = oracle.frame_waveform(oracle.message_bits(MSG))
    P = len(wave) // 10
    x = base_stream(wave, 0.0, 0.0, 0, noise="none",
                    segments=[("gap", 700), ("wave", 0, 3 * P), ("gap", 1000), ("wave", 0, 2 * P), ("gap", 8000)])
    o = run(engine, x)
    assert_selection_exact(o)
    pw = np.abs(x.astype(np.complex128)) ** 2
    zero_power = np.convolve(pw, np.ones(32), "valid")[16:16 + len(x) - 47] == 0      # sum |r[i + 16 + k]|^2, k < 32
    assert zero_power.sum() > 8000 and not o["bitmap"][zero_power].any()
    assert np.isnan(o["metric"][zero_power]).all()
    print(f"noise-free stream with zero gaps: packets {o['positions'].tolist()}, flags {o['records']['flags'].tolist()}")
    assert o["count"] >= 3 and not o["records"]["bit_err"].any()
    assert all(m.startswith(MSG.decode()) for m in o["messages"])


def test_five_symbol_packets(pkg, runs):
    for r in (q for q in runs if q["nd"] == 5 and q["snr"] == 25):
        out = r["out"]
        assert out["bits"].shape == (13, 480) and out["eq"].shape == (13, 240) and out["frames"] == 5
        assert not out["records"]["bit_err"].any()
        assert all(m == MSG5.decode() for m in out["messages"])
        assert np.array_equal(r["row"], pkg.abi.reduce_capture_records(out["records"], 5))


def test_bad_arguments_launch_nothing(engine, pkg, runs):
    torch = _torch()
    abi, lib = pkg.abi, engine.lib
    x = torch.from_numpy(runs[0]["x"]).cuda()
    for bad in (torch.zeros(4000, dtype=torch.float32, device="cuda"), torch.zeros((2, 4000), dtype=torch.complex64, device="cuda"),
                torch.zeros(4000, dtype=torch.complex64), torch.zeros(8000, dtype=torch.complex64, device="cuda")[::2],
                [0j] * 100, np.zeros(100, np.complex128)):
        with pytest.raises(ValueError):
            engine.receive_stream(bad)
    for kw in (dict(max_packets=-1), dict(max_packets=2.5), dict(counters=torch.zeros(16, dtype=torch.int64)),
               dict(counters=torch.zeros(15, dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            engine.receive_stream(x, **kw)
    with pytest.raises(abi.OfdmError):
        engine.receive_stream(x, payload="random")
    # the C entry point: OFDM_E_ARG with a text, and outputs filled with a sentinel stay as they were
    pk = torch.full((8, 64), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    words = torch.full((8, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    row = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    opts = abi.make_rx_opts("c")
    stats = abi.make_rx_opts("c")
    stats.word_stats = 1
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(ctx=engine.ctx, x=p(x), n=len(x), opts=C.byref(opts), payload=1, mp=8, pk=p(pk), cnt=p(cnt))
    for change in (dict(n=-1), dict(mp=-1), dict(opts=C.byref(stats)), dict(payload=0), dict(payload=3), dict(cnt=None),
                   dict(pk=None), dict(x=None), dict(opts=None), dict(ctx=None), dict(x=C.c_void_p(x.data_ptr() + 4))):
        a = dict(good, **change)
        rc = lib.ofdm_receive_stream(a["ctx"], a["x"], a["n"], a["opts"], a["payload"], a["mp"], a["pk"], a["cnt"],
                                     p(words), None, p(row), None, None)
        assert rc == -1 and lib.ofdm_last_error(), change
    torch.cuda.synchronize()
    assert (pk == 0x5A).all() and (cnt == -7).all() and (words == 0x5A5A5A5A).all() and (row == -7).all()
    # n < 48 writes d_count = {0, 0} and nothing else
    rc = lib.ofdm_receive_stream(engine.ctx, p(x), 47, C.byref(opts), 1, 8, p(pk), p(cnt), p(words), None, p(row), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and cnt.tolist() == [0, 0] and (pk == 0x5A).all() and (words == 0x5A5A5A5A).all() and (row == -7).all()


def test_timing_ids_and_scratch_accounting(engine, pkg, runs):
    abi = pkg.abi
    x = runs[0]["x"]
    engine.trim()
    assert engine.scratch_bytes() == 0
    engine.timing(True)
    try:
        engine.timing_reset()
        engine.receive_stream(x, want_bits=False)
        got = {k: engine.timing_query(k) for k in (abi.K_STREAM_DETECT, abi.K_STREAM_SELECT, abi.K_STREAM_DECODE)}
    finally:
        engine.timing(False)
    print("kernel ms:", {k: round(v[0], 4) for k, v in got.items()})
    assert all(v[1] == 1 and v[0] > 0 for v in got.values())
    for k in (abi.K_FFT, abi.K_TX, abi.K_RX, abi.K_FRAME):
        assert engine.timing_query(k)[1] == 0
    lc = len(x) - 47
    held = engine.scratch_bytes()
    assert held >= (lc + 31) // 32 * 4 + 8 * ((lc + 300) // 301)       # the bitmap and the front slots
    assert engine.trim() == held and engine.scratch_bytes() == 0
    again = engine.receive_stream(x, want_bits=False)
    assert again["records"].tobytes() == runs[0]["out"]["records"].tobytes()
