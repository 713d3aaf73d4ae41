"""GPU tests of the stream receiver's pilot phase tracking (include/ofdm_mi355x_track.h, ofdm_receive_stream_tracked,
Engine.receive_stream(tracking=), csrc/ofdm_stream_track.hip): OFDM_TRACK_NONE byte for byte against
ofdm_receive_stream_timed, phase steps that only the tracked decode survives, parity with the fp64 rule
(stream.track_pilots on the oracle's H and Yf dumps) over D = 1, 2, 3, 4 and 15, the recording's scale, the stream's
end, launch-shape independence, both transform conventions, the argument checks and the link sweep.

Tolerances: eq normwise 1e-4, evm_db_pre 2e-3 dB and post_axis_err 2 are test_gpu_captures.check_against_oracle's; the
tracked chain adds one unit rotation.  Bits are compared except where the fp64 |Re z'| or |Im z'| is below 1e-4 of the
packet's largest |z'| (track_ref.AXIS_BAND; tests/test_track_host.py checks that the fp64 rule alone keeps the parity
streams' share of such subcarriers under 0.2 %).  The phase is compared on symbols whose |P_d| is at least a quarter
of its noise-free value (track_ref.pilot_floor).  PHASE_DEV_MEASURED is the largest |phase_gpu - phase_fp64| over the
parity streams on an MI355X, 7.31e-7 rad (D = 15, 14 dB, -90 kHz; 1.5e-8 to 6.2e-7 on the other streams, 1.0e-7 on the
noise-free phase steps): a few fp32 steps of a phase of up to 3 rad, what an fp32 atan2 of an fp32 four-term sum gives.  The
tests assert 4 x that.  There eq stays within 7.5e-7 normwise of z', evm_db_pre within 2.3e-6 dB (1.5e-4 dB on the phase
steps, whose EVM is near -60 dB), post_axis_err exact, and no subcarrier of the 29,472 compared lies in the excluded band.
Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import detect_ref as ref
import track_ref as tk

pytestmark = pytest.mark.gpu

PHASE_DEV_MEASURED = 7.32e-7    # rad; measured on an MI355X, see the module docstring
EQ_TOL, EVM_TOL_DB, AXIS_TOL = 1e-4, 2e-3, 2


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


def rx(eng, x, tracking, detector="conjugate", timing="ltf", **kw):
    kw = dict(dict(want_bits=True, want_eq=True), **kw)
    return eng.receive_stream(x if _torch().is_tensor(x) else np.ascontiguousarray(x, np.complex64), detector=detector,
                              timing=timing, tracking=tracking, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def host(t):
    return t.cpu().numpy() if _torch().is_tensor(t) else np.asarray(t)


def check_parity(oracle, x, out, truth, worst, packets=None):
    """every record of a tracked run against the fp64 rule at the record's position; returns (compared, excluded)"""
    d = len(truth) // 96
    rec, bits, eq, phase = out["records"], host(out["bits"]), host(out["eq"]), out["phase"]
    compared = excluded = 0
    for k in (range(out["count"]) if packets is None else packets):
        r = tk.fp64_packet(oracle, x, int(rec["packet_pos"][k]), truth)
        t, want = r["t"], r["tracked"]
        z = t["z"].reshape(-1)
        e = float(np.max(np.abs(eq[k] - z)) / max(np.max(np.abs(z)), 1e-30))
        dv = abs(float(rec["evm_db_pre"][k]) - want["evm_db_pre"])
        ax = abs(int(rec["post_axis_err"][k]) - want["axis"])
        band = np.repeat(tk.axis_band(z), 2)
        ok = tk.pilot_floor(t, r["o"]["H"]) & ~t["fallback"]
        ph = float(np.abs(tk.wrap(phase[k].astype(np.float64) - t["phase"]))[ok].max()) if ok.any() else 0.0
        worst.update(eq=max(worst["eq"], e), evm=max(worst["evm"], dv), axis=max(worst["axis"], ax), phase=max(worst["phase"], ph),
                     phase_symbols=worst["phase_symbols"] + int(ok.sum()))
        assert e < EQ_TOL, (k, e)
        assert dv <= EVM_TOL_DB, (k, dv)
        assert ax <= AXIS_TOL, (k, ax)
        assert np.array_equal(bits[k][~band], want["bits"][~band]), k
        assert int(rec["bit_err"][k]) == int((bits[k] != truth).sum()), k
        assert float(rec["ber"][k]) == pytest.approx(int(rec["bit_err"][k]) / (96.0 * d), abs=1e-6)
        assert int(rec["flags"][k]) & 2 == 2 * int(r["o"]["oob"]), k
        assert ph <= 4 * PHASE_DEV_MEASURED, (k, ph)
        compared, excluded = compared + 48 * d, excluded + int(tk.axis_band(z).sum())
    return compared, excluded


def new_worst():
    return dict(eq=0.0, evm=0.0, axis=0, phase=0.0, phase_symbols=0)


# ---------------------------------------------------------------- 1. tracking off is the timed call
def raw_call(eng, pkg, x_dev, nd, sopts, timing, tracking=None, max_packets=64, want_timing=False, want_phase=False):
    """ofdm_receive_stream_timed (tracking None) or ofdm_receive_stream_tracked through ctypes on outputs prefilled with
    a sentinel: every output as host bytes"""
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
    phase = torch.full((max_packets, nd), 7.5, dtype=torch.float32, device="cuda")
    opts = abi.make_rx_opts("c")
    p = lambda t: C.c_void_p(t.data_ptr())
    so = None if sopts is None else C.byref(sopts)
    tail = (abi.PAYLOAD["message"], max_packets, p(pk), p(cnt), p(words), p(eq), p(row), p(metric), p(cross),
            p(tim) if want_timing else None)
    if tracking is None:
        rc = lib.ofdm_receive_stream_timed(eng.ctx, p(x_dev), n, C.byref(opts), so, timing, *tail)
    else:
        rc = lib.ofdm_receive_stream_tracked(eng.ctx, p(x_dev), n, C.byref(opts), so, timing, tracking, *tail,
                                             p(phase) if want_phase else None)
    assert rc == 0, lib.ofdm_last_error()
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().tobytes() for k, t in dict(pk=pk, cnt=cnt, words=words, eq=eq, row=row, metric=metric,
                                                          cross=cross, tim=tim, phase=phase).items()}, [int(v) for v in cnt.cpu()]


def test_tracking_none_is_ofdm_receive_stream_timed(eng, pkg, oracle):
    torch = _torch()
    abi = pkg.abi
    assert eng.set_long_message(" " * 24) == 2
    x, pos = ref.noisy_stream(oracle, 2, 20.0, 40e3, False, 502)
    x_dev = torch.from_numpy(x).cuda()
    ids = (abi.K_STREAM_DETECT, abi.K_STREAM_DETECT_CONJ, abi.K_STREAM_SELECT, abi.K_STREAM_TIMING, abi.K_STREAM_DECODE,
           abi.K_STREAM_DECODE_TRACK)
    query = lambda: {k: eng.timing_query(k)[1] for k in ids}
    eng.timing(True)
    try:
        for det in ("reference", "conjugate"):
            sopts = abi.StreamOpts(abi.DETECTOR[det], 0.75)
            for timing in ("none", "ltf"):
                tc, want_t = abi.TIMING[timing], timing != "none"
                eng.timing_reset()
                base, cnt = raw_call(eng, pkg, x_dev, 2, sopts, tc, want_timing=want_t)
                timed = query()
                eng.timing_reset()
                none, _ = raw_call(eng, pkg, x_dev, 2, sopts, tc, tracking=abi.TRACKING["none"], want_timing=want_t)
                untracked = query()
                eng.timing_reset()
                trk, cnt_t = raw_call(eng, pkg, x_dev, 2, sopts, tc, tracking=abi.TRACKING["pilots"], want_timing=want_t,
                                      want_phase=True)
                tracked = query()
                print(f"detector {det}, timing {timing}: {cnt[0]} packets of {len(pos)} sent; launches {timed} / {untracked} / {tracked}")
                assert cnt[0] == cnt[1] == len(pos) and cnt_t == cnt
                for k in base:
                    assert none[k] == base[k], k                     # d_phase among them: never written
                assert untracked == timed and timed[abi.K_STREAM_DECODE] == 1 and timed[abi.K_STREAM_DECODE_TRACK] == 0
                assert timed[abi.K_STREAM_TIMING] == int(want_t)
                want = dict(timed)
                want[abi.K_STREAM_DECODE], want[abi.K_STREAM_DECODE_TRACK] = 0, 1
                assert tracked == want
                # everything before the decode is untouched by the option
                for k in ("cnt", "metric", "cross", "tim"):
                    assert trk[k] == base[k], k
                dt = abi.stream_packet_dtype()
                a, b = np.frombuffer(trk["pk"], dt)[:cnt[1]], np.frombuffer(base["pk"], dt)[:cnt[1]]
                for name in ("packet_pos", "reserved8", "packet_idx", "flags", "cfo_coarse_hz", "cfo_fine_hz", "reserved"):
                    assert same_bits(a[name], b[name]), name
                ph = np.frombuffer(trk["phase"], np.float32).reshape(64, 2)
                assert (ph[cnt[1]:] == 7.5).all() and (np.abs(ph[:cnt[1]]) < 0.5).all()     # rows past d_count[1] are never written
                assert trk["pk"][64 * cnt[1]:] == base["pk"][64 * cnt[1]:]
    finally:
        eng.timing(False)
    # the Engine's default takes the same route
    a, b = eng.receive_stream(x_dev, want_eq=True), eng.receive_stream(x_dev, want_eq=True, tracking="none")
    assert a["records"].tobytes() == b["records"].tobytes() and a["phase"] is None and b["phase"] is None
    c = eng.receive_stream(x_dev, tracking="pilots", keep_device=True)
    assert c["phase"].shape == (c["count"], 2) and c["phase"].dtype == np.float32 and c["d_phase"].shape[1] == 2
    dv = eng.receive_stream_device(x_dev, tracking="pilots")
    assert dv["d_phase"] is not None and eng.receive_stream_device(x_dev)["d_phase"] is None
    assert np.array_equal(dv["d_phase"][:c["count"]].cpu().numpy(), c["phase"])
    for bad in ("PILOTS", None, 1):
        with pytest.raises(ValueError):
            eng.receive_stream(x_dev, tracking=bad)
        with pytest.raises(ValueError):
            eng.receive_stream_device(x_dev, tracking=bad)


# ---------------------------------------------------------------- 2. phase steps: the test that fails without the feature
def test_phase_steps_are_tracked(eng, oracle):
    d = 15
    assert eng.set_long_message(" " * (12 * d)) == d
    truth = tk.blank_truth(d)
    x, pos = tk.step_stream(oracle, d)
    phi = np.asarray(tk.PHI)
    assert len(phi) == d and np.abs(phi).max() == 1.2 and (np.abs(phi) > np.pi / 4).sum() >= 8
    plain, trk = rx(eng, x, "none"), rx(eng, x, "pilots")
    assert plain["count"] == trk["count"] == len(pos) and np.array_equal(trk["positions"], pos + 16)
    worst = new_worst()
    for k in range(len(pos)):
        per_symbol = (plain["bits"][k] != truth).reshape(d, 96).sum(axis=1)
        dev = np.abs(tk.wrap(trk["phase"][k] - phi))
        print(f"packet {k}: untracked bit errors per symbol {per_symbol.tolist()}, tracked {int(trk['records']['bit_err'][k])}, "
              f"|phase - phi| at most {dev.max():.4f} rad")
        assert (per_symbol[np.abs(phi) > np.pi / 4] > 0).all()
        assert int(trk["records"]["bit_err"][k]) == 0 and np.array_equal(trk["bits"][k], truth)
        assert dev.max() <= 0.02
    check_parity(oracle, x.astype(np.complex128), trk, truth, worst)
    print(f"phase steps against the fp64 rule: {worst}")


# ---------------------------------------------------------------- 3. parity with the fp64 rule
DETECTORS = (("conjugate", "ltf"), ("reference", "none"))


@pytest.fixture(scope="module")
def parity_runs(eng, oracle):
    """The parity streams through both detector settings, untracked and tracked (shared, left unchanged by the tests)"""
    out = []
    for (d, snr, noise, cfo, taps), seed in tk.PARITY_SEEDS.items():
        assert eng.set_long_message(" " * (12 * d)) == d
        x, pos = tk.noisy_stream(oracle, d, snr, noise, cfo, taps, seed)
        for det, timing in DETECTORS:
            out.append(dict(d=d, snr=snr, noise=noise, cfo=cfo, taps=taps, det=det, timing=timing, x=x, pos=pos,
                            none=rx(eng, x, "none", det, timing), trk=rx(eng, x, "pilots", det, timing)))
    _torch().cuda.synchronize()
    return out


def tag(r):
    return (f"D={r['d']:2d} {r['snr']:2d} dB {r['noise']:7s} {r['cfo']:8.0f} Hz {'3 taps' if r['taps'] else '      '} "
            f"{r['det']:9s} timing {r['timing']:4s}")


def test_parity_with_the_fp64_rule(parity_runs, oracle):
    worst, compared, excluded, packets = new_worst(), 0, 0, 0
    for r in parity_runs:
        none, trk = r["none"], r["trk"]
        w = new_worst()
        c, e = check_parity(oracle, r["x"].astype(np.complex128), trk, tk.blank_truth(r["d"]), w)
        print(f"{tag(r)}: {trk['count']} packets of {len(r['pos'])}, bit errors {int(none['records']['bit_err'].sum())} -> "
              f"{int(trk['records']['bit_err'].sum())}, eq {w['eq']:.3g}, evm_db_pre {w['evm']:.3g} dB, post_axis {w['axis']}, phase "
              f"{w['phase']:.3g} rad on {w['phase_symbols']} symbols, {e} of {c} subcarriers excluded")
        for k in ("eq", "evm", "axis", "phase"):
            worst[k] = max(worst[k], w[k])
        worst["phase_symbols"] += w["phase_symbols"]
        compared, excluded, packets = compared + c, excluded + e, packets + trk["count"]
        # what the option leaves alone is byte-equal to the untracked run on the same recording
        assert trk["count"] == none["count"] and trk["found"] == none["found"]
        for name in ("packet_pos", "reserved8", "packet_idx", "flags", "cfo_coarse_hz", "cfo_fine_hz", "reserved"):
            assert same_bits(trk["records"][name], none["records"][name]), name
        if r["timing"] != "none":
            assert np.array_equal(trk["coarse_pos"], none["coarse_pos"]) and same_bits(trk["quality"], none["quality"])
        assert trk["count"] > 0
    print(f"parity: {packets} packets, eq {worst['eq']:.4g}, evm_db_pre {worst['evm']:.4g} dB, post_axis {worst['axis']}, largest phase "
          f"deviation {worst['phase']:.4g} rad on {worst['phase_symbols']} symbols (PHASE_DEV_MEASURED {PHASE_DEV_MEASURED}), "
          f"{excluded} of {compared} subcarriers excluded")
    assert packets >= 60 and worst["phase_symbols"] > 0
    assert excluded <= 0.002 * compared
    assert worst["phase"] <= 4 * PHASE_DEV_MEASURED


# ---------------------------------------------------------------- 4. the recording's scale
def test_scale_of_the_recording(eng, parity_runs):
    torch = _torch()
    r = next(q for q in parity_runs if q["d"] == 15 and q["taps"] is not None and q["det"] == "conjugate")
    assert eng.set_long_message(" " * 180) == 15
    base = r["trk"]
    x = torch.from_numpy(r["x"]).cuda()
    for s in (2.0 ** 12, 2.0 ** -12):
        o = rx(eng, x * s, "pilots", keep_device=True)
        c = o["count"]
        assert c == base["count"] > 0 and np.array_equal(o["positions"], base["positions"])
        same_eq = same_bits(o["eq"].cpu().numpy(), base["eq"])
        print(f"recording x {s:g}: {c} packets, bits and phases compared byte for byte; eq byte-identical too: {same_eq}")
        assert same_bits(o["bits"].cpu().numpy(), base["bits"]) and same_bits(o["phase"], base["phase"])
        assert same_bits(o["d_phase"][:c].cpu().numpy(), base["phase"])
        assert same_bits(o["records"]["bit_err"], base["records"]["bit_err"])


# ---------------------------------------------------------------- 5. the stream's end
def test_stream_end(eng, oracle, parity_runs):
    # the reference detector: its fronts inside a 15-symbol packet all lie at the packet's start, so the cut packet's
    # front is the stream's last (the conjugate detector has a further, unconfirmed one 773 samples into the packet)
    r = next(q for q in parity_runs if q["d"] == 15 and q["snr"] == 14 and q["taps"] is None and q["det"] == "reference")
    d = 15
    assert eng.set_long_message(" " * 180) == d
    truth = tk.blank_truth(d)
    tr, ti = tk.truth_axes(truth)
    full = r["trk"]
    k = full["count"] - 1
    p = int(full["positions"][k])
    # cut inside data symbol 9 of the last packet: frame sample 336 + 80 s is stream sample p + 2 (336 + 80 s) - 20
    n = p + 2 * (336 + 80 * 9) - 20 + 70
    zfirst = min(s for s in range(d + 1) if s == d or p + 2 * (336 + 80 * s) >= n + 20)
    assert zfirst == 10
    x = r["x"][:n]
    none, trk = rx(eng, x, "none", "reference", "none"), rx(eng, x, "pilots", "reference", "none")
    assert trk["count"] == none["count"] == k + 1 and trk["positions"][k] == p
    assert int(trk["records"]["flags"][k]) == 2 | 4 == int(none["records"]["flags"][k])
    assert trk["records"][:k].tobytes() == full["records"][:k].tobytes()
    eq, bits, ph = trk["eq"][k].reshape(d, 48), trk["bits"][k].reshape(d, 96), trk["phase"][k]
    print(f"cut inside symbol 9: phases {ph.round(4).tolist()}, bit errors {int(none['records']['bit_err'][k])} -> "
          f"{int(trk['records']['bit_err'][k])}")
    assert not eq[zfirst:].real.any() and not eq[zfirst:].imag.any() and not ph[zfirst:].any()
    assert np.array_equal(bits[zfirst:], np.tile([1, 0], (d - zfirst, 48)))
    assert np.array_equal(none["bits"][k].reshape(d, 96)[zfirst:], bits[zfirst:])
    # their share of the counts is the payload's own, in the tracked record as in the untracked one
    share_be = int((np.tile([1, 0], 48 * (d - zfirst)) != truth[96 * zfirst:]).sum())
    share_ax = int(tr[48 * zfirst:].sum() + ti[48 * zfirst:].sum())
    for o in (trk, none):
        z = o["eq"][k][:48 * zfirst]
        head_ax = int(((z.real > 0) != tr[:48 * zfirst]).sum() + ((z.imag > 0) != ti[:48 * zfirst]).sum())
        head_be = int((o["bits"][k][:96 * zfirst] != truth[:96 * zfirst]).sum())
        assert int(o["records"]["bit_err"][k]) - head_be == share_be
        assert int(o["records"]["post_axis_err"][k]) - head_ax == share_ax
    # the partly cut symbol, and the whole record, against the fp64 rule on the zero-padded window
    worst = new_worst()
    check_parity(oracle, x.astype(np.complex128), trk, truth, worst, packets=[k])
    print(f"cut packet against the fp64 rule: {worst}")
    # a stream that ends before the long training symbols: S = 0, Z = 0 / 0
    n0 = p + 300                                                      # the front is still confirmed: n > front + 277 = p + 266
    none0, trk0 = rx(eng, r["x"][:n0], "none", "reference", "none"), rx(eng, r["x"][:n0], "pilots", "reference", "none")
    assert trk0["count"] == none0["count"] == k + 1 and trk0["positions"][k] == none0["positions"][k]
    rec = trk0["records"][k]
    print(f"cut before the training symbols: evm_pre_sum {rec['evm_pre_sum']}, evm_db_pre {rec['evm_db_pre']}, evm_db_post "
          f"{rec['evm_db_post']}, bit_err {rec['bit_err']}, phases {trk0['phase'][k].tolist()}")
    assert np.isnan(rec["evm_pre_sum"]) and np.isnan(rec["evm_db_pre"]) and np.isfinite(rec["evm_db_post"])
    assert np.array_equal(trk0["bits"][k], np.tile([1, 0], 48 * d)) and np.array_equal(none0["bits"][k], trk0["bits"][k])
    assert not trk0["phase"][k].any()
    assert int(rec["bit_err"]) == int(none0["records"]["bit_err"][k]) and int(rec["post_axis_err"]) == int(none0["records"]["post_axis_err"][k])


# ---------------------------------------------------------------- 6. launch shapes
def test_max_packets_gives_prefixes(eng, parity_runs):
    r = next(q for q in parity_runs if q["d"] == 15 and q["taps"] is not None and q["det"] == "conjugate")
    assert eng.set_long_message(" " * 180) == 15
    base = r["trk"]
    assert base["found"] > 3
    for m in (1, 3):
        o = rx(eng, r["x"], "pilots", max_packets=m)
        assert o["found"] == base["found"] and o["count"] == m
        assert o["records"].tobytes() == base["records"][:m].tobytes()
        assert same_bits(o["bits"], base["bits"][:m]) and same_bits(o["eq"], base["eq"][:m]) and same_bits(o["phase"], base["phase"][:m])
    o = rx(eng, r["x"], "pilots", max_packets=0, want_bits=False, want_eq=False)
    assert o["found"] == base["found"] and o["count"] == 0 and o["phase"].shape == (0, 15)


def test_looping_waves_and_both_alignments(eng, oracle):
    """One noisy three-packet segment of odd length tiled until the recording holds more packets than 2 x CUs x 8 waves:
    the decode's waves loop, and consecutive repeats start 8 bytes apart modulo 16"""
    torch = _torch()
    d, per = 4, 3
    assert eng.set_long_message(" " * (12 * d)) == d
    seg, pos = tk.noisy_stream(oracle, d, 14.0, "complex", 40e3, None, 6401, packets=per, gap=501)
    # fine timing on: a coarse front may move by a sample with the detection runs' absolute boundaries, which the
    # period is no multiple of; the refined position does not
    seg = seg[:-1] if len(seg) % 2 == 0 else seg
    period = len(seg)
    assert period % 2 == 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    repeats = (2 * cus * 8) // per + 2
    x = torch.from_numpy(seg).cuda().repeat(repeats + 1)               # the closing repeat is not compared: it holds the last front
    o = rx(eng, x, "pilots")
    c = per * repeats
    assert o["found"] == o["count"] == per * (repeats + 1) > 2 * cus * 8
    rec, bits, eq, ph = o["records"][:c], o["bits"][:c].cpu().numpy(), o["eq"][:c].cpu().numpy(), o["phase"][:c]
    assert np.array_equal(rec["packet_pos"].reshape(repeats, per), rec["packet_pos"][:per] + period * np.arange(repeats)[:, None])
    assert {int(v) % 2 for v in rec["packet_pos"][::per]} == {0, 1}
    print(f"{c} packets of {d} data symbols on {cus} CUs, period {period}: bit errors per repeat {int(rec['bit_err'][:per].sum())}")
    for name in rec.dtype.names:
        if name not in ("packet_pos", "packet_idx"):
            assert same_bits(rec[name].reshape(repeats, -1), np.tile(rec[name][:per].reshape(1, -1), (repeats, 1))), name
    assert same_bits(bits.reshape(repeats, -1), np.tile(bits[:per].reshape(1, -1), (repeats, 1)))
    assert same_bits(eq.reshape(repeats, -1), np.tile(eq[:per].reshape(1, -1), (repeats, 1)))
    assert same_bits(ph.reshape(repeats, -1), np.tile(ph[:per].reshape(1, -1), (repeats, 1)))
    # and the first repeat is what the segment alone gives
    alone = rx(eng, seg, "pilots")
    assert alone["count"] == per and same_bits(alone["eq"], eq[:per]) and same_bits(alone["phase"], ph[:per])


# ---------------------------------------------------------------- 7. both transform conventions
@pytest.mark.parametrize("conv,timing,cfo", [("matlab", "ltf-matlab", 200e3), ("c", "ltf", 0.0)])
def test_conventions(eng, oracle, conv, timing, cfo):
    d = 15
    assert eng.set_long_message(" " * (12 * d)) == d
    x, pos = ref.packet_stream(oracle, np.repeat(tk.blank_words(d), 4, axis=0), cfo_hz=cfo, conv=conv)
    o = rx(eng, x.astype(np.complex64), "pilots", timing=timing)
    print(f"{conv} convention, {cfo:g} Hz, timing {timing}: positions {(o['positions'] - pos).tolist()}, bit errors "
          f"{o['records']['bit_err'].tolist()}, largest |phase| {np.abs(o['phase']).max():.4g} rad")
    assert o["count"] == 4 and np.array_equal(o["positions"], pos + 16)
    assert not o["records"]["bit_err"].any() and np.array_equal(o["bits"], np.tile(tk.blank_truth(d), (4, 1)))
    assert np.abs(o["phase"]).max() < 0.05


# ---------------------------------------------------------------- 8. arguments
def test_arguments(eng, pkg, oracle):
    torch = _torch()
    abi, lib = pkg.abi, eng.lib
    assert eng.set_long_message(" " * 24) == 2
    x, pos = ref.noisy_stream(oracle, 2, 20.0, 40e3, False, 502)
    x_dev = torch.from_numpy(x).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    pk = torch.full((64, 64), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    tim = torch.full((64, 16), 0x5A, dtype=torch.uint8, device="cuda")
    ph = torch.full((64, 2), 7.5, dtype=torch.float32, device="cuda")
    opts = abi.make_rx_opts("c")
    ws = abi.make_rx_opts("c")
    ws.word_stats = 1
    conj, bad_det, bad_thr = abi.StreamOpts(1, 0.75), abi.StreamOpts(2, 0.75), abi.StreamOpts(1, 1.5)
    call = lambda timing, tracking, d_phase, o=opts, so=conj, payload=1, mp=64, d_timing=None, n=len(x_dev): lib.ofdm_receive_stream_tracked(
        eng.ctx, p(x_dev), n, C.byref(o), C.byref(so), timing, tracking, payload, mp, p(pk), p(cnt), None, None, None, None, None,
        d_timing, d_phase)
    eng.timing(True)
    try:
        eng.timing_reset()
        refused = [call(0, 2, None), call(0, -1, p(ph)), call(1, 7, p(ph)), call(0, 0, p(ph)),       # the option's own
                   call(3, 1, p(ph)), call(0, 1, p(ph), d_timing=p(tim)), call(1, 1, p(ph), so=bad_det), call(1, 1, p(ph), so=bad_thr),
                   call(1, 1, p(ph), o=ws), call(1, 1, p(ph), payload=0), call(1, 1, p(ph), mp=-1), call(1, 1, p(ph), n=-5)]
        launches = sum(eng.timing_query(k)[1] for k in range(abi.K_STREAM_DECODE_TRACK + 1))
        assert refused == [-1] * len(refused) and lib.ofdm_last_error()
        torch.cuda.synchronize()
        assert launches == 0 and (pk == 0x5A).all() and (cnt == -7).all() and (tim == 0x5A).all() and (ph == 7.5).all()
        # d_phase = NULL with OFDM_TRACK_PILOTS is accepted, and changes nothing else
        assert call(1, 1, None, d_timing=p(tim)) == 0
        torch.cuda.synchronize()
        got = [int(v) for v in cnt.cpu()]
        without = pk.cpu().numpy().tobytes()
        assert got == [len(pos), len(pos)] and (ph == 7.5).all()
        assert call(1, 1, p(ph), d_timing=p(tim)) == 0
        torch.cuda.synchronize()
        assert pk.cpu().numpy().tobytes() == without and not (ph[:got[1]] == 7.5).any() and (ph[got[1]:] == 7.5).all()
        assert eng.timing_query(abi.K_STREAM_DECODE_TRACK)[1] == 2 and eng.timing_query(abi.K_STREAM_DECODE)[1] == 0
    finally:
        eng.timing(False)


# ---------------------------------------------------------------- 9. the link sweep
def test_link_sweep_with_tracking(pkg):
    from ofdm_amd import sweep
    abi = pkg.abi
    words = ref.rand_words(15, 256, 0x7AC)
    snrs = (10.0, 30.0)
    with pkg.Engine(0) as e:
        res = {t: sweep.link_sweep(e, words, 15, 500, snrs, noise="complex", tracking=t) for t in ("none", "pilots")}
    for t, r in res.items():
        for s, row in zip(snrs, r["totals"]):
            print(f"link tracking {t} {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, received "
                  f"{row[abi.S_RECEIVED]}, bit errors {row[abi.S_BIT_ERR]} of {row[abi.S_BITS]}")
    a, b = res["none"]["totals"], res["pilots"]["totals"]
    for col in (abi.S_TRANSMITTED, abi.S_MATCHED, abi.S_RECEIVED, abi.S_BITS):       # missed and false alarms follow
        assert np.array_equal(a[:, col], b[:, col]), col
    assert a[0, abi.S_MATCHED] > 0
    assert b[0, abi.S_BIT_ERR] < a[0, abi.S_BIT_ERR]
