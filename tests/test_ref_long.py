"""Frames of 1 and 3..15 data symbols against the reference's own Receiver() (tests/golden/ref_long_*.npz and
ref_mc_curve_long.json, made by tests/golden/gen_golden.py --only long): the harness that builds such a frame from the
reference's stage functions checks itself (where oracle/_ref is built), and the oracle's restatement is pinned to the
fixtures with the tolerances of tests/test_oracle.py's 2-symbol tests.  The frame sizes: 1 the smallest, 3 and 5 the
long-capture kernel's small end, 8 the benchmarked one, 9 / 13 / 15 the ring kernel's first, short-fifth-round and
largest shapes.  tests/test_gpu_ref_long.py runs the kernels against the same fixtures."""
import sys

import numpy as np
import pytest

import ref_long
from conftest import GOLDEN, normwise


@pytest.fixture
def ref_msg(reflib):
    """the reference harness, put back on its compiled-in message afterwards; like the `reflib` fixture it skips where
    the harness is not built: here, where oracle/_ref holds a library from before ref_set_message that could not be
    built again (build() does that wherever the reference's source is)"""
    if not reflib.has_set_message:
        pytest.skip("oracle/_ref holds a build of the harness without ref_set_message (needs the reference source)")
    yield reflib
    reflib.set_message(reflib.DEFAULT_MESSAGE)


def _gen():
    sys.path.insert(0, str(GOLDEN))
    import gen_golden  # noqa: PLC0415
    return gen_golden


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------- the harness (needs oracle/_ref)
def test_stage_built_default_frame_is_transmitters(ref_msg):
    R = ref_msg
    tw = ref_long.load_golden("tx_waveform.npz")
    main = R.transmitter_waveform()                         # Transmitter()'s own output, kept aside by the harness
    assert _same_bits(main, tw["waveform"])
    assert R.set_message(R.DEFAULT_MESSAGE) == 9800
    assert _same_bits(R.waveform(), main)                   # stage-built == Transmitter(), bit for bit
    g = R.globals()
    assert np.array_equal(g["bits"], tw["bits"]) and _same_bits(g["payload_mod"], tw["payload_mod"])
    assert _same_bits(g["ltf_freq"], tw["ltf_freq"]) and g["dims"].tolist() == tw["dims"].tolist()


def test_every_entry_follows_set_message(ref_msg):
    R = ref_msg
    before = R.mc_trials(12.0, 20, 5)[1]
    for nd in (15, 1):
        t = ref_long.tx(nd)
        n = R.set_message(t["msg"])
        assert n == len(t["wave"]) == R.lib.ref_init() == 10 * (2 * (320 + 80 * nd) + 20)
        assert R.dims().tolist() == [nd, 320 + 80 * nd, n, 0] == t["dims"].tolist()
        assert _same_bits(R.waveform(), t["wave"])
        g = R.globals()
        assert np.array_equal(g["bits"], t["bits"]) and _same_bits(g["payload_mod"], t["payload_mod"])
        # the trial loops run on the new frame with the new length (Res[2] is a multiple of 1 / (96 nd))
        acc = R.mc_trials(30.0, 3, 5)[1]
        assert acc[2] == 0 and np.isfinite(acc[0]) and acc[0] / 3 < -20
    assert R.set_message(R.DEFAULT_MESSAGE) == 9800
    assert R.globals()["bits"].shape == (192,)
    assert np.array_equal(R.mc_trials(12.0, 20, 5)[1], before)          # and the default is back, draw for draw


def test_fixture_cases_regenerate(ref_msg, oracle):
    """one stages case per ring size and ten bulk captures, from the generator's own functions"""
    G = _gen()
    R = ref_msg
    for nd, case in ((15, 5), (9, 7)):
        t, g = ref_long.tx(nd), ref_long.stages(nd)
        assert G.long_message(nd) == t["msg"]
        R.set_message(t["msg"])
        w = R.waveform()
        P = float(np.mean(np.abs(w.astype(np.complex128)) ** 2))
        c = G.stages_case(R, oracle, w, P, nd, case, float(g["snr"][case]), int(g["rs"][case]), int(g["seed"][case]))
        assert c is not None and set(c) == set(g)
        for k, v in c.items():
            assert np.array_equal(np.asarray(v), g[k][case], equal_nan=v.dtype.kind == "f"), (nd, k)
        assert int(G.stage_starts(len(w), ref_long.cap_len(nd))[case]) == int(g["rs"][case])
    nd = 8
    t, b = ref_long.tx(nd), ref_long.bulk(nd)
    R.set_message(t["msg"])
    w = R.waveform()
    for k in range(10):
        row = G.bulk_capture_row(R, oracle, w, t["bits"], nd, k, int(b["rs"][k]), float(b["sigma"][k]))
        assert row[:5] == (int(b["case"][k]), int(b["packet_idx"][k]), int(b["bit_err"][k]), int(b["near"][k]),
                           bool(b["on_threshold"][k])), k
    # the test-side rule (tests/ref_long.capture) builds the generator's captures
    assert _same_bits(ref_long.bulk_captures(oracle, nd, 2)[1],
                      G.long_capture(oracle, w, nd, int(b["case"][1]), int(b["rs"][1]), float(b["sigma"][1]), G.BULK_KEY))


# ---------------------------------------------------------------- the fixtures themselves (no reference needed)
def test_fixture_shapes_and_coverage():
    assert ref_long.FRAMES == tuple(int(v) for v in ref_long._file("ref_long_tx.npz")["frames"])
    assert ref_long.tx(15)["msg"].startswith(b"The Supreme Lord") and len(ref_long.tx(15)["msg"]) == 171
    for nd, chars in zip(ref_long.FRAMES, (12, 30, 55, 96, 97, 150, 171)):
        t, g = ref_long.tx(nd), ref_long.stages(nd)
        assert len(t["msg"]) == chars and len(t["bits"]) == 96 * nd and len(t["wave"]) == 10 * (2 * (320 + 80 * nd) + 20)
        L = ref_long.cap_len(nd)
        assert g["snr"].tolist() == [100, 30, 20, 14, 12, 10, 8, 6]
        assert {0, len(t["wave"]) - L - 1, (len(t["wave"]) - L) // 2} <= set(g["rs"].tolist())
        assert not g["ints"][:, 3].any()                                 # no late frame read past the buffer
        clean = (g["packet_idx"] != 0) & (g["res"][:, 2] == 0)
        assert (g["packet_idx"] == 0).any() and clean.any(), nd          # both outcomes at every size
    for nd in ref_long.BULK_FRAMES:
        b = ref_long.bulk(nd)
        assert len(b["rs"]) == 1000 and b["on_threshold"].mean() <= 0.005
        assert set(b["snr"].tolist()) == {6, 8, 10, 12, 16, 25}
        assert 100 <= (b["packet_idx"] == 0).sum() <= 300                # the 17-20 % of sync failures
    for nd in (8, 15):
        c = ref_long.curve(nd)
        assert sorted(c) == [6, 8, 10, 12, 14, 20] and all(r["trials"] == 20000 for r in c.values())


# ---------------------------------------------------------------- the oracle against the reference
@pytest.mark.parametrize("nd", ref_long.FRAMES)
def test_oracle_waveform_vs_reference(oracle, nd):
    t = ref_long.tx(nd)
    bits = oracle.message_bits(t["msg"])
    assert np.array_equal(bits, t["bits"])
    e = normwise(oracle.frame_waveform(bits, "c", True, 10), t["wave"])
    print(f"D={nd}: waveform normwise {e:.3g}")
    assert len(t["wave"]) == 10 * (2 * (320 + 80 * nd) + 20)
    assert e < 1e-6
    mod = np.concatenate([np.asarray(_qpsk(bits[96 * d:96 * d + 96])) for d in range(nd)])
    assert normwise(mod, t["payload_mod"]) < 1e-6


def _qpsk(b):
    """QPSK_Modulator's map (OFDM.c:423-430): 00 (1+j), 01 (-1+j), 10 (-1-j), 11 (1-j), over sqrt 2"""
    b0, b1 = b[0::2], b[1::2]
    return (np.where(b0 == b1, 1.0, -1.0) + 1j * np.where(b0 == 1, -1.0, 1.0)) / np.sqrt(2)


@pytest.mark.parametrize("nd", ref_long.FRAMES)
def test_oracle_receiver_stages_vs_reference(oracle, nd):
    """test_receiver_stages_vs_reference's tolerances at every frame size"""
    t, g = ref_long.tx(nd), ref_long.stages(nd)
    caps = ref_long.stage_captures(oracle, nd)
    worst = dict(H=0.0, eq=0.0, evm=0.0)
    for k, cap in enumerate(caps):
        o = oracle.receiver_frame(cap.astype(np.complex128), t["bits"], "c", dumps=True)
        assert o["packet_idx"] == int(g["packet_idx"][k]), k
        assert o["oob"] == 0
        ref_np = g["nopilot"][k]
        eh, ee = normwise(o["H"], g["H"][k]), normwise(o["nopilot"], ref_np)
        assert eh < 1e-4 and ee < 1e-4, (k, eh, ee)
        diff = (o["bits"] != g["bits"][k]).reshape(-1, 2).any(axis=1)
        assert not np.any(np.repeat(diff, 2) & ~ref_long.near_pairs(ref_np)), k
        np.testing.assert_allclose(o["res"][0], g["res"][k][0], atol=2e-3)
        assert o["res"][2] == pytest.approx(float(g["res"][k][2]), abs=1e-6)
        worst = dict(H=max(worst["H"], eh), eq=max(worst["eq"], ee),
                     evm=max(worst["evm"], abs(o["res"][0] - float(g["res"][k][0]))))
    print(f"D={nd}: worst H {worst['H']:.3g}, equalised carriers {worst['eq']:.3g}, EVM_dB {worst['evm']:.3g}")


@pytest.mark.parametrize("nd", ref_long.BULK_FRAMES)
def test_oracle_bulk_vs_reference(oracle, nd):
    t, b = ref_long.tx(nd), ref_long.bulk(nd)
    caps = ref_long.bulk_captures(oracle, nd)
    checked = 0
    for k, cap in enumerate(caps):
        o = oracle.receiver_frame(cap.astype(np.complex128), t["bits"], "c")
        assert o["oob"] == 0, k
        if b["on_threshold"][k]:
            continue
        checked += 1
        assert o["packet_idx"] == int(b["packet_idx"][k]), k
        assert o["sync_fail"] == int(b["packet_idx"][k] == 0), k
        assert abs(int(np.sum(o["bits"] != t["bits"])) - int(b["bit_err"][k])) <= int(b["near"][k]), k
    assert checked >= 995


def test_oracle_frame_sweep_vs_reference_curve_8_symbols(oracle):
    """test_frame_mode_mc_matches_reference_curve's bound on the 8-symbol curve"""
    curve = ref_long.curve(8)
    snrs = [8.0, 10.0, 14.0]
    try:
        assert oracle.set_message(ref_long.tx(8)["msg"]) == 8
        cnt = oracle.frame_sweep(oracle.cfg(payload="message"), snrs, 0, 600, "c")
    finally:
        oracle.set_message(b"Hey! I am Vivaswan")
    for s, c in zip(snrs, cnt):
        assert c[0] == 600 and c[2] == 600 * 768
        ber = c[3] / c[2]
        ref = curve[s]["ber"]
        # frame-clustered errors: sd of mean per-trial BER ~ 0.25/sqrt(n) at these SNRs
        sd = 0.5 * np.sqrt(ref * (1 - ref) / 600) + 0.25 / np.sqrt(600) * (ref > 0.01) + 1e-3
        print(f"D=8 {s:4.1f} dB: oracle BER {ber:.4e}, reference {ref:.4e}, bound {5 * sd:.3e}")
        assert abs(ber - ref) < 5 * sd, (s, ber, ref)
