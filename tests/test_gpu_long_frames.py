"""Long messages (include/ofdm_mi355x_long.h, Engine.set_long_message): frames of 9..15 data symbols -- the
reference's second, 171-character message (OFDM.c:21) gives 15, a 30,600-sample waveform and 9,394-sample captures --
transmitted, swept and decoded by the kernels of csrc/ofdm_frame_xl.hip.  GPU against the oracle's restatement of
Transmitter() / Receiver() for the same frame count (the oracle's sweep twin stops at 96 characters, so sweep parity
is composed per trial), and the ring sync kernel against the whole-capture one.

The shapes: 9 symbols is the smallest new one (4 detection rounds), 13 has a fifth round only 428 positions long, 15 is
the largest, its matched-filter window 64 samples short of the ring.  Tolerances are those of tests/test_gpu_message.py
and tests/test_gpu_frame.py."""
import numpy as np
import pytest

from conftest import normwise

pytestmark = pytest.mark.gpu

_TEXT = (b"Long frames on the MI355X: the capture no longer fits one wave's share of the LDS, so the sync kernel keeps a "
         b"ring of it and detects a round at a time; fifteen data symbols is the cap!!")
assert len(_TEXT) >= 180


def text(n: int) -> bytes:
    return _TEXT[:n - 1] + b"."                                  # no trailing blank: decoding strips the padding


MSGS = {9: text(97), 13: text(150), 15: text(171)}
SNRS = np.arange(0.0, 31.0, 2.0)


@pytest.fixture
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


def test_limits(eng, engine, pkg):
    for n, d in ((97, 9), (150, 13), (171, 15), (180, 15)) + tuple((k, 9) for k in range(98, 109)):
        assert eng.set_long_message(text(n)) == d
        assert eng.payload_frames("message") == d
    for n in (181, 0):
        with pytest.raises(Exception):
            eng.set_long_message(b"x" * n)
    assert eng.set_long_message(text(171)) == 15
    with pytest.raises(Exception):
        eng.set_message(text(97))                                 # the base entry still stops at 96 characters
    assert eng.payload_frames("message") == 15                    # refused calls leave the message alone
    # a symbol sweep with the message payload is refused while a 15-symbol message is set
    with pytest.raises(Exception, match="symbol"):
        eng.symbol_sweep(pkg.make_cfg(payload="message"), [10.0], 64)
    assert eng.symbol_sweep(pkg.make_cfg(payload="random"), [10.0], 64)[0, 0] == 64
    # a later set_message replaces the long message
    assert eng.set_message(b"x" * 13) == 2 and eng.payload_frames("message") == 2
    assert eng.symbol_sweep(pkg.make_cfg(payload="message"), [10.0], 64)[0, 0] == 64
    # up to 96 characters the long entry is set_message itself: the same sweep counters
    msg = b"IEEE 802.11a on MI355X: a longer message, five symbols!"
    cfg = pkg.make_cfg(payload="message")
    assert eng.set_long_message(msg) == 5
    a, ap = eng.frame_sweep(cfg, [6.0, 12.0, 30.0], 300, want_packet_idx=True)
    assert eng.set_message(msg) == 5
    b, bp = eng.frame_sweep(cfg, [6.0, 12.0, 30.0], 300, want_packet_idx=True)
    assert np.array_equal(a, b) and np.array_equal(ap, bp)


@pytest.mark.parametrize("nd", [9, 13, 15])
def test_transmitter_vs_oracle(eng, oracle, pkg, nd):
    from ofdm_amd import abi
    assert eng.set_long_message(MSGS[nd]) == nd
    w = eng.transmitter("c", "message")
    assert len(w) == abi.wave_len(nd) == {9: 21000, 13: 27400, 15: 30600}[nd]
    ref = oracle.frame_waveform(oracle.message_bits(MSGS[nd]), "c", True, 10)
    assert normwise(w, ref) < 2e-6


def test_noiseless_decode(eng, pkg):
    from ofdm_amd import abi
    msg = MSGS[15]
    eng.set_long_message(msg)
    w = eng.transmitter("c", "message")
    L = abi.capture_len(15)
    assert L == 9394
    for rs in (0, 333, len(w) // 2, len(w) - L):
        o = eng.receiver(w[rs:rs + L], "c", "message")
        assert o["frames"] == 15 and not o["sync_fail"]
        assert o["message"].rstrip(" ") == msg.decode(), (rs, o["message"])


@pytest.mark.parametrize("nd", [9, 15])
def test_receiver_vs_oracle_injected_noise(eng, oracle, pkg, nd):
    from ofdm_amd import abi
    msg = MSGS[nd]
    eng.set_long_message(msg)
    w = eng.transmitter("c", "message")
    L = abi.capture_len(nd)
    bits = oracle.message_bits(msg)
    P = float(np.mean(np.abs(w.astype(np.complex128)) ** 2))
    rng = np.random.default_rng(5)
    for snr, rs in ((30.0, 100), (14.0, 2500), (10.0, 6000), (8.0, 900)):
        cap = w[rs:rs + L].astype(np.complex128)
        cap.real += np.sqrt(P / 10 ** (snr / 10)) * rng.standard_normal(L)
        cap = cap.astype(np.complex64)
        g = eng.receiver(cap, "c", "message")
        o = oracle.receiver_frame(cap, bits, "c")
        assert g["packet_idx"] == o["packet_idx"], snr
        near = np.abs(g["eq"].real) < 1e-3
        near = np.repeat(near | (np.abs(g["eq"].imag) < 1e-3), 2)
        assert not np.any((g["bits"] != o["bits"]) & ~near), snr
        assert g["res"][0] == pytest.approx(o["res"][0], abs=2e-3)


@pytest.mark.parametrize("nd", [9, 13, 15])
def test_ring_kernel_equals_whole_capture(eng, pkg, monkeypatch, nd):
    """frame_ring_xl_kernel (a 2,976-float ring per wave, a detection round's piece at a time, the missing part of the
    matched-filter window generated again) against frame_whole_xl_kernel (OFDM_FRAME_NO_LONG=1: the whole capture
    resident): every counter and every packet_idx."""
    assert eng.set_long_message(MSGS[nd]) == nd
    cfg = pkg.make_cfg(payload="message")
    rg, rp = eng.frame_sweep(cfg, SNRS, 1500, want_packet_idx=True, first_trial=3)
    monkeypatch.setenv("OFDM_FRAME_NO_LONG", "1")
    wh, wp = eng.frame_sweep(cfg, SNRS, 1500, want_packet_idx=True, first_trial=3)
    monkeypatch.delenv("OFDM_FRAME_NO_LONG")
    assert np.array_equal(rp, wp)
    assert np.array_equal(rg, wh)
    assert rg[0, 0] == 1500 and rg[0, 1] == 1500 * nd
    assert np.mean(rp[-4:] > 0) > 0.99                               # high SNR: nearly every trial synchronises
    assert rg[-1, 3] == 0                                            # 30 dB: error-free


@pytest.mark.parametrize("nd", [9, 15])
def test_lazy_rounds_equal_full_evaluation(eng, pkg, monkeypatch, nd):
    """The ring kernel stops detecting after a round (from the second on) whose rounds decide Packet_Selection; every
    counter and packet_idx equals the evaluation of every round (OFDM_FRAME_NO_LAZY=1)."""
    assert eng.set_long_message(MSGS[nd]) == nd
    cfg = pkg.make_cfg(payload="message")
    lz, lp = eng.frame_sweep(cfg, SNRS, 1500, want_packet_idx=True, first_trial=3)
    monkeypatch.setenv("OFDM_FRAME_NO_LAZY", "1")
    fu, fp = eng.frame_sweep(cfg, SNRS, 1500, want_packet_idx=True, first_trial=3)
    monkeypatch.delenv("OFDM_FRAME_NO_LAZY")
    assert np.array_equal(lp, fp)
    assert np.array_equal(lz, fu)
    assert np.mean(lp[-4:] > 0) > 0.99


@pytest.mark.parametrize("nd", [9, 15])
def test_frame_sweep_vs_oracle_per_trial(eng, oracle, pkg, nd):
    """The sweep against the oracle's Receiver(), trial by trial: the capture of (SNR q, trial t) is rebuilt from the
    sweep's own streams, as conftest.off_threshold_pidx_mismatches does."""
    from conftest import off_threshold_pidx_mismatches  # noqa: PLC0415
    from ofdm_amd import abi
    msg = MSGS[nd]
    assert eng.set_long_message(msg) == nd
    cfg = pkg.make_cfg(payload="message")
    snrs = [8.0, 14.0]
    n = 160
    seed = 0x80211A
    g, gp = eng.frame_sweep(cfg, snrs, n, want_packet_idx=True)
    w = eng.transmitter("c", "message")
    L = abi.capture_len(nd)
    bits = oracle.message_bits(msg)
    op = np.zeros_like(gp)
    oerr = np.zeros(len(snrs), np.int64)
    for q, s in enumerate(snrs):
        for t in range(n):
            rs = int(oracle.philox([t, 0, 0, 0x5B000000 | q], [seed, 0])[0] % (len(w) - L))
            cap = eng.transmission_over_air(w, s, seed, t, q)[rs:rs + L]
            o = oracle.receiver_frame(cap, bits, "c")
            op[q, t] = o["packet_idx"]
            oerr[q] += int(np.sum(o["bits"] != bits))
    assert np.all(g[:, 0] == n) and np.all(g[:, 1] == nd * n)             # frames, symbols
    assert np.all(g[:, 2] == 96 * nd * n) and np.all(g[:, 6] == 48 * nd * n)   # bits, EVM terms
    assert np.mean(gp == op) > 0.99
    assert off_threshold_pidx_mismatches(eng, oracle, w, snrs, gp, op, L) == []
    assert np.all(np.abs(g[:, 3] - oerr) <= 96 * nd * np.sum(gp != op, axis=1) + 3)


@pytest.mark.parametrize("n_snr", [35, 64])
@pytest.mark.parametrize("nd", [15, 8])
def test_many_snr_points_per_launch(eng, pkg, monkeypatch, nd, n_snr):
    """The sync kernels' dynamic LDS grows with the SNR points of a launch (up to 64): run_frame_chunk launches none
    above the CU's 160 KiB and falls back (15 symbols: the whole-capture kernel; 8 symbols through set_message: the
    generic kernel at 28..64 points).  The reference's own grid has 35 points."""
    msg = MSGS[15] if nd == 15 else (b"thirty-five SNR points, eight data symbols per frame. " * 2)[:96]
    assert (eng.set_long_message(msg) if nd == 15 else eng.set_message(msg)) == nd
    cfg = pkg.make_cfg(payload="message")
    snrs = np.linspace(6.0, 40.0, n_snr)
    a, ap = eng.frame_sweep(cfg, snrs, 200, want_packet_idx=True)
    monkeypatch.setenv("OFDM_FRAME_NO_LONG", "1")
    b, bp = eng.frame_sweep(cfg, snrs, 200, want_packet_idx=True)
    monkeypatch.delenv("OFDM_FRAME_NO_LONG")
    assert np.array_equal(ap, bp) and np.array_equal(a, b)
    assert np.all(a[:, 0] == 200) and np.mean(ap[-4:] > 0) > 0.99


def test_word_stats_leave_the_counters_alone(eng, pkg):
    assert eng.set_long_message(MSGS[15]) == 15
    cfg = pkg.make_cfg(payload="message")
    snrs = [6.0, 20.0]
    c = eng.frame_sweep(cfg, snrs, 24, word_stats=True)
    c0 = eng.frame_sweep(cfg, snrs, 24)
    assert np.array_equal(c[:, :13], c0[:, :13])
    assert np.all(c[:, 13] < 0) and np.all(c[:, 14] > 0) and np.all(c[:, 15] >= 1)


def test_reference_main_with_the_long_message(pkg, tmp_path):
    from ofdm_amd import sweep
    msg = MSGS[15].decode()
    res = sweep.reference_main(tmp_path, trials=1, message=msg)
    assert res.counters.shape[0] == 35 and np.all(res.counters[:, 1] == 15)
    for name in ("Output_SNR.txt", "Output_EVM_AGC.txt", "Output_EVM_AGC_DB.txt", "Output_BER.txt"):
        assert len(pkg.read_float_array_file(tmp_path / name)) == 35, name     # one value per SNR point
    out = list(sweep.received_messages([30.0], msg))
    assert len(out) == 1 and out[0].startswith("SNR = 30 dB")
    assert out[0].split("\n")[-1].rstrip(" ") == msg
