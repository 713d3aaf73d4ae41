"""GPU parity of the receivers on captures and streams that end before their packet does (OFDM_CAPTURE_OOB), against
the oracle in fp64 on the same samples, with the tolerances of test_gpu_captures.check_against_oracle unchanged (bits,
bit_err and flags equal, eq normwise < 1e-4, evm_db_pre within 2e-3 dB, axis errors within 2) and no packet_idx
mismatch allowed: tests/test_oob_host.py generates the inputs and proves them off Packet_Selection's threshold.

A data symbol wholly past the end reaches the demapper as 64 exact zeros.  The reference decides "-" on both axes for
a zero (Z > 0 fails), so its bits are (1, 0) throughout and its error counts depend on the payload alone; the kernels'
records must say the same as their bits (a to e, g).  With the long training symbols themselves past the end S = 0,
Z = 0 / 0 is NaN, which also decides "-", and the pre-slicer EVM is NaN (f).  h: a recording scaled by 2^-12 or 2^12
decodes the same.  i: matlab_slicer and float_taps change nothing in the GPU receivers.

Each test prints its worst figures before it asserts.  Measured on an MI355X (parity table): no
packet_idx mismatch; bits, bit_err, flags and post_axis_err equal to the oracle's everywhere; worst eq 2.2e-6 normwise
(a, L = 900), worst evm_db_pre 9.1e-6 dB (c); f: NaN eq and pre-slicer EVM, bit_err 100 of 192 and 269 of 480 as the
oracle's; h: every record field, eq and both CFO estimates bit-identical to the unscaled run at 2^-12 and 2^12 (worst
CFO deviation 0 Hz).  Before the records followed the reference's rule for a zero symbol, a (all lengths but 900, which
has no zero symbol), b, c, d, e, f and g failed: bit_err 82, 90, 96, 90 for the oracle's 100, 100, 98, 92 in a; 83 for
89, 134 for 152, 342 for 412 in b; ofdm_receiver's BER differed from its own bits on all 16 captures of a and b with a
zero symbol."""
import contextlib

import numpy as np
import pytest

from conftest import normwise
from test_gpu_captures import (CFO_TOL_HZ, check_against_oracle, impaired, impaired_gpu, msg_bits,  # noqa: F401
                               oracle_axis_errors, records_np, wave)
from test_oob_host import (MIXED_CUT_SEEDS, MIXED_LEN, MIXED_WHOLE_SEEDS, MSG, MSGS, SYNC_FAIL_LENGTHS, SYNC_FAIL_ZERO,
                           SYNCED, mixed_cut_capture, mixed_whole_capture, stream_cases, sync_fail_capture,
                           synced_capture, waves, zero_symbols)  # noqa: F401
from test_stream_host import base_stream

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


@contextlib.contextmanager
def message(engine, nd):
    """the engine decoding against the nd-symbol message of test_oob_host.MSGS; the default message afterwards"""
    try:
        assert (engine.set_long_message(MSGS[nd]) if nd > 8 else engine.set_message(MSGS[nd])) == nd
        yield
    finally:
        engine.set_message(MSG)


def self_consistent(pkg, rec, bits, eq, truth, row=None):
    """d: a record says what its bits and subcarriers say -- bit_err is the bits' distance from the payload,
    post_axis_err the axis errors recounted from eq by the reference's "> 0" rule (zero and NaN decide "-"; the truth
    has re > 0 iff b0 == b1 and im > 0 iff b0 == 0) -- and the counters row is the reduction of the records"""
    nd = len(truth) // 96
    b0, b1 = truth[0::2], truth[1::2]
    for k in range(len(rec)):
        assert int(rec["bit_err"][k]) == int(np.sum(bits[k] != truth)), k
        with np.errstate(invalid="ignore"):
            ax = int(np.sum((eq[k].real > 0) != (b0 == b1)) + np.sum((eq[k].imag > 0) != (b0 == 0)))
        assert int(rec["post_axis_err"][k]) == ax, (k, int(rec["post_axis_err"][k]), ax)
        assert abs(float(rec["ber"][k]) - int(rec["bit_err"][k]) / (96 * nd)) <= 1e-6, k
    if row is not None:
        assert np.array_equal(np.asarray(row), pkg.abi.reduce_capture_records(rec, nd))


def check_receiver(engine, cap, L, rec_k, eq_k, o, truth):
    """g: ofdm_receiver on the same capture -- its BER is its bits' distance from the payload, both are the oracle's,
    and it agrees with the batched receiver's record (test_gpu_captures.check_against_receiver's tolerances)"""
    nd = len(truth) // 96
    r = engine.receiver(cap, opts=dict(cap_len=L))
    assert round(float(r["res"][2]) * 96 * nd) == int(np.sum(r["bits"] != truth))
    assert np.array_equal(r["bits"], o["bits"]) and float(r["res"][2]) == pytest.approx(float(o["res"][2]), abs=1e-6)
    assert (r["packet_idx"], r["sync_fail"], r["oob"]) == (o["packet_idx"], o["sync_fail"], o["oob"])
    assert int(rec_k["packet_idx"]) == r["packet_idx"] and int(rec_k["flags"]) == (r["sync_fail"] | (r["oob"] << 1))
    assert normwise(eq_k, r["eq"]) < 1e-4
    assert float(rec_k["ber"]) == pytest.approx(float(r["res"][2]), abs=1e-6)
    assert float(rec_k["evm_db_pre"]) == pytest.approx(float(r["res"][0]), abs=2e-3)
    want = oracle_axis_errors(o, nd)
    got = 0 if not np.isfinite(r["res"][1]) else int(round(10 ** (float(r["res"][1]) / 10) * 48 * nd / 2))
    assert abs(got - want) <= 2


def run_captures(engine, caps, L, **kw):
    """receive_captures on a host batch of L-sample captures with every output and a counters row"""
    row = engine.new_counters(1)[0]
    out = engine.receive_captures(np.ascontiguousarray(caps, np.complex64), want_bits=True, want_eq=True, counters=row,
                                  opts=dict(cap_len=L), **kw)
    return out, row.cpu().numpy().copy()


# ---------------------------------------------------------------- a (+ d, g). no sync, past the end
@pytest.mark.parametrize("L", SYNC_FAIL_LENGTHS)
def test_sync_fail_past_the_end(engine, pkg, oracle, waves, L):  # noqa: F811
    w, truth = waves[2]["wave"], waves[2]["truth"]
    cap = sync_fail_capture(w, L)
    o = oracle.receiver_frame(cap.astype(np.complex128), truth, "c", dumps=True, cap_len=L)
    out, row = run_captures(engine, cap[None, :], L)
    rec = out["records"]
    print(f"L = {L}: zero symbols {SYNC_FAIL_ZERO[L]}, GPU bit_err {int(rec['bit_err'][0])}, oracle {int(np.sum(o['bits'] != truth))}")
    assert int(rec["packet_idx"][0]) == 0 and int(rec["flags"][0]) == 3
    for d in SYNC_FAIL_ZERO[L]:
        assert np.array_equal(out["bits"][0][96 * d:96 * d + 96], np.tile([1, 0], 48))
    same = check_against_oracle(rec, out["bits"], out["eq"], [o], cap[None, :], truth, 0)
    assert same == [0]
    self_consistent(pkg, rec, out["bits"], out["eq"], truth, row)
    check_receiver(engine, cap, L, rec[0], out["eq"][0], o, truth)
    # the kernel variant without outputs writes the same record
    bare = engine.receive_captures(cap[None, :], want_bits=False, opts=dict(cap_len=L))
    assert bare["records"].tobytes() == rec.tobytes()


# ---------------------------------------------------------------- b (+ d, g). synchronised, past the end
@pytest.mark.parametrize("nd", [s[0] for s in SYNCED])
def test_synced_past_the_end(engine, pkg, oracle, waves, nd):  # noqa: F811
    _, K, seeds, zero = next(s for s in SYNCED if s[0] == nd)
    w, truth = waves[nd]["wave"], waves[nd]["truth"]
    caps = np.stack([synced_capture(w, K, seed) for seed in seeds])
    L = caps.shape[1]
    ora = [oracle.receiver_frame(c.astype(np.complex128), truth, "c", dumps=True, cap_len=L) for c in caps]
    with message(engine, nd):
        out, row = run_captures(engine, caps, L)
        rec = out["records"]
        print(f"D = {nd}: packet_idx {rec['packet_idx'].tolist()}, zero symbols {zero}, GPU bit_err {rec['bit_err'].tolist()}, "
              f"oracle {[int(np.sum(o['bits'] != truth)) for o in ora]}")
        assert (rec["flags"] == 2).all()
        for k in range(len(caps)):
            assert zero_symbols(int(rec["packet_idx"][k]), L, nd) == zero
            for d in zero:
                assert np.array_equal(out["bits"][k][96 * d:96 * d + 96], np.tile([1, 0], 48)), (k, d)
                assert not out["eq"][k][48 * d:48 * d + 48].any()
        same = check_against_oracle(rec, out["bits"], out["eq"], ora, caps, truth, 0)
        assert same == list(range(len(caps)))
        self_consistent(pkg, rec, out["bits"], out["eq"], truth, row)
        for k in range(len(caps)):
            check_receiver(engine, caps[k], L, rec[k], out["eq"][k], ora[k], truth)
        bare = engine.receive_captures(caps, want_bits=False, opts=dict(cap_len=L))
        assert bare["records"].tobytes() == rec.tobytes()


# ---------------------------------------------------------------- c (+ d). a mixed batch
def test_mixed_batch(engine, pkg, oracle, waves):  # noqa: F811
    torch = _torch()
    w, truth = waves[2]["wave"], waves[2]["truth"]
    L = MIXED_LEN
    caps, cut = [], []
    for k in range(33):                                                  # cut, whole, cut, ...
        cut.append(k % 2 == 0)
        caps.append(mixed_cut_capture(w, MIXED_CUT_SEEDS[k // 2]) if cut[-1] else mixed_whole_capture(w, MIXED_WHOLE_SEEDS[k // 2]))
    caps, cut = np.stack(caps), np.array(cut)
    ora = [oracle.receiver_frame(c.astype(np.complex128), truth, "c", dumps=True, cap_len=L) for c in caps]
    assert [int(o["oob"]) for o in ora] == cut.astype(int).tolist()
    opts = dict(cap_len=L)
    single = [engine.receive_captures(caps[k:k + 1], want_bits=True, want_eq=True, opts=opts) for k in range(33)]
    one = np.concatenate([s["records"] for s in single])
    assert np.array_equal(one["flags"], 2 * cut.astype(np.int32))
    for n in (1, 7, 8, 9, 33):
        buf = torch.zeros((n, L + 1), dtype=torch.complex64, device="cuda")     # odd pitch: odd rows 8 bytes off a 16-byte line
        buf[:, :L] = torch.from_numpy(caps[:n]).cuda()
        view = buf[:, :L]
        assert n == 1 or view.stride() == (L + 1, 1)
        row = engine.new_counters(1)[0]
        full = engine.receive_captures(view, want_bits=True, want_eq=True, counters=row, opts=opts)
        bare = engine.receive_captures(view, want_bits=False, opts=opts)
        rec, bits, eq = records_np(full), full["bits"].cpu().numpy(), full["eq"].cpu().numpy()
        assert rec.tobytes() == one[:n].tobytes(), n
        assert records_np(bare).tobytes() == rec.tobytes(), n
        for k in range(n):
            assert np.array_equal(bits[k], single[k]["bits"][0]) and np.array_equal(eq[k].view(np.float32), single[k]["eq"][0].view(np.float32)), (n, k)
        # the whole captures' records do not depend on the cut ones beside them
        keep = np.nonzero(~cut[:n])[0]
        if len(keep):
            alone = engine.receive_captures(view[torch.from_numpy(keep).cuda()], want_bits=True, want_eq=True, opts=opts)
            assert records_np(alone).tobytes() == rec[keep].tobytes(), n
            assert torch.equal(alone["bits"], full["bits"][torch.from_numpy(keep).cuda()])
        self_consistent(pkg, rec, bits, eq, truth, row.cpu().numpy())
        if n == 33:
            same = check_against_oracle(rec, bits, eq, ora, caps, truth, 0)
            assert same == list(range(33))
            assert row.cpu().numpy()[pkg.abi.C_OOB] == 17


# ---------------------------------------------------------------- e, f (+ d). the stream's cut-off last packet
def _run_stream(engine, x):
    row = engine.new_counters(1)[0]
    out = engine.receive_stream(np.ascontiguousarray(x, np.complex64), want_bits=True, want_eq=True, counters=row)
    return out, row.cpu().numpy().copy()


@pytest.fixture(scope="module")
def cut_streams(oracle, waves):  # noqa: F811
    return stream_cases(oracle, waves)


@pytest.mark.parametrize("case", range(5))
def test_stream_cut_inside_its_last_packet(engine, pkg, oracle, waves, cut_streams, case):  # noqa: F811
    abi = pkg.abi
    c = cut_streams[case]
    nd, x, pos = c["nd"], c["cut"], c["pos"]
    truth = waves[nd]["truth"]
    with message(engine, nd):
        full, _ = _run_stream(engine, c["full"])
        out, row = _run_stream(engine, x)
    rec = out["records"]
    print(f"{c['name']}: positions {out['positions'].tolist()} (fp64 rule {pos.tolist()}), flags {rec['flags'].tolist()}, "
          f"last record bit_err {int(rec['bit_err'][-1])}, evm_db_pre {float(rec['evm_db_pre'][-1])}")
    assert np.array_equal(full["positions"], pos) and np.array_equal(out["positions"], pos)       # no mismatch
    assert rec["flags"].tolist() == [0, 0, 2 | 4]
    assert rec[:2].tobytes() == full["records"][:2].tobytes()
    assert np.array_equal(out["bits"][:2], full["bits"][:2])
    assert np.array_equal(out["eq"][:2].view(np.float32), full["eq"][:2].view(np.float32))
    # the last record against orc_decode_at on the window at the stream's position
    p = int(pos[-1])
    win = x[p - 411:]
    o = oracle.decode_at(win.astype(np.complex128), truth, 411, "c", dumps=True, cap_len=len(win))
    assert zero_symbols(411, len(win), nd) == c["zero"]
    for d in c["zero"]:
        assert np.array_equal(out["bits"][2][96 * d:96 * d + 96], np.tile([1, 0], 48)), d
    last = rec[2:3].copy()
    last["packet_idx"] = 411
    last["flags"] &= 3
    if not c["no_ltf"]:
        same = check_against_oracle(last, out["bits"][2:3], out["eq"][2:3], [o], win[None, :], truth, 0)
        assert same == [0]
        assert abs(float(last["cfo_coarse_hz"][0]) - float(o["cfo"][0])) <= CFO_TOL_HZ
        assert abs(float(last["cfo_fine_hz"][0]) - float(o["cfo"][1])) <= CFO_TOL_HZ
    else:
        # f: S = 0 in every bin: NaN subcarriers, (1, 0) throughout, NaN pre-slicer EVM, a finite post-slicer one
        assert np.isnan(o["nopilot"].view(np.float64)).all() and np.isnan(o["res"][0]) and np.isfinite(o["res"][1])
        assert np.array_equal(out["bits"][2], o["bits"]) and np.array_equal(o["bits"], np.tile([1, 0], 48 * nd))
        assert int(last["bit_err"][0]) == int(np.sum(o["bits"] != truth))
        assert int(last["flags"][0]) == 2
        assert np.isnan(out["eq"][2].view(np.float32)).all()
        assert not np.isfinite(last["evm_pre_sum"][0]) and not np.isfinite(last["evm_db_pre"][0])
        assert abs(int(last["post_axis_err"][0]) - oracle_axis_errors(o, nd)) <= 2
        assert np.isfinite(last["evm_db_post"][0]) and abs(float(last["evm_db_post"][0]) - float(o["res"][1])) <= 2e-3
        # the non-finite terms are left out of the counters row: its EVM sums are the first two records'
        two = abi.reduce_capture_records(rec[:2], nd)
        assert row[abi.C_EVM_PRE_Q] == two[abi.C_EVM_PRE_Q] and row[abi.C_EVMDB_PRE_Q] == two[abi.C_EVMDB_PRE_Q]
        assert row[abi.C_FRAMES] == 3 and row[abi.C_EVMDB_POST_FINITE] == two[abi.C_EVMDB_POST_FINITE] + 1
    self_consistent(pkg, rec, out["bits"], out["eq"], truth, row)
    # the kernel variant without outputs writes the same records
    with message(engine, nd):
        bare = engine.receive_stream(np.ascontiguousarray(x, np.complex64), want_bits=False)
    assert bare["records"].tobytes() == rec.tobytes()


# ---------------------------------------------------------------- h. power-of-two scale
def _close_records(rec, ref, eq, ref_eq, worst):
    for name in ("packet_idx", "flags", "bit_err", "post_axis_err"):
        assert np.array_equal(rec[name], ref[name]), name
    assert np.array_equal(rec["ber"], ref["ber"])
    for k in range(len(rec)):
        worst["eq"] = max(worst["eq"], normwise(eq[k], ref_eq[k]))
        worst["evm"] = max(worst["evm"], abs(float(rec["evm_db_pre"][k]) - float(ref["evm_db_pre"][k])))
        worst["cfo"] = max(worst["cfo"], abs(float(rec["cfo_coarse_hz"][k]) - float(ref["cfo_coarse_hz"][k])),
                           abs(float(rec["cfo_fine_hz"][k]) - float(ref["cfo_fine_hz"][k])))
    assert np.array_equal(np.isfinite(rec["evm_db_post"]), np.isfinite(ref["evm_db_post"]))
    fin = np.isfinite(ref["evm_db_post"])
    assert np.array_equal(rec["evm_db_post"][fin], ref["evm_db_post"][fin])           # a function of post_axis_err alone


@pytest.mark.parametrize("exp", [-12, 12])
def test_power_of_two_scale(engine, oracle, impaired, impaired_gpu, wave, exp):  # noqa: F811
    g = np.float32(2.0 ** exp)
    worst = dict(eq=0.0, evm=0.0, cfo=0.0)
    out = engine.receive_captures(impaired["caps"] * g, want_bits=True, want_eq=True)
    ref = impaired_gpu["out"]
    assert np.array_equal(out["bits"], ref["bits"].cpu().numpy())
    _close_records(out["records"], impaired_gpu["rec"], out["eq"], ref["eq"].cpu().numpy(), worst)
    x = base_stream(wave, 14.0, 40e3, 1000 * 2 + 10 * 14 + 1)                          # a base stream of test_gpu_stream
    s0 = engine.receive_stream(x, want_bits=True, want_eq=True)
    s1 = engine.receive_stream(x * g, want_bits=True, want_eq=True)
    assert s0["count"] == s1["count"] == 13 and np.array_equal(s0["positions"], s1["positions"])
    assert np.array_equal(s0["bits"], s1["bits"])
    _close_records(s1["records"], s0["records"], s1["eq"], s0["eq"], worst)
    print(f"scale 2^{exp}: worst eq {worst['eq']:.3g}, evm_db_pre {worst['evm']:.3g} dB, CFO {worst['cfo']:.6g} Hz "
          f"against the unscaled run")
    assert worst["eq"] < 1e-4 and worst["evm"] <= 2e-3 and worst["cfo"] <= CFO_TOL_HZ


# ---------------------------------------------------------------- i. options
def test_slicer_and_taps_options_change_nothing(engine, impaired, impaired_gpu, wave):  # noqa: F811
    ref = impaired_gpu["rec"]
    x = base_stream(wave, 14.0, 40e3, 1000 * 2 + 10 * 14 + 1)
    s0 = engine.receive_stream(x, want_bits=True, want_eq=True)
    r0 = [engine.receiver(impaired["caps"][k]) for k in range(0, 96, 12)]
    for matlab in (0, 1):
        for taps in (0, 1):
            opts = dict(matlab_slicer=matlab, float_taps=taps)
            out = engine.receive_captures(impaired["caps"], want_bits=True, want_eq=True, opts=opts)
            assert out["records"].tobytes() == ref.tobytes(), opts
            assert np.array_equal(out["bits"], impaired_gpu["out"]["bits"].cpu().numpy())
            assert np.array_equal(out["eq"].view(np.float32), impaired_gpu["out"]["eq"].cpu().numpy().view(np.float32))
            s = engine.receive_stream(x, want_bits=True, want_eq=True, opts=opts)
            assert s["records"].tobytes() == s0["records"].tobytes() and np.array_equal(s["bits"], s0["bits"]), opts
            assert np.array_equal(s["eq"].view(np.float32), s0["eq"].view(np.float32))
            for j, k in enumerate(range(0, 96, 12)):
                r = engine.receiver(impaired["caps"][k], opts=opts)
                assert r["res"].tobytes() == r0[j]["res"].tobytes() and r["packet_idx"] == r0[j]["packet_idx"], (opts, k)
                assert np.array_equal(r["bits"], r0[j]["bits"]) and r["eq"].tobytes() == r0[j]["eq"].tobytes(), (opts, k)
