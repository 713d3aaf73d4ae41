"""Receivers past the capture's end, the checks that need no GPU: the oracle's rule for a data symbol that arrives as
exact zeros, its decode entry orc_decode_at, and the inputs of tests/test_gpu_oob.py -- generated here, so that the
GPU module imports them -- with the proof that none of them sits on Packet_Selection's threshold.

Samples the receiver needs past a capture's end read as zero (include/ofdm_mi355x_captures.h).  A data symbol whose
window starts at or past cap_len + 20 -- p + 2 (336 + 80 d) - 20 >= cap_len -- is then 64 exact zeros: Y = 0, Z = 0 / H
= 0, the C slicer decides "-" on both axes (Z > 0 fails, OFDM.c:858-866) and the demapper (1, 0) for every pair; the
MATLAB slicer leaves a zero at zero and its demapper then [0 0] (Tester.m:338-411).

Off the threshold.  The GPU's detection metric is fp32 (sliding sums), the oracle's fp64; tests/test_gpu_stream.py
records 1.184e-4 as the largest deviation.  A crossing is UNCERTAIN when its fp64 M lies within BAND = 2e-3 x 0.75 of
0.75 (the project's +-0.1 % band doubled, 16 x that deviation), CERTAIN when it is a crossing outside the band.  The
selection cannot depend on the uncertain positions when (off_threshold below):
  a. every uncertain position has a certain crossing among the 300 positions before it (it is never a front),
  b. no certain crossing without one there (a front) has an uncertain position among them (its front status is fixed),
  c. no front has an uncertain position at + 230 (its confirmation is fixed).
a to c are sufficient, not necessary; where they fail and at most 10 positions are uncertain, every assignment of those
is tried and the selection (a stream's positions and flags, stream.select_packets; a capture's packet_idx,
stream.first_packet) must be the same for all.
Every generated input passes (seeds that do not were rejected when the cases were chosen: the issue's example,
seed 2 with wave[0:640] | wave[0:120], sits 1.2e-5 from the threshold), so the GPU tests demand zero packet_idx
mismatches."""
import numpy as np
import pytest

import ofdm_pkg

ofdm_pkg.load()
from ofdm_amd.stream import first_packet, select_packets  # noqa: E402
from test_gpu_captures import MSG, impaired, msg_bits, wave  # noqa: E402,F401  (module-scoped fixtures, used by name)
from test_stream_host import MSG5, base_stream  # noqa: E402

MSG15 = ("fifteen data symbols per frame through ofdm_set_long_message: captures of 9,394 samples. " * 3)[:171].encode()
MSGS = {2: MSG, 5: MSG5, 15: MSG15}
BAND = 2e-3 * 0.75
SNR_DB = 25.0


def metric64(x):
    """Packet_Detection's M in double precision; NaN where the power window is exactly zero"""
    x = np.asarray(x).astype(np.complex128)
    lc = len(x) - 47
    cs = np.concatenate([[0], np.cumsum(x[:-16] * x[16:])])
    cp = np.concatenate([[0], np.cumsum(np.abs(x[16:]) ** 2)])
    n = np.arange(lc)
    with np.errstate(all="ignore"):
        return np.abs(cs[n + 32] - cs[n]) ** 2 / (cp[n + 32] - cp[n]) ** 2


def off_threshold(m, band=BAND, capture=False):
    """The uncertain positions of the fp64 metric m that the selection could depend on (rules a to c of the module's
    docstring), and the number of uncertain positions in all: ([], k) is a stream whose selection is fixed.  capture:
    the decision is Packet_Selection's one packet_idx (stream.first_packet), not every position and flag."""
    with np.errstate(invalid="ignore"):
        unc = np.abs(m - 0.75) <= band
        cert = (m > 0.75) & ~unc
    lc = len(m)
    # certain crossings among the 300 positions before i
    cc = np.concatenate([[0], np.cumsum(cert)])
    before = lambda i: cc[i] - cc[max(i - 300, 0)]
    uc = np.concatenate([[0], np.cumsum(unc)])
    bad = [int(i) for i in np.nonzero(unc)[0] if before(i) == 0]                          # a
    for j in np.nonzero(cert)[0]:
        if before(j) == 0:                                                                  # j is a front
            if uc[j] - uc[max(j - 300, 0)]:
                bad += [int(i) for i in range(max(j - 300, 0), j) if unc[i]]               # b
            if j + 230 < lc and unc[j + 230]:
                bad.append(int(j + 230))                                                    # c
    bad, k = sorted(set(bad)), int(unc.sum())
    if bad and k <= 10:
        # a to c are sufficient, not necessary (a front that moves by one position but can never be confirmed decides
        # nothing): with few uncertain positions, try every assignment of them
        outcomes = set()
        cross = cert.copy()
        where = np.nonzero(unc)[0]
        for bits in range(1 << k):
            cross[where] = [(bits >> b) & 1 for b in range(k)]
            sel = select_packets(cross)
            outcomes.add(first_packet(sel) if capture else (tuple(sel["positions"]), tuple(sel["flags"])))
        if len(outcomes) == 1:
            bad = []
    return bad, k


def zero_symbols(p, cap_len, nd):
    """the data symbols wholly past the end of a cap_len-sample capture decoded at packet_idx p"""
    return [d for d in range(nd) if p + 2 * (336 + 80 * d) - 20 >= cap_len]


def _noise(n, power, seed):
    rng = np.random.default_rng(seed)
    s = np.sqrt(power / 10 ** (SNR_DB / 10) / 2)
    return s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


# ---------------------------------------------------------------- the generated inputs
# a. wave[400:400 + L], noise-free: no packet starts in it early enough, sync fails, packet_idx 0
SYNC_FAIL_LENGTHS = (400, 652, 700, 812, 900)
SYNC_FAIL_ZERO = {400: [0, 1], 652: [0, 1], 700: [1], 812: [1], 900: []}
# b. zeros(300) | wave[0:K] | wave[0:100] under complex noise at 25 dB: the packet's front near 305 is confirmed, the
# second piece gives the later front the rule needs, and the capture ends inside the packet's data.  (D, K, seeds,
# data symbols wholly past the end); the symbol before the first of those is cut, the ones before it are whole
SYNCED = ((2, 700, (1, 2, 3, 4), [1]), (5, 1000, (1, 2, 4, 6), [3, 4]), (15, 1800, (2, 5, 6, 7), list(range(8, 15))))


def sync_fail_capture(wave, L):  # noqa: F811
    return wave[400:400 + L].astype(np.complex64)


def synced_capture(wave, K, seed, lead=300, tail=100):  # noqa: F811
    x = np.concatenate([np.zeros(lead), wave[:K], wave[:tail]])
    return (x + _noise(len(x), np.mean(np.abs(wave) ** 2), seed)).astype(np.complex64)


# c. the mixed batch, all of MIXED_LEN samples (a front counts from position 300 on and needs a later front, so a
# capture that holds a whole 980-sample packet is at least 1328 long): past the end zeros(600) | wave[0:700] |
# wave[0:100] (packet_idx near 616: symbol 0 cut, symbol 1 zero), whole zeros(300) | wave[0:1100] (near 316)
MIXED_LEN = 1400
MIXED_CUT_SEEDS = tuple(range(201, 214)) + tuple(range(215, 219))
MIXED_WHOLE_SEEDS = tuple(range(302, 317)) + (319,)


def mixed_cut_capture(wave, seed):  # noqa: F811
    return synced_capture(wave, 700, seed, lead=600)


def mixed_whole_capture(wave, seed):  # noqa: F811
    return synced_capture(wave, 1100, seed, lead=300, tail=0)


def three_packet_stream(wave, seed=51):  # noqa: F811
    """tests/test_gpu_stream.py test_truncated_last_packet_and_start_inside_a_plateau's stream"""
    P = len(wave) // 10
    return base_stream(wave, SNR_DB, 0.0, seed, segments=[("gap", 700), ("wave", 0, 3 * P), ("gap", 400)])


# e, f. cuts of the three-packet stream relative to its last packet's position p (front = p - 11):
# (name, D, offset of the stream's end from p, data symbols wholly past the end, the long training symbols past it)
STREAM_CUTS = (("symbol 0 cut, symbol 1 zero", 2, 640 + 100, [1], False),
               ("both symbols zero", 2, 640 - 30, [0, 1], False),
               ("inside the data of D = 5", 5, 640 + 160 * 2 + 100, [3, 4], False),
               ("before the long training symbols", 2, 300 - 11, [0, 1], True),
               ("before the long training symbols, D = 5", 5, 350 - 11, [0, 1, 2, 3, 4], True))


def waves_of(oracle):
    out = {}
    for nd, msg in MSGS.items():
        tb = oracle.message_bits(msg)
        assert len(tb) == 96 * nd
        out[nd] = dict(truth=tb, wave=oracle.frame_waveform(tb))
    return out


@pytest.fixture(scope="module")
def waves(oracle):
    return waves_of(oracle)


def stream_cases(oracle, waves):  # noqa: F811
    """[(name, nd, full stream, cut stream, expected positions)] of STREAM_CUTS, positions by the fp64 rule"""
    out = []
    full = {nd: three_packet_stream(waves[nd]["wave"]) for nd in (2, 5)}
    for name, nd, off, zero, no_ltf in STREAM_CUTS:
        x = full[nd]
        pos = select_packets(metric64(x))["positions"]
        out.append(dict(name=name, nd=nd, full=x, cut=x[:int(pos[-1]) + off], pos=pos, zero=zero, no_ltf=no_ltf))
    return out


# ---------------------------------------------------------------- 1. the oracle's zero rule
def test_oracle_zero_symbol_rule(oracle, waves):
    w, tb = waves[2]["wave"], waves[2]["truth"]
    cap = sync_fail_capture(w, 652).astype(np.complex128)
    got = {}
    for matlab in (0, 1):
        o = oracle.receiver_frame(cap, tb, "c", dumps=True, cap_len=652, opts=dict(matlab_slicer=matlab))
        assert o["packet_idx"] == 0 and o["sync_fail"] == 1 and o["oob"] == 1
        assert zero_symbols(0, 652, 2) == [0, 1]
        assert not o["nopilot"].view(np.float64).any()                  # 96 exact zeros
        got[matlab] = [int(np.sum(o["bits"][96 * d:96 * d + 96] != tb[96 * d:96 * d + 96])) for d in (0, 1)]
        if not matlab:
            assert np.array_equal(o["bits"], np.tile([1, 0], 96))       # the C slicer: (1, 0) for every pair
            assert o["res"][2] == (53 + 47) / 192
        else:
            assert not o["bits"].any()                                  # MATLAB: [0 0]
    assert got == {0: [53, 47], 1: [35, 33]}
    # one symbol alone: symbol 1 at L = 700, and it alone (symbol 0 is cut, not zero)
    o = oracle.receiver_frame(sync_fail_capture(w, 700).astype(np.complex128), tb, "c", dumps=True, cap_len=700)
    assert o["nopilot"][:48].all() and not o["nopilot"][48:].view(np.float64).any()
    assert np.array_equal(o["bits"][96:], np.tile([1, 0], 48)) and int(np.sum(o["bits"][96:] != tb[96:])) == 47


def test_oracle_receiver_frame_arguments(oracle, waves):
    w, tb = waves[2]["wave"], waves[2]["truth"]
    base = oracle.receiver_frame(w, tb, "c", dumps=True)
    same = oracle.receiver_frame(w, tb, "c", dumps=True, cap_len=3008, opts=dict(float_cfo=1, matlab_slicer=0, float_taps=1))
    for k, v in base.items():
        assert np.array_equal(v, same[k]), k
    with pytest.raises(ValueError):
        oracle.receiver_frame(w, tb, "c", opts=dict(cap_len=100))
    with pytest.raises(ValueError):
        oracle.receiver_frame(w[:500], tb, "c", cap_len=501)


# ---------------------------------------------------------------- 2. the decode entry
def test_decode_at_reproduces_receiver_frame(oracle, impaired, msg_bits):  # noqa: F811
    fails = 0
    for cap, o in zip(impaired["caps"], impaired["ora"]):
        d = oracle.decode_at(cap.astype(np.complex128), msg_bits, o["packet_idx"], "c", dumps=True)
        fails += int(o["sync_fail"])
        for k, v in o.items():
            if k == "corr":
                assert k not in d
                continue
            assert np.array_equal(np.asarray(v), np.asarray(d[k]), equal_nan=True), k
    assert 10 <= fails < 96                                             # both outcomes were compared


# ---------------------------------------------------------------- 3. the GPU tests' inputs are off the threshold
def test_sync_fail_captures_are_off_the_threshold(oracle, waves):
    w, tb = waves[2]["wave"], waves[2]["truth"]
    for L in SYNC_FAIL_LENGTHS:
        assert L < 4 * 480 + 20                                         # the kernel's fr_sep layout
        x = sync_fail_capture(w, L)
        bad, unc = off_threshold(metric64(x), capture=True)
        o = oracle.receiver_frame(x.astype(np.complex128), tb, "c", dumps=True, cap_len=L)
        zero = [d for d in (0, 1) if not o["nopilot"][48 * d:48 * d + 48].view(np.float64).any()]
        print(f"L = {L}: {unc} uncertain positions, {len(bad)} decision-relevant; zero symbols {zero}")
        assert not bad
        assert (o["packet_idx"], o["sync_fail"], o["oob"]) == (0, 1, 1)
        assert zero == SYNC_FAIL_ZERO[L] == zero_symbols(0, L, 2)


def test_synced_captures_are_off_the_threshold(oracle, waves):
    for nd, K, seeds, zero in SYNCED:
        w, tb = waves[nd]["wave"], waves[nd]["truth"]
        for seed in seeds:
            x = synced_capture(w, K, seed)
            L = len(x)
            assert L == 400 + K
            m = metric64(x)
            bad, unc = off_threshold(m, capture=True)
            o = oracle.receiver_frame(x.astype(np.complex128), tb, "c", dumps=True, cap_len=L)
            got = [d for d in range(nd) if not o["nopilot"][48 * d:48 * d + 48].view(np.float64).any()]
            print(f"D = {nd} seed {seed}: packet_idx {o['packet_idx']}, {unc} uncertain positions, {len(bad)} "
                  f"decision-relevant, closest M to 0.75 {np.nanmin(np.abs(m - 0.75)):.3g}, zero symbols {got}")
            assert not bad
            assert o["packet_idx"] in (316, 317) and (o["sync_fail"], o["oob"]) == (0, 1)
            assert got == zero == zero_symbols(o["packet_idx"], L, nd)
            # the symbol before the zero ones is cut (it reads samples past the packet's piece), the rest are whole
            first_cut = o["packet_idx"] + 2 * (336 + 80 * (zero[0] - 1) + 63)
            assert first_cut >= 300 + K and o["packet_idx"] + 2 * (336 + 80 * (zero[0] - 2) + 63) < 300 + K


def test_mixed_batch_captures_are_off_the_threshold(oracle, waves):
    w, tb = waves[2]["wave"], waves[2]["truth"]
    for gen, seeds, p0, oob in ((mixed_cut_capture, MIXED_CUT_SEEDS, 616, 1), (mixed_whole_capture, MIXED_WHOLE_SEEDS, 316, 0)):
        assert len(seeds) >= 16
        for seed in seeds:
            x = gen(w, seed)
            assert len(x) == MIXED_LEN
            bad, unc = off_threshold(metric64(x), capture=True)
            o = oracle.receiver_frame(x.astype(np.complex128), tb, "c", dumps=True, cap_len=MIXED_LEN)
            assert not bad, (seed, bad)
            assert o["packet_idx"] in (p0, p0 + 1) and (o["sync_fail"], o["oob"]) == (0, oob), (seed, o["packet_idx"])
            assert zero_symbols(o["packet_idx"], MIXED_LEN, 2) == ([1] if oob else [])
            assert o["nopilot"][:48].all() and o["nopilot"][48:].view(np.float64).any() == (not oob)


def test_cut_streams_are_off_the_threshold(oracle, waves):
    for c in stream_cases(oracle, waves):
        nd, x, pos = c["nd"], c["cut"], c["pos"]
        assert len(pos) == 3
        for name, s in (("full", c["full"]), ("cut", x)):
            bad, unc = off_threshold(metric64(s))
            print(f"{c['name']} ({name}, {len(s)} samples): {unc} uncertain positions, {len(bad)} decision-relevant")
            assert not bad
        sel = select_packets(metric64(x))
        assert np.array_equal(sel["positions"], pos) and sel["flags"].tolist() == [0, 0, 4]
        p, n = int(pos[-1]), len(x)
        assert [d for d in range(nd) if p + 2 * (336 + 80 * d) - 20 >= n] == c["zero"]
        assert (p + 2 * 192 - 20 >= n) == c["no_ltf"]
        if c["no_ltf"]:
            assert p - 11 + 290 <= n <= p - 11 + 360                    # the front is still confirmed at + 230
        # the oracle on the window at the stream's position: the last packet's window holds no second front, so its
        # own selection fails there and the decode entry is what the GPU test compares with
        s0 = p - 411
        win = x[s0:].astype(np.complex128)
        o = oracle.receiver_frame(win, waves[nd]["truth"], "c", cap_len=len(win))
        assert o["sync_fail"] == 1
        d = oracle.decode_at(win, waves[nd]["truth"], 411, "c", dumps=True, cap_len=len(win))
        assert d["oob"] == 1 and d["packet_idx"] == 411
        if c["no_ltf"]:
            assert not d["H"].view(np.float64).any() and np.isnan(d["nopilot"].view(np.float64)).all()
            assert np.array_equal(d["bits"], np.tile([1, 0], 48 * nd)) and np.isnan(d["res"][0])
            assert np.isfinite(d["res"][1])                             # the slicer's output is +-1/sqrt 2 all the same
