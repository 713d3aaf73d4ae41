"""The packet transmitter on the GPU (include/ofdm_mi355x_tx.h, Engine.transmit_packets, csrc/ofdm_transmit.hip):
every packet against the oracle's Transmitter(), launch-shape invariance, placement and truncation, accumulate mode,
per-packet gain and carrier offset against fp64 numpy, the argument errors, and the loopback through
Engine.receive_stream that the feature exists for.

The shapes: D in {1, 2, 7, 15} data symbols and n = 67 packets -- no multiple of a wave nor of the 62, 31, 8 or 4
packets a block takes at once -- and n = 1.  Payload bits are random."""
import ctypes as C

import numpy as np
import pytest

from conftest import normwise

pytestmark = pytest.mark.gpu

DS = (1, 2, 7, 15)
N = 67
GAINS = np.array([1, 0.5j, -0.8 + 0.3j, 2, 0.25 - 0.25j], np.complex64)
TS = 25e-9
SENTINEL = np.complex64(12345.678 - 9876.5j)

# Test 6, measured on the MI355X: the largest normwise deviation of a rotated packet from the fp64 rotation of the
# GPU's own unrotated packet, over D in {2, 15} and the four offsets, was 1.05e-7 (D = 2 at 110 kHz, D = 15 at
# -60 kHz; the others 6.9e-8 .. 9.4e-8).  Asserted at 4 x.  It is a deviation from numpy fp64, never from the kernel.
CFO_DEV_MEASURED = 1.05e-7
# Test 8, measured on the MI355X: the largest difference between the total CFO estimates (coarse + fine) of the
# GPU-built and the numpy-fp64-built recording, over D in {1, 2, 5, 15} and the five packets, was 8.74e-4 Hz (D = 15;
# 7.1e-4, 8.2e-4 and 6.3e-4 Hz at D = 1, 2 and 5).  Asserted at 4 x.  The estimates themselves were within 58.1 Hz of
# the applied offsets, at packet offsets 16, 17, 18, 17, 17 for every D.
LOOPBACK_CFO_DEV_MEASURED_HZ = 8.74e-4


def rand_words(d: int, n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, 3 * d), dtype=np.uint64).astype(np.uint32)


def bits_of(words: np.ndarray) -> np.ndarray:
    """[n, 96 D] int32, MSB first"""
    w = np.asarray(words, np.uint32)
    return ((w[..., None] >> np.arange(31, -1, -1, dtype=np.uint32)) & 1).astype(np.int32).reshape(len(w), -1)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def rotation(f_hz: float, n: int) -> np.ndarray:
    return np.exp(2j * np.pi * f_hz * np.arange(n) * TS)


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches(eng, pkg):
    """D -> (words [67, 3 D], the 67 packets of the dense store-mode batch, conv c), built once and left unchanged"""
    out = {}
    for d in DS:
        words = rand_words(d, N, 0x7A00 + d)
        rec = eng.transmit_packets(words, d).cpu().numpy()
        assert rec.shape == (N * pkg.abi.packet_len(d),)
        out[d] = (words, rec.reshape(N, -1))
    return out


# ------------------------------------------------------------------------------------------- 1. waveform parity
@pytest.mark.parametrize("conv,d,float_taps", [(c, d, True) for c in ("c", "matlab") for d in DS] + [("c", 2, False)])
def test_every_packet_is_the_oracles_transmitter(eng, oracle, pkg, batches, conv, d, float_taps):
    words = batches[d][0]
    if conv == "c" and float_taps:
        pk = batches[d][1]
    else:
        pk = eng.transmit_packets(words, d, conv=conv, float_taps=float_taps).cpu().numpy().reshape(N, -1)
    assert pk.shape[1] == pkg.abi.packet_len(d) == {1: 820, 2: 980, 7: 1780, 15: 3060}[d]
    worst = 0.0
    for k, b in enumerate(bits_of(words)):
        worst = max(worst, normwise(pk[k], oracle.frame_waveform(b, conv, float_taps, 1)))
    print(f"transmit parity conv {conv} D {d} float_taps {float_taps}: worst normwise {worst:.3g}")
    assert worst < 2e-6
    one = eng.transmit_packets(words[:1], d, conv=conv, float_taps=float_taps).cpu().numpy()
    assert normwise(one, oracle.frame_waveform(bits_of(words[:1])[0], conv, float_taps, 1)) < 2e-6


@pytest.mark.parametrize("d", DS)
def test_the_contexts_message_gives_the_transmitters_first_period(eng, pkg, d):
    from ofdm_amd.stream import pack_messages
    msg = ("A packet's worth of text per symbol." * 6)[:12 * d - 1] + "."
    assert eng.set_long_message(msg) == d
    words, dd = pack_messages([msg])
    assert dd == d
    plen = pkg.abi.packet_len(d)
    for conv in ("c", "matlab"):
        w = eng.transmitter(conv, "message")
        got = eng.transmit_packets(words, d, conv=conv).cpu().numpy()
        dev = normwise(got, w[:plen])
        print(f"transmit_packets against transmitter, conv {conv} D {d}: normwise {dev:.3g}")
        assert dev < 4e-6


# ------------------------------------------------------------------------------------------- 2. launch shape
@pytest.mark.parametrize("d", DS)
def test_a_packet_does_not_depend_on_the_launch_shape(eng, pkg, batches, d):
    import torch
    words, pk = batches[d]
    plen = pkg.abi.packet_len(d)
    for k in (0, 1, 3, 4, 7, 8, 30, 31, 61, 62, 66):            # first and last packets of the blocks' groups
        alone = eng.transmit_packets(words[k:k + 1], d).cpu().numpy()
        assert same_bits(alone, pk[k]), k
    acc = eng.transmit_packets(words, d, accumulate=True).cpu().numpy()          # onto zeros
    assert same_bits(acc, pk.ravel())
    one = eng.transmit_packets(words[66:], d, out=torch.zeros(plen, dtype=torch.complex64, device="cuda"),
                               accumulate=True).cpu().numpy()
    assert same_bits(one, pk[66])


# ------------------------------------------------------------------------------------------- 3. placement
def placed(n_out, positions, packets, base):
    exp = base.copy()
    for p, w in zip(positions, packets):
        lo, hi = max(int(p), 0), min(int(p) + len(w), n_out)
        if lo < hi:
            exp[lo:hi] = w[lo - int(p):hi - int(p)]
    return exp


@pytest.mark.parametrize("d", DS)
def test_placement_truncation_and_untouched_samples(eng, pkg, batches, d):
    import torch
    words, pk = batches[d]
    plen = pkg.abi.packet_len(d)
    n_out = 5 * plen + 1001
    # cut at the start, cut at the end, nothing written (twice), then descending, odd (8-byte aligned only) and even
    pos = np.array([-300, n_out - 100, -plen, n_out, 3 * plen + 701, 2 * plen + 412, plen + 101], np.int64)
    out = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    got = eng.transmit_packets(words[:len(pos)], d, positions=pos, out=out)
    assert got is out
    exp = placed(n_out, pos, pk, np.full(n_out, SENTINEL, np.complex64))
    assert same_bits(out.cpu().numpy(), exp)
    assert (exp == SENTINEL).sum() == n_out - (plen - 300) - 100 - 3 * plen
    # device positions give the same recording
    out2 = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    eng.transmit_packets(torch.from_numpy(words[:len(pos)].view(np.int32)).cuda(), d, positions=torch.from_numpy(pos).cuda(),
                         out=out2)
    assert same_bits(out2.cpu().numpy(), exp)
    # pos0 and stride: all 67 packets, the first cut at the start, the last ones cut or outside at the end
    stride = plen + 13
    n_out = 60 * stride + 55
    out = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    eng.transmit_packets(words, d, pos0=-300, stride=stride, out=out)
    exp = placed(n_out, -300 + stride * np.arange(N), pk, np.full(n_out, SENTINEL, np.complex64))
    assert same_bits(out.cpu().numpy(), exp)
    assert (exp[plen - 300:stride - 300] == SENTINEL).all() and exp[n_out - 1] != SENTINEL
    # an empty batch and an empty recording launch nothing and touch nothing
    eng.transmit_packets(words[:0], d, out=out)
    assert same_bits(out.cpu().numpy(), exp)
    assert eng.transmit_packets(words, d, n_out=0).shape == (0,)


# ------------------------------------------------------------------------------------------- 4. accumulate
@pytest.mark.parametrize("d", DS)
def test_accumulate_composes_collisions_and_a_base(eng, pkg, batches, d):
    import torch
    words, pk = batches[d]
    plen = pkg.abi.packet_len(d)
    pos = np.array([101, 101 + plen - 500], np.int64)            # two packets overlapping by 500 samples
    n_out = 2 * plen
    got = eng.transmit_packets(words[5:7], d, positions=pos, n_out=n_out, accumulate=True).cpu().numpy()
    exp = np.zeros(n_out, np.complex64)
    for p, w in zip(pos, pk[5:7]):
        exp[p:p + plen] += w                                      # fp32, per component; two addends commute
    assert np.array_equal(got, exp)
    assert np.abs(exp[pos[1]:pos[0] + plen]).min() > 0 and len(exp[pos[1]:pos[0] + plen]) == 500
    rng = np.random.default_rng(d)
    base = (rng.standard_normal(plen + 77) + 1j * rng.standard_normal(plen + 77)).astype(np.complex64)
    out = torch.from_numpy(base).cuda()
    eng.transmit_packets(words[9:10], d, pos0=-40, out=out, accumulate=True)
    exp = base.copy()
    exp[:plen - 40] += pk[9][40:]
    assert np.array_equal(out.cpu().numpy(), exp)


# ------------------------------------------------------------------------------------------- 5. gain
@pytest.mark.parametrize("d", DS)
def test_gain_against_fp64(eng, pkg, batches, d):
    words, pk = batches[d]
    for accumulate in (False, True):
        got = eng.transmit_packets(words[:5], d, gains=GAINS, accumulate=accumulate).cpu().numpy().reshape(5, -1)
        for k, g in enumerate(GAINS):
            w = pk[k].astype(np.complex128)
            err = np.abs(got[k] - complex(g) * w).max()
            # two fp32 roundings per component and their sum
            assert err <= 4 * 2.0 ** -23 * abs(complex(g)) * np.abs(w).max(), (k, g, err)
        assert same_bits(got[0], pk[0])                          # a gain of one changes nothing


# ------------------------------------------------------------------------------------------- 6. carrier offset
def test_carrier_offset_against_fp64(eng, pkg, batches):
    cfos = np.array([-60e3, 25e3, 110e3, 1e6], np.float32)
    worst = 0.0
    for d in (2, 15):
        words, pk = batches[d]
        got = eng.transmit_packets(words[:4], d, cfo_hz=cfos).cpu().numpy().reshape(4, -1)
        for k, f in enumerate(cfos):
            ref = pk[k].astype(np.complex128) * rotation(float(f), pk.shape[1])
            dev = normwise(got[k], ref)
            print(f"transmit carrier offset D {d} f {float(f):.0f} Hz: normwise {dev:.3g}")
            worst = max(worst, dev)
        # an offset of zero changes nothing, and the phase counts from the packet's own first sample
        zero = eng.transmit_packets(words[:2], d, cfo_hz=np.zeros(2, np.float32)).cpu().numpy().reshape(2, -1)
        assert same_bits(zero, pk[:2])
        far = eng.transmit_packets(words[:4], d, cfo_hz=cfos, pos0=12345, stride=5000).cpu().numpy()
        assert same_bits(far[12345 + 3 * 5000:][:pk.shape[1]], got[3])
    print(f"transmit carrier offset: worst normwise {worst:.3g}")
    assert worst <= 4 * CFO_DEV_MEASURED


# ------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_come_before_any_launch(eng, pkg):
    import torch
    abi, lib = pkg.abi, eng.lib
    d, n = 2, 3
    words = torch.from_numpy(rand_words(d, n, 7).view(np.int32)).cuda()
    n_out = n * abi.packet_len(d)
    out = torch.zeros(n_out + 1, dtype=torch.complex64, device="cuda")
    ok = abi.TxOpts(0, 1, d, 0)
    W, O = C.c_void_p(words.data_ptr()), C.c_void_p(out.data_ptr())

    def call(ctx=eng.ctx, opts=ok, w=W, nn=n, o=O, no=n_out):
        return lib.ofdm_transmit_packets(ctx, None if opts is None else C.byref(opts), w, nn, None, 0, n_out // n, None,
                                         None, o, no)

    eng.timing(True)
    try:
        eng.timing_reset()
        before = eng.timing_query(abi.K_TRANSMIT)[1]
        bad = [dict(ctx=None), dict(opts=None), dict(w=None), dict(o=None), dict(nn=-1), dict(no=-1),
               dict(opts=abi.TxOpts(0, 1, 0, 0)), dict(opts=abi.TxOpts(0, 1, 16, 0)), dict(opts=abi.TxOpts(2, 1, d, 0)),
               dict(opts=abi.TxOpts(-1, 1, d, 0)), dict(opts=abi.TxOpts(0, 1, d, 2)), dict(opts=abi.TxOpts(0, 1, d, 3)),
               dict(o=C.c_void_p(out.data_ptr() + 4))]
        for kw in bad:
            assert call(**kw) == -1, kw
            assert len(lib.ofdm_last_error()) > 0, kw
        assert eng.timing_query(abi.K_TRANSMIT)[1] == before
        assert not out.abs().any()
        # nothing to do is no error and no launch; NULL buffers are fine then
        assert call(w=None, nn=0) == 0 and call(o=None, no=0) == 0
        assert eng.timing_query(abi.K_TRANSMIT)[1] == before
        assert call() == 0 and call(opts=abi.TxOpts(1, 0, d, 1)) == 0
        assert call(o=C.c_void_p(out.data_ptr() + 8)) == 0                       # 8-byte alignment is enough
        assert eng.timing_query(abi.K_TRANSMIT)[1] == before + 3                 # one launch per call
    finally:
        eng.timing(False)
    # the Python layer refuses malformed inputs itself
    w_np = rand_words(d, n, 7)
    for kw in (dict(words=w_np.astype(np.int64)), dict(words=w_np[:, :5]), dict(words=w_np.ravel()),
               dict(words=torch.from_numpy(w_np.view(np.int32))), dict(n_data=0), dict(n_data=16), dict(conv="x"),
               dict(positions=np.zeros(n, np.int32)), dict(positions=np.zeros(n + 1, np.int64)),
               dict(gains=np.ones(n, np.complex128)), dict(cfo_hz=np.zeros(n, np.float64)),
               dict(cfo_hz=torch.zeros(n, dtype=torch.float32)), dict(out=torch.zeros(8, dtype=torch.complex64)),
               dict(out=torch.zeros(8, dtype=torch.float32, device="cuda")),
               dict(out=torch.zeros(16, dtype=torch.complex64, device="cuda")[::2]),
               dict(out=out, n_out=5), dict(n_out=-1), dict(positions=torch.zeros(n, dtype=torch.int64, device="cuda")),
               dict(words=words.t().contiguous().t())):
        args = dict(words=w_np, n_data=d)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.transmit_packets(**args)


# ------------------------------------------------------------------------------------------- 8. loopback
@pytest.mark.parametrize("d", [1, 2, 5, 15])
def test_loopback_through_the_stream_receiver(eng, oracle, pkg, d):
    from ofdm_amd.stream import pack_messages, select_packets
    rng = np.random.default_rng(0x100B + d)
    texts = ["".join(chr(c) for c in rng.integers(33, 127, 12 * d)) for _ in range(5)]
    assert len(set(texts)) == 5
    words, dd = pack_messages(texts)
    assert dd == d
    plen = pkg.abi.packet_len(d)
    gaps = (700, 400, 301, 1000, 700)
    cfos = np.array([0.0, -60e3, 110e3, 40e3, 25e3], np.float32)
    pos = np.cumsum(gaps) + plen * np.arange(5)
    n_out = int(pos[-1]) + plen + 400
    gpu = eng.transmit_packets(words, d, positions=pos.astype(np.int64), gains=GAINS, cfo_hz=cfos, n_out=n_out)
    ref = np.zeros(n_out, np.complex128)
    for k, b in enumerate(bits_of(words)):
        ref[pos[k]:pos[k] + plen] = complex(GAINS[k]) * oracle.frame_waveform(b, "c", True, 1) * rotation(float(cfos[k]), plen)
    assert normwise(gpu.cpu().numpy(), ref) < 4e-6
    assert eng.set_long_message(texts[2]) == d                   # any text of the same D
    a = eng.receive_stream(gpu, want_metric=True)
    b = eng.receive_stream(ref.astype(np.complex64))
    assert a["count"] == a["found"] == 5
    assert np.array_equal(a["positions"], select_packets(a["metric"].cpu().numpy())["positions"])
    off = a["positions"] - pos
    assert ((off >= 15) & (off <= 19)).all(), off
    assert a["messages"] == texts
    est = a["records"]["cfo_coarse_hz"].astype(np.float64) + a["records"]["cfo_fine_hz"]
    assert (np.abs(est - cfos) <= 110.0).all(), est - cfos
    # the reference-built recording decodes alike
    assert b["count"] == 5 and np.array_equal(a["positions"], b["positions"])
    assert np.array_equal(a["bits"].cpu().numpy(), b["bits"])
    est_ref = b["records"]["cfo_coarse_hz"].astype(np.float64) + b["records"]["cfo_fine_hz"]
    dev = np.abs(est - est_ref).max()
    print(f"loopback D {d}: offsets {off.tolist()}, CFO error {np.abs(est - cfos).max():.1f} Hz, "
          f"GPU-built against reference-built estimates {dev:.4g} Hz")
    assert dev <= 4 * LOOPBACK_CFO_DEV_MEASURED_HZ


# ------------------------------------------------------------------------------------------- the command lines
def test_transmit_command_writes_what_the_stream_command_decodes(pkg, tmp_path):
    """python ofdm_pkg.py transmit | stream, in process: line for line, with per-packet offsets and gains"""
    import csv
    from ofdm_amd import stream
    lines = ["first packet, 2 symbols", "the second one is longer", "third", "4th: !\"#$%&'()*+,-./:;"]
    assert max(len(t) for t in lines) == 24                      # two data symbols
    (tmp_path / "lines.txt").write_text("\n".join(lines) + "\n", encoding="latin-1")
    rec = tmp_path / "rec.npy"
    assert stream.transmit_main(["--messages", str(tmp_path / "lines.txt"), "--gap", "500", "--out", str(rec),
                                 "--cfo-hz", "0,-60e3,110e3", "--gain", "1,0.5j,-0.8+0.3j"]) == 0
    x = np.load(rec)
    assert x.dtype == np.complex64 and x.shape == (4 * (980 + 500) + 500,)
    assert not x[:500].any() and not x[-500:].any() and x[500] != 0
    assert stream.main(["--in", str(rec), "--out", str(tmp_path / "out"), "--message", "x" * 24]) == 0
    with open(tmp_path / "out" / "packets.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["message"] for r in rows] == [t.ljust(24) for t in lines]
    est = [float(r["cfo_coarse_hz"]) + float(r["cfo_fine_hz"]) for r in rows]
    assert np.abs(np.array(est) - [0, -60e3, 110e3, 0]).max() <= 110.0
    # noise from channel.impair_stream: 25 dB against the packets' mean power still decodes every line
    assert stream.transmit_main(["--messages", str(tmp_path / "lines.txt"), "--out", str(rec), "--snr", "25", "--noise",
                                 "complex", "--n-data", "3"]) == 0
    y = np.load(rec)
    assert y.shape == (4 * (1140 + 500) + 500,) and y[:500].any()
    assert stream.main(["--in", str(rec), "--out", str(tmp_path / "out3"), "--message", "y" * 36]) == 0
    with open(tmp_path / "out3" / "packets.csv", newline="") as f:
        assert [r["message"] for r in csv.DictReader(f)] == [t.ljust(36) for t in lines]
