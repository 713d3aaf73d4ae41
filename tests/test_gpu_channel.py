"""The device channel and the per-packet scoring on the MI355X (include/ofdm_mi355x_channel.h): ofdm_impair_stream
against its header semantics -- bit for bit where the header fixes the arithmetic, against fp64 with derived bounds
where it does not -- and ofdm_score_packets against stream.score_packets, the rule in numpy.  Recordings hold 19 k
samples or fewer."""
import ctypes as C
import csv

import numpy as np
import pytest

import channel_ref as ref
from conftest import normwise
from test_gpu_transmit import CFO_DEV_MEASURED

pytestmark = pytest.mark.gpu

SENTINEL = np.complex64(12345.678 - 9876.5j)
TAPS3 = np.array([1, 0, 0.4 + 0.3j], np.complex64)
TAPS8 = np.array([0.8, 0, 0, 0.5j, 0, 0, 0, -0.3], np.complex64)
TRIAL, Q = 7, 3
# (taps, cfo_hz, noise, snr_db) of test 9's four channels
CHANNELS = {"a": (None, 0.0, "real", 25.0), "b": (TAPS3, 40e3, "complex", 25.0), "c": (TAPS3, 40e3, "complex", 14.0),
            "d": (TAPS8, -60e3, "complex", 25.0)}


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def rand_c64(n: int, seed: int) -> np.ndarray:
    r = np.random.default_rng(seed)
    return (r.standard_normal(n) + 1j * r.standard_normal(n)).astype(np.complex64)


def taps32() -> np.ndarray:
    return (rand_c64(32, 0x7A95) * np.float32(0.25)).astype(np.complex64)


def lengths(pkg):
    t = pkg.abi.CHANNEL_TILE
    return (1, 3, 4, 5, t - 1, t, t + 1, 2 * t + 3)


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context (the reference message: two data symbols per packet)"""
    e = pkg.Engine(0)
    assert e.payload_frames("message") == ref.N_DATA
    yield e
    e.close()


@pytest.fixture(scope="module")
def clean(eng, pkg):
    """The 12-packet recording: words, positions, samples (device), its host copy and the packets' mean power; built
    once and left unchanged"""
    words, (pos, n) = ref.words(), ref.layout()
    assert n == 18747
    rec = eng.transmit_packets(words, ref.N_DATA, positions=pos, n_out=n)
    host = rec.cpu().numpy()
    pk = np.concatenate([host[p:p + ref.PLEN] for p in pos]).astype(np.complex128)
    power = float(np.mean(pk.real ** 2 + pk.imag ** 2))
    return dict(words=words, pos=pos, n=n, rec=rec, host=host, power=power)


@pytest.fixture(scope="module")
def impaired(eng, clean):
    """channel name -> the impaired recording (device), built once and left unchanged"""
    return {name: eng.impair_stream(clean["rec"], clean["power"], snr, cfo, taps=taps, noise=noise, seed=ref.SEED,
                                    trial=TRIAL, snr_index=Q)
            for name, (taps, cfo, noise, snr) in CHANNELS.items()}


# ------------------------------------------------------------------------------------------- 1. identity
def test_identity_copies_bit_for_bit_and_writes_nothing_else(eng, pkg):
    import torch
    x = rand_c64(2 * pkg.abi.CHANNEL_TILE + 3, 1)
    dx = torch.from_numpy(x).cuda()
    for n in lengths(pkg):
        for index0 in (0, 1, 3, 4 * 311 + 3):
            for shift in (4, 5):                                  # 16-byte aligned and not
                buf = torch.full((n + 12,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
                got = eng.impair_stream(dx[:n], 1.0, 10.0, noise="none", index0=index0, out=buf[shift:shift + n])
                assert got.data_ptr() == buf.data_ptr() + 8 * shift
                h = buf.cpu().numpy()
                assert same_bits(h[shift:shift + n], x[:n]), (n, index0, shift)
                assert (h[:shift] == SENTINEL).all() and (h[shift + n:] == SENTINEL).all(), (n, index0, shift)
    # a source that is not 16-byte aligned either
    assert same_bits(eng.impair_stream(dx[1:1 + 1027], 1.0, 10.0, noise="none").cpu().numpy(), x[1:1 + 1027])
    assert eng.impair_stream(dx[:0], 1.0, 10.0).shape == (0,)


# ------------------------------------------------------------------------------------------- 2. real noise
@pytest.mark.parametrize("n", [9800, 9797])
def test_real_noise_is_transmission_over_air(eng, n):
    wave = eng.transmitter("c", "message")
    assert len(wave) == 9800
    x = wave[:n].copy()
    power = float(np.mean(x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2))
    for snr in (6.0, 25.0):
        want = eng.transmission_over_air(x, snr, seed=ref.SEED, trial=5, snr_index=3)
        got = eng.impair_stream(x, power, snr, noise="real", seed=ref.SEED, trial=5, snr_index=3).cpu().numpy()
        sigma = np.float32(np.sqrt(power / 10.0 ** (snr / 10.0)))
        print(f"real noise n {n} snr {snr}: sigma {sigma!r} from power {power!r}, "
              f"{int((got.view(np.int32) != want.view(np.int32)).sum())} words differ")
        assert same_bits(got, want), (n, snr)
        assert not same_bits(got, x) and (got.imag == x.imag).all()               # all of it in the real part


# ------------------------------------------------------------------------------------------- 3. absolute indexing
@pytest.mark.parametrize("noise", ["real", "complex"])
def test_a_sample_depends_on_its_absolute_index_only(eng, noise):
    import torch
    x = torch.from_numpy(rand_c64(4 * 311 + 2 * 1024 + 7, 3)).cuda()
    kw = dict(cfo_hz=40e3, noise=noise, seed=ref.SEED, trial=TRIAL, snr_index=Q)
    whole = eng.impair_stream(x, 2.0, 12.0, **kw).cpu().numpy()
    for s in (4 * 311, 4 * 311 + 1, 4 * 311 + 3):
        part = eng.impair_stream(x[s:], 2.0, 12.0, index0=s, **kw).cpu().numpy()
        assert same_bits(part, whole[s:]), s
    # another trial or SNR index is another stream
    other = eng.impair_stream(x, 2.0, 12.0, **dict(kw, snr_index=Q + 1)).cpu().numpy()
    assert not same_bits(other, whole)


# ------------------------------------------------------------------------------------------- 4. complex layout
def test_complex_noise_layout(eng):
    import torch
    n, p = 2 * 1024 + 3, 0.37
    kw = dict(seed=ref.SEED, trial=TRIAL, snr_index=Q)
    zc = eng.impair_stream(torch.zeros(n, dtype=torch.complex64, device="cuda"), p, 9.0, noise="complex", **kw).cpu().numpy()
    zr = eng.impair_stream(torch.zeros(2 * n, dtype=torch.complex64, device="cuda"), p / 2, 9.0, noise="real", **kw).cpu().numpy()
    assert not zr.imag.any() and zr.real.any()
    k = np.arange(n)
    at = 4 * (k >> 1) + 2 * (k & 1)
    assert np.array_equal(zc.real.view(np.int32), zr.real[at].view(np.int32))
    assert np.array_equal(zc.imag.view(np.int32), zr.real[at + 1].view(np.int32))
    # the variance is split across both axes: each carries p / 2 / 10^0.9 (loose: 2,051 draws)
    var = p / 2 / 10 ** 0.9
    assert abs(zc.real.var() / var - 1) < 0.2 and abs(zc.imag.var() / var - 1) < 0.2


# ------------------------------------------------------------------------------------------- 5. filter
@pytest.mark.parametrize("name", ["one", "three", "thirty-two"])
def test_filter_impulse_and_fp64_bound(eng, pkg, name):
    h = {"one": np.array([0.7 - 0.2j], np.complex64), "three": TAPS3, "thirty-two": taps32()}[name]
    L, n = len(h), 2 * pkg.abi.CHANNEL_TILE + 3
    imp = np.zeros(n, np.complex64)
    imp[0] = 1
    got = eng.impair_stream(imp, 1.0, 10.0, taps=h, noise="none").cpu().numpy()
    assert same_bits(got[:L], h) and not got[L:].any()
    x = rand_c64(n, 5)
    for index0 in (0, 1, 3):
        got = eng.impair_stream(x, 1.0, 10.0, taps=h, noise="none", index0=index0).cpu().numpy()
        want = ref.fir64(x, h)
        # the gamma-bound of a 2 L-term fma dot product, per component
        bound = (2 * L + 2) * 2.0 ** -24 * np.sqrt(2) * np.abs(h.astype(np.complex128)).sum() * np.abs(x).max()
        err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
        print(f"filter L {L} index0 {index0}: max component error {err:.3g}, bound {bound:.3g}")
        assert err <= bound


# ------------------------------------------------------------------------------------------- 6. rotation
@pytest.mark.parametrize("index0", [0, 2 ** 33 - 5000])
def test_rotation_against_fp64(eng, pkg, index0):
    n = 2 * pkg.abi.CHANNEL_TILE + 3
    x = rand_c64(n, 6)
    plain = eng.impair_stream(x, 1.0, 10.0, noise="none", index0=index0).cpu().numpy()
    assert same_bits(plain, x)
    worst = 0.0
    for f in (-60e3, 40e3, 110e3):
        got = eng.impair_stream(x, 1.0, 10.0, cfo_hz=f, noise="none", index0=index0).cpu().numpy()
        want = plain.astype(np.complex128) * ref.rotation64(f, index0, n)
        dev = normwise(got, want)
        print(f"channel rotation index0 {index0} f {f:.0f} Hz: normwise {dev:.3g}")
        worst = max(worst, dev)
    assert worst <= 4 * CFO_DEV_MEASURED


# ------------------------------------------------------------------------------------------- 7. chunks
def test_chunks_equal_the_whole(eng, clean):
    h = taps32()
    kw = dict(cfo_hz=40e3, taps=h, noise="complex", seed=ref.SEED, trial=TRIAL, snr_index=Q)
    rec, n = clean["rec"], clean["n"]
    whole = eng.impair_stream(rec, clean["power"], 25.0, **kw).cpu().numpy()
    cuts = [0, 1, 1023, 4099, 12290, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        lead = min(31, lo)                                        # 31 from the second cut on; in front of the recording u = 0
        parts.append(eng.impair_stream(rec[lo - lead:hi], clean["power"], 25.0, index0=lo, lead=lead, **kw).cpu().numpy())
        assert len(parts[-1]) == hi - lo
    assert same_bits(np.concatenate(parts), whole)
    assert not same_bits(whole, clean["host"])


# ------------------------------------------------------------------------------------------- 8. in place, errors
def test_in_place_overlap_and_argument_errors(eng, pkg):
    import torch
    abi, lib = pkg.abi, eng.lib
    n = 1024 + 5
    x = rand_c64(n, 8)
    kw = dict(cfo_hz=40e3, noise="complex", seed=ref.SEED, trial=TRIAL, snr_index=Q)
    eng.timing(True)
    try:
        eng.timing_reset()
        launches = lambda: eng.timing_query(abi.K_CHANNEL)[1]
        before = launches()
        for h in (None, np.array([0.5 + 0.25j], np.complex64)):
            want = eng.impair_stream(x, 1.0, 20.0, taps=h, **kw).cpu().numpy()
            buf = torch.from_numpy(x).cuda()
            got = eng.impair_stream(buf, 1.0, 20.0, taps=h, out=buf, **kw)
            assert got is buf and same_bits(buf.cpu().numpy(), want)
        assert launches() == before + 4                                      # one launch per successful call
        before = launches()
        big = torch.from_numpy(np.concatenate([x, x])).cuda()
        keep = big.clone()
        bad = [dict(x=big[:n], out=big[:n], taps=TAPS3),                      # in place with three taps
               dict(x=big[:n], out=big[5:5 + n]),                            # shifted overlap
               dict(x=big[5:5 + n], out=big[:n]),
               dict(x=big[:n], out=big[:n], lead=0, taps=np.zeros(2, np.complex64)),
               dict(x=big[:n + 3], out=big[3:n + 3], lead=3),                # in place needs lead 0
               dict(x=big[:n], out=big[n:2 * n - 1]),                        # wrong length
               dict(x=big[:n], power=-1.0), dict(x=big[:n], power=float("nan")), dict(x=big[:n], snr_db=float("inf")),
               dict(x=big[:n], cfo_hz=float("nan")), dict(x=big[:n], snr_index=1 << 24), dict(x=big[:n], snr_index=-1),
               dict(x=big[:n], index0=-1), dict(x=big[:n], lead=-1), dict(x=big[:n], lead=n + 1),
               dict(x=big[:n], taps=np.zeros(33, np.complex64)), dict(x=big[:n], noise="pink"),
               dict(x=big[:n], noise="real", index0=(1 << 34) - n + 1), dict(x=big[:n], noise="complex", index0=(1 << 33) - n + 1),
               dict(x=big[:n].to(torch.complex128)), dict(x=big[::2]), dict(x=x.astype(np.complex128)), dict(x=[1, 2])]
        for b in bad:
            args = dict(power=1.0, snr_db=20.0)
            args.update(b)
            with pytest.raises(ValueError):
                eng.impair_stream(args.pop("x"), args.pop("power"), args.pop("snr_db"), **args)
        # the C entry refuses the same things itself, before any launch
        X, O = C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 8 * n)
        T = TAPS3.ctypes.data_as(C.c_void_p)
        ok = dict(power=1.0, snr_db=20.0, cfo_hz=0.0, seed=1, trial=0, index0=0, noise=abi.NOISE_REAL, snr_index=0, n_taps=0, lead=0)

        def call(ctx=eng.ctx, taps=None, din=X, dout=O, nn=n, null_opts=False, **o):
            opts = abi.ChannelOpts(**dict(ok, **o))
            return lib.ofdm_impair_stream(ctx, None if null_opts else C.byref(opts), taps, din, dout, nn)

        cbad = [dict(ctx=None), dict(null_opts=True), dict(din=None), dict(dout=None), dict(n_taps=3), dict(nn=-1),
                dict(lead=-1), dict(index0=-1), dict(n_taps=-1), dict(n_taps=33, taps=T), dict(noise=3), dict(noise=-1),
                dict(snr_index=-1), dict(snr_index=1 << 24), dict(power=float("nan")), dict(power=float("inf")),
                dict(power=-1.0), dict(snr_db=float("nan")), dict(cfo_hz=float("inf")),
                dict(din=C.c_void_p(big.data_ptr() + 4)), dict(dout=C.c_void_p(big.data_ptr() + 8 * n + 4)),
                dict(index0=(1 << 34) - n + 1), dict(noise=abi.NOISE_COMPLEX, index0=(1 << 33) - n + 1),
                dict(dout=X, n_taps=3, taps=T), dict(dout=X, lead=1, nn=n - 1),
                dict(dout=C.c_void_p(big.data_ptr() + 40)), dict(din=C.c_void_p(big.data_ptr() + 40), dout=X)]
        for kwc in cbad:
            assert call(**kwc) == -1, kwc
            assert len(lib.ofdm_last_error()) > 0, kwc
        assert launches() == before
        assert torch.equal(big, keep)                                        # nothing was written
        # nothing to do is no error and no launch; the limits themselves are allowed
        assert call(nn=0, din=None, dout=None) == 0 and launches() == before
        assert call(index0=(1 << 34) - n) == 0 and call(noise=abi.NOISE_COMPLEX, index0=(1 << 33) - n) == 0
        assert call(noise=abi.NOISE_NONE, index0=1 << 40) == 0 and call(dout=X, n_taps=1, taps=T) == 0
        assert launches() == before + 4
    finally:
        eng.timing(False)


# ------------------------------------------------------------------------------------------- 9. scoring
def score_both(eng, pkg, clean, rx, n_tx=12):
    """Engine.score_packets and stream.score_packets on the same received records"""
    from ofdm_amd.stream import score_packets
    words, pos = clean["words"][:n_tx], clean["pos"][:n_tx]
    dev = eng.score_packets(words, ref.N_DATA, rx, positions=pos)
    scores, totals = dev["scores"].cpu().numpy(), dev["totals"].cpu().numpy()
    count = rx["count"]
    rw = rx["d_words"][:count].cpu().numpy().view(np.uint32)
    host = score_packets(pos, words, rx["positions"], rw)
    assert scores.shape == (n_tx, 2) and scores.dtype == np.int32
    assert np.array_equal(scores[:, 0], host["rx_index"]) and np.array_equal(scores[:, 1], host["bit_err"])
    assert np.array_equal(totals, host["totals"]) and totals.dtype == np.int64
    abi = pkg.abi
    assert totals[abi.S_TRANSMITTED] == n_tx and totals[abi.S_RECEIVED] == count
    assert totals[abi.S_MATCHED] + int((scores[:, 0] < 0).sum()) == n_tx
    assert totals[abi.S_BITS] == 96 * ref.N_DATA * totals[abi.S_MATCHED]
    return scores, totals


@pytest.mark.parametrize("name", list(CHANNELS))
def test_scoring_is_exact(eng, pkg, clean, impaired, name):
    abi = pkg.abi
    rx = eng.receive_stream(impaired[name], keep_device=True)
    assert rx["d_packets"].shape[1] == 64 and rx["d_count"].cpu().tolist() == [rx["found"], rx["count"]]
    scores, totals = score_both(eng, pkg, clean, rx)
    offs = [int(rx["positions"][j] - clean["pos"][k]) for k, j in enumerate(scores[:, 0]) if j >= 0]
    print(f"channel ({name}): found {rx['found']}, matched {totals[abi.S_MATCHED]}, offsets {offs}, "
          f"bit_err {scores[:, 1].tolist()}")
    if name in "ab":
        assert totals[abi.S_MATCHED] == 12 and (scores[:, 0] >= 0).all()
    if name == "d":
        assert totals[abi.S_MATCHED] == 0 and (scores[:, 0] == -1).all() and not scores[:, 1].any()
    # fewer records than packets found, and no transmitted packet at all
    few = eng.receive_stream(impaired[name], max_packets=5, keep_device=True)
    assert few["count"] == min(5, few["found"]) and few["found"] == rx["found"]
    score_both(eng, pkg, clean, few)
    s0, t0 = score_both(eng, pkg, clean, rx, n_tx=0)
    assert len(s0) == 0 and t0.tolist() == [0, 0, rx["count"], 0, 0, 0, 0, 0]
    # totals are added to, and a dense layout needs no positions
    import torch
    acc = torch.full((abi.NSCORE,), 5, dtype=torch.int64, device="cuda")
    eng.score_packets(clean["words"], ref.N_DATA, (rx["d_packets"], rx["d_count"], rx["d_words"]),
                      positions=clean["pos"], totals=acc)
    assert np.array_equal(acc.cpu().numpy() - 5, totals)
    one = eng.score_packets(clean["words"][:1], ref.N_DATA, rx, pos0=int(clean["pos"][0]), stride=1)
    assert np.array_equal(one["scores"].cpu().numpy()[0], scores[0])


def test_scoring_argument_errors(eng, pkg, clean, impaired):
    abi, lib = pkg.abi, eng.lib
    rx = eng.receive_stream(impaired["a"], keep_device=True)
    for bad in (dict(window=(0, 301)), dict(window=(-1, 40)), dict(window=(41, 40)), dict(window=8), dict(n_data=0),
                dict(n_data=16), dict(n_data=3), dict(rx=eng.receive_stream(impaired["a"])), dict(rx=(1, 2)),
                dict(positions=clean["pos"][:5]), dict(positions=clean["pos"].astype(np.int32)),
                dict(words=clean["words"].astype(np.float32))):
        args = dict(words=clean["words"], n_data=ref.N_DATA, rx=rx, positions=clean["pos"])
        args.update(bad)
        with pytest.raises(ValueError):
            eng.score_packets(args.pop("words"), args.pop("n_data"), args.pop("rx"), **args)
    import torch
    w = torch.from_numpy(clean["words"].view(np.int32)).cuda()
    tot = torch.zeros(abi.NSCORE, dtype=torch.int64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    ok = dict(ctx=eng.ctx, d=2, w=P(w), n=12, pk=P(rx["d_packets"]), cnt=P(rx["d_count"]), bits=P(rx["d_words"]),
              lo=8, hi=40, tot=P(tot))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ofdm_score_packets(a["ctx"], a["d"], a["w"], a["n"], None, 700, 5000, a["pk"], a["cnt"], a["bits"],
                                      a["lo"], a["hi"], None, a["tot"])

    eng.timing(True)
    try:
        eng.timing_reset()
        before = eng.timing_query(abi.K_SCORE)[1]
        for kw in (dict(ctx=None), dict(w=None), dict(pk=None), dict(cnt=None), dict(bits=None), dict(tot=None), dict(n=-1),
                   dict(d=0), dict(d=16), dict(lo=-1), dict(lo=41), dict(lo=0, hi=301)):
            assert call(**kw) == -1, kw
            assert len(lib.ofdm_last_error()) > 0, kw
        assert eng.timing_query(abi.K_SCORE)[1] == before and not tot.any()
        assert call() == 0 and call(w=None, n=0) == 0
        assert eng.timing_query(abi.K_SCORE)[1] == before + 2                 # one launch per call
        assert tot.cpu().tolist()[:3] == [12, 1, 2 * rx["count"]]              # only packet 0 sits on the dense layout
    finally:
        eng.timing(False)


# ------------------------------------------------------------------------------------------- 10. fp64 channel
@pytest.mark.parametrize("name", ["a", "b"])
def test_device_channel_against_an_fp64_channel(eng, pkg, oracle, clean, impaired, name):
    taps, cfo, noise, snr = CHANNELS[name]
    want = ref.channel64(oracle, clean["host"], clean["power"], snr, cfo, taps, noise, TRIAL, Q)
    got = impaired[name].cpu().numpy()
    print(f"channel ({name}) against fp64: normwise {normwise(got, want):.3g}")
    # the same noise realisation: fp32 rounding and the hardware logarithm and sine leave parts in 1e7 of the largest
    # sample, another realisation would differ by the noise itself, sigma / max|x| > 1e-2
    assert normwise(got, want) < 1e-5
    out = []
    for rec in (got, want.astype(np.complex64)):
        import torch
        rx = eng.receive_stream(torch.from_numpy(rec).cuda(), keep_device=True)
        scores, _ = score_both(eng, pkg, clean, rx)
        out.append(scores)
    print(f"channel ({name}): bit_err device {out[0][:, 1].tolist()}, fp64 {out[1][:, 1].tolist()}")
    assert (out[0][:, 0] >= 0).all() and (out[1][:, 0] >= 0).all()
    assert np.array_equal(out[0][:, 1], out[1][:, 1])


# ------------------------------------------------------------------------------------------- 11. link
def test_link_command_in_process(pkg, tmp_path):
    from ofdm_amd import sweep
    from ofdm_amd.fileio import read_float_array_file
    out = tmp_path / "link"
    assert sweep.link_main(["--packets", "12", "--n-data", "2", "--gap", "500", "--snr", "25:40:15", "--taps",
                            "1,0,0.4+0.3j", "--cfo-hz", "40e3", "--noise", "complex", "--out", str(out)]) == 0
    assert read_float_array_file(out / "Output_SNR.txt").tolist() == [25.0, 40.0]
    ber = read_float_array_file(out / "Output_BER.txt")
    rows = list(csv.reader(open(out / "link.csv")))
    assert tuple(rows[0]) == sweep.LINK_COLUMNS and len(rows) == 3
    for k, row in enumerate(rows[1:]):
        snr, tx, matched, missed, fa, perr, berr, bits = (float(v) for v in row)
        print(f"link {snr:g} dB: matched {matched:g} missed {missed:g} false alarms {fa:g} packet_err {perr:g} "
              f"bit_err {berr:g} of {bits:g}")
        assert snr == (25.0, 40.0)[k] and tx == 12 and matched + missed == 12 and fa >= 0
        assert bits == 192 * matched and perr <= matched and berr <= bits
        assert abs(ber[k] - berr / max(bits, 1)) <= 5e-3 * max(ber[k], 1e-30) + 1e-12      # the file holds '%.2e'
    # 40 dB under this channel loses nothing (the transmit command's loop-back decodes it at 25 dB)
    assert float(rows[2][2]) == 12 and float(rows[2][6]) == 0
    # the same sweep through the library calls, scored on the host
    from ofdm_amd.stream import score_packets
    words = np.random.default_rng(0x80211A).integers(0, 1 << 32, (12, 6), dtype=np.uint64).astype(np.uint32)
    with pkg.Engine(0) as e:
        res = sweep.link_sweep(e, words, 2, 500, [25.0, 40.0], cfo_hz=40e3, taps=TAPS3, noise="complex")
        plen = pkg.abi.packet_len(2)
        rec = e.transmit_packets(words, 2, pos0=500, stride=plen + 500, n_out=12 * (plen + 500) + 500)
        for q, s in enumerate((25.0, 40.0)):
            y = e.impair_stream(rec, res["power"], s, 40e3, taps=TAPS3, noise="complex", snr_index=q)
            rx = e.receive_stream(y, keep_device=True)
            host = score_packets(500 + (plen + 500) * np.arange(12), words, rx["positions"],
                                 rx["d_words"][:rx["count"]].cpu().numpy().view(np.uint32))
            assert np.array_equal(res["totals"][q], host["totals"])
            assert [int(v) for v in rows[1 + q][1:]] == [12, host["totals"][1], 12 - host["totals"][1],
                                                         host["totals"][2] - host["totals"][1], host["totals"][5],
                                                         host["totals"][4], host["totals"][3]]
