"""The coded link on the GPU (include/ofdm_mi355x_code.h, csrc/ofdm_code.hip): the encoder against stream.conv_encode, the
Viterbi decoder against the fp32 rule of stream.conv_soft and stream.viterbi_decode bit for bit -- bits and path metric,
special values, looping waves, d_count -- the gains against stream.channel_gain, and encoder -> transmitter -> receiver ->
gains -> decoder end to end.  Each test prints its figures before it asserts.

Measured on an MI355X: ofdm_stream_csi against the fp64 rule over the four streams of test_csi_against_the_fp64_rule,
relative to the packet's largest gain: 7.2e-7 (D = 2, B = 1), 9.03e-7 (D = 2, B = 2), 6.1e-7 (D = 1, B = 4) and 6.3e-7 (D = 15,
B = 2); CSI_DEV_MEASURED is the largest and the test's bound four times that.  The end-to-end test through four taps on two
branches at 30 dB receives 24 of 24 packets with no payload bit error; the 256-packet link sweep (one branch, four taps)
matches 106 / 223 / 254 packets at 8 / 14 / 20 dB with 403 / 406 / 113 payload bit errors and no information bit error."""
import ctypes as C

import numpy as np
import pytest

import code_ref as cr
from code_ref import bits_of, ideal_eq, rand_info

pytestmark = pytest.mark.gpu

CSI_DEV_MEASURED = 9.03e-7
SENTINEL = 0x5A5A5A5A


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


def dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- 1. the encoder
@pytest.mark.parametrize("d", [1, 2, 3, 15])
def test_encode_is_conv_encode(eng, d):
    from ofdm_amd import stream
    for n in (1, 67, 1000):
        info = rand_info(d, n, 100 * d + n % 97)
        want = stream.conv_encode(info, d)
        got = eng.encode_packets(info, d).cpu().numpy().view(np.uint32)
        assert got.shape == (n, 3 * d) and np.array_equal(got, want), (d, n)
        if n == 67:                                                   # the last word's unused bits are ignored
            dirty = info.copy()
            dirty[:, -1] |= np.uint32((1 << (32 * cr.info_words(d) - cr.info_bits(d))) - 1)
            assert np.array_equal(eng.encode_packets(dirty, d).cpu().numpy().view(np.uint32), want)
    # n = 0: nothing is written
    torch = _torch()
    words = torch.full((4, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.zeros((4, cr.info_words(d)), dtype=torch.int32, device="cuda")
    assert eng.lib.ofdm_code_encode(eng.ctx, d, p(info), 0, p(words)) == 0
    torch.cuda.synchronize()
    assert bool((words == SENTINEL).all())
    assert tuple(eng.encode_packets(np.zeros((0, cr.info_words(d)), np.uint32), d).shape) == (0, 3 * d)


# ---------------------------------------------------------------- 2. the decoder, bit for bit
def noisy_eq(d: int, n: int, seed: int):
    """n encoded packets, the first half at 2 dB and the second at 6 dB of complex noise on the unit-power
    subcarriers: (information words, complex64 [n, 48 D])"""
    from ofdm_amd import stream
    info = rand_info(d, n, seed)
    eq = ideal_eq(stream.conv_encode(info, d)).astype(np.complex128)
    rng = np.random.default_rng(seed + 1)
    snr = np.where(np.arange(n) < (n + 1) // 2, 2.0, 6.0)[:, None]
    sigma = np.sqrt(10 ** (-snr / 10) / 2)
    eq = eq + sigma * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))
    return info, eq.astype(np.complex64)


def add_specials(eq, csi):
    """NaN, +-inf and +-0 in eq, csi = 0, an all-zero row and values that clamp or overflow, spread over the last rows"""
    n = len(eq)
    if n < 8:
        return
    eq[n - 1] = 0
    eq[n - 2, 3] = complex(np.nan, 1.0)
    eq[n - 2, 7] = complex(np.inf, -np.inf)
    eq[n - 2, 11] = complex(-0.0, 0.0)
    eq[n - 3, ::5] = complex(0.0, -0.0)
    eq[n - 4, 5] = complex(3e38, -3e38)
    eq[n - 4, 9] = complex(1e37, -1e37)
    if csi is not None:
        csi[n - 5] = 0
        csi[n - 6, ::3] = 0
        csi[n - 2, 20] = np.inf
        csi[n - 2, 21] = np.nan


def gpu_decode(eng, d, eq, csi=None, count=None, fill=False):
    """ofdm_code_decode through ctypes on sentinel-filled outputs: (info uint32 [n, W_i], path float32 [n])"""
    torch = _torch()
    n = len(eq)
    info = torch.full((n, cr.info_words(d)), SENTINEL, dtype=torch.int32, device="cuda")
    path = torch.full((n,), 7.5, dtype=torch.float32, device="cuda")
    teq, tcsi = dev(eq), None if csi is None else dev(csi)
    cnt = None if count is None else torch.tensor([n + 5, count], dtype=torch.int64, device="cuda")
    rc = eng.lib.ofdm_code_decode(eng.ctx, d, p(teq), p(tcsi), p(cnt), n, p(info), p(path))
    assert rc == 0, eng.lib.ofdm_last_error()
    torch.cuda.synchronize()
    return info.cpu().numpy().view(np.uint32), path.cpu().numpy()


@pytest.mark.parametrize("d,big", [(1, 300), (2, 5000), (3, 300), (15, 300)])
def test_decode_is_the_fp32_rule_bit_for_bit(eng, d, big):
    from ofdm_amd import stream
    for n in (1, 63, big):                                            # big: more rows than waves, so that the waves loop
        info, eq = noisy_eq(d, n, 1000 * d + n)
        for weighted in (False, True):
            csi = np.random.default_rng(d + n).uniform(0, 4, (n, 48)).astype(np.float32) if weighted else None
            z = eq.copy()
            add_specials(z, csi)
            want = stream.viterbi_decode(stream.conv_soft(z, csi))
            got_info, got_path = gpu_decode(eng, d, z, csi)
            wrong = int((want["info"] != info).any(axis=1).sum())
            bad = int((got_info != want["info"]).any(axis=1).sum())
            badp = int((got_path != want["path"]).sum())
            print(f"D = {d}, {n} rows, csi {'random in [0, 4]' if weighted else 'NULL'}: the rule decodes {wrong} rows wrong; "
                  f"{bad} rows differ from the rule in their bits, {badp} in the path metric")
            assert bad == 0 and badp == 0
            assert np.array_equal(got_path.view(np.uint32) & 0x7fffffff, want["path"].view(np.uint32) & 0x7fffffff)
            if n == big:
                assert 0 < wrong < n                                  # wrong and right decodes both occur
            if weighted and n == 63:
                # scaling the gains by 2^7 leaves every bit unchanged and scales the path metric (on the rows as they
                # were: a value that overflows or meets the clamp at one scale only is another input)
                w = np.random.default_rng(d).uniform(0, 4, (n, 48)).astype(np.float32)
                i1, p1 = gpu_decode(eng, d, eq, w)
                i2, p2 = gpu_decode(eng, d, eq, w * np.float32(128))
                assert np.array_equal(i2, i1) and np.array_equal(p2, p1 * np.float32(128))


def test_decode_count_and_untouched_rows(eng):
    from ofdm_amd import stream
    d, n = 2, 200
    info, eq = noisy_eq(d, n, 77)
    want = stream.viterbi_decode(stream.conv_soft(eq))
    for count in (0, 1, 37, 200, 1000):
        got_info, got_path = gpu_decode(eng, d, eq, count=count)
        rows = min(count, n)
        assert np.array_equal(got_info[:rows], want["info"][:rows]) and np.array_equal(got_path[:rows], want["path"][:rows])
        assert (got_info[rows:] == SENTINEL).all() and (got_path[rows:] == 7.5).all(), count
    # d_path is optional, and n = 0 launches nothing
    torch = _torch()
    out = torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda")
    teq = dev(eq)
    assert eng.lib.ofdm_code_decode(eng.ctx, d, p(teq), None, None, n, p(out), None) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want["info"])
    out.fill_(SENTINEL)
    assert eng.lib.ofdm_code_decode(eng.ctx, d, p(teq), None, None, 0, p(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the engine's call: the same bits
    r = eng.decode_coded(teq, want_path=True)
    assert np.array_equal(r["d_info"].cpu().numpy().view(np.uint32), want["info"])
    assert np.array_equal(r["d_path"].cpu().numpy(), want["path"]) and eng.decode_coded(teq)["d_path"] is None


# ---------------------------------------------------------------- 3. the gains
def csi_stream(eng, pkg, d: int, nb: int, cfo_hz: float, seed: int):
    """nb recordings of five packets of `d` data symbols behind idle gaps through multipath channels of their own, one
    carrier offset and complex noise at 18 dB; the last packet is cut by the recording's end inside its training field"""
    from ofdm_amd import channel
    torch = _torch()
    assert eng.set_long_message(" " * (12 * d)) == d
    wave = torch.from_numpy(eng.transmitter(payload="message")).cuda()
    plen = pkg.abi.packet_len(d)
    seg = []
    for k in range(4):
        seg += [("gap", 400 + 37 * k), ("wave", 0, plen)]
    seg += [("gap", 450), ("wave", 0, 560)]                           # the fifth is cut inside its long training symbols
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rows = []
    for b in range(nb):
        taps = (rng.standard_normal(4) + 1j * rng.standard_normal(4)) * np.sqrt(np.array([1, 0.5, 0.25, 0.125]) / 3.75)
        x = channel.make_stream(wave, seg, 18.0, cfo_hz=cfo_hz, taps=taps, noise="complex", generator=g)
        buf = torch.zeros(len(x) + 2, dtype=torch.complex64, device="cuda")
        k = (b + seed) & 1                                            # the branches at different 16-byte alignments
        buf[k:k + len(x)] = x
        rows.append(buf[k:k + len(x)])
        assert rows[-1].data_ptr() % 16 == 8 * k
    return rows


@pytest.mark.parametrize("d,nb,cfo_hz", [(2, 1, 200e3), (2, 2, -200e3), (1, 4, 200e3), (15, 2, -200e3)])
def test_csi_against_the_fp64_rule(eng, pkg, d, nb, cfo_hz):
    """Measured on an MI355X: the deviation from stream.channel_gain relative to the packet's largest gain is at most
    9.03e-7 over the four streams (CSI_DEV_MEASURED); the bound is four times that, 3.6e-6."""
    from ofdm_amd import stream
    torch = _torch()
    abi = pkg.abi
    rows = csi_stream(eng, pkg, d, nb, cfo_hz, 300 + 10 * d + nb)
    n = int(rows[0].shape[0])
    if nb == 1:
        rx = eng.receive_stream(rows[0], detector="conjugate", timing="ltf", keep_device=True)
    else:
        rx = eng.receive_diversity(rows, detector="conjugate", timing="ltf", keep_device=True)
    assert rx["count"] >= 4
    # the receiver's records, and records of this test's own: the packet cut by the end (its training field runs past
    # the last sample), one wholly past the end, one whose training field starts ahead of the first sample and the first
    # record again at the recording's very start
    rec = rx["records"].copy()
    extra = np.repeat(rec[:1], 4)
    extra["packet_pos"] = [n - 500, n + 100, -380, 0]
    rec = np.concatenate([rec, extra])
    m = len(rec)
    pk = torch.from_numpy(rec.view(np.uint8).reshape(m, 64).copy()).cuda()
    cnt = torch.tensor([m, m], dtype=torch.int64, device="cuda")
    csi = eng.stream_csi(rows if nb > 1 else rows[0], dict(d_packets=pk, d_count=cnt)).cpu().numpy()
    f = rec["cfo_coarse_hz"].astype(np.float64) + rec["cfo_fine_hz"].astype(np.float64)
    want = stream.channel_gain([r.cpu().numpy() for r in rows], rec["packet_pos"], f)
    assert csi.shape == want.shape == (m, 48)
    top = want.max(axis=1)
    live = top > 0
    dev_rel = float((np.abs(csi - want)[live] / top[live, None]).max())
    print(f"D = {d}, B = {nb}, {cfo_hz / 1e3:+.0f} kHz: {m} records (estimated offsets {f[:rx['count']].round(0).tolist()} Hz), "
          f"|csi - rule| / the packet's largest gain at most {dev_rel:.3g}; largest gains {top.round(3).tolist()}")
    assert abs(f[0] - cfo_hz) < 5e3
    assert np.array_equal(csi[~live], want[~live]) and (~live).sum() == 1            # the record past the end: exact zeros
    assert dev_rel <= 4 * CSI_DEV_MEASURED
    # fewer rows than records: max_packets rows are written; a count below the rows: the rest is untouched
    out = torch.full((3, 48), 7.5, dtype=torch.float32, device="cuda")
    table = (C.c_void_p * nb)(*[r.data_ptr() for r in rows])
    assert eng.lib.ofdm_stream_csi(eng.ctx, table, nb, n, p(pk), p(cnt), 3, p(out)) == 0
    assert np.array_equal(out.cpu().numpy(), csi[:3])
    out = torch.full((m, 48), 7.5, dtype=torch.float32, device="cuda")
    cnt2 = torch.tensor([m, 2], dtype=torch.int64, device="cuda")
    assert eng.lib.ofdm_stream_csi(eng.ctx, table, nb, n, p(pk), p(cnt2), m, p(out)) == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:2], csi[:2]) and (got[2:] == 7.5).all()


# ---------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("d", [2, 15])
def test_end_to_end_noise_free(eng, pkg, d):
    torch = _torch()
    n = 40
    assert eng.set_long_message(" " * (12 * d)) == d
    info = rand_info(d, n, 500 + d)
    words = eng.encode_packets(info, d)
    stride = pkg.abi.packet_len(d) + 400
    x = eng.transmit_packets(words, d, pos0=400, stride=stride, n_out=400 + n * stride)
    rx = eng.receive_stream_device(x, want_eq=True)
    assert "d_eq" in rx and "d_eq" not in eng.receive_stream_device(x)
    csi = eng.stream_csi(x, rx)
    out = eng.decode_coded(rx, csi=csi, want_path=True)
    found, count = (int(v) for v in rx["d_count"].cpu())
    got = out["d_info"][:count].cpu().numpy().view(np.uint32)
    gains = csi[:count].cpu().numpy()
    print(f"D = {d}: {count} of {n} packets received, gains between {gains.min():.3g} and {gains.max():.3g}, path metrics "
          f"{out['d_path'][:count].min().item():.4g} .. {out['d_path'][:count].max().item():.4g}")
    assert count == found == n and np.array_equal(got, info)
    # the payload the receiver sliced is the encoder's
    assert np.array_equal(rx["d_words"][:count].cpu().numpy().view(np.uint32), words.cpu().numpy().view(np.uint32))
    # unweighted soft values decode the noise-free packets as well
    assert np.array_equal(eng.decode_coded(rx)["d_info"][:count].cpu().numpy().view(np.uint32), info)


def test_end_to_end_four_taps_two_branches(eng, pkg):
    from ofdm_amd import channel
    torch = _torch()
    d, n, pdp = 2, 24, np.array([1, 0.5, 0.25, 0.125]) / 1.875
    assert eng.set_long_message(" " * (12 * d)) == d
    info = rand_info(d, n, 600)
    words = eng.encode_packets(info, d)
    stride = pkg.abi.faded_len(d, 4) + 400
    n_out = 400 + n * stride
    unit = eng.transmit_packets(words[:1], d)
    power = float((unit.abs() ** 2).mean())
    g = torch.Generator(device="cuda")
    g.manual_seed(601)
    rows = []
    for b in range(2):
        taps = eng.draw_taps(n, pdp, seed=602 + b)
        x = eng.transmit_faded(words, d, taps, pos0=400, stride=stride, n_out=n_out)
        rows.append(channel.impair_stream(x, power, 30.0, noise="complex", generator=g))
    rx = eng.receive_diversity_device(rows, detector="conjugate", timing="ltf", want_eq=True)
    csi = eng.stream_csi(rows, rx)
    out = eng.decode_coded(rx, csi=csi)
    count = int(rx["d_count"].cpu()[1])
    rec = rx["d_packets"][:count].cpu().numpy().view(pkg.abi.stream_packet_dtype()).reshape(count)
    k = np.rint((rec["packet_pos"] - 400) / stride).astype(int)
    got = out["d_info"][:count].cpu().numpy().view(np.uint32)
    raw = int(bits_of(rx["d_words"][:count].cpu().numpy().view(np.uint32) ^ words.cpu().numpy().view(np.uint32)[k]).sum())
    print(f"four taps, two branches, 30 dB: {count} of {n} packets received, {raw} payload bit errors before the decoder, "
          f"{int(bits_of(got ^ info[k]).sum())} information bit errors after it")
    assert count == n and np.array_equal(k, np.arange(n))
    assert np.array_equal(got, info)


# ---------------------------------------------------------------- 5. the link sweep
def test_link_sweep_with_the_code(pkg):
    from ofdm_amd import stream, sweep
    abi = pkg.abi
    d, n, gap, seed, snrs = 2, 256, 500, 0xC0DE, (8.0, 14.0, 20.0)
    pdp = np.array([1, 0.5, 0.25, 0.125]) / 1.875
    info = rand_info(d, n, 700)
    kw = dict(noise="complex", fading=dict(pdp=pdp), detector="conjugate", timing="ltf", seed=seed)
    ids = (abi.K_CODE_ENCODE, abi.K_STREAM_CSI, abi.K_CODE_DECODE)
    with pkg.Engine(0) as e:
        e.timing(True)
        coded = sweep.link_sweep(e, info, d, gap, snrs, code="conv", **kw)
        assert [e.timing_query(k)[1] for k in ids] == [1, 3, 3]
        e.timing_reset()
        plain = sweep.link_sweep(e, stream.conv_encode(info, d), d, gap, snrs, **kw)
        assert [e.timing_query(k)[1] for k in ids] == [0, 0, 0] and "info_totals" not in plain
        e.timing(False)
        # the pieces: the sweep's calls again, d_eq, d_csi and the scores read back, the rule in numpy
        words = e.encode_packets(info, d)
        stride = abi.faded_len(d, len(pdp)) + gap
        clean = e.transmit_faded(words, d, e.draw_taps(n, pdp, seed=seed), pos0=gap, stride=stride, n_out=n * stride + gap)
        power = float((clean.real.double() ** 2 + clean.imag.double() ** 2).sum()) / (n * abi.packet_len(d))
        want = np.zeros((len(snrs), 3), np.int64)
        for q, s in enumerate(snrs):
            rec = e.impair_stream(clean, power, s, noise="complex", seed=seed, trial=0, snr_index=q)
            rx = e.receive_stream_device(rec, detector="conjugate", timing="ltf", want_eq=True)
            csi = e.stream_csi(rec, rx)
            sc = e.score_packets(words, d, rx, pos0=gap, stride=stride, window=(8, 43))["scores"].cpu().numpy()
            count = int(rx["d_count"].cpu()[1])
            dec = stream.viterbi_decode(stream.conv_soft(rx["d_eq"][:count].cpu().numpy(), csi[:count].cpu().numpy()))["info"]
            hit = sc[:, 0] >= 0
            err = bits_of(dec[sc[hit, 0]] ^ info[hit]).reshape(int(hit.sum()), -1).sum(axis=1)
            want[q] = (cr.info_bits(d) * int(hit.sum()), int(err.sum()), int((err > 0).sum()))
    for s, row, irow in zip(snrs, coded["totals"], coded["info_totals"]):
        print(f"coded link {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, payload bit errors {row[abi.S_BIT_ERR]} of "
              f"{row[abi.S_BITS]}, information bit errors {irow[1]} of {irow[0]} in {irow[2]} packets")
    assert coded["info_totals"].shape == (3, 3) and np.array_equal(coded["info_totals"], want)
    assert np.array_equal(coded["totals"], plain["totals"]) and coded["power"] == plain["power"]
    assert coded["totals"][0, abi.S_BIT_ERR] > 0 and coded["info_totals"][0, 0] == 90 * coded["totals"][0, abi.S_MATCHED]
    # the decoder removes errors: fewer information bit errors per bit than payload bit errors per bit at every point
    t, it = coded["totals"], coded["info_totals"]
    assert (it[:, 1] * t[:, abi.S_BITS] <= t[:, abi.S_BIT_ERR] * it[:, 0]).all()
