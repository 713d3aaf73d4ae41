"""Self-describing coded packets on the GPU (include/ofdm_mi355x_ppdu.h, csrc/ofdm_ppdu.hip): the two encoder launches
against stream.ppdu_encode; the fused decoder against the fp32 rule stream.ppdu_decode bit for bit -- status, rate, length,
seed, PSDU and both path metrics, special values, crafted rows, looping waves, d_count; encoder -> transmitter -> receiver ->
gains -> decoder end to end; the link sweep with mixed rates; and the argument checks.  Each test prints its figures before
it asserts.

The decode cases take tests/test_gpu_punct.py's noise recipe (complex noise on the unit-power subcarriers, two levels, one
per half of the rows) at 0 dB and 6 dB: at that recipe's own 2 dB the rate-1/2 header symbol is never decoded wrong without
gains, and the rule has to see invalid headers, failed and passed checks at every rate.

Measured on an MI355X: no row of any decode case differs from the rule in any of the six outputs, while the rule itself
sees 11 to 54 invalid headers, 15 to 51 failed and 31 to 75 passed checks per rate among each case's 300 rows, and 3,326 /
6,241 / 10,416 among the 20,000; both noise-free end-to-end runs receive 40 of 40 packets with status 0; the 255-packet link
sweep (D = 3, one branch, four taps) matches 94 / 219 / 255 packets at 8 / 14 / 20 dB, every header among them right, one
rate-3/4 packet at 8 dB failing its FCS (7 PSDU bit errors), no false accept."""
import ctypes as C
import zlib

import numpy as np
import pytest

import ppdu_ref as ppr
from code_ref import ideal_eq

pytestmark = pytest.mark.gpu

RATES = ("1/2", "2/3", "3/4")
SENTINEL = 0x5A5A5A5A
DECODE_SNR_DB = (0.0, 6.0)
_RULE = {}                                                            # the rule's decodes, computed once per input


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


def psdu_rows(bodies):
    return np.array([ppr.psdu_words(b) for b in bodies], np.uint32).reshape(len(bodies), ppr.PSDU_WORDS)


def sent_rows(bodies):
    return np.array([ppr.psdu_words(b + zlib.crc32(b).to_bytes(4, "big")) for b in bodies], np.uint32).reshape(len(bodies), 31)


def junk_behind(psdu, lengths, seed):
    """the rows with random bytes in the FCS place and past LENGTH"""
    rng = np.random.default_rng(seed)
    by = rng.integers(0, 256, (len(psdu), 4 * ppr.PSDU_WORDS), dtype=np.uint8)
    clean = psdu.astype(">u4").view(np.uint8).reshape(len(psdu), -1)
    for row, src, k in zip(by, clean, lengths):
        row[:k - 4] = src[:k - 4]
    return np.ascontiguousarray(by).view(">u4").astype(np.uint32)


# ---------------------------------------------------------------- 1. the encoder
@pytest.mark.parametrize("d", [2, 3, 15])
def test_encode_is_the_rule(eng, pkg, d):
    from ofdm_amd import stream
    torch = _torch()
    for n in (1, 67, 1000):
        bodies, rates, lengths, seeds = ppr.random_packets(d, n, 100 * d + n)
        psdu = psdu_rows(bodies)
        want_words, want_info = stream.ppdu_encode(psdu, lengths, rates, seeds, d)
        for rows in (psdu, junk_behind(psdu, lengths, n)):
            got = eng.encode_ppdu(rows, np.array(lengths), np.array(rates), np.array(seeds), d)
            words, info = (got[k].cpu().numpy().view(np.uint32) for k in ("d_words", "d_info"))
            bad = int((words != want_words).any(axis=1).sum()), int((info != want_info).any(axis=1).sum())
            print(f"D = {d}, {n} packets: {bad[0]} rows of d_words and {bad[1]} rows of d_info differ from the rule")
            assert words.shape == (n, 3 * d) and info.shape == (n, 36) and bad == (0, 0)
    # out-of-range values per packet, given as device tensors: the documented header, zero data, the neighbours untouched
    n = 67
    bodies, rates, lengths, seeds = ppr.random_packets(d, n, 7 * d)
    rates, lengths, seeds = np.array(rates, np.int32), np.array(lengths, np.int32), np.array(seeds, np.int32)
    rates[3], rates[4] = 3, -1
    lengths[10], lengths[11], lengths[12] = 3, ppr.cap(d, rates[11]) + 1, -5
    seeds[20], seeds[21] = 0, 128
    psdu = psdu_rows(bodies)
    want_words, want_info = stream.ppdu_encode(psdu, lengths, rates, seeds, d, strict=False)
    refused = [3, 4, 10, 11, 12, 20, 21]
    assert (want_info[refused, 0] >> 28 == 0).all() and not want_info[refused, 1:].any() and not want_words[refused, 3:].any()
    got = eng.encode_ppdu(dev(psdu), dev(lengths), dev(rates), dev(seeds), d)
    assert np.array_equal(got["d_words"].cpu().numpy().view(np.uint32), want_words)
    assert np.array_equal(got["d_info"].cpu().numpy().view(np.uint32), want_info)
    assert stream.ppdu_decode(ideal_eq(want_words))["status"][refused].tolist() == [1] * len(refused)
    with pytest.raises(ValueError):                                   # host arrays are checked before anything is launched
        eng.encode_ppdu(psdu, lengths, rates, seeds, d)
    for bad_d in (1, 16):
        with pytest.raises(ValueError):
            eng.encode_ppdu(psdu, lengths, rates, seeds, bad_d)
    # n = 0: nothing is written
    info = torch.full((4, 36), SENTINEL, dtype=torch.int32, device="cuda")
    words = torch.full((4, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    tp, tl, tr, ts = dev(psdu[:4]), dev(lengths[:4]), dev(rates[:4]), dev(seeds[:4])
    assert eng.lib.ofdm_ppdu_encode(eng.ctx, d, p(tp), p(tl), p(tr), p(ts), 0, p(info), p(words)) == 0
    torch.cuda.synchronize()
    assert bool((info == SENTINEL).all()) and bool((words == SENTINEL).all())
    empty = eng.encode_ppdu(np.zeros((0, 31), np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), d)
    assert tuple(empty["d_words"].shape) == (0, 3 * d) and tuple(empty["d_info"].shape) == (0, 36)


# ---------------------------------------------------------------- 2. the decoder, bit for bit
def noisy_eq(d: int, n: int, seed: int):
    """n encoded packets of mixed rates, the first half at DECODE_SNR_DB[0] and the second at DECODE_SNR_DB[1] of complex
    noise on the unit-power subcarriers: (rate codes, sent PSDU rows, complex64 [n, 48 D])"""
    from ofdm_amd import stream
    bodies, rates, lengths, seeds = ppr.random_packets(d, n, seed)
    words, _ = stream.ppdu_encode(psdu_rows(bodies), lengths, rates, seeds, d)
    eq = ideal_eq(words).astype(np.complex128)
    rng = np.random.default_rng(seed + 1)
    snr = np.where(np.arange(n) < (n + 1) // 2, DECODE_SNR_DB[0], DECODE_SNR_DB[1])[:, None]
    sigma = np.sqrt(10 ** (-snr / 10) / 2)
    eq = eq + sigma * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))
    return np.array(rates), sent_rows(bodies), eq.astype(np.complex64)


def crafted_rows(d: int):
    """noise-free rows that the noise does not make: a valid header whose first seven data bits decode to zero; a
    well-formed header that names LENGTH = cap + 1; a header with the reserved bit set; a packet with a broken SERVICE
    field; one whose FCS is off by one bit: complex64 [5, 48 D]"""
    from ofdm_amd import stream
    rate = 1
    hb, db, _ = ppr.build(b"\x5a" * (ppr.cap(d, rate) - 4), rate, 77, d)
    reserved = list(hb)
    reserved[4] = 1
    rows = [(hb, [0] * 7 + db[7:]), (ppr.header_bits(5 + rate, ppr.cap(d, rate) + 1), db), (reserved, db),
            (hb, db[:12] + [db[12] ^ 1] + db[13:]), (hb, db[:16] + [db[16] ^ 1] + db[17:])]
    words = [np.concatenate([stream.conv_encode_rate(ppr.pack_words(h)[None], 1, "1/2")[0],
                             stream.conv_encode_rate(ppr.pack_words(x)[None], d - 1, RATES[rate])[0]]) for h, x in rows]
    return ideal_eq(np.array(words, np.uint32))


def add_specials(eq, csi):
    """NaN, +-inf, +-0, 1e38 and values that clamp or overflow in eq, zeros and non-finite gains in csi, an all-zero row,
    spread over the last rows (tests/test_gpu_punct.py's special values, restated, in the header's and the data's columns)"""
    n = len(eq)
    eq[n - 1] = 0
    eq[n - 2, 3] = complex(np.nan, 1.0)
    eq[n - 2, 7] = complex(np.inf, -np.inf)
    eq[n - 2, 11] = complex(-0.0, 0.0)
    eq[n - 2, 48 + 5] = complex(np.nan, np.nan)
    eq[n - 2, 48 + 9] = complex(-np.inf, np.inf)
    eq[n - 3, ::5] = complex(0.0, -0.0)
    eq[n - 4, 5] = complex(3e38, -3e38)
    eq[n - 4, 9] = complex(1e37, -1e37)
    eq[n - 4, 48 + 2] = complex(1e38, -1e38)
    eq[n - 7, 48:] = eq[n - 7, 48:] * np.complex64(1e37)              # every data value clamps; the header stays
    if csi is not None:
        csi[n - 5] = 0
        csi[n - 6, ::3] = 0
        csi[n - 2, 20] = np.inf
        csi[n - 2, 21] = np.nan
        csi[n - 8] = np.float32(1e38)


def decode_case(d: int, n: int, weighted: bool):
    """(rate codes, sent PSDU rows, eq with the crafted rows and the special values, csi or None, the rule's decode),
    computed once"""
    from ofdm_amd import stream
    key = (d, n, weighted)
    if key not in _RULE:
        rates, sent, eq = noisy_eq(d, n, 1000 * d + n)
        csi = np.random.default_rng(d + n).uniform(0, 4, (n, 48)).astype(np.float32) if weighted else None
        if n >= 40:
            eq[n - 20:n - 15] = crafted_rows(d)
            if csi is not None:
                csi[n - 20:n - 15] = 1.0
            add_specials(eq, csi)
        _RULE[key] = (rates, sent, eq, csi, stream.ppdu_decode(eq, csi))
    return _RULE[key]


def gpu_decode(eng, d, eq, csi=None, count=None, want_path=True):
    """ofdm_ppdu_decode through ctypes on sentinel-filled outputs: (meta int32 [n, 4], psdu uint32 [n, 31], path [n, 2])"""
    torch = _torch()
    n = len(eq)
    meta = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    psdu = torch.full((n, 31), SENTINEL, dtype=torch.int32, device="cuda")
    path = torch.full((n, 2), 7.5, dtype=torch.float32, device="cuda") if want_path else None
    teq, tcsi = dev(eq), None if csi is None else dev(csi)
    cnt = None if count is None else torch.tensor([n + 5, count], dtype=torch.int64, device="cuda")
    rc = eng.lib.ofdm_ppdu_decode(eng.ctx, d, p(teq), p(tcsi), p(cnt), n, p(meta), p(psdu), p(path))
    assert rc == 0, eng.lib.ofdm_last_error()
    torch.cuda.synchronize()
    return meta.cpu().numpy(), psdu.cpu().numpy().view(np.uint32), None if path is None else path.cpu().numpy()


def differing(got, want):
    """rows that differ from the rule, per output: status, rate, length, seed, psdu, header path, data path"""
    meta, psdu, path = got
    out = [int((meta[:, k] != want[key]).sum()) for k, key in enumerate(("status", "rate", "length", "seed"))]
    out.append(int((psdu != want["psdu"]).any(axis=1).sum()))
    out += [int((path[:, k].view(np.uint32) != want["path"][:, k].view(np.uint32)).sum()) for k in (0, 1)]
    return out


@pytest.mark.parametrize("d", [2, 3, 15])
def test_decode_is_the_fp32_rule_bit_for_bit(eng, d):
    for n in (1, 63, 300):                                            # 300: more rows than waves, so that the waves loop
        for weighted in (False, True):
            rates, sent, z, csi, want = decode_case(d, n, weighted)
            st = want["status"]
            classes = [[int(((st == 1) & (rates == r)).sum()), int((((st & 4) != 0) & (rates == r)).sum()),
                        int(((st == 0) & (rates == r)).sum())] for r in range(3)]
            print(f"D = {d}, {n} rows at {DECODE_SNR_DB[0]:g} and {DECODE_SNR_DB[1]:g} dB, csi {'random in [0, 4]' if weighted else 'NULL'}: "
                  f"the rule's [header invalid, FCS failed, FCS passed] per rate {classes}, bad service {int(((st & 2) != 0).sum())}")
            if n == 300:                                              # the rule alone sees every class at every rate
                for r in range(3):
                    assert min(classes[r]) > 0 or (d == 2 and r == 0 and classes[r] == [0, 0, 0]), (r, classes)
                assert (want["psdu"][st == 0] == sent[st == 0]).all()
                # the crafted rows: seven zero state bits; LENGTH = cap + 1; the reserved bit; SERVICE; FCS
                assert st[n - 20:n - 15].tolist()[1:] == [1, 1, 2, 4] and st[n - 20] & 2 and want["seed"][n - 20] == 0
                assert not want["psdu"][n - 19].any() and want["rate"][n - 19] == -1
            bad = differing(gpu_decode(eng, d, z, csi), want)
            print(f"    rows that differ from the rule in status, rate, length, seed, psdu, header path, data path: {bad}")
            assert bad == [0] * 7
    # d_count below n: the rows past it keep their sentinels
    rates, sent, z, csi, want = decode_case(d, 300, True)
    for count in (0, 37, 1000):
        meta, psdu, path = gpu_decode(eng, d, z, csi, count=count)
        rows = min(count, 300)
        assert differing((meta[:rows], psdu[:rows], path[:rows]), {k: v[:rows] for k, v in want.items()}) == [0] * 7
        assert (meta[rows:] == np.int32(SENTINEL)).all() and (psdu[rows:] == SENTINEL).all() and (path[rows:] == 7.5).all(), count
    # d_path is optional, n = 0 launches nothing, and the engine's call gives the same
    torch = _torch()
    meta, psdu, _ = gpu_decode(eng, d, z, csi, want_path=False)
    assert np.array_equal(meta[:, 0], want["status"]) and np.array_equal(psdu, want["psdu"])
    teq, tcsi = dev(z), dev(csi)
    out = torch.full((300, 4), SENTINEL, dtype=torch.int32, device="cuda")
    out2 = torch.full((300, 31), SENTINEL, dtype=torch.int32, device="cuda")
    assert eng.lib.ofdm_ppdu_decode(eng.ctx, d, p(teq), p(tcsi), None, 0, p(out), p(out2), None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out2 == SENTINEL).all())
    r = eng.decode_ppdu(teq, csi=tcsi, want_path=True)
    assert differing((r["d_meta"].cpu().numpy(), r["d_psdu"].cpu().numpy().view(np.uint32), r["d_path"].cpu().numpy()), want) == [0] * 7
    assert eng.decode_ppdu(teq, csi=tcsi)["d_path"] is None
    for kw in (dict(n_data=d + 1), dict(csi=tcsi[:, :47].contiguous())):
        with pytest.raises(ValueError):
            eng.decode_ppdu(teq, **kw)
    with pytest.raises(ValueError):
        eng.decode_ppdu(teq[:, :48].contiguous())                     # one symbol holds no packet


def test_decode_waves_loop_past_the_grid_cap(eng):
    """20,000 rows at D = 2: 16 blocks per CU of two waves with two rows each are fewer"""
    from ofdm_amd import stream
    d, n = 2, 20000
    rates, sent, z = noisy_eq(d, n, 31)
    want = stream.ppdu_decode(z)
    st = want["status"]
    bad = differing(gpu_decode(eng, d, z), want)
    print(f"D = {d}, {n} rows: the rule sees {int((st == 1).sum())} invalid headers, {int(((st & 4) != 0).sum())} failed and "
          f"{int((st == 0).sum())} passed checks; rows that differ from the rule per output: {bad}")
    assert bad == [0] * 7 and (st == 1).any() and (st == 0).any() and ((st & 4) != 0).any()
    assert n // 4 > 16 * 256                                          # more blocks of two waves with two rows each than the cap


# ---------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("d", [3, 15])
def test_end_to_end_noise_free(eng, pkg, d):
    n = 40
    assert eng.set_long_message(" " * (12 * d)) == d
    bodies, rates, lengths, seeds = ppr.random_packets(d, n, 500 + d)
    enc = eng.encode_ppdu(psdu_rows(bodies), np.array(lengths), np.array(rates), np.array(seeds), d)
    stride = pkg.abi.packet_len(d) + 400
    x = eng.transmit_packets(enc["d_words"], d, pos0=400, stride=stride, n_out=400 + n * stride)
    rx = eng.receive_stream_device(x, want_eq=True)
    csi = eng.stream_csi(x, rx)
    out = eng.decode_ppdu(rx, csi=csi, want_path=True)
    found, count = (int(v) for v in rx["d_count"].cpu())
    meta = out["d_meta"][:count].cpu().numpy()
    psdu = out["d_psdu"][:count].cpu().numpy().view(np.uint32)
    print(f"D = {d}: {count} of {n} packets received, statuses {sorted(set(meta[:, 0].tolist()))}, data path metrics "
          f"{out['d_path'][:count, 1].min().item():.4g} .. {out['d_path'][:count, 1].max().item():.4g}")
    assert count == found == n
    assert not meta[:, 0].any() and meta[:, 1].tolist() == rates and meta[:, 2].tolist() == lengths and meta[:, 3].tolist() == seeds
    assert np.array_equal(psdu, sent_rows(bodies))
    assert np.array_equal(rx["d_words"][:count].cpu().numpy(), enc["d_words"].cpu().numpy())


# ---------------------------------------------------------------- 4. the link sweep
def test_link_sweep_with_mixed_rates(pkg):
    from ofdm_amd import sweep
    abi = pkg.abi
    d, n, gap, seed, snrs = 3, 255, 500, 0xC0DE, (8.0, 14.0, 20.0)
    pdp = np.array([1, 0.5, 0.25, 0.125]) / 1.875
    psdu = np.random.default_rng(900).integers(0, 1 << 32, (n, 31), dtype=np.uint64).astype(np.uint32)
    kw = dict(noise="complex", fading=dict(pdp=pdp), detector="conjugate", timing="ltf", seed=seed)
    ids = (abi.K_CODE_ENCODE, abi.K_STREAM_CSI, abi.K_CODE_DECODE)
    with pkg.Engine(0) as e:
        e.timing(True)
        res = sweep.link_sweep(e, psdu, d, gap, snrs, code="ppdu", rate="mixed", **kw)
        assert [e.timing_query(k)[1] for k in ids] == [1, 3, 3]
        e.timing_reset()
        # the same payload words without a code: the same calls and totals as before this layer
        rates, lengths = np.arange(n) % 3, np.array([abi.ppdu_cap(d, RATES[i % 3]) for i in range(n)])
        words = e.encode_ppdu(psdu, lengths, rates, 1 + np.arange(n) % 127, d)["d_words"]
        e.timing_reset()
        plain = sweep.link_sweep(e, words, d, gap, snrs, **kw)
        assert [e.timing_query(k)[1] for k in ids] == [0, 0, 0] and "ppdu_totals" not in plain and "info_totals" not in plain
        e.timing(False)
    pt = res["ppdu_totals"]
    assert pt.shape == (3, 3, 5) and pt.dtype == np.int64 and "info_totals" not in res
    for s, row, c in zip(snrs, res["totals"], pt):
        print(f"link {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, payload bit errors {row[abi.S_BIT_ERR]}; "
              + "; ".join(f"rate {r}: matched {v[0]}, header right {v[1]}, FCS passed {v[2]}, false accepts {v[3]}, PSDU bit errors {v[4]}"
                          for r, v in zip(RATES, c)))
    assert np.array_equal(res["totals"], plain["totals"]) and res["power"] == plain["power"]
    assert np.array_equal(pt[:, :, 0].sum(axis=1), res["totals"][:, abi.S_MATCHED]) and (pt[:, :, 0] <= 85).all()
    assert (pt[:, :, 2] <= pt[:, :, 1]).all() and (pt[:, :, 1] <= pt[:, :, 0]).all()
    assert not pt[:, :, 3].any()
    assert (pt[-1, :, 2] > 0).all()
    assert res["rates"].tolist() == rates.tolist() and res["lengths"].tolist() == lengths.tolist()


# ---------------------------------------------------------------- 5. the argument checks, with a live context
def test_argument_checks_come_before_any_launch(eng):
    torch = _torch()
    lib, err = eng.lib, eng.lib.ofdm_last_error
    d, n = 3, 4
    info = torch.full((n, 36), SENTINEL, dtype=torch.int32, device="cuda")
    words = torch.full((n, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    psdu = torch.zeros((n, 31), dtype=torch.int32, device="cuda")
    per = torch.ones(n, dtype=torch.int32, device="cuda")
    good = dict(nd=d, psdu=psdu.data_ptr(), ln=per.data_ptr(), rate=per.data_ptr(), seed=per.data_ptr(), n=n,
                info=info.data_ptr(), words=words.data_ptr())
    enc = lambda **kw: (lambda a: lib.ofdm_ppdu_encode(eng.ctx, a["nd"], a["psdu"], a["ln"], a["rate"], a["seed"], a["n"],
                                                       a["info"], a["words"]))({**good, **kw})
    cases = [(dict(nd=1), b"n_data"), (dict(nd=16), b"n_data"), (dict(n=-1), b"negative")]
    cases += [({k: None}, b"is NULL") for k in ("psdu", "ln", "rate", "seed", "info", "words")]
    cases += [({k: good[k] + 2}, b"4-byte aligned") for k in ("psdu", "ln", "rate", "seed", "info", "words")]
    for kw, text in cases:
        assert enc(**kw) == -1 and text in err(), kw
    meta = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
    out = torch.full((n, 31), SENTINEL, dtype=torch.int32, device="cuda")
    eq = torch.zeros((n, 48 * d), dtype=torch.complex64, device="cuda")
    gd = dict(nd=d, eq=eq.data_ptr(), csi=None, cnt=None, n=n, meta=meta.data_ptr(), psdu=out.data_ptr(), path=None)
    dec = lambda **kw: (lambda a: lib.ofdm_ppdu_decode(eng.ctx, a["nd"], a["eq"], a["csi"], a["cnt"], a["n"], a["meta"],
                                                       a["psdu"], a["path"]))({**gd, **kw})
    cases = [(dict(nd=1), b"n_data"), (dict(nd=16), b"n_data"), (dict(n=-1), b"negative"), (dict(eq=None), b"d_eq is NULL"),
             (dict(meta=None), b"d_meta is NULL"), (dict(psdu=None), b"d_psdu is NULL"), (dict(eq=gd["eq"] + 4), b"d_eq must"),
             (dict(csi=gd["eq"] + 2), b"d_csi"), (dict(cnt=gd["eq"] + 4), b"d_count"), (dict(meta=gd["meta"] + 8), b"d_meta must"),
             (dict(psdu=gd["psdu"] + 2), b"d_psdu must"), (dict(path=gd["eq"] + 2), b"d_path")]
    for kw, text in cases:
        assert dec(**kw) == -1 and text in err(), kw
    torch.cuda.synchronize()
    for t in (info, words, meta, out):                                # nothing was launched
        assert bool((t == SENTINEL).all())
    print(f"{len(cases) + 15} refusals, each OFDM_E_ARG with a message; no output was written")
