"""The punctured rates on the GPU (include/ofdm_mi355x_punct.h, csrc/ofdm_punct.hip): the encoder against
stream.conv_encode_rate; the Viterbi decoder against the fp32 rule of stream.conv_soft_rate and stream.viterbi_decode_rate
bit for bit -- bits and path metric, special values, looping waves, d_count; rate code 0 against the coded link's own
kernels; encoder -> transmitter -> receiver -> gains -> decoder end to end; and the link sweep at rate 3/4.  Each test
prints its figures before it asserts.

Measured on an MI355X: no row of any decode case differs from the rule, in bits or in path metric, while the rule itself
decodes 49 to 238 of the 300 rows wrong (rate, D and gains varied); the noise-free end-to-end runs receive 40 of 40
packets at both rates and D = 2 and 15; the 256-packet link sweep at rate 3/4 (one branch, four taps) matches 106 / 224 /
254 packets at 8 / 14 / 20 dB with 421 / 467 / 128 payload bit errors and 120 / 0 / 0 information bit errors."""
import ctypes as C

import numpy as np
import pytest

import code_ref as cr
import punct_ref as pr
from code_ref import bits_of, ideal_eq

pytestmark = pytest.mark.gpu

PUNCTURED = ("2/3", "3/4")
SENTINEL = 0x5A5A5A5A
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


def dirty_tail(info, d, rate):
    out = info.copy()
    out[:, -1] |= np.uint32((1 << (32 * pr.info_words(d, rate) - pr.info_bits(d, rate))) - 1)
    return out


# ---------------------------------------------------------------- 1. the encoder
@pytest.mark.parametrize("rate", PUNCTURED)
@pytest.mark.parametrize("d", [1, 2, 3, 15])
def test_encode_is_conv_encode_rate(eng, pkg, d, rate):
    from ofdm_amd import stream
    for n in (1, 67, 1000):
        info = pr.rand_info(d, n, 100 * d + n % 97, rate)
        want = stream.conv_encode_rate(info, d, rate)
        got = eng.encode_packets(info, d, rate=rate).cpu().numpy().view(np.uint32)
        assert got.shape == (n, 3 * d) and np.array_equal(got, want), (d, n)
        if n == 67:                                                   # the last word's unused bits are ignored
            assert np.array_equal(eng.encode_packets(dirty_tail(info, d, rate), d, rate=rate).cpu().numpy().view(np.uint32), want)
    # n = 0: nothing is written
    torch = _torch()
    words = torch.full((4, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.zeros((4, pr.info_words(d, rate)), dtype=torch.int32, device="cuda")
    assert eng.lib.ofdm_punct_encode(eng.ctx, pr.RATE_CODE[rate], d, p(info), 0, p(words)) == 0
    torch.cuda.synchronize()
    assert bool((words == SENTINEL).all())
    assert tuple(eng.encode_packets(np.zeros((0, pr.info_words(d, rate)), np.uint32), d, rate=rate).shape) == (0, 3 * d)
    # the other rate's shape is refused
    other = PUNCTURED[1 - PUNCTURED.index(rate)]
    if pr.info_words(d, other) != pr.info_words(d, rate):
        with pytest.raises(ValueError):
            eng.encode_packets(np.zeros((2, pr.info_words(d, other)), np.uint32), d, rate=rate)
    with pytest.raises(ValueError):
        eng.encode_packets(np.zeros((2, pr.info_words(d, rate)), np.uint32), d, rate="5/6")


# ---------------------------------------------------------------- 2. the decoder, bit for bit
def noisy_eq(d: int, n: int, seed: int, rate: str):
    """tests/test_gpu_code.py's recipe: n encoded packets, the first half at 2 dB and the second at 6 dB of complex noise
    on the unit-power subcarriers: (information words, complex64 [n, 48 D])"""
    from ofdm_amd import stream
    info = pr.rand_info(d, n, seed, rate)
    eq = ideal_eq(stream.conv_encode_rate(info, d, rate)).astype(np.complex128)
    rng = np.random.default_rng(seed + 1)
    snr = np.where(np.arange(n) < (n + 1) // 2, 2.0, 6.0)[:, None]
    sigma = np.sqrt(10 ** (-snr / 10) / 2)
    eq = eq + sigma * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))
    return info, eq.astype(np.complex64)


def add_specials(eq, csi):
    """NaN, +-inf and +-0 in eq, csi = 0, an all-zero row and values that clamp or overflow, spread over the last rows
    (tests/test_gpu_code.py's special values, restated)"""
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


def decode_case(d: int, n: int, rate: str, weighted: bool):
    """(information words, eq with the special values, csi or None, the rule's decode), computed once"""
    from ofdm_amd import stream
    key = (d, n, rate, weighted)
    if key not in _RULE:
        info, eq = noisy_eq(d, n, 1000 * d + n + pr.RATE_CODE[rate], rate)
        csi = np.random.default_rng(d + n).uniform(0, 4, (n, 48)).astype(np.float32) if weighted else None
        add_specials(eq, csi)
        _RULE[key] = (info, eq, csi, stream.viterbi_decode_rate(stream.conv_soft_rate(eq, csi, rate), rate))
    return _RULE[key]


def gpu_decode(eng, d, eq, rate, csi=None, count=None):
    """ofdm_punct_decode through ctypes on sentinel-filled outputs: (info uint32 [n, W_i], path float32 [n])"""
    torch = _torch()
    n = len(eq)
    info = torch.full((n, pr.info_words(d, rate)), SENTINEL, dtype=torch.int32, device="cuda")
    path = torch.full((n,), 7.5, dtype=torch.float32, device="cuda")
    teq, tcsi = dev(eq), None if csi is None else dev(csi)
    cnt = None if count is None else torch.tensor([n + 5, count], dtype=torch.int64, device="cuda")
    rc = eng.lib.ofdm_punct_decode(eng.ctx, pr.RATE_CODE[rate], d, p(teq), p(tcsi), p(cnt), n, p(info), p(path))
    assert rc == 0, eng.lib.ofdm_last_error()
    torch.cuda.synchronize()
    return info.cpu().numpy().view(np.uint32), path.cpu().numpy()


@pytest.mark.parametrize("rate", PUNCTURED)
@pytest.mark.parametrize("d", [1, 2, 3, 15])
def test_decode_is_the_fp32_rule_bit_for_bit(eng, d, rate):
    for n in (1, 63, 300):                                            # 300: more rows than waves, so that the waves loop
        for weighted in (False, True):
            info, z, csi, want = decode_case(d, n, rate, weighted)
            got_info, got_path = gpu_decode(eng, d, z, rate, csi)
            wrong = int((want["info"] != info).any(axis=1).sum())
            bad = int((got_info != want["info"]).any(axis=1).sum())
            badp = int((got_path != want["path"]).sum())
            print(f"rate {rate}, D = {d}, {n} rows, csi {'random in [0, 4]' if weighted else 'NULL'}: the rule decodes {wrong} rows "
                  f"wrong; {bad} rows differ from the rule in their bits, {badp} in the path metric")
            assert bad == 0 and badp == 0
            assert np.array_equal(got_path.view(np.uint32) & 0x7fffffff, want["path"].view(np.uint32) & 0x7fffffff)
            if n == 300:
                assert 0 < wrong < n                                  # wrong and right decodes both occur
    # d_count below n: the rows past it keep their sentinels
    info, z, csi, want = decode_case(d, 300, rate, True)
    for count in (0, 37, 1000):
        got_info, got_path = gpu_decode(eng, d, z, rate, csi, count=count)
        rows = min(count, 300)
        assert np.array_equal(got_info[:rows], want["info"][:rows]) and np.array_equal(got_path[:rows], want["path"][:rows])
        assert (got_info[rows:] == SENTINEL).all() and (got_path[rows:] == 7.5).all(), count
    # d_path is optional, n = 0 launches nothing, and the engine's call gives the same bits
    torch = _torch()
    teq, tcsi = dev(z), dev(csi)
    out = torch.full((300, pr.info_words(d, rate)), SENTINEL, dtype=torch.int32, device="cuda")
    assert eng.lib.ofdm_punct_decode(eng.ctx, pr.RATE_CODE[rate], d, p(teq), p(tcsi), None, 0, p(out), None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert eng.lib.ofdm_punct_decode(eng.ctx, pr.RATE_CODE[rate], d, p(teq), p(tcsi), None, 300, p(out), None) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want["info"])
    r = eng.decode_coded(teq, csi=tcsi, want_path=True, rate=rate)
    assert np.array_equal(r["d_info"].cpu().numpy().view(np.uint32), want["info"])
    assert np.array_equal(r["d_path"].cpu().numpy(), want["path"])


# ---------------------------------------------------------------- 3. rate code 0 is the coded link
@pytest.mark.parametrize("d", [1, 2, 15])
def test_rate_code_0_is_the_coded_links_kernels(eng, d):
    torch = _torch()
    n = 300
    info = cr.rand_info(d, n, 40 + d)
    tinfo = dev(dirty_tail(info, d, "1/2"))
    a = torch.full((n, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    b = torch.full((n, 3 * d), SENTINEL, dtype=torch.int32, device="cuda")
    assert eng.lib.ofdm_code_encode(eng.ctx, d, p(tinfo), n, p(a)) == 0
    assert eng.lib.ofdm_punct_encode(eng.ctx, 0, d, p(tinfo), n, p(b)) == 0, eng.lib.ofdm_last_error()
    torch.cuda.synchronize()
    assert bool((a == b).all()) and not bool((a == SENTINEL).all())
    _, z, csi, _ = decode_case(d, n, "2/3", True)                     # any noisy rows with the special values will do
    teq, tcsi = dev(z), dev(csi)
    outs = []
    for call in (lambda *r: eng.lib.ofdm_code_decode(eng.ctx, *r), lambda *r: eng.lib.ofdm_punct_decode(eng.ctx, 0, *r)):
        wi = cr.info_words(d)
        got = torch.full((n, wi), SENTINEL, dtype=torch.int32, device="cuda")
        path = torch.full((n,), 7.5, dtype=torch.float32, device="cuda")
        assert call(d, p(teq), p(tcsi), None, n, p(got), p(path)) == 0, eng.lib.ofdm_last_error()
        torch.cuda.synchronize()
        outs.append((got.cpu().numpy(), path.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    assert not (outs[1][0] == np.int32(SENTINEL)).all(axis=1).any() and not (outs[1][1] == 7.5).any()


# ---------------------------------------------------------------- 4. end to end
@pytest.mark.parametrize("rate", PUNCTURED)
@pytest.mark.parametrize("d", [2, 15])
def test_end_to_end_noise_free(eng, pkg, d, rate):
    n = 40
    assert eng.set_long_message(" " * (12 * d)) == d
    info = pr.rand_info(d, n, 500 + d, rate)
    words = eng.encode_packets(info, d, rate=rate)
    stride = pkg.abi.packet_len(d) + 400
    x = eng.transmit_packets(words, d, pos0=400, stride=stride, n_out=400 + n * stride)
    rx = eng.receive_stream_device(x, want_eq=True)
    csi = eng.stream_csi(x, rx)
    out = eng.decode_coded(rx, csi=csi, want_path=True, rate=rate)
    found, count = (int(v) for v in rx["d_count"].cpu())
    got = out["d_info"][:count].cpu().numpy().view(np.uint32)
    print(f"rate {rate}, D = {d}: {count} of {n} packets received, path metrics "
          f"{out['d_path'][:count].min().item():.4g} .. {out['d_path'][:count].max().item():.4g}")
    assert count == found == n and got.shape[1] == pkg.abi.punct_info_words(d, rate) and np.array_equal(got, info)
    assert np.array_equal(rx["d_words"][:count].cpu().numpy().view(np.uint32), words.cpu().numpy().view(np.uint32))
    # a decode that does not fit the rate's shape is refused: a rate that does not exist, rows of another length than
    # n_data says, gains of another shape
    for kw in (dict(rate="5/6"), dict(rate=rate, n_data=d + 1), dict(rate=rate, csi=csi[:, :47].contiguous())):
        with pytest.raises(ValueError):
            eng.decode_coded(rx, **kw)
    # the other rate decodes the same rows into its own shape, and not into these words
    other = PUNCTURED[1 - PUNCTURED.index(rate)]
    wrong = eng.decode_coded(rx, csi=csi, rate=other)["d_info"]
    assert wrong.shape[1] == pkg.abi.punct_info_words(d, other) != got.shape[1]


# ---------------------------------------------------------------- 5. the link sweep
def test_link_sweep_at_rate_three_quarters(pkg):
    from ofdm_amd import stream, sweep
    abi = pkg.abi
    rate, d, n, gap, seed, snrs = "3/4", 2, 256, 500, 0xC0DE, (8.0, 14.0, 20.0)
    pdp = np.array([1, 0.5, 0.25, 0.125]) / 1.875
    info = pr.rand_info(d, n, 700, rate)
    assert info.shape == (n, 5)
    kw = dict(noise="complex", fading=dict(pdp=pdp), detector="conjugate", timing="ltf", seed=seed)
    ids = (abi.K_CODE_ENCODE, abi.K_STREAM_CSI, abi.K_CODE_DECODE)
    with pkg.Engine(0) as e:
        e.timing(True)
        coded = sweep.link_sweep(e, info, d, gap, snrs, code="conv", rate=rate, **kw)
        assert [e.timing_query(k)[1] for k in ids] == [1, 3, 3]
        e.timing_reset()
        plain = sweep.link_sweep(e, stream.conv_encode_rate(info, d, rate), d, gap, snrs, **kw)
        assert [e.timing_query(k)[1] for k in ids] == [0, 0, 0] and "info_totals" not in plain
        e.timing(False)
        with pytest.raises(ValueError):                               # the rate-1/2 shape at rate 3/4
            sweep.link_sweep(e, cr.rand_info(d, n, 700), d, gap, snrs, code="conv", rate=rate, **kw)
        # the pieces: the sweep's calls again, d_eq, d_csi and the scores read back, the rule in numpy
        words = e.encode_packets(info, d, rate=rate)
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
            soft = stream.conv_soft_rate(rx["d_eq"][:count].cpu().numpy(), csi[:count].cpu().numpy(), rate)
            dec = stream.viterbi_decode_rate(soft, rate)["info"]
            hit = sc[:, 0] >= 0
            err = bits_of(dec[sc[hit, 0]] ^ info[hit]).reshape(int(hit.sum()), -1).sum(axis=1)
            want[q] = (pr.info_bits(d, rate) * int(hit.sum()), int(err.sum()), int((err > 0).sum()))
    for s, row, irow in zip(snrs, coded["totals"], coded["info_totals"]):
        print(f"rate {rate} link {s:g} dB: matched {row[abi.S_MATCHED]} of {row[abi.S_TRANSMITTED]}, payload bit errors "
              f"{row[abi.S_BIT_ERR]} of {row[abi.S_BITS]}, information bit errors {irow[1]} of {irow[0]} in {irow[2]} packets")
    assert coded["info_totals"].shape == (3, 3) and np.array_equal(coded["info_totals"], want)
    assert np.array_equal(coded["totals"], plain["totals"]) and coded["power"] == plain["power"]
    assert np.array_equal(coded["info_totals"][:, 0], 138 * coded["totals"][:, abi.S_MATCHED])
    assert coded["totals"][:, abi.S_MATCHED].min() > 0
