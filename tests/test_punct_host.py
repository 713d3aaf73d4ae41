"""The punctured rates of the coded link (include/ofdm_mi355x_punct.h), the checks that need no GPU: the header, the binding
and the build of the new translation unit; the packet's figures; the free distances that anchor the patterns; the rules of
stream.py against the plain second implementation of tests/punct_ref.py, bit for bit; rate "1/2" against the coded link's
rules; the argument checks; and what each rate costs on the subcarrier-level model.  Each test prints its figures before it
asserts.

Measured here (tests/code_ref.py's model: Rayleigh taps of profile 1, 0.5, 0.25, 0.125 at 40 MS/s, complex noise, an LS
estimate from two training symbols, zero-forcing, |H|^2 weights; 3,000 two-symbol packets, seed 0xC0DE), information bit
error rates for rates 1/2 / 2/3 / 3/4 against the uncoded payload's: 10 dB 2.4e-2 / 6.5e-2 / 1.0e-1 against 8.4e-2; 12 dB
8.8e-3 / 3.1e-2 / 6.0e-2 against 5.6e-2; 14 dB 2.7e-3 / 1.3e-2 / 2.9e-2 against 3.7e-2; 16 dB 7.5e-4 / 4.3e-3 / 1.3e-2
against 2.4e-2; 18 dB 3.8e-4 / 1.6e-3 / 4.1e-3 against 1.6e-2; 20 dB 6.3e-5 / 9.1e-4 / 1.7e-3 against 1.0e-2.  The order
uncoded > 3/4 > 2/3 > 1/2 is asserted at 16 dB, the first point of that grid at which every neighbouring pair is apart by a
factor of 1.8 or more (203, 1,560 and 5,325 information bit errors, 13,888 payload bit errors of 576,000)."""
import json
import re
import subprocess

import numpy as np
import pytest

import code_ref as cr
import punct_ref as pr
from code_ref import bits_of, ideal_eq
from conftest import ROOT

RATES = ("1/2", "2/3", "3/4")
PUNCTURED = ("2/3", "3/4")
COSTS_PACKETS, COSTS_SEED, COSTS_PDP, COSTS_SNR_DB = 3000, 0xC0DE, (1.0, 0.5, 0.25, 0.125), 16.0
# the words no header but its own may hold (tests/test_code_host.py, tests/test_diversity_host.py and the older ones)
OLDER_WORDS = ("ofdm_code_encode", "ofdm_code_decode", "ofdm_stream_csi", "OFDM_K_CODE_ENCODE", "OFDM_K_STREAM_CSI",
               "OFDM_K_CODE_DECODE", "OFDM_CODE_", "ofdm_receive_stream_diversity", "OFDM_DIVERSITY_MAX_BRANCHES",
               "OFDM_K_STREAM_DETECT_DIV", "OFDM_K_STREAM_TIMING_DIV", "OFDM_K_STREAM_DECODE_DIV", "ofdm_receive_stream_tracked",
               "OFDM_TRACK_PILOTS", "ofdm_receive_stream_timed", "OFDM_TIMING_LTF")


# ---------------------------------------------------------------- 1. the header, the binding, the build
def test_punct_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.PUNCT_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.PUNCT_FUNCTIONS) == ["ofdm_punct_decode", "ofdm_punct_encode"]
    for k, v in vars(abi).items():
        if k.endswith("EXPORTS") or (k.endswith("_FUNCTIONS") and k != "PUNCT_FUNCTIONS"):
            assert not set(names) & set(v), k
    assert not any(k.endswith("EXPORTS") and v is abi.PUNCT_FUNCTIONS for k, v in vars(abi).items())
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_code.h"' in h
    for word in OLDER_WORDS:
        assert word not in h, word
    new = abi.PUNCT_FUNCTIONS + ("OFDM_PUNCT_",)
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != abi.PUNCT_HEADER.name:
            text = other.read_text()
            for word in new:
                assert word not in text, (other.name, word)
    # the header says what the issue asks it to say
    for word in ("70 or 78", "four input words", "id 18", "id 20", "14,400", "28,800", "five blocks", "free distances are 10, 6 and 5"):
        assert word in h, word
    # the coded link's header and translation unit are as they were: puncturing stays among its out-of-scope words
    assert "puncturing (rates 2/3 and 3/4)" in abi.CODE_HEADER.read_text()


def test_punct_constants_match_the_header(pkg, tmp_path):
    abi = pkg.abi
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_punct.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", OFDM_PUNCT_RATE_1_2, OFDM_PUNCT_RATE_2_3, OFDM_PUNCT_RATE_3_4, '
                   "OFDM_PUNCT_RATES, OFDM_PUNCT_TAIL_BITS);\n"
                   "for (int r = 0; r < OFDM_PUNCT_RATES; ++r) { printf(\"%d\\n\", OFDM_PUNCT_STEPS(r));\n"
                   "for (int d = 1; d <= 15; ++d) printf(\"%d %d\\n\", OFDM_PUNCT_INFO_BITS(d, r), OFDM_PUNCT_INFO_WORDS(d, r)); }\n"
                   "return 0; }\n")
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[:5] == [abi.RATE["1/2"], abi.RATE["2/3"], abi.RATE["3/4"], len(abi.RATE), abi.CODE_TAIL_BITS] == [0, 1, 2, 3, 6]
    from ofdm_amd import stream
    assert stream.RATES == RATES == tuple(abi.RATE) and stream.RATE_STEPS == dict(zip(RATES, (48, 64, 72)))
    body = got[5:]
    for rate in RATES:
        assert body[0] == abi.PUNCT_STEPS[abi.rate_code(rate)] == stream.RATE_STEPS[rate] == pr.STEPS[rate]
        for d in range(1, 16):
            bits, words = body[1 + 2 * (d - 1)], body[2 + 2 * (d - 1)]
            assert bits == abi.punct_info_bits(d, rate) == stream.rate_info_bits(d, rate) == pr.info_bits(d, rate)
            assert words == abi.punct_info_words(d, rate) == stream.rate_info_words(d, rate) == pr.info_words(d, rate)
        body = body[31:]
    assert not body


def test_packet_figures(pkg):
    from ofdm_amd import stream
    abi = pkg.abi
    assert [abi.punct_info_bits(d, "2/3") for d in (1, 2, 15)] == [58, 122, 954]
    assert [abi.punct_info_words(d, "2/3") for d in (1, 2, 15)] == [2, 4, 30]
    assert [abi.punct_info_bits(d, "3/4") for d in (1, 2, 15)] == [66, 138, 1074]
    assert [abi.punct_info_words(d, "3/4") for d in (1, 2, 15)] == [3, 5, 34]
    assert [stream.rate_info_bits(d, "2/3") for d in (1, 2, 15)] == [58, 122, 954]
    assert [stream.rate_info_words(d, "3/4") for d in (1, 2, 15)] == [3, 5, 34]
    for d in (1, 2, 15):
        assert abi.punct_info_bits(d, "1/2") == abi.code_info_bits(d) == stream.INFO_BITS(d) == stream.rate_info_bits(d)
        assert abi.punct_info_words(d, "1/2") == abi.code_info_words(d) == stream.rate_info_words(d)
    for bad in ("5/6", "", None, 1, 0.5, "1/2 "):
        with pytest.raises(ValueError):
            abi.rate_code(bad)
        with pytest.raises(ValueError):
            stream.puncture_index(bad)
        with pytest.raises(ValueError):
            stream.rate_info_bits(2, bad)
    for bad in (0, 16, 1.5):
        with pytest.raises(ValueError):
            stream.rate_info_bits(bad, "3/4")
    # the kept places: 96 of 2 S, ascending, the sent order of the standard
    for rate in RATES:
        idx = stream.puncture_index(rate)
        s = stream.RATE_STEPS[rate]
        assert idx.shape == (96,) and (np.diff(idx) > 0).all() and idx[-1] < 2 * s
        name = lambda place: f"{'AB'[place & 1]}{place >> 1}"
        print(f"rate {rate}: S = {s}, sent order {' '.join(name(int(v)) for v in idx[:8])} ..")
        table = pr.steal_table(rate)
        assert [int(v) for v in idx] == [2 * (pr.PERIOD[rate] * p + tau) + ab for p in range(96 // len(table)) for tau, ab in table]
    assert [f"{'AB'[v & 1]}{v >> 1}" for v in stream.puncture_index("2/3")[:6]] == ["A0", "B0", "A1", "A2", "B2", "A3"]
    assert [f"{'AB'[v & 1]}{v >> 1}" for v in stream.puncture_index("3/4")[:8]] == ["A0", "B0", "A1", "B2", "A3", "B3", "A4", "B5"]
    # the LDS of the decode kernel
    assert abi.punct_decode_lds_bytes(15, "3/4") == abi.PUNCT_DECODE_WAVES * (8640 + 5760) == 28800
    assert 160 * 1024 // abi.punct_decode_lds_bytes(15, "3/4") == 5 and abi.punct_decode_lds_bytes(15, "3/4") <= 64 * 1024
    assert abi.punct_decode_lds_bytes(15, "1/2") // abi.PUNCT_DECODE_WAVES == abi.code_decode_lds_bytes(15) // abi.CODE_DECODE_WAVES
    # texts into information bits at a rate
    words, d = stream.pack_coded_messages(["Hello", "x" * 16], rate="3/4")
    assert d == 2 and words.shape == (2, 5) and words.dtype == np.uint32
    assert bytes(np.packbits(bits_of(words)[0, :136])) == b"Hello" + b" " * 12 and not bits_of(words)[:, 136:].any()
    assert stream.pack_coded_messages(["x" * 7], rate="2/3")[1] == 1 and stream.pack_coded_messages(["x" * 8], rate="2/3")[1] == 2
    assert stream.pack_coded_messages(["x" * 134], rate="3/4")[1] == 15
    with pytest.raises(ValueError):
        stream.pack_coded_messages(["x" * 135], rate="3/4")
    with pytest.raises(ValueError):
        stream.pack_coded_messages(["x"], rate="5/6")


def test_punct_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    abi = pkg.abi
    assert "ofdm_punct.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_punct.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = {x["name"]: x for x in report if x["source"] == "ofdm_punct.hip"}
    assert set(rows) == {"ofdm::punct_encode_kernel", "ofdm::punct_decode_kernel"}
    for name, x in rows.items():
        print(f"{name}: {x['VGPRs']} VGPRs, {x['LDS Size [bytes/block]']} B of static LDS, {x['Occupancy [waves/SIMD]']} waves per SIMD")
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), name
        assert x["VGPRs"] <= 128
    assert rows["ofdm::punct_decode_kernel"]["LDS Size [bytes/block]"] == 0
    src = (build_lib.CSRC / "ofdm_punct.hip").read_text()
    assert int(re.search(r"constexpr int PDEC_WAVES = (\d+);", src).group(1)) == abi.PUNCT_DECODE_WAVES
    # the coded link's translation unit keeps its three kernels
    assert len([x for x in report if x["source"] == "ofdm_code.hip"]) == 3


# ---------------------------------------------------------------- 2. the patterns' anchor
@pytest.mark.parametrize("rate,dfree", [("1/2", 10), ("2/3", 6), ("3/4", 5)])
def test_free_distance(pkg, rate, dfree):
    """the published free distances of the punctured 133/171 code"""
    got = pr.free_distance(rate)
    print(f"rate {rate}: free distance {got}")
    assert got == dfree
    # and with the rule's own bits: the lightest of all input patterns that span at most 12 steps, at every phase
    from ofdm_amd import stream
    s, period = stream.RATE_STEPS[rate], pr.PERIOD[rate]
    rows = []
    for mask in range(1, 1 << 12, 2):
        for phase in range(period):
            row = np.zeros(s, np.uint8)
            for k in range(12):
                row[2 * period + phase + k] = (mask >> k) & 1
            rows.append(row)
    u = np.array(rows)
    c = stream.conv_code_bits(u)[:, stream.puncture_index(rate)]
    assert int(c.sum(axis=1).min()) == dfree


# ---------------------------------------------------------------- 3. the rules against the plain implementation
def specials(eq, csi):
    """NaN, +-inf, +-0, values that clamp or overflow in eq, zeros and non-finite gains in csi, an all-zero row"""
    n = len(eq)
    eq[n - 1] = 0
    eq[n - 2, 3] = complex(np.nan, 1.0)
    eq[n - 2, 7] = complex(np.inf, -np.inf)
    eq[n - 2, 11] = complex(-0.0, 0.0)
    eq[n - 3, ::5] = complex(0.0, -0.0)
    eq[n - 4, 5] = complex(3e38, -3e38)
    eq[n - 4, 9] = complex(1e37, -1e37)
    if csi is not None:
        csi[n - 3] = 0
        csi[n - 4, ::3] = 0
        csi[n - 2, 20] = np.inf
        csi[n - 2, 21] = np.nan


@pytest.mark.parametrize("rate", PUNCTURED)
@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_rules_are_the_plain_implementation_bit_for_bit(pkg, rate, d):
    from ofdm_amd import stream
    n = 6
    info = pr.rand_info(d, n, 10 * d + pr.RATE_CODE[rate], rate)
    words = stream.conv_encode_rate(info, d, rate)
    assert words.shape == (n, 3 * d) and words.dtype == np.uint32
    assert [pr.encode_packet(row, d, rate) for row in info] == words.tolist()
    dirty = info.copy()
    dirty[:, -1] |= np.uint32((1 << (32 * pr.info_words(d, rate) - pr.info_bits(d, rate))) - 1)
    assert np.array_equal(stream.conv_encode_rate(dirty, d, rate), words)
    rng = np.random.default_rng(100 + d)
    eq = ideal_eq(words)
    eq = (eq + 0.5 * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))).astype(np.complex64)
    for weighted in (False, True):
        csi = rng.uniform(0, 4, (n, 48)).astype(np.float32) if weighted else None
        z = eq.copy()
        specials(z, csi)
        soft = stream.conv_soft_rate(z, csi, rate)
        assert soft.dtype == np.float32 and soft.shape == (n, 2 * pr.STEPS[rate] * d)
        out = stream.viterbi_decode_rate(soft, rate)
        assert out["info"].shape == (n, pr.info_words(d, rate)) and out["path"].dtype == np.float32
        stolen = np.ones(soft.shape[1], bool)
        stolen[(2 * pr.STEPS[rate] * np.arange(d)[:, None] + stream.puncture_index(rate)).ravel()] = False
        assert not soft[:, stolen].any() and not np.signbit(soft[:, stolen]).any() and stolen.sum() == (2 * pr.STEPS[rate] - 96) * d
        for i in range(n):
            want_soft = pr.soft_packet_rate(z[i], None if csi is None else csi[i], d, rate)
            assert np.array_equal(soft[i].view(np.uint32), want_soft.view(np.uint32)), (i, weighted)
            w, path = pr.decode_packet(want_soft)
            assert w == out["info"][i].tolist(), (i, weighted)
            assert np.float32(path) == out["path"][i]
            assert (np.float32(path).view(np.uint32) & 0x7fffffff) == (out["path"][i].view(np.uint32) & 0x7fffffff)
        print(f"rate {rate}, D = {d}, csi {'random' if weighted else 'None'}: {n} rows equal the plain implementation; "
              f"{int((out['info'] != info).any(axis=1).sum())} decoded wrong")
    for bad in (np.zeros((2, 2 * pr.STEPS[rate])), np.zeros((2, 96 if rate == "2/3" else 100), np.float32),
                np.zeros(2 * pr.STEPS[rate], np.float32)):
        with pytest.raises(ValueError):
            stream.viterbi_decode_rate(bad, rate)
    with pytest.raises(ValueError):
        stream.conv_encode_rate(np.zeros((2, pr.info_words(d, rate) + 1), np.uint32), d, rate)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("d", [1, 2, 15])
def test_noise_free_round_trip_at_every_rate(pkg, rate, d):
    from ofdm_amd import stream
    info = pr.rand_info(d, 12, 20 + d, rate)
    eq = ideal_eq(stream.conv_encode_rate(info, d, rate))
    out = stream.viterbi_decode_rate(stream.conv_soft_rate(eq, None, rate), rate)
    assert np.array_equal(out["info"], info)
    # every sent value agrees with its bit: the path metric is their sum, 2 S D fp32 additions of at most half an ulp of
    # the growing sum each
    assert np.allclose(out["path"], 96 * d / np.sqrt(2), rtol=2 * pr.STEPS[rate] * d * 2.0 ** -24, atol=0)


@pytest.mark.parametrize("d", [1, 2, 15])
def test_rate_one_half_is_the_coded_link(pkg, d):
    from ofdm_amd import stream
    n = 8
    info = cr.rand_info(d, n, 30 + d)
    words = stream.conv_encode(info, d)
    assert np.array_equal(stream.conv_encode_rate(info, d, "1/2"), words) and np.array_equal(stream.conv_encode_rate(info, d), words)
    rng = np.random.default_rng(31 + d)
    eq = ideal_eq(words)
    eq = (eq + 0.6 * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))).astype(np.complex64)
    csi = rng.uniform(0, 4, (n, 48)).astype(np.float32)
    specials(eq, csi)
    soft = stream.conv_soft(eq, csi)
    assert np.array_equal(stream.conv_soft_rate(eq, csi, "1/2").view(np.uint32), soft.view(np.uint32))
    want, got = stream.viterbi_decode(soft), stream.viterbi_decode_rate(stream.conv_soft_rate(eq, csi, "1/2"), "1/2")
    assert np.array_equal(got["info"], want["info"]) and np.array_equal(got["path"].view(np.uint32), want["path"].view(np.uint32))
    assert np.array_equal(stream.puncture_index("1/2"), np.arange(96))
    # the contracts that stay
    for bad in (np.zeros((2, 96)), np.zeros((2, 95), np.float32), np.zeros(96, np.float32)):
        with pytest.raises(ValueError):
            stream.viterbi_decode(bad)
    with pytest.raises(ValueError):
        stream.conv_soft(np.zeros((2, 47), np.complex64))


# ---------------------------------------------------------------- 4. argument errors come before any device work
def test_punct_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    err = lib.ofdm_last_error
    fake = 0x1000                                                     # never dereferenced: the call fails first
    enc = lambda rate=1, nd=2, info=fake, n=4, words=fake: lib.ofdm_punct_encode(None, rate, nd, info, n, words)
    for rate in (-1, 3, 100):
        assert enc(rate=rate, nd=0, info=None) == -1 and b"rate" in err()
    for rate in (0, 1, 2):
        for nd in (0, 16, -1):
            assert enc(rate=rate, nd=nd) == -1 and b"n_data" in err()
        assert enc(rate=rate, n=-1) == -1 and b"negative" in err()
        assert enc(rate=rate, info=None) == -1 and b"d_info is NULL" in err()
        assert enc(rate=rate, words=None) == -1 and b"d_words is NULL" in err()
        assert enc(rate=rate, info=fake + 2) == -1 and b"d_info must be 4-byte aligned" in err()
        assert enc(rate=rate, words=fake + 1) == -1 and b"d_words must be 4-byte aligned" in err()
        assert enc(rate=rate) == -1 and b"ctx" in err()
        # the order is the coded link's: n_data before n before the pointers
        assert enc(rate=rate, nd=0, n=-1, info=None) == -1 and b"n_data" in err()
        assert enc(rate=rate, n=-1, info=None) == -1 and b"negative" in err()

    dec = lambda rate=2, nd=2, eq=fake, w=None, cnt=None, n=4, info=fake, path=None: \
        lib.ofdm_punct_decode(None, rate, nd, eq, w, cnt, n, info, path)
    for rate in (-1, 3):
        assert dec(rate=rate, nd=0, eq=None) == -1 and b"rate" in err()
    for rate in (0, 1, 2):
        for nd in (0, 16):
            assert dec(rate=rate, nd=nd) == -1 and b"n_data" in err()
        assert dec(rate=rate, n=-1) == -1 and b"negative" in err()
        assert dec(rate=rate, eq=None) == -1 and b"d_eq is NULL" in err()
        assert dec(rate=rate, info=None) == -1 and b"d_info is NULL" in err()
        assert dec(rate=rate, eq=fake + 4) == -1 and b"d_eq must be 8-byte aligned" in err()
        assert dec(rate=rate, w=fake + 2) == -1 and b"d_csi" in err()
        assert dec(rate=rate, cnt=fake + 4) == -1 and b"d_count" in err()
        assert dec(rate=rate, info=fake + 2) == -1 and b"d_info must" in err()
        assert dec(rate=rate, path=fake + 2) == -1 and b"d_path" in err()
        assert dec(rate=rate, w=fake, cnt=fake, path=fake) == -1 and b"ctx" in err()
        assert dec(rate=rate, eq=None, info=None) == -1 and b"d_eq is NULL" in err()


def test_link_sweep_refuses_a_bad_rate_before_any_launch(pkg):
    from ofdm_amd import sweep

    class NoEngine:                                                   # any use of the engine would raise AttributeError
        pass
    for bad in ("5/6", "", 1, None):
        with pytest.raises(ValueError, match="rate"):
            sweep.link_sweep(NoEngine(), pr.rand_info(2, 4, 1, "3/4"), 2, 500, [20.0], code="conv", rate=bad)
    for rate in PUNCTURED:
        with pytest.raises(ValueError, match="code"):
            sweep.link_sweep(NoEngine(), pr.rand_info(2, 4, 1, rate), 2, 500, [20.0], rate=rate)
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--code", "conv", "--rate", "5/6"])
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--rate", "3/4"])
    assert sweep.LINK_COLUMNS[-1] == "bits" and sweep.LINK_CODE_COLUMNS == ("info_bits", "info_bit_err", "info_packet_err")


# ---------------------------------------------------------------- 5. what each rate costs
def test_what_each_rate_costs_on_the_four_tap_link(pkg):
    """Measured here at 16 dB: uncoded 13,888 of 576,000 (2.4e-2, the rate-3/4 packets' payload); information bit errors
    5,325 of 414,000 at rate 3/4 (1.3e-2), 1,560 of 366,000 at 2/3 (4.3e-3), 203 of 270,000 at 1/2 (7.5e-4)."""
    from ofdm_amd import stream
    ber, uncoded = {}, {}
    for rate in RATES:
        info = pr.rand_info(2, COSTS_PACKETS, COSTS_SEED + 7, rate)
        rng = np.random.default_rng(COSTS_SEED + 8)                  # the same channels and noise for every rate
        H = cr.model_channel(rng, COSTS_PACKETS, COSTS_PDP)
        payload = bits_of(stream.conv_encode_rate(info, 2, rate))
        z, g = cr.model_receive(rng, payload, H, COSTS_SNR_DB)
        unc = int((stream.slice_bits(z) != payload).sum())
        dec = stream.viterbi_decode_rate(stream.conv_soft_rate(z, g, rate), rate)["info"]
        err, ni = int(bits_of(dec ^ info).sum()), pr.info_bits(2, rate) * COSTS_PACKETS
        ber[rate], uncoded[rate] = err / ni, unc / payload.size
        print(f"rate {rate}, {COSTS_PACKETS} two-symbol packets, four taps, {COSTS_SNR_DB:g} dB: uncoded {unc} of {payload.size} "
              f"({unc / payload.size:.2g}); information bit errors {err} of {ni} ({err / ni:.2g})")
    assert min(uncoded.values()) > ber["3/4"] > ber["2/3"] > ber["1/2"] > 0
