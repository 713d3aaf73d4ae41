"""Self-describing coded packets (include/ofdm_mi355x_ppdu.h), the checks that need no GPU: the header, the binding and the
build of the new translation unit; the known answers of the scrambler, the CRC-32 and the header; what the header's checks
catch; the rules of stream.py against the plain second implementation of tests/ppdu_ref.py; the noise-free round trip; the
refusals; the argument checks of the two calls; and a noisy batch on the subcarrier-level model in which the FCS alone tells
the right packets from the wrong ones.  Each test prints its figures before it asserts.

Measured here (tests/code_ref.py's model: Rayleigh taps of profile 1, 0.5, 0.25, 0.125, complex noise, an LS estimate from
two training symbols, zero-forcing, |H|^2 weights; 900 three-symbol packets of mixed rates, seed 0x9D0, the first half at
5 dB and the second at 10 dB): per rate 1/2 / 2/3 / 3/4, header invalid 66 / 76 / 58, FCS failed 17 / 47 / 88, FCS
passed 216 / 177 / 154; no packet whose FCS passed differs from the sent one, and every packet whose FCS failed does.  One
packet (rate 1/2) has "bad service" alone: its decode errors lie in SERVICE bits 7..15, its FCS passes and its PSDU is the
sent one.  So "bad service implies that the PSDU differs" is not a property of this format -- the SERVICE bits are outside
the PSDU -- and the test asserts what is: a failed FCS means another PSDU, a passed FCS means the sent one, with or without
the SERVICE flag."""
import itertools
import json
import re
import subprocess
import zlib

import numpy as np
import pytest

import code_ref as cr
import ppdu_ref as ppr
from code_ref import bits_of, ideal_eq
from conftest import ROOT

RATES = ("1/2", "2/3", "3/4")
NOISY_PACKETS, NOISY_SEED, NOISY_PDP, NOISY_SNR_DB, NOISY_D = 900, 0x9D0, (1.0, 0.5, 0.25, 0.125), (5.0, 10.0), 3
STANDARD_SEQUENCE = ("00001110 11110010 11001001 00000010 00100110 00101110 10110110 00001100 11010100 11100111 10110100 "
                     "00101010 11111010 01010001 10111000 1111111").replace(" ", "")


def encode_ref(stream, bodies, rates, seeds, d):
    """the payload and info words of packets built from ppdu_ref's bits and the rate-taking encoder, one by one"""
    words, info = [], []
    for body, r, s in zip(bodies, rates, seeds):
        hb, db, _ = ppr.build(body, r, s, d)
        hw, dw = ppr.pack_words(hb), ppr.pack_words(db)
        words.append(np.concatenate([stream.conv_encode_rate(hw[None], 1, "1/2")[0],
                                     stream.conv_encode_rate(dw[None], d - 1, RATES[r])[0]]))
        info.append(np.concatenate([hw, dw, np.zeros(ppr.INFO_WORDS - 2 - len(dw), np.uint32)]))
    return np.array(words, np.uint32), np.array(info, np.uint32)


def psdu_rows(bodies):
    return np.array([ppr.psdu_words(b) for b in bodies], np.uint32).reshape(len(bodies), ppr.PSDU_WORDS)


# ---------------------------------------------------------------- 1. the header, the binding, the build
def test_ppdu_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.PPDU_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.PPDU_FUNCTIONS) == ["ofdm_ppdu_decode", "ofdm_ppdu_encode"]
    for k, v in vars(abi).items():
        if k.endswith("EXPORTS") or (k.endswith("_FUNCTIONS") and k != "PPDU_FUNCTIONS"):
            assert not set(names) & set(v), k
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_punct.h"' in h
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != abi.PPDU_HEADER.name:
            text = other.read_text()
            for word in abi.PPDU_FUNCTIONS + ("OFDM_PPDU_",):
                assert word not in text, (other.name, word)
    # the header says what the issue asks it to say
    for word in ("LSB-first octets", "tail-before-pad", "0x703DF9C0", "13,440", "26,880", "six blocks", "id 18", "id 20",
                 "RATE field of 0", "447,720"):
        assert word in h, word


def test_ppdu_constants_match_the_header(pkg, tmp_path):
    abi = pkg.abi
    from ofdm_amd import stream
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_ppdu.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d %d\\n", OFDM_PPDU_MIN_SYMBOLS, OFDM_PPDU_PSDU_WORDS, '
                   "OFDM_PPDU_INFO_WORDS, OFDM_PPDU_SERVICE_BITS, OFDM_PPDU_MIN_LENGTH, OFDM_PPDU_BAD_HEADER, "
                   "OFDM_PPDU_BAD_SERVICE, OFDM_PPDU_BAD_FCS); return 0; }\n")
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [abi.PPDU_MIN_SYMBOLS, abi.PPDU_PSDU_WORDS, abi.PPDU_INFO_WORDS, abi.PPDU_SERVICE_BITS, abi.PPDU_MIN_LENGTH,
                   abi.PPDU_BAD_HEADER, abi.PPDU_BAD_SERVICE, abi.PPDU_BAD_FCS] == [2, 31, 36, 16, 4, 1, 2, 4]
    assert got == [stream.PPDU_MIN_DATA_SYMBOLS, stream.PPDU_PSDU_WORDS, stream.PPDU_INFO_WORDS, stream.PPDU_SERVICE_BITS,
                   stream.PPDU_MIN_LENGTH, stream.PPDU_BAD_HEADER, stream.PPDU_BAD_SERVICE, stream.PPDU_BAD_FCS]
    # the issue's table of caps, and the rows' sizes
    table = {2: (3, 5, 6), 3: (9, 13, 15), 15: (81, 109, 123)}
    for d, caps in table.items():
        assert tuple(stream.ppdu_cap(d, r) for r in RATES) == tuple(abi.ppdu_cap(d, r) for r in RATES) == caps
        assert tuple(ppr.cap(d, r) for r in range(3)) == caps
    assert 4 * abi.PPDU_PSDU_WORDS >= 123 and abi.PPDU_INFO_WORDS >= 2 + abi.punct_info_words(14, "3/4")
    # the header's words lie in the data part's decision area: the region is the punctured kernel's at rate 2/3
    assert abi.ppdu_decode_lds_bytes(15) == 2 * 13440 == 26880 == abi.punct_decode_lds_bytes(15, "2/3")
    assert 160 * 1024 // abi.ppdu_decode_lds_bytes(15) == 6
    assert abi.ppdu_decode_lds_bytes(2) == 2 * (96 * 8 + 96 * 4) and abi.ppdu_decode_lds_bytes(3) == 2 * (144 * 8 + 192 * 4)


def test_ppdu_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    abi = pkg.abi
    assert "ofdm_ppdu.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_ppdu.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = {x["name"]: x for x in report if x["source"] == "ofdm_ppdu.hip"}
    assert set(rows) == {"ofdm::ppdu_info_kernel", "ofdm::ppdu_encode_kernel", "ofdm::ppdu_decode_kernel"}
    for name, x in rows.items():
        print(f"{name}: {x['VGPRs']} VGPRs, {x['LDS Size [bytes/block]']} B of static LDS, {x['Occupancy [waves/SIMD]']} waves per SIMD")
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), name
        assert x["VGPRs"] <= 128
    assert rows["ofdm::ppdu_decode_kernel"]["LDS Size [bytes/block]"] == 0
    src = (build_lib.CSRC / "ofdm_ppdu.hip").read_text()
    assert int(re.search(r"constexpr int PPDU_WAVES = (\d+);", src).group(1)) == abi.PPDU_DECODE_WAVES
    # the older translation units keep their kernels
    assert len([x for x in report if x["source"] == "ofdm_code.hip"]) == 3
    assert len([x for x in report if x["source"] == "ofdm_punct.hip"]) == 2


# ---------------------------------------------------------------- 2. known answers
def test_known_answers(pkg):
    from ofdm_amd import stream
    seq = "".join(str(int(b)) for b in stream.scramble_sequence(0b1111111, 127))
    print(f"seed 1111111: {seq[:32]} ..")
    assert seq == STANDARD_SEQUENCE and len(STANDARD_SEQUENCE) == 127
    assert "".join(str(int(b)) for b in stream.scramble_sequence(0b1011101, 24)) == "011011000001100110101001"
    assert stream.fcs32(b"123456789") == 0xCBF43926 == zlib.crc32(b"123456789")
    head = stream.ppdu_header("3/4", 123)
    print(f"header (3/4, 123): {int(head[0]):#010x} {int(head[1]):#010x}")
    assert head.dtype == np.uint32 and head.tolist() == [0x703DF9C0, 0]
    assert stream.ppdu_header_check(head) == (True, 2, 123) == stream.ppdu_header_check(head, 15)
    assert stream.ppdu_header_check(head, 14) == (False, -1, 0)       # 123 bytes need 15 symbols
    assert stream.ppdu_header(2, 123).tolist() == head.tolist()
    # the same from the plain implementation
    assert "".join(map(str, ppr.scrambler(127, 127))) == STANDARD_SEQUENCE
    assert ppr.pack_words(ppr.header_bits(7, 123)).tolist() == [0x703DF9C0, 0]
    assert stream.crc8([1, 0, 1, 1, 0, 0, 1] * 3) == ppr.crc8([1, 0, 1, 1, 0, 0, 1] * 3)


def test_scrambler_period_and_rotations(pkg):
    from ofdm_amd import stream
    ones = stream.scramble_sequence(127, 3 * 127)
    assert np.array_equal(ones[:127], ones[127:254]) and np.array_equal(ones[:127], ones[254:])
    assert not any(np.array_equal(ones[:127], np.roll(ones[:127], k)) for k in range(1, 127))      # no shorter period
    shifts = set()
    for seed in range(1, 128):
        q = stream.scramble_sequence(seed, 300)
        assert q.tolist() == ppr.scrambler(seed, 300)
        k = [k for k in range(127) if np.array_equal(np.roll(ones[:127], -k), q[:127])]
        assert len(k) == 1, seed
        shifts.add(k[0])
        # what the receiver relies on: bits 0..6 are the state from which bit 7 on follows
        state = int("".join(map(str, q[:7])), 2)
        assert np.array_equal(q[7:], stream.scramble_sequence(state, 293))
    assert shifts == set(range(127))
    for bad in (0, 128, -1, 1.5):
        with pytest.raises(ValueError):
            stream.scramble_sequence(bad, 10)


def test_fcs32_is_zlib(pkg):
    from ofdm_amd import stream
    rng = np.random.default_rng(32)
    for k in range(120):
        body = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
        assert stream.fcs32(body) == zlib.crc32(body), k


# ---------------------------------------------------------------- 3. what the header's checks catch
def test_no_flip_of_up_to_three_header_bits_is_valid(pkg):
    from ofdm_amd import stream
    total = 0
    for rate, length in (("1/2", 4), ("3/4", 123), ("1/2", 81), ("2/3", 57)):
        head = stream.ppdu_header(rate, length)
        base = (int(head[0]) << 32) | int(head[1])
        assert stream.ppdu_header_check(head)[0] and ppr.parse_header(bits_of(head)[:42]) == (True, RATES.index(rate), length)
        flips = [sum(1 << (63 - b) for b in c) for k in (1, 2, 3) for c in itertools.combinations(range(42), k)]
        v = np.array([base ^ f for f in flips], np.uint64)
        words = np.stack([(v >> np.uint64(32)).astype(np.uint32), (v & np.uint64(0xffffffff)).astype(np.uint32)], axis=1)
        valid, r, ln = stream.ppdu_header_check(words)                # without a cap: the widest check
        print(f"header ({rate}, {length}): {len(flips)} flips of 1 to 3 bits, {int(valid.sum())} valid")
        assert len(flips) == 42 + 861 + 11480 and not valid.any() and (r == -1).all() and (ln == 0).all()
        for row in words[::997]:                                      # and the plain implementation agrees
            assert ppr.parse_header(bits_of(row)[:42]) == (False, -1, 0)
        total += len(flips)
    assert total == 4 * 12383
    # a flip in the six unused bits behind the 42 is no header bit: word 1's low 22 bits are not the rule's business,
    # but bits 26..41 are
    head = stream.ppdu_header("2/3", 20)
    assert not stream.ppdu_header_check(np.array([head[0], 1 << 22], np.uint32))[0]


# ---------------------------------------------------------------- 4. the rules against the plain implementation
@pytest.mark.parametrize("d", [2, 3, 15])
def test_encode_is_the_stated_composition(pkg, d):
    from ofdm_amd import stream
    n = 24
    bodies, rates, lengths, seeds = ppr.random_packets(d, n, 50 + d)
    want_words, want_info = encode_ref(stream, bodies, rates, seeds, d)
    rng = np.random.default_rng(d)
    junk = rng.integers(0, 1 << 32, (n, ppr.PSDU_WORDS), dtype=np.uint64).astype(np.uint32)
    psdu = psdu_rows(bodies)
    by = junk.astype(">u4").view(np.uint8).reshape(n, -1).copy()      # junk in the FCS place and past LENGTH
    for row, clean, k in zip(by, psdu.astype(">u4").view(np.uint8).reshape(n, -1), lengths):
        row[:k - 4] = clean[:k - 4]
    dirty = by.view(">u4").astype(np.uint32)
    for rows in (psdu, dirty):
        words, info = stream.ppdu_encode(rows, lengths, rates, seeds, d)
        assert words.shape == (n, 3 * d) and info.shape == (n, 36) and words.dtype == info.dtype == np.uint32
        assert np.array_equal(words, want_words) and np.array_equal(info, want_info)
    assert np.array_equal(stream.ppdu_encode(psdu, lengths, [RATES[r] for r in rates], seeds, d)[0], want_words)
    sent = stream.ppdu_fill(dirty, lengths)
    for row, body in zip(sent, bodies):
        assert row.tolist() == ppr.psdu_words(body + zlib.crc32(body).to_bytes(4, "big")).tolist()
    # the parse of the plain implementation takes the info words apart again
    for row, body, r, k, s in zip(want_info, bodies, rates, lengths, seeds):
        assert ppr.parse_header(bits_of(row[:2])[:42], d) == (True, r, k)
        status, seed, got = ppr.parse_data(bits_of(row[2:])[:ppr.data_bits(d, r)], k)
        assert (status, seed, got[:-4]) == (0, s, body)
    print(f"D = {d}: {n} packets equal the composition of the header's and the data part's encodes")


@pytest.mark.parametrize("d", [2, 3, 15])
def test_noise_free_round_trip(pkg, d):
    from ofdm_amd import stream
    cases = [(r, k) for r in range(3) for k in (4, ppr.cap(d, r)) if ppr.cap(d, r) >= 4]      # D = 2 holds no rate 1/2
    assert len(cases) == (4 if d == 2 else 6)
    rates = [r for r, _ in cases]
    lengths = [k for _, k in cases]
    seeds = list(range(1, 1 + len(cases)))
    if d == 3:                                                        # all 127 seeds at one shape
        rates, lengths, seeds = rates + [1] * 127, lengths + [11] * 127, seeds + list(range(1, 128))
    bodies = ppr.random_packets(d, len(rates), 70 + d, rates, lengths)[0]
    words, _ = stream.ppdu_encode(psdu_rows(bodies), lengths, rates, seeds, d)
    out = stream.ppdu_decode(ideal_eq(words))
    print(f"D = {d}: {len(rates)} packets, statuses {sorted(set(out['status'].tolist()))}, path metrics "
          f"{out['path'].min(axis=0)} .. {out['path'].max(axis=0)}")
    assert not out["status"].any()
    assert out["rate"].tolist() == rates and out["length"].tolist() == lengths and out["seed"].tolist() == seeds
    for row, body in zip(out["psdu"], bodies):
        assert row.tolist() == ppr.psdu_words(body + zlib.crc32(body).to_bytes(4, "big")).tolist()
    assert out["psdu"].shape == (len(rates), 31) and out["path"].shape == (len(rates), 2) and out["path"].dtype == np.float32
    for key in ("status", "rate", "length", "seed"):
        assert out[key].dtype == np.int32 and out[key].shape == (len(rates),)


def test_decode_statuses(pkg):
    """a header that names too long a LENGTH, seven zero state bits, a broken SERVICE field and a broken FCS"""
    from ofdm_amd import stream
    d = 3
    body = b"abcde"
    hb, db, _ = ppr.build(body, 1, 93, d)
    k = ppr.data_bits(d, 1)

    def decode(header_bits, data):
        words = np.concatenate([stream.conv_encode_rate(ppr.pack_words(header_bits)[None], 1, "1/2")[0],
                                stream.conv_encode_rate(ppr.pack_words(data)[None], d - 1, "2/3")[0]])
        out = stream.ppdu_decode(ideal_eq(words[None]))
        return {key: v[0] for key, v in out.items()}
    ok = decode(hb, db)
    assert (ok["status"], ok["rate"], ok["length"], ok["seed"]) == (0, 1, 9, 93)
    long_ = decode(ppr.header_bits(6, ppr.cap(d, 1) + 1), db)
    assert (long_["status"], long_["rate"], long_["length"], long_["seed"]) == (1, -1, 0, 0)
    assert not long_["psdu"].any() and long_["path"][1] == 0 and long_["path"][0] > 0
    zeros = decode(hb, [0] * 7 + db[7:])
    assert zeros["status"] & 2 and zeros["seed"] == 0 and zeros["rate"] == 1 and zeros["length"] == 9
    assert zeros["psdu"].tolist() == ppr.pack_words(([0] * 7 + db[7:])[16:16 + 72], 31).tolist()      # nothing is descrambled
    service = decode(hb, db[:9] + [db[9] ^ 1] + db[10:])
    assert service["status"] == 2 and service["seed"] == 93 and service["psdu"].tolist() == ok["psdu"].tolist()
    fcs = decode(hb, db[:20] + [db[20] ^ 1] + db[21:])
    assert fcs["status"] == 4 and fcs["seed"] == 93 and fcs["psdu"].tolist() != ok["psdu"].tolist()
    pad = decode(hb, db[:k - 1] + [db[k - 1] ^ 1])                     # the pad is not checked: it is not the PSDU
    assert pad["status"] == 0 and pad["psdu"].tolist() == ok["psdu"].tolist()
    # and the plain parse says the same
    assert ppr.parse_data([0] * 7 + db[7:], 9)[:2] == (zeros["status"], 0)
    assert ppr.parse_data(db[:9] + [db[9] ^ 1] + db[10:], 9)[:2] == (2, 93)
    assert ppr.parse_data(db[:20] + [db[20] ^ 1] + db[21:], 9)[:2] == (4, 93)


def test_refusals(pkg):
    from ofdm_amd import stream
    psdu = np.zeros((1, 31), np.uint32)
    enc = lambda length=8, rate="2/3", seed=1, d=3: stream.ppdu_encode(psdu, [length], [rate], [seed], d)
    enc()
    for kw in (dict(length=3), dict(length=14), dict(length=0), dict(length=-1), dict(d=2, rate="1/2", length=4), dict(d=1),
               dict(d=16), dict(d=0), dict(seed=0), dict(seed=128), dict(rate="5/6"), dict(rate=3), dict(rate=-1),
               dict(rate=None)):
        with pytest.raises(ValueError):
            enc(**kw)
    enc(length=13), enc(length=4), enc(d=2, rate="2/3", length=5), enc(d=2, rate="3/4", length=6), enc(seed=127)
    with pytest.raises(ValueError):
        stream.ppdu_encode(np.zeros((1, 30), np.uint32), [8], [1], [1], 3)
    with pytest.raises(ValueError):
        stream.ppdu_encode(psdu, [8, 8], [1], [1], 3)
    for bad in (np.zeros((2, 48), np.complex64), np.zeros((2, 48 * 16), np.complex64), np.zeros((2, 100), np.complex64)):
        with pytest.raises(ValueError):
            stream.ppdu_decode(bad)
    for d, rate in ((1, "1/2"), (16, "3/4"), (3, "5/6")):
        with pytest.raises(ValueError):
            stream.ppdu_cap(d, rate)
    # strict=False is the device encoder's rule for a refused packet: a header no receiver takes, zero data
    words, info = stream.ppdu_encode(np.ones((3, 31), np.uint32), [3, 8, 8], [1, 5, 1], [1, 1, 0], 3, strict=False)
    assert (info[:, 0] == info[0, 0]).all() and info[0, 0] >> 28 == 0 and not info[:, 1:].any() and not words[:, 3:].any()
    assert info[0, :2].tolist() == ppr.pack_words(ppr.header_bits(0, 0)).tolist()
    out = stream.ppdu_decode(ideal_eq(words))
    assert out["status"].tolist() == [1, 1, 1] and out["rate"].tolist() == [-1] * 3
    # texts into packets
    psdu, lengths, d = stream.pack_ppdu_messages(["Hello", "x" * 11], None, "3/4")
    assert d == 3 and lengths.tolist() == [9, 15] and psdu.shape == (2, 31)
    assert bytes(np.packbits(bits_of(psdu)[0, :40])) == b"Hello" and not bits_of(psdu)[0, 40:].any()
    assert stream.pack_ppdu_messages(["x" * 119], None, "3/4")[2] == 15 and stream.pack_ppdu_messages(["x"], 7, "1/2")[2] == 7
    for texts, nd, rate in ((["x" * 120], None, "3/4"), (["x" * 12], 3, "3/4"), (["x"], 2, "1/2"), (["x"], 3, "5/6")):
        with pytest.raises(ValueError):
            stream.pack_ppdu_messages(texts, nd, rate)


# ---------------------------------------------------------------- 5. argument errors come before any device work
def test_ppdu_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    err = lib.ofdm_last_error
    fake = 0x1000                                                     # never dereferenced: the call fails first
    enc = lambda nd=3, psdu=fake, ln=fake, rate=fake, seed=fake, n=4, info=fake, words=fake: \
        lib.ofdm_ppdu_encode(None, nd, psdu, ln, rate, seed, n, info, words)
    for nd in (1, 0, 16, -1):
        assert enc(nd=nd, n=-1, psdu=None) == -1 and b"n_data" in err()
    assert enc(n=-1, psdu=None) == -1 and b"negative" in err()
    for name in ("psdu", "ln", "rate", "seed", "info", "words"):
        text = {"ln": b"d_len"}.get(name, b"d_" + name.encode())
        assert enc(**{name: None}) == -1 and text + b" is NULL" in err(), name
        assert enc(**{name: fake + 2}) == -1 and text + b" must be 4-byte aligned" in err(), name
    assert enc(psdu=None, words=fake + 1) == -1 and b"d_psdu is NULL" in err()            # NULL before alignment
    assert enc() == -1 and b"ctx" in err()
    assert enc(n=0) == -1 and b"ctx" in err()

    dec = lambda nd=3, eq=fake, w=None, cnt=None, n=4, meta=fake, psdu=fake, path=None: \
        lib.ofdm_ppdu_decode(None, nd, eq, w, cnt, n, meta, psdu, path)
    for nd in (1, 16):
        assert dec(nd=nd, n=-1) == -1 and b"n_data" in err()
    assert dec(n=-1, eq=None) == -1 and b"negative" in err()
    assert dec(eq=None, meta=None) == -1 and b"d_eq is NULL" in err()
    assert dec(meta=None) == -1 and b"d_meta is NULL" in err()
    assert dec(psdu=None) == -1 and b"d_psdu is NULL" in err()
    assert dec(eq=fake + 4) == -1 and b"d_eq must be 8-byte aligned" in err()
    assert dec(w=fake + 2) == -1 and b"d_csi" in err()
    assert dec(cnt=fake + 4) == -1 and b"d_count" in err()
    assert dec(meta=fake + 8) == -1 and b"d_meta must be 16-byte aligned" in err()
    assert dec(psdu=fake + 2) == -1 and b"d_psdu must" in err()
    assert dec(path=fake + 2) == -1 and b"d_path" in err()
    assert dec(w=fake, cnt=fake, path=fake) == -1 and b"ctx" in err()


def test_link_sweep_refuses_bad_ppdu_arguments_before_any_launch(pkg):
    from ofdm_amd import sweep

    class NoEngine:                                                   # any use of the engine would raise AttributeError
        pass
    psdu = np.zeros((6, 31), np.uint32)
    for kw in (dict(rate="5/6"), dict(rate=["1/2"] * 5), dict(rate="mixed", lengths=[4] * 5), dict(rate="3/4", lengths=[16] * 6),
               dict(rate="1/2", lengths=[3] * 6), dict(rate=None)):
        with pytest.raises(ValueError):
            sweep.link_sweep(NoEngine(), psdu, 3, 500, [20.0], code="ppdu", **kw)
    with pytest.raises(ValueError):
        sweep.link_sweep(NoEngine(), psdu, 2, 500, [20.0], code="ppdu", rate="1/2")      # D = 2 holds no rate-1/2 packet
    with pytest.raises(ValueError):
        sweep.link_sweep(NoEngine(), psdu[:, :30], 3, 500, [20.0], code="ppdu", rate="mixed")
    with pytest.raises(ValueError):
        sweep.link_sweep(NoEngine(), psdu, 3, 500, [20.0], code="conv", rate="mixed")
    with pytest.raises(ValueError):
        sweep.link_sweep(NoEngine(), psdu, 3, 500, [20.0], code="conv", lengths=[4] * 6)
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--code", "conv", "--rate", "mixed"])
    assert sweep.LINK_PPDU_COLUMNS == tuple(f"{name}_{r}" for r in ("1of2", "2of3", "3of4") for name in
                                            ("matched", "header_ok", "fcs_ok", "false_accept", "psdu_bit_err"))


# ---------------------------------------------------------------- 6. the FCS tells right from wrong
def test_noisy_batch_the_fcs_tells_right_from_wrong(pkg):
    from ofdm_amd import stream
    n, d = NOISY_PACKETS, NOISY_D
    bodies, rates, lengths, seeds = ppr.random_packets(d, n, NOISY_SEED)
    words, _ = stream.ppdu_encode(psdu_rows(bodies), lengths, rates, seeds, d)
    sent = np.array([ppr.psdu_words(b + zlib.crc32(b).to_bytes(4, "big")) for b in bodies], np.uint32)
    rng = np.random.default_rng(NOISY_SEED + 1)
    H = cr.model_channel(rng, n, NOISY_PDP)
    payload = bits_of(words)
    half = n // 2
    z = np.zeros((n, 48 * d), np.complex128)
    g = np.zeros((n, 48))
    for rows, snr in ((slice(0, half), NOISY_SNR_DB[0]), (slice(half, n), NOISY_SNR_DB[1])):
        z[rows], g[rows] = cr.model_receive(rng, payload[rows], H[rows], snr)
    out = stream.ppdu_decode(z.astype(np.complex64), g.astype(np.float32))
    rates = np.array(rates)
    same = (out["psdu"] == sent).all(axis=1)
    bad_header = out["status"] == 1
    passed = out["status"] == 0
    failed = (out["status"] & 4) != 0                                 # with or without the SERVICE flag
    service_alone = out["status"] == 2
    for r in range(3):
        m = rates == r
        print(f"rate {RATES[r]}: {int(m.sum())} packets, header invalid {int((bad_header & m).sum())}, FCS failed "
              f"{int((failed & m).sum())}, bad service alone {int((service_alone & m).sum())}, FCS passed "
              f"{int((passed & m).sum())}; header valid but another rate or LENGTH "
              f"{int((~bad_header & m & ((out['rate'] != rates) | (out['length'] != lengths))).sum())}")
        assert (bad_header & m).sum() >= 10 and (failed & m).sum() >= 10 and (passed & m).sum() >= 10
    print(f"FCS passed and PSDU differs: {int((passed & ~same).sum())}; FCS failed and PSDU equal: {int((failed & same).sum())}; "
          f"bad service alone and PSDU equal: {int((service_alone & same).sum())} of {int(service_alone.sum())}")
    assert (bad_header | failed | service_alone | passed).all()
    assert same[passed].all()
    assert not same[failed].any()
    # an invalid header leaves a zero PSDU (which is the sent one for an empty body: LENGTH 4, crc32 of nothing is 0)
    assert not out["psdu"][bad_header].any() and (out["rate"][bad_header] == -1).all()
    # bad service without a failed FCS: the errors lie in the SERVICE bits, which are no part of the PSDU
    assert same[service_alone].all()
    assert np.array_equal(out["rate"][passed], rates[passed]) and np.array_equal(out["length"][passed], np.array(lengths)[passed])
    assert np.array_equal(out["seed"][passed], np.array(seeds)[passed])
