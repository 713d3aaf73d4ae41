"""The coded link (include/ofdm_mi355x_code.h), the checks that need no GPU: the header, the binding and the build of the
new translation unit; the argument checks; the encoder's facts; the noise-free round trip; the code's guaranteed
correction; stream.viterbi_decode against the plain second implementation of tests/code_ref.py, bit for bit; and what the
code is worth on the subcarrier-level model.  Each test prints its figures before it asserts.

Measured here (tests/code_ref.py's model: Rayleigh taps of profile 1, 0.5, 0.25, 0.125 at 40 MS/s, complex noise, an LS
estimate from two training symbols, zero-forcing, unit noise-free subcarrier power; 2,000 two-symbol packets, seed 0xC0DE):
at 20 dB 3,249 uncoded errors of 384,000 bits (8.5e-3) against 0 information bit errors of 180,000 with |H|^2 weights, 27
with sign-only input and 430 with unweighted soft values; at 6 dB AWGN 24 information bit errors with the precoding
against 496 without (the XOR's max-log value on the second bit)."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import code_ref as cr
from code_ref import bits_of, ideal_eq, rand_info
from conftest import ROOT

PAYS_PACKETS, PAYS_SEED, PAYS_PDP = 2000, 0xC0DE, (1.0, 0.5, 0.25, 0.125)


# ---------------------------------------------------------------- 1. the header, the binding, the build
def test_code_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.CODE_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int(?:64_t)?\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.CODE_FUNCTIONS) == ["ofdm_code_decode", "ofdm_code_encode", "ofdm_stream_csi"]
    for k, v in vars(abi).items():
        if k.endswith("EXPORTS") or k == "DIVERSITY_FUNCTIONS":
            assert not set(names) & set(v), k
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n) and re.search(rf"\bT {n}\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    assert '#include "ofdm_mi355x_diversity.h"' in h
    for word in ("scrambler", "puncturing", "SIGNAL field", "interleaving across packets", "ofdm_receive_captures",
                 "frame-mode", "hard-decision"):
        assert word in h, word
    new = abi.CODE_FUNCTIONS + ("OFDM_K_CODE_ENCODE", "OFDM_K_STREAM_CSI", "OFDM_K_CODE_DECODE", "OFDM_CODE_")
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != abi.CODE_HEADER.name:
            text = other.read_text()
            for word in new:
                assert word not in text, (other.name, word)


def test_code_constants_match_the_header(pkg, tmp_path):
    abi = pkg.abi
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_code.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d %d %d %d\\n", OFDM_K_CODE_ENCODE, OFDM_K_STREAM_CSI, '
                   "OFDM_K_CODE_DECODE, OFDM_K_STREAM_DECODE_DIV, OFDM_CODE_TAIL_BITS, OFDM_CODE_MAX_DATA_SYMBOLS, "
                   "OFDM_CODE_INFO_BITS(2), OFDM_CODE_INFO_WORDS(1), OFDM_CODE_INFO_WORDS(2), OFDM_CODE_INFO_WORDS(15)); "
                   "return 0; }\n")
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [abi.K_CODE_ENCODE, abi.K_STREAM_CSI, abi.K_CODE_DECODE, abi.K_STREAM_DECODE_DIV, abi.CODE_TAIL_BITS,
                   abi.LONG_MAX_DATA_SYMBOLS, abi.code_info_bits(2), abi.code_info_words(1), abi.code_info_words(2),
                   abi.code_info_words(15)]
    assert got == [18, 19, 20, 17, 6, 15, 90, 2, 3, 23]
    from ofdm_amd import stream
    assert [stream.INFO_BITS(d) for d in (1, 2, 15)] == [42, 90, 714]
    assert [stream.INFO_WORDS(d) for d in (1, 2, 15)] == [2, 3, 23]
    for bad in (0, 16, 1.5):
        with pytest.raises(ValueError):
            stream.INFO_BITS(bad)
    ctx_h = (ROOT / "ieee-802.11-ofdm-qpsk-simulator_amd" / "csrc" / "ofdm_ctx.h").read_text()
    assert re.search(r"K_CODE_ENCODE = 18, K_STREAM_CSI = 19, K_CODE_DECODE = 20, NK = 21", ctx_h)


def test_code_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    abi = pkg.abi
    assert "ofdm_code.hip" in build_lib.SOURCES and build_lib.SOURCE_FLAGS["ofdm_code.hip"] == []
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    rows = {x["name"]: x for x in report if x["source"] == "ofdm_code.hip"}
    assert set(rows) == {"ofdm::code_encode_kernel", "ofdm::stream_csi_kernel", "ofdm::code_decode_kernel"}
    for name, x in rows.items():
        print(f"{name}: {x['VGPRs']} VGPRs, {x['LDS Size [bytes/block]']} B of static LDS, {x['Occupancy [waves/SIMD]']} waves per SIMD")
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), name
        assert x["VGPRs"] <= 128
    # the decode kernel: no static LDS; dynamic LDS per wave 96 D floats and 48 D 64-bit words, 11.25 KiB at D = 15,
    # and CODE_DECODE_WAVES waves per block so that several blocks fit a CU's 160 KiB at D = 15
    assert rows["ofdm::code_decode_kernel"]["LDS Size [bytes/block]"] == 0
    src = (build_lib.CSRC / "ofdm_code.hip").read_text()
    assert int(re.search(r"constexpr int CDEC_WAVES = (\d+);", src).group(1)) == abi.CODE_DECODE_WAVES
    for d in (1, 2, 15):
        assert abi.code_decode_lds_bytes(d) == abi.CODE_DECODE_WAVES * (96 * d * 4 + 48 * d * 8)
    assert abi.code_decode_lds_bytes(15) // abi.CODE_DECODE_WAVES == 11520 == int(11.25 * 1024)
    assert 160 * 1024 // abi.code_decode_lds_bytes(15) >= 3 and abi.code_decode_lds_bytes(15) <= 64 * 1024
    # the gains kernel: two staging planes of 276 floats and a frame of 2 x 128 per wave, four waves, 64 twiddles
    assert rows["ofdm::stream_csi_kernel"]["LDS Size [bytes/block]"] == 4 * (2 * 276 + 2 * 128) * 4 + 64 * 8


# ---------------------------------------------------------------- 2. argument errors come before any device work
def test_code_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    err = lib.ofdm_last_error
    fake = 0x1000                                                     # never dereferenced: the call fails first
    enc = lambda nd=2, info=fake, n=4, words=fake: lib.ofdm_code_encode(None, nd, info, n, words)
    for nd in (0, 16, -1):
        assert enc(nd=nd) == -1 and b"n_data" in err()
    assert enc(n=-1) == -1 and b"negative" in err()
    assert enc(info=None) == -1 and b"d_info is NULL" in err()
    assert enc(words=None) == -1 and b"d_words is NULL" in err()
    assert enc(info=fake + 2) == -1 and b"d_info must be 4-byte aligned" in err()
    assert enc(words=fake + 1) == -1 and b"d_words must be 4-byte aligned" in err()
    assert enc() == -1 and b"ctx" in err()

    def csi(ptrs=(fake,), nb=1, n=100, pk=fake, cnt=fake, mp=4, out=fake, table=True):
        tab = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if table else None
        return lib.ofdm_stream_csi(None, tab, nb, n, pk, cnt, mp, out)
    for nb in (0, 5, -1):
        assert csi((fake,) * 4, nb) == -1 and b"n_branches" in err()
    assert csi(n=-1) == -1 and b"n_samples" in err()
    assert csi(mp=-1) == -1 and b"max_packets" in err()
    assert csi(table=False) == -1 and b"d_branches is NULL" in err()
    assert csi((fake, None), 2) == -1 and b"d_branches[1] is NULL" in err()
    assert csi((fake, fake + 4), 2) == -1 and b"d_branches[1] must be 8-byte aligned" in err()
    assert csi(cnt=None) == -1 and b"d_count is NULL" in err()
    assert csi(cnt=fake + 4) == -1 and b"d_count" in err()
    assert csi(pk=None) == -1 and b"d_packets is NULL" in err()
    assert csi(out=None) == -1 and b"d_csi is NULL" in err()
    assert csi(pk=fake + 4) == -1 and b"d_packets" in err()
    assert csi(out=fake + 2) == -1 and b"d_csi" in err()
    assert csi((fake, fake + 8, fake + 16, fake + 24), 4) == -1 and b"ctx" in err()

    dec = lambda nd=2, eq=fake, w=None, cnt=None, n=4, info=fake, path=None: lib.ofdm_code_decode(None, nd, eq, w, cnt, n, info, path)
    for nd in (0, 16):
        assert dec(nd=nd) == -1 and b"n_data" in err()
    assert dec(n=-1) == -1 and b"negative" in err()
    assert dec(eq=None) == -1 and b"d_eq is NULL" in err()
    assert dec(info=None) == -1 and b"d_info is NULL" in err()
    assert dec(eq=fake + 4) == -1 and b"d_eq must be 8-byte aligned" in err()
    assert dec(w=fake + 2) == -1 and b"d_csi" in err()
    assert dec(cnt=fake + 4) == -1 and b"d_count" in err()
    assert dec(info=fake + 2) == -1 and b"d_info must" in err()
    assert dec(path=fake + 2) == -1 and b"d_path" in err()
    assert dec(w=fake, cnt=fake, path=fake) == -1 and b"ctx" in err()


def test_link_sweep_refuses_a_bad_code_before_any_launch(pkg):
    from ofdm_amd import stream, sweep

    class NoEngine:                                                   # any use of the engine would raise AttributeError
        pass
    for bad in ("viterbi", "", 1):
        with pytest.raises(ValueError, match="code"):
            sweep.link_sweep(NoEngine(), rand_info(2, 4, 1), 2, 500, [20.0], code=bad)
    with pytest.raises(SystemExit):
        sweep.link_main(["--packets", "4", "--code", "turbo"])
    assert sweep.LINK_COLUMNS[-1] == "bits" and sweep.LINK_CODE_COLUMNS == ("info_bits", "info_bit_err", "info_packet_err")
    # texts into information bits: D from 48 D - 6 >= 8 x length
    words, d = stream.pack_coded_messages(["Hello", "x" * 11])
    assert d == 2 and words.shape == (2, 3) and words.dtype == np.uint32
    assert bytes(np.packbits(bits_of(words)[0, :88])) == b"Hello" + b" " * 6 and not bits_of(words)[:, 88:].any()
    assert stream.pack_coded_messages(["x" * 5])[1] == 1 and stream.pack_coded_messages(["x" * 6])[1] == 2
    assert stream.pack_coded_messages(["x" * 89])[1] == 15 and stream.pack_coded_messages([], 3)[0].shape == (0, 5)
    for bad in (["x" * 90], ):
        with pytest.raises(ValueError):
            stream.pack_coded_messages(bad)
    with pytest.raises(ValueError):
        stream.pack_coded_messages(["x" * 12], 2)


# ---------------------------------------------------------------- 3. the encoder's facts
def test_impulse_response_linearity_and_shift_invariance(pkg):
    from ofdm_amd import stream
    u = np.zeros((1, 48), np.uint8)
    u[0, 0] = 1
    c = stream.conv_code_bits(u)[0]
    assert c[0:14:2].tolist() == [1, 0, 1, 1, 0, 1, 1] and c[1:14:2].tolist() == [1, 1, 1, 1, 0, 0, 1]
    assert int(c.sum()) == 10 and not c[14:].any()
    assert cr.code_bits(u[0].tolist()) == c.tolist()
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 2, (2, 5, 90), dtype=np.uint8)
    assert np.array_equal(stream.conv_code_bits(a ^ b), stream.conv_code_bits(a) ^ stream.conv_code_bits(b))
    shifted = np.concatenate([np.zeros((5, 7), np.uint8), a], axis=1)
    assert np.array_equal(stream.conv_code_bits(shifted)[:, 14:], stream.conv_code_bits(a))
    for row in a[:2]:
        assert cr.code_bits(row.tolist()) == stream.conv_code_bits(row[None])[0].tolist()


def test_interleaver_and_precoding(pkg):
    from ofdm_amd import stream
    j = stream.interleave_index()
    assert sorted(j.tolist()) == list(range(96))
    assert all(int(j[k]) == 6 * (k % 16) + k // 16 == cr.interleave(k) for k in range(96))
    assert j[:3].tolist() == [0, 6, 12] and j[16] == 1 and j[95] == 95
    for d in (1, 2, 3, 15):
        info = rand_info(d, 6, 10 + d)
        words = stream.conv_encode(info, d)
        assert words.shape == (6, 3 * d) and words.dtype == np.uint32
        assert [cr.encode_packet(row, d) for row in info] == words.tolist()
        raw = stream.conv_encode(info, d, precode=False)
        assert [cr.encode_packet(row, d, precode=False) for row in info] == raw.tolist()
        # through the existing map: re > 0 iff b0 == b1 and im > 0 iff b0 == 0 become re > 0 iff g[2 m + 1] = 0 and
        # im > 0 iff g[2 m] = 0, with g the interleaved coded bits
        b, g = bits_of(words).reshape(6, -1, 2), bits_of(raw).reshape(6, -1, 2)
        re, im = b[..., 0] == b[..., 1], b[..., 0] == 0
        assert np.array_equal(re, g[..., 1] == 0) and np.array_equal(im, g[..., 0] == 0)
        x = cr.qpsk_map(bits_of(words))
        assert np.array_equal(x.real > 0, (g[..., 1] == 0).reshape(-1)) and np.array_equal(x.imag > 0, (g[..., 0] == 0).reshape(-1))
        # the unused low bits of the last information word are ignored
        dirty = info.copy()
        dirty[:, -1] |= np.uint32((1 << (32 * cr.info_words(d) - cr.info_bits(d))) - 1)
        assert np.array_equal(stream.conv_encode(dirty, d), words)
    with pytest.raises(ValueError):
        stream.conv_encode(np.zeros((2, 2), np.uint32), 2)


# ---------------------------------------------------------------- 4. the noise-free round trip
@pytest.mark.parametrize("d", [1, 2, 3, 15])
def test_noise_free_round_trip(pkg, d):
    from ofdm_amd import stream
    info = rand_info(d, 20, 20 + d)
    eq = ideal_eq(stream.conv_encode(info, d))
    soft = stream.conv_soft(eq)
    assert soft.dtype == np.float32 and soft.shape == (20, 96 * d)
    out = stream.viterbi_decode(soft)
    assert np.array_equal(out["info"], info) and out["info"].dtype == np.uint32
    # every soft value agrees with its coded bit: the path metric is their sum
    assert np.allclose(out["path"], 96 * d / np.sqrt(2), rtol=1e-5)
    # the slicer's bits are the payload
    assert np.array_equal(stream.slice_bits(eq), bits_of(stream.conv_encode(info, d)))
    # gains scale the soft values and leave the bits alone
    w = np.random.default_rng(d).uniform(0.1, 4.0, (20, 48)).astype(np.float32)
    assert np.array_equal(stream.viterbi_decode(stream.conv_soft(eq, w))["info"], info)
    assert np.array_equal(stream.conv_soft(eq, w)[0], cr.soft_packet(eq[0], w[0], d))


# ---------------------------------------------------------------- 5. the guaranteed correction
def coded_signs(info, d) -> np.ndarray:
    """+-1 soft values of the sent coded bits in trellis order, float32 [n, 96 D]"""
    from ofdm_amd import stream
    return (stream.conv_soft(ideal_eq(stream.conv_encode(info, d))) * np.float32(np.sqrt(2))).round().astype(np.float32)


def test_every_single_flip_is_corrected(pkg):
    from ofdm_amd import stream
    info = rand_info(1, 1, 30)
    s = coded_signs(info, 1)
    assert set(np.unique(s)) == {-1.0, 1.0}
    flipped = np.repeat(s, 96, axis=0)
    flipped[np.arange(96), np.arange(96)] *= -1
    out = stream.viterbi_decode(flipped)
    assert np.array_equal(out["info"], np.repeat(info, 96, axis=0))
    assert np.array_equal(out["path"], np.full(96, 94, np.float32))


@pytest.mark.parametrize("d", [1, 2, 15])
def test_any_four_flips_are_corrected(pkg, d):
    """the free distance is 10: with +-1 soft values any 4 flipped coded bits leave the sent path the best by 2 at least"""
    from ofdm_amd import stream
    n = 2000
    info = rand_info(d, n, 40 + d)
    s = coded_signs(info, d)
    rng = np.random.default_rng(50 + d)
    for i in range(n):
        s[i, rng.choice(96 * d, 4, replace=False)] *= -1
    out = stream.viterbi_decode(s)
    wrong = int((out["info"] != info).any(axis=1).sum())
    print(f"D = {d}: {n} patterns of 4 flipped coded bits, {wrong} decoded wrong")
    assert wrong == 0 and np.array_equal(out["path"], np.full(n, 96 * d - 8, np.float32))


# ---------------------------------------------------------------- 6. the rule against the plain implementation
def test_viterbi_decode_is_the_plain_decoder_bit_for_bit(pkg):
    from ofdm_amd import stream
    rng = np.random.default_rng(60)
    total = ties = 0
    for d, n in ((1, 8), (2, 6), (15, 2)):
        soft = rng.integers(-3, 4, (n, 96 * d)).astype(np.float32)     # small integers: exact sums and many ties
        soft[0] = 0                                                    # the all-zero row: every comparison is a tie
        soft[1, ::2] = 0
        out = stream.viterbi_decode(soft)
        for i in range(n):
            words, path = cr.viterbi_packet(soft[i])
            assert words == out["info"][i].tolist(), (d, i)
            assert np.float32(path) == out["path"][i] and np.float32(path).dtype == out["path"].dtype, (d, i)
            total += 1
        assert not out["info"][0].any() and out["path"][0] == 0
        ties += int((soft == 0).sum())
    print(f"{total} packets of integer-valued soft input, {ties} zero soft values among them: bits and path metric equal")
    # noisy encoded packets as well: both implementations see the same float32 values
    info = rand_info(2, 4, 61)
    eq = ideal_eq(stream.conv_encode(info, 2))
    eq = (eq + 0.6 * (rng.standard_normal(eq.shape) + 1j * rng.standard_normal(eq.shape))).astype(np.complex64)
    w = rng.uniform(0, 4, (4, 48)).astype(np.float32)
    soft = stream.conv_soft(eq, w)
    out = stream.viterbi_decode(soft)
    for i in range(4):
        assert np.array_equal(soft[i], cr.soft_packet(eq[i], w[i], 2))
        words, path = cr.viterbi_packet(soft[i])
        assert words == out["info"][i].tolist() and np.float32(path) == out["path"][i]
    # special values: non-finite products become 0, the clamp holds
    z = np.array([[complex(np.nan, np.inf)] + [complex(-np.inf, 3e38)] + [complex(1e37, -1e37)] + [1 + 1j] * 45], np.complex64)
    s = stream.conv_soft(z, np.full((1, 48), 4.0, np.float32))
    assert np.isfinite(s).all() and np.abs(s).max() == np.float32(2.0 ** 100) and int((s == 0).sum()) == 4      # 4 x 3e38 overflows: 0
    assert np.array_equal(s[0], cr.soft_packet(z[0], np.full(48, 4.0, np.float32), 1))
    for bad in (np.zeros((2, 96)), np.zeros((2, 95), np.float32), np.zeros(96, np.float32)):
        with pytest.raises(ValueError):
            stream.viterbi_decode(bad)


# ---------------------------------------------------------------- 7. it pays
def _info_errors(soft, info) -> int:
    from ofdm_amd import stream
    return int(bits_of(stream.viterbi_decode(soft)["info"] ^ info).sum())


def test_the_code_pays_on_the_four_tap_link(pkg):
    from ofdm_amd import stream
    info = rand_info(2, PAYS_PACKETS, PAYS_SEED)
    rng = np.random.default_rng(PAYS_SEED + 1)
    H = cr.model_channel(rng, PAYS_PACKETS, PAYS_PDP)
    payload = bits_of(stream.conv_encode(info, 2))
    z, g = cr.model_receive(rng, payload, H, 20.0)
    uncoded = int((stream.slice_bits(z) != payload).sum())
    weighted = _info_errors(stream.conv_soft(z, g), info)
    plain = _info_errors(stream.conv_soft(z), info)
    signs = _info_errors(np.sign(stream.conv_soft(z)).astype(np.float32), info)
    nu, ni = payload.size, 90 * PAYS_PACKETS
    print(f"{PAYS_PACKETS} two-symbol packets, four taps, 20 dB: uncoded {uncoded} of {nu} ({uncoded / nu:.2g}); information bit "
          f"errors of {ni}: |H|^2 weights {weighted} ({weighted / ni:.2g}), sign-only {signs}, unweighted soft {plain}")
    assert uncoded > 0
    assert weighted / ni <= 0.1 * uncoded / nu
    assert weighted <= signs


def test_the_precoding_pays_in_awgn(pkg):
    from ofdm_amd import stream
    info = rand_info(2, PAYS_PACKETS, PAYS_SEED + 2)
    errors = {}
    for precode in (True, False):
        rng = np.random.default_rng(PAYS_SEED + 3)
        payload = bits_of(stream.conv_encode(info, 2, precode=precode))
        z, _ = cr.model_receive(rng, payload, cr.model_channel(rng, PAYS_PACKETS, None), 6.0)
        if precode:
            soft = stream.conv_soft(z)
        else:
            # the coded bits fed straight to the map: g[2 m] is on the imaginary axis, g[2 m + 1] on both -- the max-log
            # value of the XOR of the two axes
            re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
            both = np.sign(re) * np.sign(im) * np.minimum(np.abs(re), np.abs(im))
            v = np.stack([im, both], axis=-1).reshape(PAYS_PACKETS, 2, 96)
            soft = np.ascontiguousarray(v[:, :, stream.interleave_index()].reshape(PAYS_PACKETS, 192), np.float32)
        errors[precode] = _info_errors(soft, info)
    print(f"{PAYS_PACKETS} two-symbol packets, AWGN, 6 dB: information bit errors of {90 * PAYS_PACKETS}: {errors[True]} with the "
          f"precoding, {errors[False]} without")
    assert errors[False] > 0 and 4 * errors[True] <= errors[False]
