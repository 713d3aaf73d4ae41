"""The stream receiver (include/ofdm_mi355x_stream.h), the checks that need no GPU: stream.select_packets -- the
executable specification of the rule -- against the reference's Packet_Selection on single captures and against the
windowed oracle on whole streams, its edge cases on synthetic bitmaps, channel.make_stream, and the header, binding and
resource report of the new translation unit."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, normwise
from test_lazy_rule import corr_out, packet_selection

MSG = b"Hey! I am Vivaswan"
MSG5 = (b"five data symbols per packet: a sixty-byte message for the stream") [:60]
CFOS = (0.0, 40e3, -90e3)


def base_segments(period):
    """the issue's base stream: zeros(700) | wave | zeros(1500) | wave[:3 period] | zeros(400)"""
    return [("gap", 700), ("wave", 0, 10 * period), ("gap", 1500), ("wave", 0, 3 * period), ("gap", 400)]


def base_stream(wave, snr_db, cfo_hz, seed, taps=None, noise="real", segments=None):
    import torch
    from ofdm_amd.channel import make_stream
    gen = torch.Generator()
    gen.manual_seed(seed)
    seg = segments or base_segments(len(wave) // 10)
    return make_stream(torch.from_numpy(wave.astype(np.complex64)), seg, snr_db, cfo_hz, taps=taps, noise=noise,
                       generator=gen).numpy()


@pytest.fixture(scope="module")
def waves(pkg, oracle):
    return {2: oracle.frame_waveform(oracle.message_bits(MSG)), 5: oracle.frame_waveform(oracle.message_bits(MSG5))}


# ---------------------------------------------------------------- 1. one capture: the reference's Packet_Selection
def test_first_unflagged_packet_is_packet_selection(pkg, waves):
    from ofdm_amd.stream import first_packet, select_packets
    wave = waves[2]
    rng = np.random.default_rng(0x57EA)
    hits = 0
    for k in range(200):
        snr = rng.uniform(0.0, 30.0)
        s = int(rng.integers(0, len(wave) - 3008))
        sigma = np.sqrt(np.mean(np.abs(wave) ** 2) / 10 ** (snr / 10))
        m = corr_out(wave[s:s + 3008] + sigma * rng.standard_normal(3008))
        want = packet_selection(m)
        assert first_packet(select_packets(m)) == want, (k, snr, s)
        hits += want != 0
    assert 40 <= hits < 200                       # both outcomes are covered


# ---------------------------------------------------------------- 2. whole streams against the windowed oracle
@pytest.mark.parametrize("nd", [2, 5])
def test_stream_packets_agree_with_the_windowed_oracle(pkg, oracle, waves, nd):
    from ofdm_amd.stream import select_packets
    wave = waves[nd]
    truth = oracle.message_bits(MSG if nd == 2 else MSG5)
    cap_len = int(len(wave) * 0.307)
    n = 700 + len(wave) + 1500 + 3 * (len(wave) // 10) + 400
    assert n == {2: 15340, 5: 21580}[nd] and cap_len == {2: 3008, 5: 4482}[nd]
    checked = 0
    for snr in (10, 14, 25):
        for q, cfo in enumerate(CFOS):
            x = base_stream(wave, snr, cfo, 1000 * nd + 10 * snr + q)
            assert len(x) == n
            sel = select_packets(corr_out(x.astype(np.complex128)))
            assert 8 <= len(sel["positions"]) <= 13
            if snr >= 14:
                assert len(sel["positions"]) == 13
            assert (np.diff(sel["fronts"]) > 300).all() and len(sel["fronts"]) <= n // 301 + 1
            assert int((sel["flags"] != 0).sum()) <= 1
            for p in sel["positions"]:
                f = int(p) - 11
                if f - 400 < 0 or f - 400 + cap_len > n:
                    continue
                o = oracle.receiver_frame(x[f - 400:f - 400 + cap_len].astype(np.complex128), truth, "c")
                assert o["packet_idx"] - 11 + (f - 400) == f, (snr, cfo, f, o["packet_idx"])
                checked += 1
    assert checked >= 9 * 9


# ---------------------------------------------------------------- 3. the rule's edges on synthetic bitmaps
def _bitmap(lc, at):
    c = np.zeros(lc, bool)
    c[list(at)] = True
    return c


def test_select_packets_edges(pkg):
    from ofdm_amd.stream import LAST_FRONT, select_packets, unpack_cross
    # the virtual crossing at -1: a first crossing at 299 is no front, at 300 it is
    assert len(select_packets(_bitmap(2000, [299, 529]))["fronts"]) == 0
    s = select_packets(_bitmap(2000, [300, 530]))
    assert s["fronts"].tolist() == [300] and s["positions"].tolist() == [311] and s["flags"].tolist() == [LAST_FRONT]
    # a gap of exactly 300 is no front, 301 is
    assert select_packets(_bitmap(3000, [400, 700, 930]))["fronts"].tolist() == [400]
    assert select_packets(_bitmap(3000, [400, 630, 930, 1160]))["fronts"].tolist() == [400]
    s = select_packets(_bitmap(3000, [400, 630, 931, 1161]))
    assert s["fronts"].tolist() == [400, 931] and s["positions"].tolist() == [411, 942]
    assert s["flags"].tolist() == [0, LAST_FRONT]
    # an unconfirmed later front takes the flag away from every packet
    s = select_packets(_bitmap(3000, [400, 630, 1500]))
    assert s["fronts"].tolist() == [400, 1500] and s["positions"].tolist() == [411] and s["flags"].tolist() == [0]
    # front + 230 = Lc - 1 is confirmed, front + 230 = Lc is not
    assert select_packets(_bitmap(731, [500, 730]))["positions"].tolist() == [511]
    s = select_packets(_bitmap(730, [500]))
    assert s["fronts"].tolist() == [500] and len(s["positions"]) == 0
    # the front bound: a crossing every 301 positions
    for n in (348, 3008, 30100, 30101 + 47):
        lc = n - 47
        s = select_packets(_bitmap(lc, range(300, lc, 301)))
        assert len(s["fronts"]) == len(range(300, lc, 301)) <= n // 301 + 1
    # a metric with NaN (zero power) has no crossing there; the bitmap unpacks LSB first
    m = np.full(1000, np.nan, np.float32)
    m[[300, 530]] = 0.9
    assert select_packets(m)["positions"].tolist() == [311]
    words = np.array([0x80000001, 0x2], np.uint32)
    assert np.nonzero(unpack_cross(words, 40))[0].tolist() == [0, 31, 33]
    with pytest.raises(ValueError):
        unpack_cross(words, 65)


# ---------------------------------------------------------------- 4. channel.make_stream
def test_make_stream_layout_noise_and_errors(pkg, waves):
    import torch
    from ofdm_amd.channel import make_captures, make_stream
    wave = waves[2]
    w = torch.from_numpy(wave.astype(np.complex64))
    x = make_stream(w, [("gap", 5), ("wave", 9790, 9810), ("gap", 0), ("wave", 3, 3), ("gap", 7)], 10.0, noise="none")
    assert x.dtype == torch.complex64 and tuple(x.shape) == (32,) and x.device.type == "cpu"
    assert not x[:5].abs().any() and not x[25:].abs().any()
    assert np.array_equal(x[5:25].numpy(), np.concatenate([wave[9790:], wave[:10]]).astype(np.complex64))
    assert tuple(make_stream(w, [], 10.0).shape) == (0,)
    # one whole wave: the impairments are make_captures', noise included
    for noise in ("none", "real", "complex"):
        g1, g2 = torch.Generator(), torch.Generator()
        g1.manual_seed(5)
        g2.manual_seed(5)
        a = make_stream(w, [("wave", 0, len(wave))], 12.0, -90e3, taps=[1, 0, 0.4 + 0.3j], noise=noise, generator=g1)
        b = make_captures(w, 0, 12.0, -90e3, taps=[1, 0, 0.4 + 0.3j], noise=noise, generator=g2, cap_len=len(wave))[0]
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), noise
    # the noise covers the gaps too, at the power measured on wave; real noise leaves the imaginary part alone
    g = torch.Generator()
    g.manual_seed(6)
    z = make_stream(w, [("gap", 40000)], 10.0, noise="real", generator=g).numpy()
    P = np.mean(np.abs(wave) ** 2)
    assert abs(np.mean(z.real.astype(np.float64) ** 2) / (P / 10.0) - 1.0) < 0.05 and not z.imag.any()
    z = make_stream(w, [("gap", 40000)], 10.0, noise="complex", generator=g).numpy()
    assert abs(np.mean(z.imag.astype(np.float64) ** 2) / (P / 20.0) - 1.0) < 0.05
    # the rotation goes by the stream index and the FIR crosses segment borders
    y = make_stream(w, [("gap", 3), ("wave", 0, 50)], 10.0, 40e3, taps=[1, 0, 0.5], noise="none").numpy()
    lay = np.concatenate([np.zeros(3), wave[:50]])
    ref = np.convolve(lay, [1, 0, 0.5])[:53] * np.exp(2j * np.pi * 40e3 * np.arange(53) * 25e-9)
    assert normwise(y, ref) < 2e-6
    for bad in ([("gap", -1)], [("wave", 5, 4)], [("wave", -1, 4)], [("noise", 3)], [("gap",)]):
        with pytest.raises(ValueError):
            make_stream(w, bad, 10.0)
    with pytest.raises(ValueError):
        make_stream(w, [("gap", 3)], 10.0, noise="pink")
    with pytest.raises(ValueError):
        make_stream(torch.zeros(4), [("gap", 3)], 10.0)


# ---------------------------------------------------------------- the header, the binding, the build
def test_stream_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.STREAM_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.STREAM_EXPORTS) == ["ofdm_receive_stream"]
    assert not set(names) & (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS))
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert hasattr(lib, "ofdm_receive_stream") and re.search(r"\bT ofdm_receive_stream\b", out)
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    base = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    assert "ofdm_receive_stream" not in base and re.search(r"#define OFDM_ABI_VERSION 1\b", base)


def test_stream_packet_layout_matches_the_header(pkg, tmp_path):
    abi = pkg.abi
    st = abi.StreamPacket
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_stream.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(ofdm_stream_packet), '
                   "offsetof(ofdm_stream_packet, packet_pos), offsetof(ofdm_stream_packet, reserved), "
                   "offsetof(ofdm_stream_packet, r), OFDM_STREAM_LAST_FRONT, OFDM_STREAM_TILE, OFDM_STREAM_RUN, "
                   "OFDM_K_STREAM_DETECT, OFDM_K_STREAM_SELECT, OFDM_K_STREAM_DECODE); return 0; }\n")
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [64, st.packet_pos.offset, st.reserved.offset, st.r.offset, abi.STREAM_LAST_FRONT, abi.STREAM_TILE,
                   abi.STREAM_RUN, abi.K_STREAM_DETECT, abi.K_STREAM_SELECT, abi.K_STREAM_DECODE]
    assert C.sizeof(st) == 64 and (st.packet_pos.offset, st.reserved.offset, st.r.offset) == (0, 8, 16)
    dt, cr = abi.stream_packet_dtype(), abi.capture_result_dtype()
    assert dt.itemsize == 64 and dt.names[:2] == ("packet_pos", "reserved8") and dt.names[2:] == cr.names
    assert all(dt.fields[f][1] == 16 + cr.fields[f][1] for f in cr.names)
    assert abi.STREAM_TILE % 32 == 0 and abi.STREAM_RUN % 2 == 1 and abi.STREAM_TILE == 256 * abi.STREAM_RUN
    from ofdm_amd import stream
    assert abi.STREAM_LAST_FRONT == stream.LAST_FRONT


def test_stream_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    opts = pkg.abi.make_rx_opts("c")
    assert lib.ofdm_receive_stream(None, None, 100, C.byref(opts), 1, 4, None, None, None, None, None, None, None) == -1
    assert b"ctx" in lib.ofdm_last_error()


def test_stream_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_stream.hip" in build_lib.SOURCES and "ofdm_stream.hip" in build_lib.SOURCE_FLAGS
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_stream.hip"]
    names = {x["name"] for x in rows}
    assert names == {"ofdm::stream_detect_kernel<true>", "ofdm::stream_detect_kernel<false>",
                     "ofdm::stream_select_kernel<0>", "ofdm::stream_select_kernel<1>", "ofdm::stream_select_kernel<2>",
                     "ofdm::stream_decode_kernel<true>", "ofdm::stream_decode_kernel<false>"}
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        if "decode" in x["name"]:
            assert x["VGPRs"] <= 256                                   # eight-wave blocks: two waves per SIMD
        if "detect" in x["name"]:
            assert x["LDS Size [bytes/block]"] <= 80 * 1024 and x["VGPRs"] <= 256      # two blocks per CU: two waves per SIMD
