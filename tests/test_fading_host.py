"""The per-packet fading transmitter (include/ofdm_mi355x_fading.h), the checks that need no GPU: the header against
the binding and the built library, ofdm_faded_len, the new translation unit's place in the build and in the resource
report, channel.fade_packets and channel.parse_pdp, and link_sweep's gap rule under fading."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_fading_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.FADING_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.FADING_EXPORTS) == ["ofdm_draw_taps", "ofdm_faded_len", "ofdm_transmit_faded"]
    others = (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS) | set(abi.STREAM_EXPORTS)
              | set(abi.TX_EXPORTS) | set(abi.CHANNEL_EXPORTS))
    assert not set(names) & others
    assert re.search(r'#include "ofdm_mi355x_channel.h"', h)
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    base = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    assert "ofdm_draw_" not in base and "_faded" not in base and re.search(r"#define OFDM_ABI_VERSION 1\b", base)
    # the header says what the drawn taps are, and that the symbol-mode identity is by construction
    assert "0xC4A00000" in h and "OFDM_CHAN_RAYLEIGH4" in h and "by construction" in h.replace("\n * ", " ")


def test_fading_header_compiles_as_c_and_matches_the_binding(pkg, tmp_path):
    abi = pkg.abi
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ofdm_mi355x_fading.h"\nint main(void) {\n'
                   ' printf("%d %d %d %d\\n", OFDM_FADE_MAX_TAPS, OFDM_K_FADE, OFDM_K_DRAW_TAPS, OFDM_K_SCORE);\n'
                   " return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c",
                        str(ROOT / "include" / "ofdm_mi355x_fading.h"), f"-I{ROOT / 'include'}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = tmp_path / "consts"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [abi.FADE_MAX_TAPS, abi.K_FADE, abi.K_DRAW_TAPS, abi.K_SCORE] == [32, 10, 11, 9]
    assert abi.FADE_MAX_TAPS == abi.CHANNEL_MAX_TAPS                 # the single-packet equivalence needs K8 to take them


def test_faded_len_and_argument_errors_need_no_device(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    n = C.c_int32(-1)
    for d in (1, 2, 7, 15):
        for taps in (1, 2, 4, 5, 32):
            assert lib.ofdm_faded_len(d, taps, C.byref(n)) == 0
            assert n.value == 2 * (320 + 80 * d) + 20 + taps - 1 == abi.faded_len(d, taps) == abi.packet_len(d) + taps - 1
    assert abi.faded_len(15, 32) == 3091 and abi.faded_len(2, 1) == 980
    for d, taps in ((0, 1), (16, 1), (-1, 4), (2, 0), (2, 33), (2, -1)):
        n.value = 77
        assert lib.ofdm_faded_len(d, taps, C.byref(n)) == -1 and n.value == 77, (d, taps)
        assert len(lib.ofdm_last_error()) > 0
    assert lib.ofdm_faded_len(2, 4, None) == -1 and b"len" in lib.ofdm_last_error()
    # a NULL context is refused before anything else
    opts = abi.TxOpts(0, 1, 2, 0)
    assert lib.ofdm_transmit_faded(None, C.byref(opts), None, 0, None, 0, 0, None, None, None, 1, None, 0) == -1
    assert b"ctx" in lib.ofdm_last_error()
    pdp = (C.c_float * 1)(1.0)
    assert lib.ofdm_draw_taps(None, 1, 0, 0, 1, pdp, None) == -1
    assert b"ctx" in lib.ofdm_last_error()


def test_fade_packets_is_the_convolution_per_packet(pkg):
    from ofdm_amd.channel import fade_packets
    rng = np.random.default_rng(5)
    for n, p, taps in ((3, 40, 1), (4, 33, 5), (2, 50, 32), (1, 7, 9)):
        x = rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p))
        h = rng.standard_normal((n, taps)) + 1j * rng.standard_normal((n, taps))
        got = fade_packets(x.astype(np.complex64), h.astype(np.complex64))
        assert got.dtype == np.complex128 and got.shape == (n, p + taps - 1)
        for k in range(n):
            want = np.convolve(x[k].astype(np.complex64).astype(np.complex128), h[k].astype(np.complex64).astype(np.complex128))
            assert np.abs(got[k] - want).max() <= 1e-13 * np.abs(want).max()
    one = fade_packets(np.ones((2, 4)), np.array([[2.0], [1j]]))
    assert np.array_equal(one, np.array([[2.0] * 4, [1j] * 4]))
    for bad in ((np.ones(4), np.ones((1, 1))), (np.ones((2, 4)), np.ones((3, 1))), (np.ones((2, 4)), np.ones((2, 0)))):
        with pytest.raises(ValueError):
            fade_packets(*bad)


def test_parse_pdp_normalises_and_rejects(pkg):
    from ofdm_amd.channel import parse_pdp
    p = parse_pdp("1,0.5,0.25,0.125")
    assert p.dtype == np.float64 and np.allclose(p, np.array([8, 4, 2, 1]) / 15.0, rtol=1e-15) and abs(p.sum() - 1) < 1e-15
    assert parse_pdp("1").tolist() == [1.0] and parse_pdp(" 3 , 1 ").tolist() == [0.75, 0.25]
    assert parse_pdp("0,2").tolist() == [0.0, 1.0]
    assert len(parse_pdp(",".join(["1"] * 32))) == 32
    for bad in ("1,-0.5", "nan", "1,inf", ",".join(["1"] * 33), "", "0,0", "a,b"):
        with pytest.raises(ValueError):
            parse_pdp(bad)


class NoDevice:
    """link_sweep's argument checks run before it touches the engine"""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was used ({name})")


def test_link_sweep_refuses_a_gap_shorter_than_the_grown_window(pkg):
    from ofdm_amd import sweep
    words = np.zeros((3, 6), np.uint32)
    # unfaded the default window ends at 40; four taps move it to 43
    with pytest.raises(ValueError, match="shorter than the scoring window"):
        sweep.link_sweep(NoDevice(), words, 2, 39, [30.0])
    with pytest.raises(ValueError, match=r"shorter than the scoring window \(8, 43\)"):
        sweep.link_sweep(NoDevice(), words, 2, 42, [30.0], fading=dict(pdp=[0.25] * 4))
    with pytest.raises(ValueError, match=r"\(8, 71\)"):
        sweep.link_sweep(NoDevice(), words, 2, 70, [30.0], fading=dict(pdp=[1 / 32] * 32, index0=5))
    # a gap that covers it gets past the check and reaches the engine
    with pytest.raises(AssertionError, match="the engine was used"):
        sweep.link_sweep(NoDevice(), words, 2, 43, [30.0], fading=dict(pdp=[0.25] * 4))
    for bad in (dict(), dict(pdp=[]), dict(pdp=[1] * 33), dict(pdp=[1], taps=3)):
        with pytest.raises(ValueError):
            sweep.link_sweep(NoDevice(), words, 2, 500, [30.0], fading=bad)


def test_fading_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_fading.hip" in build_lib.SOURCES and "ofdm_fading.hip" in build_lib.SOURCE_FLAGS
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_fading.hip"]
    names = sorted(x["name"] for x in rows)
    want = [f"ofdm::transmit_faded_kernel<{c}, {i}, {a}>" for c in (0, 1) for i in ("true", "false")
            for a in ("true", "false")] + ["ofdm::draw_taps_kernel"]
    assert names == sorted(want)
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        if "transmit_faded_kernel" in x["name"]:
            # K7's 4,500 samples and the packet buffer [35 | 3,060 | 35]; two blocks per CU need two waves per SIMD
            assert x["LDS Size [bytes/block]"] == 8 * (4500 + 3060 + 2 * 31 + 8) and 2 * x["LDS Size [bytes/block]"] <= 160 * 1024
            assert x["VGPRs"] <= 256 and x["Occupancy [waves/SIMD]"] >= 2
        else:
            assert x["LDS Size [bytes/block]"] == 0
    # K7's and K8's rows are what they were
    allrows = json.loads(build_lib.RESOURCE_REPORT.read_text())
    assert len([x for x in allrows if x["source"] == "ofdm_transmit.hip"]) == 8
    assert len([x for x in allrows if x["source"] == "ofdm_channel.hip"]) == 13
