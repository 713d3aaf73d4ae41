"""The device channel and the per-packet scoring (include/ofdm_mi355x_channel.h), the checks that need no GPU: the
header against the binding and the built library, the new translation unit's place in the build and in the resource
report, and stream.score_packets -- the scoring rule in numpy -- on hand-built cases."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_channel_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.CHANNEL_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.CHANNEL_EXPORTS) == ["ofdm_impair_stream", "ofdm_score_packets"]
    others = (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS) | set(abi.STREAM_EXPORTS)
              | set(abi.TX_EXPORTS))
    assert not set(names) & others
    assert re.search(r'#include "ofdm_mi355x_tx.h"', h)
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    base = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    assert "ofdm_impair_" not in base and "ofdm_score_" not in base and re.search(r"#define OFDM_ABI_VERSION 1\b", base)


def test_channel_header_compiles_as_c_and_matches_the_binding(pkg, tmp_path):
    abi = pkg.abi
    o, s = abi.ChannelOpts, abi.Score
    fields = [f for f, _ in o._fields_]
    src = tmp_path / "offsets.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_channel.h"\nint main(void) {\n'
        ' printf("%zu", sizeof(ofdm_channel_opts));\n'
        + "".join(f' printf(" %zu", offsetof(ofdm_channel_opts, {f}));\n' for f in fields)
        + ' printf(" %zu %zu %zu", sizeof(ofdm_score), offsetof(ofdm_score, rx_index), offsetof(ofdm_score, bit_err));\n'
        ' printf(" %d %d %d %d %d %d %d %d\\n", OFDM_NOISE_REAL, OFDM_NOISE_COMPLEX, OFDM_NOISE_NONE,\n'
        "        OFDM_CHANNEL_MAX_TAPS, OFDM_CHANNEL_TILE, OFDM_K_CHANNEL, OFDM_K_SCORE, OFDM_NSCORE);\n return 0; }\n")
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(o) == 64
    assert got[1:11] == [getattr(o, f).offset for f in fields] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    dt = abi.score_dtype()
    assert got[11:14] == [C.sizeof(s), s.rx_index.offset, s.bit_err.offset] == [8, 0, 4]
    assert dt.itemsize == 8 and dt.names == ("rx_index", "bit_err") and [dt.fields[n][1] for n in dt.names] == [0, 4]
    assert got[14:] == [abi.NOISE_REAL, abi.NOISE_COMPLEX, abi.NOISE_NONE, abi.CHANNEL_MAX_TAPS, abi.CHANNEL_TILE,
                        abi.K_CHANNEL, abi.K_SCORE, abi.NSCORE]
    assert (abi.K_CHANNEL, abi.K_SCORE, abi.NSCORE, abi.CHANNEL_MAX_TAPS) == (abi.K_TRANSMIT + 1, abi.K_TRANSMIT + 2, 8, 32)
    assert abi.NOISE == {"real": abi.NOISE_REAL, "complex": abi.NOISE_COMPLEX, "none": abi.NOISE_NONE}


def test_argument_errors_need_no_device(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    opts = abi.ChannelOpts(1.0, 20.0, 0.0, 1, 0, 0, abi.NOISE_REAL, 0, 0, 0)
    assert lib.ofdm_impair_stream(None, C.byref(opts), None, None, None, 0) == -1
    assert b"ctx" in lib.ofdm_last_error()
    assert lib.ofdm_score_packets(None, 2, None, 0, None, 0, 0, None, None, None, 8, 40, None, None) == -1
    assert b"ctx" in lib.ofdm_last_error()


def test_channel_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    abi = pkg.abi
    assert "ofdm_channel.hip" in build_lib.SOURCES and "ofdm_channel.hip" in build_lib.SOURCE_FLAGS
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_channel.hip"]
    names = sorted(x["name"] for x in rows)
    # <filter, rotation, noise> and the scoring kernel
    want = [f"ofdm::channel_kernel<{f}, {c}, {n}>" for f in ("true", "false") for c in ("true", "false")
            for n in (abi.NOISE_REAL, abi.NOISE_COMPLEX, abi.NOISE_NONE)] + ["ofdm::score_kernel"]
    assert names == sorted(want)
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("SGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        # the tile and its history are staged only for the filter
        lds = x["LDS Size [bytes/block]"]
        if "channel_kernel<true" in x["name"]:
            assert lds == 8 * (abi.CHANNEL_TILE + abi.CHANNEL_MAX_TAPS)
        elif "channel_kernel<false" in x["name"]:
            assert lds == 0
    # the transmitter's instantiations are what they were: the shared phasor header adds no kernel
    tx = {x["name"] for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_transmit.hip"}
    assert len(tx) == 8 and all(n.startswith("ofdm::transmit_kernel<") for n in tx)
    src = (build_lib.CSRC / "ofdm_transmit.hip").read_text() + (build_lib.CSRC / "ofdm_channel.hip").read_text()
    assert src.count('#include "ofdm_phasor.h"') == 2 and "sincospif" not in src         # one construction, shared


# ------------------------------------------------------------------------------------------- the scoring rule
def words_of(rows, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, (rows, 6), dtype=np.uint64).astype(np.uint32)


def test_score_window_edges(pkg):
    from ofdm_amd.stream import score_packets
    tw = words_of(4)
    tx = np.array([1000, 3000, 5000, 7000], np.int64)
    # offsets exactly at off_lo and off_hi, and one past each
    rx = tx + np.array([8, 40, 7, 41])
    rw = tw.copy()
    rw[0, 0] ^= 0x80000001                                        # two bit errors in packet 0
    rw[1, 5] ^= 0x00010000                                        # one in packet 1
    r = score_packets(tx, tw, rx, rw, window=(8, 40))
    assert r["rx_index"].tolist() == [0, 1, -1, -1] and r["bit_err"].tolist() == [2, 1, 0, 0]
    assert r["rx_index"].dtype == np.int32 and r["bit_err"].dtype == np.int32 and r["totals"].dtype == np.int64
    assert r["totals"].tolist() == [4, 2, 4, 2 * 192, 3, 2, 0, 0]
    # a degenerate window of one offset
    r = score_packets(tx, tw, rx, rw, window=(40, 40))
    assert r["rx_index"].tolist() == [-1, 1, -1, -1] and r["totals"].tolist() == [4, 1, 4, 192, 1, 1, 0, 0]


def test_score_false_alarm_and_the_smallest_index(pkg):
    from ofdm_amd.stream import score_packets
    tw = words_of(2)
    tx = np.array([1000, 3000], np.int64)
    # a false alarm between the two packets, one in front of the first, and a clean match each
    rx = np.array([400, 1016, 2000, 3017], np.int64)
    rw = np.stack([words_of(1, 9)[0], tw[0], words_of(1, 10)[0], tw[1]])
    r = score_packets(tx, tw, rx, rw)
    assert r["rx_index"].tolist() == [1, 3] and r["bit_err"].tolist() == [0, 0]
    t = r["totals"]
    assert t.tolist() == [2, 2, 4, 384, 0, 0, 0, 0] and t[2] - t[1] == 2                 # two false alarms
    # two records inside one window (the caller's spacing rule broken): the smallest index wins
    r = score_packets(tx[:1], tw[:1], np.array([1010, 1030]), np.stack([tw[0] ^ np.uint32(1), tw[0]]))
    assert r["rx_index"].tolist() == [0] and r["bit_err"].tolist() == [6]


def test_score_empty_sides_and_bad_windows(pkg):
    from ofdm_amd.stream import score_packets
    tw = words_of(3)
    tx = np.array([10, 2000, 4000], np.int64)
    none = score_packets(tx, tw, np.zeros(0, np.int64), np.zeros((0, 6), np.uint32))
    assert none["rx_index"].tolist() == [-1] * 3 and not none["bit_err"].any()
    assert none["totals"].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]
    empty = score_packets(np.zeros(0, np.int64), np.zeros((0, 6), np.uint32), np.array([26, 2016]), tw[:2])
    assert len(empty["rx_index"]) == 0 and len(empty["bit_err"]) == 0
    assert empty["totals"].tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
    for bad in ((0, 301), (-1, 40), (41, 40), (8, 400)):
        with pytest.raises(ValueError):
            score_packets(tx, tw, tx + 16, tw, window=bad)
    assert score_packets(tx, tw, tx + 300, tw, window=(0, 300))["totals"][1] == 3       # 300 wide is the limit
    with pytest.raises(ValueError):
        score_packets(tx, tw, np.array([50, 20]), tw[:2])                                # records must ascend


def test_link_command_grid_and_columns(pkg):
    from ofdm_amd import sweep
    assert sweep.parse_snr_grid("25:40:15").tolist() == [25.0, 40.0]
    assert sweep.parse_snr_grid("6:40:1").tolist() == list(np.arange(6.0, 41.0))
    assert sweep.parse_snr_grid("12.5").tolist() == [12.5]
    for bad in ("1:2", "5:1:1", "1:5:0"):
        with pytest.raises(ValueError):
            sweep.parse_snr_grid(bad)
    assert sweep.LINK_COLUMNS == ("snr_db", "transmitted", "matched", "missed", "false_alarms", "packet_err", "bit_err", "bits")
