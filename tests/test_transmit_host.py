"""The packet transmitter (include/ofdm_mi355x_tx.h), the checks that need no GPU: the header against the binding and
the built library, stream.pack_messages against the oracle's Data_Generator and fileio.decode_message, and the new
translation unit's place in the build and in the resource report."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

_TEXT = ("Packets for the stream receiver, each with a payload of its own: the transmitter packs a text into three "
         "MSB-first words per data symbol and pads it with blanks to whole symbols, 180 characters at most!!")
assert len(_TEXT) >= 181


def text(n: int) -> str:
    return _TEXT[:n - 1] + "."                                   # no trailing blank


def test_tx_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    h = abi.TX_HEADER.read_text()
    names = sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))
    assert names == sorted(abi.TX_EXPORTS) == ["ofdm_transmit_len", "ofdm_transmit_packets"]
    assert not set(names) & (set(abi.EXPORTS) | set(abi.LONG_EXPORTS) | set(abi.CAPTURES_EXPORTS) | set(abi.STREAM_EXPORTS))
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    base = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    assert "ofdm_transmit_" not in base and re.search(r"#define OFDM_ABI_VERSION 1\b", base)


def test_tx_header_compiles_as_c_and_matches_the_binding(pkg, tmp_path):
    abi = pkg.abi
    o = abi.TxOpts
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_tx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(ofdm_tx_opts), '
                   "offsetof(ofdm_tx_opts, conv), offsetof(ofdm_tx_opts, float_taps), offsetof(ofdm_tx_opts, n_data), "
                   "offsetof(ofdm_tx_opts, flags), OFDM_TX_ACCUMULATE, OFDM_K_TRANSMIT); return 0; }\n")
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [16, o.conv.offset, o.float_taps.offset, o.n_data.offset, o.flags.offset, abi.TX_ACCUMULATE, abi.K_TRANSMIT]
    assert C.sizeof(o) == 16 and got[1:5] == [0, 4, 8, 12] and abi.K_TRANSMIT == abi.K_STREAM_DECODE + 1 == 7


def test_transmit_len_and_argument_errors_need_no_device(pkg):
    lib, abi = pkg.load_library(), pkg.abi
    n = C.c_int32()
    for d in (1, 2, 7, 15):
        assert lib.ofdm_transmit_len(d, C.byref(n)) == 0
        assert n.value == abi.packet_len(d) == 2 * (320 + 80 * d) + 20 == abi.wave_len(d) // 10
    for d in (0, 16, -1):
        assert lib.ofdm_transmit_len(d, C.byref(n)) == -1 and b"n_data" in lib.ofdm_last_error()
    assert lib.ofdm_transmit_len(2, None) == -1
    opts = abi.TxOpts(0, 1, 2, 0)
    assert lib.ofdm_transmit_packets(None, C.byref(opts), None, 0, None, 0, 0, None, None, None, 0) == -1
    assert b"ctx" in lib.ofdm_last_error()


@pytest.mark.parametrize("n", [1, 12, 13, 18, 171, 180])
def test_pack_messages_is_data_generator(pkg, oracle, n):
    from ofdm_amd.fileio import decode_message
    from ofdm_amd.stream import pack_messages
    t = text(n)
    words, d = pack_messages([t])
    assert d == (8 * n + 95) // 96 and words.dtype == np.uint32 and words.shape == (1, 3 * d)
    bits = ((words[0][:, None] >> np.arange(31, -1, -1, dtype=np.uint32)) & 1).astype(np.int32).ravel()   # MSB first
    assert np.array_equal(bits, oracle.message_bits(t.encode("latin-1")))
    assert decode_message(bits) == t + " " * (12 * d - n)
    # bytes are taken as they are, and a larger n_data pads with whole symbols of blanks
    wb, db = pack_messages([t.encode("latin-1")], n_data=15)
    assert db == 15 and np.array_equal(wb[0, :3 * d], words[0]) and (wb[0, 3 * d:] == 0x20202020).all()


def test_pack_messages_batches_and_limits(pkg):
    from ofdm_amd.fileio import decode_message
    from ofdm_amd.stream import pack_messages
    texts = [text(5), text(13), text(60), "x"]
    words, d = pack_messages(texts)
    assert d == 5 and words.shape == (4, 15)
    for row, t in zip(words, texts):
        bits = ((row[:, None] >> np.arange(31, -1, -1, dtype=np.uint32)) & 1).ravel()
        assert decode_message(bits) == t.ljust(60)
    assert pack_messages([], n_data=3)[0].shape == (0, 9) and pack_messages([])[1] == 1
    assert pack_messages([""])[0].tolist() == [[0x20202020] * 3]
    with pytest.raises(ValueError):
        pack_messages([text(181)])
    with pytest.raises(ValueError):
        pack_messages([text(13)], n_data=1)
    with pytest.raises(ValueError):
        pack_messages([text(5)], n_data=16)
    assert pack_messages([text(180)])[1] == 15


def test_transmit_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_transmit.hip" in build_lib.SOURCES and "ofdm_transmit.hip" in build_lib.SOURCE_FLAGS
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_transmit.hip"]
    names = {x["name"] for x in rows}
    # <conv, gain or carrier offset, accumulate>
    assert names == {f"ofdm::transmit_kernel<{c}, {i}, {a}>" for c in (0, 1) for i in ("true", "false")
                     for a in ("true", "false")}
    for x in rows:
        assert not x["dump_variant"]
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        # four-wave blocks, at least two of them per CU
        assert x["VGPRs"] <= 256 and x["LDS Size [bytes/block]"] <= 80 * 1024
