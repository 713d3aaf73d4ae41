"""A compiled C caller of the stream receiver (tests/c_caller/stream_caller.c: include/ofdm_mi355x.h and
include/ofdm_mi355x_stream.h only).

* CPU: gcc compiles and links it against the two headers and the library; the binary binds the library by its
  relative rpath and needs ofdm_receive_stream from it.
* GPU: the program builds the base stream, decodes it and prints its packet list; every field and every bit word
  equals what Engine.receive_stream (ctypes) returns for the stream the program wrote.
"""
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT / "tests" / "c_caller"))
import build_stream_caller  # noqa: E402


def _build(pkg, out_dir):
    from ofdm_amd import build_lib
    return build_stream_caller.build(pkg.abi.LIB_PATH, build_lib.HIPCC, out_dir)


def test_stream_caller_compiles_against_the_headers(pkg, tmp_path):
    exe = _build(pkg, tmp_path)
    assert exe.exists()
    dyn = subprocess.run(["readelf", "-d", str(exe)], capture_output=True, text=True).stdout
    assert "libofdm_mi355x.so" in dyn and "$ORIGIN/" in dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", str(exe)], capture_output=True, text=True).stdout
    for name in ("ofdm_receive_stream", "ofdm_transmitter", "ofdm_ctx_scratch_bytes"):
        assert name in und, name
    src = build_stream_caller.SRC.read_text()
    assert sorted(set(re.findall(r'#include "(\w+\.h)"', src))) == ["ofdm_mi355x.h", "ofdm_mi355x_stream.h"]


@pytest.mark.gpu
def test_stream_caller_matches_engine(engine, pkg, tmp_path):
    exe = build_stream_caller.OUT / "stream_caller"
    if not exe.exists():                       # __graft_entry__.build() makes it in-tree
        exe = _build(pkg, tmp_path / "bin")
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = (tmp_path / "packets.txt").read_text().splitlines()
    found, written = (int(v) for v in lines[0].split())
    x = np.fromfile(tmp_path / "stream.bin", np.float32).view(np.complex64)
    assert len(x) == 15340 and not x[:700].any() and not x[-400:].any()
    got = engine.receive_stream(x, want_bits=True)
    assert (found, written) == (got["found"], got["count"]) and len(lines) == 1 + written
    assert 8 <= found <= 13
    rec = got["records"]
    words = np.packbits(got["bits"].astype(np.uint8), axis=1).view(">u4")
    for k, line in enumerate(lines[1:]):
        v = line.split()
        assert [int(t) for t in v[:5]] == [int(rec[name][k]) for name in ("packet_pos", "flags", "packet_idx", "bit_err",
                                                                          "post_axis_err")], k
        for t, name in zip(v[5:10], ("evm_pre_sum", "evm_db_pre", "ber", "cfo_coarse_hz", "cfo_fine_hz")):
            assert np.float32(float(t)) == rec[name][k], (k, name)
        assert [int(t) for t in v[10:]] == words[k].tolist(), k
