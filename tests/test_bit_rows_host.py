"""Bit rows 3..9 of a Tx batch (no GPU): demap_word / pair_words (ofdm_rxcommon.h), which build the words by
two-bit field moves, against the reference loops that state them a bit at a time (demap_word_ref, pair_words_ref),
and against this suite's own numpy statement of the words (test_gpu_symbol.py).  The functions are
__host__ __device__; tests/host/bitrows_check.hip calls them on the host (compiled here for the host alone, with
the library's compiler and include paths).  The QPSK map's own check is a static_assert in the same header, so
compiling the program checks it too."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_symbol import demap_words, pair_words


@pytest.fixture(scope="module")
def exe(pkg, tmp_path_factory):
    from ofdm_amd import build_lib as bl
    out = tmp_path_factory.mktemp("bitrows") / "bitrows_check"
    cmd = [bl.HIPCC, "--cuda-host-only", "-O1", "-std=c++17", f"-I{bl.INCLUDE}", f"-I{bl.CSRC}",
           str(ROOT / "tests" / "host" / "bitrows_check.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _words():
    rng = np.random.default_rng(96)
    rnd = rng.integers(0, 2 ** 32, (10 ** 4, 3), dtype=np.uint64).astype(np.uint32)
    single = np.zeros((96, 3), np.uint32)
    for b in range(96):
        single[b, b >> 5] = np.uint32(1) << np.uint32(31 - (b & 31))
    return np.concatenate([rnd, np.zeros((1, 3), np.uint32), np.full((1, 3), 0xFFFFFFFF, np.uint32), single, ~single])


def test_field_moves_equal_the_bit_loops(exe, tmp_path):
    w = _words()
    assert w.shape == (10 ** 4 + 2 + 2 * 96, 3)
    w.tofile(tmp_path / "in.bin")
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.uint32).reshape(-1, 14)
    assert out.shape[0] == w.shape[0]
    bad = np.nonzero(np.any(out[:, :7] != out[:, 7:], axis=1))[0]
    assert bad.size == 0, (bad[:5], w[bad[:5]], out[bad[:5]])
    # the words themselves: every payload bit is used (all-ones maps to a non-zero pattern, a single bit moves it)
    assert np.all(out[10 ** 4] == 0) and np.all(out[10 ** 4 + 1, :7] != 0)
    assert np.all(np.any(out[10 ** 4 + 2:10 ** 4 + 2 + 96, :7] != 0, axis=1))
    # and against the suite's numpy statement of rows 3..6 and 7..9, on a sample
    for k in list(range(0, 200)) + list(range(10 ** 4, w.shape[0])):
        b96 = ((w[k][:, None] >> (31 - np.arange(32, dtype=np.uint32))) & 1).reshape(96)
        assert np.array_equal(out[k, :4], demap_words(b96)), k
        assert np.array_equal(out[k, 4:7], pair_words(b96)), k
