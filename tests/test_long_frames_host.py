"""Long messages (include/ofdm_mi355x_long.h: frames of 9..15 data symbols), the checks that need no GPU: the
extension header against the library and the binding, the frame geometry, the build-id guard of the PMC-certified
kernels, and frame_ring_xl_kernel's capture ring (csrc/ofdm_frame_xl.hip) with its index arithmetic restated in numpy
as tests/test_long_ring.py does for frame_sync_long_kernel: every float a detection round or a matched-filter run
reads must be the capture sample it means and lie inside ring + mirror, for every capture offset, packet position and
lazy stopping round.  A ring slot here holds the sample index last written to it."""
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

XL_CHUNK, XL_ROUND = 31, 64 * 31
XL_PIECE = XL_ROUND + 47
XL_RING, XL_EXT = 2976, 96
XL_TABLE_REACH = 2048
MF_RUN = 5


def long_header_functions():
    h = (ROOT / "include" / "ofdm_mi355x_long.h").read_text()
    return sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))


def test_long_header_is_exported_and_bound(pkg):
    names = long_header_functions()
    assert "ofdm_set_long_message" in names
    assert names == sorted(pkg.abi.LONG_EXPORTS)
    assert not set(names) & set(pkg.abi.EXPORTS)                 # the base header's list is frozen
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg.abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), name
    assert lib.ofdm_set_long_message(None, None, 0, None) == -1 and lib.ofdm_last_error()
    h = pkg.abi.LONG_HEADER.read_text()
    assert re.search(r"#define OFDM_LONG_MSG_MAX_CHARS 180\b", h) and re.search(r"#define OFDM_LONG_MAX_DATA_SYMBOLS 15\b", h)
    assert pkg.abi.LONG_MSG_MAX_CHARS == 180 and pkg.abi.LONG_MAX_DATA_SYMBOLS == 15
    assert "2,909" in h and "2,973" in h                          # the cap and its reason are stated
    assert lib.ofdm_abi_version() == 1


def test_long_frame_geometry(pkg):
    abi = pkg.abi
    assert abi.wave_len(15) == 30600 and abi.capture_len(15) == 9394
    assert abi.wave_len(9) == 21000 and abi.wave_len(13) == 27400
    # detection rounds per frame length, and the matched-filter window against the ring
    for nd, rounds, last in ((9, 4, 448), (13, 5, 428), (15, 5, 1411)):
        lc = abi.capture_len(nd) - 47
        assert -(-lc // XL_ROUND) == rounds and lc - (rounds - 1) * XL_ROUND == last
        assert 2 * (320 + 80 * nd) - 131 <= XL_RING - 3
    assert 2 * (320 + 80 * 15) - 131 == 2909 and 2 * (320 + 80 * 16) - 131 > XL_RING - 3


def test_certified_kernels_did_not_move(pkg):
    """The PMC records (profiles/pmc_summary.json) are measurements of one build of each kernel; bench.py reports a
    roofline fraction only while the library's kernels still carry the recorded build ids."""
    from ofdm_amd import codeobj
    rec = json.loads((ROOT / "profiles" / "pmc_summary.json").read_text())
    ids = {w: r["build_id"] for w, r in rec.items() if isinstance(r, dict) and "build_id" in r}
    assert {"c2", "c3", "c5", "fft64", "frame", "frame8"} <= set(ids)
    for w, bid in ids.items():
        assert codeobj.workload_build_id(pkg.abi.LIB_PATH, w) == bid, w


def test_long_kernels_are_built_spill_free(pkg):
    from ofdm_amd import build_lib
    if not build_lib.RESOURCE_REPORT.exists():
        pytest.skip("library not built in this tree (no resource report)")
    rows = {x["name"]: x for x in json.loads(build_lib.RESOURCE_REPORT.read_text())}
    for k in ("ofdm::frame_ring_xl_kernel", "ofdm::frame_whole_xl_kernel", "ofdm::frame_sym_xl_kernel<false>"):
        assert k in rows, k
        assert not rows[k].get("VGPRs Spill", 0) and not rows[k].get("ScratchSize [bytes/lane]", 0), k
    assert rows["ofdm::frame_sym_xl_kernel<true>"]["dump_variant"]
    # 11-wave blocks need 3 waves on a SIMD: at most 168 VGPRs
    assert rows["ofdm::frame_ring_xl_kernel"]["VGPRs"] <= 168
    assert rows["ofdm::frame_sym_xl_kernel<false>"]["VGPRs"] <= 168


# ---------------------------------------------------------------- the ring kernel's index arithmetic
def red(x):
    """the kernel's three unsigned reductions: x mod XL_RING for 0 <= x < 4 XL_RING"""
    m = 0xFFFFFFFF
    x &= m
    for _ in range(3):
        x = min(x, (x - XL_RING) & m)
    return x


class Ring:
    def __init__(self, rx_start):
        self.off, self.b0 = rx_start & 3, rx_start >> 2
        self.rx = rx_start
        self.f = np.full(XL_RING + XL_EXT, -10**9, np.int64)

    def gen(self, n_lo, n_hi):
        """capture_blocks_xl(..., b0, (rx + n_lo) >> 2, (rx + n_hi - 1) >> 2)"""
        for b in range((self.rx + n_lo) >> 2, ((self.rx + n_hi - 1) >> 2) + 1):
            assert 0 <= 4 * (b - self.b0) < 4 * XL_RING
            pos = red(4 * (b - self.b0))
            assert pos % 4 == 0 and pos + 4 <= XL_RING
            samples = 4 * b - self.rx + np.arange(4)
            self.f[pos:pos + 4] = samples
            if pos < XL_EXT:
                self.f[pos + XL_RING:pos + XL_RING + 4] = samples

    def at(self, n):
        assert 0 <= n + self.off < 4 * XL_RING
        return red(n + self.off)


def check_round(ring, rho, L, period, im0):
    """detection round rho: lane l loads 80 floats (5 blocks of 16) from ring(n0) and from the table at the round's
    reduced base + 31 l; positions [n0, n1) use samples [n0, n1 + 47)"""
    Lc = L - 47
    base_i = (im0 + rho * XL_ROUND) % period
    for lane in range(64):
        n0 = rho * XL_ROUND + lane * XL_CHUNK
        n1 = min(n0 + XL_CHUNK, Lc)
        if n0 >= n1:
            continue
        base = ring.at(n0)
        assert base + 80 <= XL_RING + XL_EXT                      # the block loads stay inside ring + mirror
        need = np.arange(n0, n1 + 47)
        assert np.array_equal(ring.f[base:base + len(need)], need), (rho, lane)
        assert base_i + lane * XL_CHUNK + 80 <= period + XL_TABLE_REACH
        # table float base_i + 31 l + k is Im of waveform sample (rx + n0 + k) mod period
        assert (base_i + lane * XL_CHUNK) % period == (ring.rx + n0) % period


def mf_starts(n_data):
    return [s for a, e in [(80, 112), (192, 320)] + [(336 + 80 * d, 400 + 80 * d) for d in range(n_data)]
            for s in range(a, e, MF_RUN)]


@pytest.mark.parametrize("n_data", [9, 13, 15])
def test_ring_reads_are_the_samples_meant(n_data):
    rng = np.random.default_rng(n_data)
    nfr = 320 + 80 * n_data
    wave_len = 10 * (2 * nfr + 20)
    period = wave_len // 10
    L = int(0.307 * wave_len)
    Lc = L - 47
    R = -(-Lc // XL_ROUND)
    assert R == (4 if n_data == 9 else 5)
    assert len(mf_starts(n_data)) == 33 + 13 * n_data <= 4 * 64   # XL_MAXP passes of 64 runs
    starts = mf_starts(n_data)
    cases = 0
    # every rx_start & 3, every stopping round (lazy after rounds 1..R-2, the full rule after R-1), packets across the capture
    for off in range(4):
        for stop in range(1, R):
            for k in range(14):
                rx = 4 * int(rng.integers(0, (wave_len - L) // 4)) + off
                if k == 0:
                    rx = off
                elif k == 1:
                    rx = (wave_len - L - 1) // 4 * 4 - 4 + off
                im0 = rx % period
                ring = Ring(rx)
                ring.gen(0, min(L, XL_PIECE))
                check_round(ring, 0, L, period, im0)
                for rho in range(1, stop + 1):
                    ring.gen(rho * XL_ROUND, min(L, rho * XL_ROUND + XL_PIECE))
                    check_round(ring, rho, L, period, im0)
                held = stop
                # a lazily decided front has its +230 check and a later front inside the rounds done; the full rule
                # (stop == R - 1) can pick any front of the capture; a failed sync gives p = 0
                limit = min((stop + 1) * XL_ROUND, Lc)
                hi_p = limit - 300 if stop < R - 1 else Lc - 300
                grid = np.linspace(11, hi_p + 10, 12).astype(int)
                p = 0 if k == 2 else int(grid[k - 2]) if k >= 2 else int(rng.integers(11, hi_p + 11))
                lo, hi = p + 2 * 80 - 20, min(p + 2 * (nfr - 1) + 10, L - 1)
                res_hi = min(L, held * XL_ROUND + XL_PIECE)
                res_lo = res_hi + 3 - XL_RING
                if hi >= res_hi:
                    ring.gen(max(lo, res_hi), hi + 1)
                elif lo < res_lo:
                    ring.gen(lo, min(hi + 1, res_lo))
                im_mf = im0 + p - 20 + period
                for s0 in starts:
                    n_lo = p + 2 * s0 - 20
                    e = min(s0 + MF_RUN, next(b for a, b in [(80, 112), (192, 320)] +
                                              [(336 + 80 * d, 400 + 80 * d) for d in range(n_data)] if a <= s0 < b))
                    if n_lo < 0 or p + 2 * (e - 1) >= L:
                        continue                                  # the per-instant path (ring(mc) per sample)
                    base = ring.at(n_lo)
                    assert base + 2 * MF_RUN + 19 <= XL_RING + XL_EXT
                    # the floats the run's outputs use: [n_lo, n_lo + 2 (e - s0 - 1) + 21)
                    need = np.arange(n_lo, n_lo + 2 * (e - s0 - 1) + 21)
                    assert np.array_equal(ring.f[base:base + len(need)], need), (rx, stop, p, s0)
                    assert 0 <= im_mf + 2 * s0 < 1 << 14          # ImMod's exact range
                    si = (im_mf + 2 * s0) % period
                    assert si + 2 * MF_RUN + 19 <= period + XL_TABLE_REACH
                    assert si == (rx + n_lo) % period
                for mc in ((lo, hi, (lo + hi) // 2) if lo <= hi else ()):   # the per-instant path's single reads
                    assert ring.f[ring.at(mc)] == mc
                cases += 1
    assert cases == 4 * (R - 1) * 14
