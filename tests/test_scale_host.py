"""What tests/test_gpu_scale.py rests on, checked without a GPU: the kernels' constants it mirrors are still what the
sources say (a later change of one cannot silently turn its tests back into single-trip tests), its two recordings'
layouts reach the selection branches they are for on a 256-CU device, and the reference alone -- the oracle's noise-free
packet of every one of its 67 payload rows per D, in double precision -- is found exactly once, at packet offset 16,
with a further unconfirmed front and with no position near the threshold.  A noise-free packet's crossings depend on its
own samples only, so the 67 rows decide `found == n_tx`, `positions == tx_pos + 16` and `nothing in the band` for any
number of packets."""
import re

import numpy as np
import pytest

import test_gpu_scale as gs
from conftest import ROOT
from test_gpu_stream import BAND, metric64
from test_gpu_transmit import bits_of

CSRC = ROOT / "ieee-802.11-ofdm-qpsk-simulator_amd" / "csrc"


def test_mirrored_constants_are_the_sources(pkg):
    seen = 0
    for name, consts in gs.MIRRORED.items():
        text = (CSRC / name).read_text()
        for const, value in consts.items():
            m = re.findall(rf"^constexpr int {const} = (\d+);", text, re.M)
            assert m == [str(value)], (name, const, m, value)
            seen += 1
    assert seen == 13
    # samples per channel quad: the tile is CH_QUAD quads' worth of samples per thread
    m = re.findall(r"^constexpr int CH_TILE = (\d+) \* CH_THREADS;", (CSRC / "ofdm_channel.hip").read_text(), re.M)
    assert m == [str(gs.CH_QUAD)] and gs.CH_TILE == 1024
    # the launches are sized as the tests compute them
    stream = (CSRC / "ofdm_stream.hip").read_text()
    assert "std::min<int64_t>(blocks, 2 * (int64_t)c->cus)" in stream
    assert "(nslots + SS_THREADS - 1) / SS_THREADS" in stream and "(lc + SS_SLOT - 1) / SS_SLOT" in stream
    for name, prefix in (("ofdm_transmit.hip", "TXP"), ("ofdm_fading.hip", "FD")):
        text = (CSRC / name).read_text()
        assert f"(int64_t){prefix}_BLOCKS_PER_CU * c->cus" in text and f"{prefix}_GROUP_SYMS / opts->n_data" in text
    chan = (CSRC / "ofdm_channel.hip").read_text()
    assert "std::min<int64_t>(a.tiles, CH_MAX_GRID)" in chan and "(n_tx + SC_THREADS - 1) / SC_THREADS" in chan
    timing = (CSRC / "ofdm_stream_timing.hip").read_text()
    assert "(r.max_packets + TM_WAVES - 1) / TM_WAVES" in timing
    assert "std::min<int64_t>(blocks, TM_BLOCKS_PER_CU * (int64_t)c->cus)" in timing
    assert "i += (int64_t)gridDim.x * TM_WAVES" in timing and "__launch_bounds__(64 * TM_WAVES)" in timing
    abi = pkg.abi
    assert abi.STREAM_TILE == gs.DETECT_TILE and abi.CHANNEL_TILE == gs.CH_TILE
    assert [abi.packet_len(d) for d in gs.DS] == [gs.packet_len(d) for d in gs.DS]


def test_the_recordings_reach_their_branches_on_256_cus():
    cap = 2 * 256
    a, b = gs.layout("A", 256), gs.layout("B", 256)
    for r, lo, hi in ((a, 301, 1000), (b, 301, 2700)):
        plen = gs.packet_len(r["d"])
        gaps = np.diff(np.concatenate([[-plen], r["pos"]])) - plen
        assert gaps.min() >= lo and gaps.max() <= hi and r["n"] - (r["pos"][-1] + plen) >= gs.CLOSING_GAP
        assert r["n"] < 2 ** 31
    assert (a["d"], a["n_tx"]) == (15, 4101) and (b["d"], b["n_tx"]) == (2, 31749)
    # A: three trips of the transmitters with a ragged last group, the decode loop wraps, seven sweeps of the channel
    assert -(-a["n_tx"] // (gs.TXP_GROUP_SYMS // 15)) == 1026 > 2 * cap and a["n_tx"] > gs.SDEC_MAX_WAVES * cap
    assert 1.4e7 < a["n"] < 1.6e7 and a["n"] > 7 * gs.CH_MAX_GRID * gs.CH_TILE
    # B: 1,026 selection blocks, the last ragged, and packets in the slots of phase 1's second trip
    assert b["n"] == 78_995_691
    nslots = -(-(b["n"] - 47) // gs.SS_SLOT)
    assert nslots == 262_444 and -(-nslots // gs.SS_THREADS) == 1026 and nslots % gs.SS_THREADS == 44
    assert -(-b["n_tx"] // (gs.TXP_GROUP_SYMS // 2)) == 1025 > 2 * cap
    late = (b["pos"] + gs.OFFSET - 11) // gs.SS_SLOT >= gs.SS_THREADS * gs.SS_SCAN_THREADS
    assert late[-1] and late.sum() >= 2
    # the same layout every time
    assert np.array_equal(gs.layout("B", 256)["pos"], b["pos"])


@pytest.mark.parametrize("d", gs.DS)
def test_every_payload_row_alone_is_found_once_at_offset_16(pkg, oracle, d):
    from detect_ref import band_is_harmless
    from ofdm_amd.stream import detection_metric, select_packets
    rows = gs.rows_of(d)
    assert rows.shape == (gs.N, 3 * d)
    plen = gs.packet_len(d)
    fronts, margin, last_conf = [], np.inf, 0
    for k, b in enumerate(bits_of(rows)):
        wave = oracle.frame_waveform(b, "c", True, 1)
        assert len(wave) == plen
        for g in (301, 1000):
            x = np.concatenate([np.zeros(g), wave, np.zeros(gs.CLOSING_GAP)])
            m = metric64(x)
            sel = select_packets(m)
            assert sel["positions"].tolist() == [g + gs.OFFSET], (d, k, g, sel["positions"])
            assert len(sel["fronts"]) >= 2 and int(sel["confirmed"].sum()) == 1, (d, k, g, sel["fronts"])
            ok = np.isfinite(m)
            margin = min(margin, float(np.abs(m[ok] - 0.75).min()))
            fronts.append(len(sel["fronts"]))
            last_conf += int(sel["flags"][0] != 0)
            # the conjugate detector places the row alike, and no decision of its lies in the band (a position may)
            mc = detection_metric(x, "conjugate")
            assert select_packets(mc)["positions"].tolist() == [g + gs.OFFSET], (d, k, g)
            assert band_is_harmless(mc, 0.75, BAND), (d, k, g)
    print(f"D {d}: {gs.N} rows x 2 gaps, {np.mean(fronts):.2f} fronts per packet, LAST_FRONT on {last_conf} packets, "
          f"nearest position to the threshold {margin:.3g} away (band {BAND:.3g})")
    assert margin > BAND
