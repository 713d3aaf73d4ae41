"""The packet, fading and frame transmitters write, byte for byte, what the library wrote before what the three kernels
share of the transmit chain went into csrc/ofdm_txchain.h.

tests/golden/transmit_chain_parent.npz holds that library's outputs (tools/record_transmit_exact.py) on the runs of
transmit_exact_cases.py, compared as 32-bit integers, so signed zeros count: short recordings raw, long ones as a
sha256 of the whole recording (untouched samples count) and a digest per packet window (a failure names the packet).
Inputs are made on the host from fixed seeds; the fixture holds their sha256, checked first."""
import numpy as np
import pytest

import transmit_exact_cases as tc
from conftest import load_golden

pytestmark = pytest.mark.gpu

PACKET_CASES = [(k, n) for k in tc.PACKETS for n in tc.PACKETS[k]]


@pytest.fixture(scope="module")
def parent():
    return load_golden("transmit_chain_parent.npz")


def test_fixture_is_complete(parent):
    assert sorted(parent) == sorted(tc.all_keys())
    for kernel, name in PACKET_CASES:
        case = tc.PACKETS[kernel][name]
        pos, n_out = tc.layout(kernel, name)
        assert len(pos) == case["n"]
        if case.get("acc"):                                              # one atomic add per float: no two packets overlap
            assert (np.diff(pos) >= tc.packet_len(case)).all(), name
        if tc.is_raw(kernel, name):
            raw = parent[tc.packet_key(kernel, name, "raw")]
            assert raw.dtype == np.uint32 and raw.shape == (2 * n_out,)
            base = tc.packet_inputs(kernel, name)["base"].view(np.uint32)
            inside = np.zeros(n_out, bool)
            for p in pos:
                inside[min(max(p, 0), n_out):min(max(p + tc.packet_len(case), 0), n_out)] = True
            touched = (raw != base).reshape(-1, 2).any(axis=1)
            assert not touched[~inside].any() and touched[inside].mean() > 0.99, name
        else:
            assert parent[tc.packet_key(kernel, name, "whole")].shape == (32,)
            assert parent[tc.packet_key(kernel, name, "packets")].shape == (case["n"], tc.DIGEST)
    assert {k for k, n in PACKET_CASES if tc.is_raw(k, n)} == {"k7", "k10"}
    for conv in tc.CONVS:
        for nd in tc.WAVE_SYMBOLS:
            assert parent[tc.wave_key(conv, nd, "period")].shape == (2 * (2 * (320 + 80 * nd) + 20),)
        cnt = parent[tc.sweep_key(conv)]
        assert cnt.shape[0] == len(tc.SWEEP_SNRS) and (cnt[:, 0] == tc.SWEEP_TRIALS).all()
        assert cnt[0, 3] > cnt[1, 3] >= 0                                # bit errors at the lower SNR: the rows are not trivial


def compare(parent, got):
    key = next(k for k in got if k.endswith("|input"))
    assert np.array_equal(got[key], parent[key]), f"{key}: the test's input is not the recorded one"
    bad = {}
    for k, g in got.items():
        w = parent[k]
        if g.shape != w.shape:
            bad[k] = f"shape {g.shape} for {w.shape}"
        elif k.endswith("|packets"):
            rows = np.flatnonzero((g != w).any(axis=1))
            if len(rows):
                bad[k] = f"{len(rows)} of {len(w)} packets, first {rows[:8].tolist()}"
        elif not np.array_equal(g, w):
            words = np.flatnonzero(g != w)
            bad[k] = f"{len(words)} of {len(w)} words, first at {words[:8].tolist()}"
    assert not bad, bad


@pytest.mark.parametrize("kernel,name", PACKET_CASES)
def test_packet_outputs_are_the_parents(engine, parent, kernel, name):
    compare(parent, tc.run_packets(engine, kernel, name))


@pytest.mark.parametrize("conv", tc.CONVS)
@pytest.mark.parametrize("nd", tc.WAVE_SYMBOLS)
def test_waveform_is_the_parents(engine, parent, conv, nd):
    got = tc.run_wave(engine, conv, nd)
    bad = {k: int((g != parent[k]).sum()) for k, g in got.items() if g.shape != parent[k].shape or (g != parent[k]).any()}
    assert not bad, bad


@pytest.mark.parametrize("conv", tc.CONVS)
def test_frame_sweep_counters_are_the_parents(engine, pkg, parent, conv):
    got = tc.run_sweep(engine, pkg, conv)
    assert np.array_equal(got[tc.sweep_key(conv)], parent[tc.sweep_key(conv)])
