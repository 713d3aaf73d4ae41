"""The capture, stream and tracking receivers write, byte for byte, what the library wrote before the three kernels'
copies of the post-selection chain became one (csrc/ofdm_rxchain.h).

tests/golden/decode_chain_parent.npz holds that library's raw outputs (tools/record_decode_exact.py) on the runs of
decode_exact_cases.py: the records, d_bits, d_eq, the counters row and d_phase, compared as integers, so NaN payloads and
signed zeros count.  Inputs are made on the host from fixed seeds; the fixture holds their sha256, checked first."""
import numpy as np
import pytest

import decode_exact_cases as dc
from conftest import load_golden

pytestmark = pytest.mark.gpu

OOB, LAST_FRONT, SYNC_FAIL = 2, 4, 1


@pytest.fixture(scope="module")
def parent():
    return load_golden("decode_chain_parent.npz")


def stream_records(pkg, parent, name, tracking):
    raw = parent[dc.stream_key(name, tracking, "records")]
    return raw.view(pkg.abi.stream_packet_dtype()).reshape(-1)


def test_fixture_is_complete(pkg, parent):
    assert sorted(parent) == sorted(dc.all_keys())
    for name, (nd, packets, _, _, _, bits, eq, counters, max_packets, _, cut, _) in dc.STREAMS.items():
        for tracking in dc.TRACKING:
            found, count = parent[dc.stream_key(name, tracking, "count")]
            rec = stream_records(pkg, parent, name, tracking)
            assert found == packets and count == len(rec) == (packets if max_packets is None else max_packets), name
            assert parent[dc.stream_key(name, tracking, "words")].size == (3 * nd * count if bits else 0)
            assert parent[dc.stream_key(name, tracking, "eq")].size == (2 * 48 * nd * count if eq else 0)
            assert parent[dc.stream_key(name, tracking, "phase")].size == (nd * count if tracking == "pilots" else 0)
            row = parent[dc.stream_key(name, tracking, "counters")]
            assert len(row) == (pkg.abi.NCOUNTERS if counters else 0)
            if counters:
                assert row[pkg.abi.C_FRAMES] == count and row[pkg.abi.C_BIT_ERR] == rec["bit_err"].sum()
            if name in dc.NOISY_STREAMS:
                assert rec["bit_err"].sum() > 0, (name, tracking)        # bit errors: the records are not trivial
            if cut is None:
                assert not (rec["flags"] & OOB).any(), name
                continue
            # the last packet runs past the end; zfirst as the kernels form it
            p, n = int(rec["packet_pos"][-1]), 700 + (packets - 1) * (2 * (320 + 80 * nd) + 20) + cut
            zfirst = min(max((n - 652 - p + 159) // 160, 0), nd)
            assert rec["flags"][-1] & OOB and not (rec["flags"][:-1] & OOB).any(), name
            if name == "d4-noltf":
                assert zfirst == 0 and np.isnan(rec["evm_pre_sum"][-1]) and np.isnan(rec["evm_db_pre"][-1])
            else:
                assert 0 < zfirst < nd and np.isfinite(rec["evm_pre_sum"][-1]), (name, zfirst)
    for name, (nd, L, _, _, _, _, bits, eq, counters) in dc.CAPTURES.items():
        rec = parent[dc.capture_key(name, "records")].view(pkg.abi.capture_result_dtype()).reshape(-1)
        kinds = np.array([k for k, _ in dc.ROWS])
        assert len(rec) == len(kinds)
        assert parent[dc.capture_key(name, "words")].size == (3 * nd * len(rec) if bits else 0)
        assert parent[dc.capture_key(name, "eq")].size == (2 * 48 * nd * len(rec) if eq else 0)
        assert parent[dc.capture_key(name, "counters")].size == (pkg.abi.NCOUNTERS if counters else 0)
        assert (rec["flags"][kinds == "noise"] == SYNC_FAIL).all(), name
        assert (rec["flags"][kinds == "early"] == 0).all() and (rec["flags"][kinds == "oob"] == OOB).all(), name
        assert rec["bit_err"][kinds == "early"].sum() > 0, name
        nfr = 320 + 80 * nd
        if L >= 4 * nfr + 20:                                            # the late row's packet: lo = p - 20 >= nfr
            late = rec[kinds == "late"]
            assert (late["flags"] == 0).all() and (late["packet_idx"] - 20 >= nfr).all(), name
        p = int(rec["packet_idx"][kinds == "oob"][0])
        assert 0 < min(max((L - 652 - p + 159) // 160, 0), nd) < nd, name


def differing(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} for {want.shape}"
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else f"{len(bad)} of {len(want)} words, first at {bad[:8].tolist()}"


def compare(parent, got):
    key = next(k for k in got if k.startswith("input|"))
    assert np.array_equal(got[key], parent[key]), f"{key}: the test's input is not the recorded one"
    bad = {k: d for k in got if (d := differing(got[k], parent[k])) is not None}
    assert not bad, bad


@pytest.mark.parametrize("name", list(dc.STREAMS))
def test_stream_outputs_are_the_parents(engine, pkg, parent, name):
    compare(parent, dc.run_stream(engine, pkg, name))


@pytest.mark.parametrize("name", list(dc.CAPTURES))
def test_capture_outputs_are_the_parents(engine, pkg, parent, name):
    compare(parent, dc.run_captures(engine, pkg, name))
