"""The packed receivers' counters are bit for bit those of the library before the truth signs moved from the
pair-order words (Tx rows 7..9) to the sign bits of the clean spectra (demap_bin, ofdm_rxpack.hip).

tests/golden/pack_counters_parent.npz holds the counters that library gave (tools/record_pack_counters.py) for every
configuration rx_pack_applies accepts, on the runs of pack_exact_cases.py: 5 ragged groups in two launches, a group
that straddles frame index 2^32, the boundary between two groups (on one block, which crosses it between two of its
items, and uncapped), and a 64-bit seed -- each through ofdm_rx_frames, ofdm_txrx_frames with a pending
ofdm_set_next_tx and the chunked ofdm_symbol_sweep.  The two boundary cases are also held against the oracle."""
import numpy as np
import pytest

import pack_exact_cases as pc
from conftest import load_golden
from test_gpu_symbol_shapes import PACKED, check_vs_oracle, oracle_rows, set_cap

pytestmark = pytest.mark.gpu

assert all(kw in pc.PACKED for kw in PACKED) and len(pc.PACKED) == len(PACKED) == 6
assert dict(est="ls", noise="real", channel="awgn", conv="matlab") in pc.PACKED

_GPU = {}


@pytest.fixture(scope="module")
def parent():
    return load_golden("pack_counters_parent.npz")


def gpu_case(engine, pkg, monkeypatch, kw, case):
    k = (pc.config_id(kw), case)
    if k not in _GPU:
        res = pc.run_case(engine, pkg, kw, case, lambda cap: set_cap(monkeypatch, cap))
        for a in res.values():
            a.setflags(write=False)
        _GPU[k] = res
    return _GPU[k]


def test_fixture_is_complete(parent):
    assert sorted(parent) == sorted(pc.key(kw, case, path) for kw in pc.PACKED for case in pc.CASES for path in pc.PATHS)
    for kw in pc.PACKED:
        base = parent[pc.key(kw, "base", "rx_frames")]
        assert base.shape[0] == 70 and np.all(base[:, 0] == pc.NF)
        assert np.count_nonzero(base[:, 3]) >= 30                # bit errors: the rows are not trivial


@pytest.mark.parametrize("case", list(pc.CASES))
@pytest.mark.parametrize("kw", pc.PACKED, ids=pc.config_id)
def test_counters_are_the_parents(engine, pkg, monkeypatch, parent, kw, case):
    got = gpu_case(engine, pkg, monkeypatch, kw, case)
    bad = []
    for path in pc.PATHS:
        want = parent[pc.key(kw, case, path)]
        if not np.array_equal(got[path], want):
            diff = np.argwhere(got[path] != want) if got[path].shape == want.shape else None
            bad.append((path, None if diff is None else (sorted(set(diff[:, 0].tolist()))[:8],
                                                         sorted(set(diff[:, 1].tolist())))))
    assert not bad, bad


@pytest.mark.parametrize("case", ["straddle", "edge-cap1", "edge"])
@pytest.mark.parametrize("kw", pc.PACKED, ids=pc.config_id)
def test_boundary_cases_vs_oracle(engine, oracle, pkg, monkeypatch, kw, case):
    seed, first, snr, _ = pc.CASES[case]
    o, N, NFq = oracle_rows(oracle, kw, seed, first, pc.NF, snr)
    g = gpu_case(engine, pkg, monkeypatch, kw, case)["rx_frames"]
    check_vs_oracle(f"pack-exact {pc.config_id(kw)} {case}", kw, g, o, N, NFq, pc.NF)
