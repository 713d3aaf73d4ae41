"""The reference fixtures for frames of 1 and 3..15 data symbols (tests/golden/ref_long_*.npz, ref_mc_curve_long.json,
written by tests/golden/gen_golden.py --only long from the compiled reference) and the rule that rebuilds their captures.
Shared by tests/test_ref_long.py (the oracle and the harness, CPU) and tests/test_gpu_ref_long.py (the kernels); nothing
here needs the reference."""
from __future__ import annotations

import functools
import json

import numpy as np

from conftest import GOLDEN, load_golden

FRAMES = (1, 3, 5, 8, 9, 13, 15)
BULK_FRAMES = (1, 8, 15)
FIXTURE_TAG = 0xF1000000
BULK_KEY = (0xB01C, 1)


@functools.lru_cache(maxsize=None)
def _file(name: str) -> dict:
    return load_golden(name)


def _of(name: str, nd: int) -> dict:
    pre = f"d{nd}_"
    return {k[len(pre):]: v for k, v in _file(name).items() if k.startswith(pre)}


@functools.lru_cache(maxsize=None)
def tx(nd: int) -> dict:
    """msg (bytes), wave (ten periods, complex64), bits, payload_mod, dims of the nd-symbol frame"""
    g = _of("ref_long_tx.npz", nd)
    wave = np.tile(g["period"], 10)
    wave.setflags(write=False)
    return dict(msg=g["msg"].tobytes(), wave=wave, bits=g["bits"].astype(np.int32), payload_mod=g["payload_mod"],
                dims=g["dims"])


def cap_len(nd: int) -> int:
    return int(len(tx(nd)["wave"]) * 0.307)                              # OFDM.c:945


def capture(oracle, nd: int, case: int, rs: int, sigma: float, key) -> np.ndarray:
    """The fixtures' rule (their `rule` entry): wave[rs:rs+L] + float32(sigma z), z the oracle's Philox Gaussians of
    the blocks (b, case, nd, FIXTURE_TAG) under `key` -- real-only noise on the captured window."""
    w = tx(nd)["wave"]
    L = cap_len(nd)
    z = oracle.gauss_fill([case, nd, FIXTURE_TAG], key, L)
    return (w[rs:rs + L] + (float(sigma) * z).astype(np.float32)).astype(np.complex64)


def stages(nd: int) -> dict:
    """the 8 stage cases of the nd-symbol frame: arrays with the case as the first axis"""
    return _of("ref_long_stages.npz", nd)


def stage_captures(oracle, nd: int) -> np.ndarray:
    g = stages(nd)
    return np.stack([capture(oracle, nd, k, int(g["rs"][k]), float(g["sigma"][k]), (int(g["seed"][k]), 0))
                     for k in range(len(g["rs"]))])


def bulk(nd: int) -> dict:
    return _of("ref_long_bulk.npz", nd)


def bulk_captures(oracle, nd: int, count: int | None = None) -> np.ndarray:
    g = bulk(nd)
    n = len(g["rs"]) if count is None else count
    return np.stack([capture(oracle, nd, int(g["case"][k]), int(g["rs"][k]), float(g["sigma"][k]), BULK_KEY)
                     for k in range(n)])


def near_pairs(ref_eq: np.ndarray) -> np.ndarray:
    """per bit: its carrier has a component within 1e-4 of the slicer threshold (test_receiver_stages_vs_reference)"""
    return np.repeat((np.abs(ref_eq.real) < 1e-4) | (np.abs(ref_eq.imag) < 1e-4), 2)


def curve(nd: int) -> dict:
    rows = json.loads((GOLDEN / "ref_mc_curve_long.json").read_text())["rows"]
    return {r["snr_db"]: r for r in rows if r["frames"] == nd}
