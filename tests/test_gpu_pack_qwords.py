"""The LS AWGN packed receiver's staged Philox products (ofdm_rxpack.hip `qw`, ofdm_device.h philox_qword) against
the oracle, at the smallest shapes that reach each way the array is filled and read.

The item's prologue stages, per (table slot, lane), round 3's c2 product of the lane's frame; the SNR loop reads it
back with one per-lane read per Philox block.  A wrong staged word changes all four Gaussians of that block at
every SNR point of the frame, so the counters of the row leave test C's bounds (tests/test_gpu_symbol_shapes.py
check_vs_oracle) at once.  The cases:
  frames   1, 63, 64, 65 and 3 x 64 + 1: one lane, a ragged group, a full one, a second group of one lane, four;
  points   1, 3, 5, 17: waves with no iteration, an uneven split over the four waves, more than one round per wave;
  grid     capped at 1 and 2 blocks (OFDM_RX_GRID_CAP): one block refills the array item after item; with 3 blocks
           the 193 frames' fourth group is a tail group whose SNR points are split over three items (sub > 0);
  row      first_frame = 2^32 - 128 with 3 x 64 frames: two groups on table row 0, neither straddling, and the third
           starting exactly at 2^32 on row 1.
An SNR point's counters depend only on (frame, q, snr[q]) (test B of test_gpu_symbol_shapes.py), so the oracle runs
once per (convention, first frame, frames) on the 17-point grid and its leading rows serve the shorter grids.  The
oracle alone is checked first, without a GPU: its rows stay inside check_vs_oracle's own condition on the number of
near-threshold decisions, and they are not trivial (bit errors at the low points, none at the high ones)."""
import numpy as np
import pytest

from test_gpu_symbol_shapes import F0, SEED, check_vs_oracle, oracle_rows, set_cap

SNR17 = np.linspace(-2.0, 22.0, 17)
FRAMES = (1, 63, 64, 65, 3 * 64 + 1)
POINTS = (1, 3, 5, 17)
ROW_FIRST, ROW_FRAMES = 2 ** 32 - 128, 3 * 64
CONVS = ("c", "matlab")


def _kw(conv):
    return dict(est="ls", noise="real", channel="awgn", conv=conv)


def _caps(nf):
    return (1, 2, 3) if nf == 3 * 64 + 1 else (1, 2)


@pytest.mark.parametrize("conv", CONVS)
def test_oracle_alone_meets_the_bounds_conditions(oracle, conv):
    """no GPU: what check_vs_oracle asks of the oracle's own rows, for every input of this file"""
    for first, nf in [(F0, n) for n in FRAMES] + [(ROW_FIRST, ROW_FRAMES)]:
        o, N, NFq = oracle_rows(oracle, _kw(conv), SEED, first, nf, SNR17)
        assert np.all(N <= 28), (first, nf, N.max())
        assert o.shape[0] == 17 and np.all(o[:, 0] == nf)
        if nf >= 63:
            assert np.all(o[:3, 3] > 0) and np.all(o[-3:, 3] == 0), (first, nf, o[:, 3])


@pytest.mark.gpu
@pytest.mark.parametrize("nf", FRAMES)
@pytest.mark.parametrize("conv", CONVS)
def test_staged_words_vs_oracle(engine, oracle, pkg, monkeypatch, conv, nf):
    kw = _kw(conv)
    cfg = pkg.make_cfg(**kw)
    o, N, NFq = oracle_rows(oracle, kw, SEED, F0, nf, SNR17)
    tx, bits = engine.tx_frames(cfg, F0, nf)
    for cap in _caps(nf):
        set_cap(monkeypatch, cap)
        for n in POINTS:
            g = engine.rx_frames(cfg, tx, bits, F0, nf, SNR17[:n]).cpu().numpy()
            check_vs_oracle(f"qwords {conv} frames {nf} points {n} cap {cap}", kw, g, o[:n], N[:n], NFq[:n], nf)


@pytest.mark.gpu
@pytest.mark.parametrize("conv", CONVS)
def test_table_row_switch_at_2_to_32(engine, oracle, pkg, monkeypatch, conv):
    kw = _kw(conv)
    cfg = pkg.make_cfg(**kw)
    o, N, NFq = oracle_rows(oracle, kw, SEED, ROW_FIRST, ROW_FRAMES, SNR17)
    tx, bits = engine.tx_frames(cfg, ROW_FIRST, ROW_FRAMES)
    for cap in (None, 1, 2):
        set_cap(monkeypatch, cap)
        for n in (3, 17):
            g = engine.rx_frames(cfg, tx, bits, ROW_FIRST, ROW_FRAMES, SNR17[:n]).cpu().numpy()
            check_vs_oracle(f"qwords {conv} row switch points {n} cap {cap}", kw, g, o[:n], N[:n], NFq[:n], ROW_FRAMES)
