"""The runs behind tests/golden/pack_counters_parent.npz, shared by the test that compares with the fixture
(test_gpu_pack_exact.py) and the script that records it (tools/record_pack_counters.py).

Every configuration the packed receivers take (rx_pack_applies, ofdm_rxpack.hip), 293 frames (5 ragged groups):
  base      first frame 123456789 on the 70-point grid (two launches: q_base 0 and 64);
  straddle  first frame 2^32 - 150: group 2's 64 frames straddle the frame index's high word;
  edge      first frame 2^32 - 128: the high word changes between groups 1 and 2 -- with the grid capped to one
            block that block crosses the boundary between two of its items, uncapped no block does;
  seed64    a seed with a non-zero high word (Philox key word 1).
Each through ofdm_rx_frames on an ofdm_tx_frames batch, ofdm_txrx_frames with a pending ofdm_set_next_tx, and
ofdm_symbol_sweep in chunks of 128 frames."""
import numpy as np

NF, F0, SEED = 293, 123456789, 0x80211A
SNR70 = np.concatenate([np.linspace(-2, 21, 64), [3.0, 9.0, 15.0, 27.0, 40.0, 0.5]])
SNR3 = np.array([0.0, 6.0, 20.0])

PACKED = [
    dict(est="ls", noise="real", channel="awgn", conv="c"),
    dict(est="ls", noise="real", channel="awgn", conv="matlab"),
    dict(est="ideal", noise="real", channel="awgn", conv="c"),
    dict(est="ideal", noise="real", channel="awgn", conv="matlab"),
    dict(est="ls", noise="real", channel="rayleigh4", conv="c"),
    dict(est="ls", noise="real", channel="rayleigh4", conv="matlab"),
]

# name -> (seed, first frame, SNR grid, grid cap)
CASES = {
    "base": (SEED, F0, SNR70, None),
    "straddle": (SEED, 2 ** 32 - 150, SNR3, None),
    "edge-cap1": (SEED, 2 ** 32 - 128, SNR3, 1),
    "edge": (SEED, 2 ** 32 - 128, SNR3, None),
    "seed64": (0x5EED00C0FFEE1234, F0, SNR3, None),
}
PATHS = ("rx_frames", "txrx_frames", "symbol_sweep")


def config_id(kw):
    return "-".join(kw.values())


def key(kw, case, path):
    return f"{config_id(kw)}|{case}|{path}"


def run_case(engine, pkg, kw, case, set_cap):
    """{path: counters} of one configuration and case; set_cap(cap) sets OFDM_RX_GRID_CAP (None: unset)"""
    import torch
    seed, first, snr, cap = CASES[case]
    cfg = pkg.make_cfg(seed=seed, **kw)
    set_cap(cap)
    out = {}
    tx, bits = engine.tx_frames(cfg, first, NF)
    out["rx_frames"] = engine.rx_frames(cfg, tx, bits, first, NF, snr).cpu().numpy()
    tx, bits = engine.tx_buffers(NF)
    nx, nxb = engine.tx_buffers(700)
    engine.set_next_tx(cfg, first + NF, 700, nx, nxb)
    _, _, cnt = engine.txrx_frames(cfg, first, NF, snr, tx, bits)
    torch.cuda.synchronize()
    out["txrx_frames"] = cnt.cpu().numpy()
    out["symbol_sweep"] = engine.symbol_sweep(cfg, snr, NF, first_frame=first, chunk_frames=128)
    set_cap(None)
    return out
