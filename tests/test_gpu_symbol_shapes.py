"""The symbol-mode receivers (rx_pack_kernel, rx_ls_kernel, rx_ideal_kernel) against the oracle at every launch
shape and across the SNR slices of one call.

A launch's grid is min(groups, blocks per CU x CUs): on a large device every small batch runs one item per block
and the work queue (a.work), the strided rounds and the packed receiver's split tail are never taken.  The test
switch OFDM_RX_GRID_CAP (rx_grid, read on every call) limits the grid, so that a few hundred frames reach every
shape on any device:
  A  every capped shape gives the uncapped launch's counters bit for bit (all 11 configurations);
  B  an SNR point's counters depend only on (frame, q, snr[q]): prefixes of a 70-point grid (two launches: q_base 0
     and 64), the fused Tx builds and chunked sweeps reproduce the rows of the one-batch result exactly;
  C  that result against the oracle, every counter, every row;
  D  the dump launches across the slice boundary against the oracle's soft values and bits;
  E  frame indices across 2^31 (the symbol index 2f + d carries into Philox counter word 1) and 2^32 (the frame's
     own high word), and a seed with a non-zero high word (Philox key word 1).

Tolerances.  Integer counters are exact except for decisions whose oracle soft value lies within DECISION_EPS of
the slicer threshold (N[q] subcarriers in NF[q] frames of row q, counted on the oracle's dump): one such
subcarrier flips at most one axis = at most two bits, one such frame at most one frame-level count.  The EVM sums
use the bounds the suite asserts for the same counters elsewhere (test_rx_chain_vs_oracle,
test_rayleigh_ls_mc_matches_oracle_mc, test_frame_sweep_evm_counters_vs_oracle).  In the noiseless chains the
per-frame EVM_dB (counter 9) is each side's own rounding floor (double: about -305 dB; fp32: 96 terms of
(a few 2^-24)^2, about -130 dB; the kernels floor it at -400 dB), so there the two are not compared with each
other: the GPU's mean must lie in [-400, -100] dB (test_noiseless_full_size's bound) and the oracle's below -250 dB."""
import ctypes

import numpy as np
import pytest

from test_gpu_symbol import CONFIGS, DECISION_EPS, tile_symbol

pytestmark = pytest.mark.gpu

NF, F0 = 293, 123456789          # 4 x 64 + 37: 5 packed groups, 14 LS groups of 21 frames, 10 ideal groups, all ragged
SEED = 0x80211A
SNR70 = np.concatenate([np.linspace(-2, 21, 64), [3.0, 9.0, 15.0, 27.0, 40.0, 0.5]])   # rows 64..69: second launch
SNR3 = np.array([0.0, 6.0, 20.0])
Q20 = 2.0 ** 20


def _id(kw):
    return "-".join(kw.values())


def _packed(kw):          # rx_pack_applies (ofdm_rxpack.hip)
    return kw["noise"] == "real" and (kw["channel"] == "awgn" or kw["est"] == "ls")


PACKED = [kw for kw in CONFIGS if _packed(kw)]
assert len(CONFIGS) == 11 and len(PACKED) == 6


def set_cap(monkeypatch, cap):
    """OFDM_RX_GRID_CAP for the following receiver calls (None: unset); the C library must see it"""
    if cap is None:
        monkeypatch.delenv("OFDM_RX_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("OFDM_RX_GRID_CAP", str(cap))
    getenv = ctypes.CDLL(None).getenv
    getenv.restype = ctypes.c_char_p
    assert getenv(b"OFDM_RX_GRID_CAP") == (None if cap is None else str(cap).encode())


# ---------------------------------------------------------------------------------------------- shared results
_ORACLE, _GPU = {}, {}
FIGURES = {}              # (test, config, case) -> the largest deviation per counter, printed by the tests


def oracle_rows(oracle, kw, seed, f0, nf, snr):
    """the oracle's counters, and per row N (subcarriers within DECISION_EPS of a threshold) and NF (frames that
    hold one); computed once per (config, seed, first frame, frames, grid) and shared"""
    key = (_id(kw), seed, f0, nf, np.asarray(snr, np.float64).tobytes())
    if key not in _ORACLE:
        cnt, eq, _ = oracle.symbol_sweep(oracle.cfg(seed=seed, **kw), snr, f0, nf, dumps=True)
        near = (np.abs(eq.real) < DECISION_EPS) | (np.abs(eq.imag) < DECISION_EPS)
        res = (cnt, near.sum(axis=(1, 2, 3)), near.any(axis=(2, 3)).sum(axis=1))
        for a in res:
            a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def gpu_rows(engine, pkg, monkeypatch, kw, nf=NF):
    """the uncapped one-batch result on SNR70: ofdm_rx_frames on an ofdm_tx_frames batch (two launches)"""
    key = (_id(kw), nf)
    if key not in _GPU:
        set_cap(monkeypatch, None)
        cfg = pkg.make_cfg(**kw)
        tx, bits = engine.tx_frames(cfg, F0, nf)
        c = engine.rx_frames(cfg, tx, bits, F0, nf, SNR70).cpu().numpy()
        c.setflags(write=False)
        _GPU[key] = c
    return _GPU[key]


def check_vs_oracle(tag, kw, g, o, N, NFq, nf):
    """test C's bounds, every counter of every row; records and prints the largest deviations first"""
    d = np.abs(g - o)
    rel7 = d[:, 7] / np.maximum(o[:, 7], 1)
    noiseless = kw["noise"] == "none"
    fig = {"N_max": int(N.max()), "NF_max": int(NFq.max()), "bit_err": int(d[:, 3].max()), "frame_err": int(d[:, 4].max()),
           "evm_post_axis": int(d[:, 8].max()), "evmdb_post_finite": int(d[:, 11].max()),
           "evm_pre_rel": float(rel7.max()), "evmdb_pre_db_per_frame": float((d[:, 9] / Q20 / nf).max()),
           "evmdb_post_db_per_frame": float((d[:, 10] / Q20 / nf).max())}
    if noiseless:
        fig["evmdb_pre_db_per_frame"] = None
        fig["gpu_mean_frame_evm_db"] = [float((g[:, 9] / Q20 / nf).min()), float((g[:, 9] / Q20 / nf).max())]
    FIGURES[tag] = fig
    print(f"{tag}: {fig}")
    assert np.all(N <= 28), N.max()                      # 0.1 % of a row's 293 x 96 decisions
    for k in (0, 1, 2, 5, 6, 12, 13, 14, 15):            # frames, symbols, bits, (sync failures), EVM terms, (unused)
        assert np.array_equal(g[:, k], o[:, k]), k
    bad = np.nonzero(d[:, 3] > 2 * N)[0]
    assert bad.size == 0, ("bit_err", bad, g[bad, 3], o[bad, 3], N[bad])
    bad = np.nonzero(d[:, 8] > 2 * N)[0]
    assert bad.size == 0, ("evm_post_axis", bad, g[bad, 8], o[bad, 8], N[bad])
    bad = np.nonzero(d[:, 4] > NFq)[0]
    assert bad.size == 0, ("frame_err", bad, g[bad, 4], o[bad, 4], NFq[bad])
    bad = np.nonzero(d[:, 11] > NFq)[0]
    assert bad.size == 0, ("evmdb_post_finite", bad, g[bad, 11], o[bad, 11], NFq[bad])
    # EVM sums: the pooled one as test_rx_chain_vs_oracle (AWGN, ideal CSI) / test_rayleigh_ls_mc_matches_oracle_mc
    # (LS estimate of the Rayleigh channel), the per-frame dB ones as test_frame_sweep_evm_counters_vs_oracle
    tol7 = 1e-3 if kw["channel"] == "rayleigh4" and kw["est"] == "ls" else 1e-4
    bad = np.nonzero(rel7 >= tol7)[0]
    assert bad.size == 0, ("evm_pre_q", bad, g[bad, 7], o[bad, 7])
    if noiseless:
        m_g, m_o = g[:, 9] / Q20 / nf, o[:, 9] / Q20 / nf
        assert np.all((m_g >= -400.0) & (m_g <= -100.0)) and np.all(m_o < -250.0), (m_g, m_o)
    else:
        bad = np.nonzero(d[:, 9] / Q20 > 1e-3 * nf)[0]
        assert bad.size == 0, ("evmdb_pre_q", bad, g[bad, 9], o[bad, 9])
    bad = np.nonzero(d[:, 10] / Q20 > 1e-3 * nf + 25.0 * (d[:, 8] + d[:, 11]))[0]
    assert bad.size == 0, ("evmdb_post_q", bad, g[bad, 10], o[bad, 10], d[bad, 8], d[bad, 11])


# ---------------------------------------------------------------------------------------------- A
def tail_split(G, B):
    """rx_pack_kernel's items: R full rounds of B groups, then T tail groups with their SNR points split S ways"""
    R = G // B
    T = G - R * B
    S = max(1, min(4, B // T)) if T else 1
    return R, T, S


A_SHAPES = [(NF, None), (NF, 1), (NF, 2), (NF, 3), (NF, 4), (229, 3)]        # (frames, cap)


def test_shapes_cover_the_tail_rule():
    """what A's shapes are for: the packed receiver's (groups G, blocks B) pairs reach every split S = 1..4, a
    launch with full rounds ahead of a tail, and a one-block launch"""
    gb = [((nf + 63) // 64, min((nf + 63) // 64, cap)) for nf, cap in A_SHAPES if cap is not None]
    rts = {p: tail_split(*p) for p in gb}
    assert rts[(5, 4)] == (1, 1, 4) and rts[(5, 3)] == (1, 2, 1) and rts[(5, 2)] == (2, 1, 2)
    assert rts[(5, 1)] == (5, 0, 1) and rts[(4, 3)] == (1, 1, 3)
    assert {s for r, t, s in rts.values() if t > 0} == {1, 2, 3, 4}
    assert any(r >= 2 and t > 0 for r, t, s in rts.values())
    assert any(b == 1 for g, b in gb)


@pytest.mark.parametrize("kw", CONFIGS, ids=_id)
def test_launch_shape_identity(engine, pkg, monkeypatch, kw):
    """A: the counters of a launch do not depend on its grid (rounds, queue order, tail split)"""
    cfg = pkg.make_cfg(**kw)
    base, bad = {}, []
    for nf, cap in A_SHAPES:
        if cap is None or nf not in base:
            base[nf] = gpu_rows(engine, pkg, monkeypatch, kw, nf)
        if cap is None:
            continue
        set_cap(monkeypatch, cap)
        tx, bits = engine.tx_frames(cfg, F0, nf)
        got = engine.rx_frames(cfg, tx, bits, F0, nf, SNR70).cpu().numpy()
        diff = np.argwhere(got != base[nf])
        if diff.size:
            bad.append((nf, cap, "rows", sorted(set(diff[:, 0].tolist())), "columns", sorted(set(diff[:, 1].tolist()))))
    assert not bad, bad
    assert base[NF][0, 0] == NF and base[229][0, 0] == 229


# ---------------------------------------------------------------------------------------------- B
def _same_batch(torch, a, b, abits, bbits, nf):
    n_sym = (2 * nf + 63) // 64 * 64
    ga = a.view(torch.uint8).cpu().numpy().reshape(80, -1)[:, :8 * n_sym]
    gb = b.view(torch.uint8).cpu().numpy().reshape(80, -1)[:, :8 * n_sym]
    return np.array_equal(ga, gb) and np.array_equal(abits.cpu().numpy().reshape(10, -1)[:, :n_sym],
                                                     bbits.cpu().numpy().reshape(10, -1)[:, :n_sym])


@pytest.mark.parametrize("kw", PACKED, ids=_id)
def test_snr_prefixes_slices_and_fused_builds(engine, pkg, monkeypatch, kw):
    """B: row q depends only on (frame, q, snr[q]) -- not on how many points the call has, which launch of the
    call holds it, which block of a split tail runs it, or which launch builds the batches"""
    import torch
    cfg = pkg.make_cfg(**kw)
    full = gpu_rows(engine, pkg, monkeypatch, kw)
    tx_ref, bits_ref = engine.tx_frames(cfg, F0, NF)
    nx_ref, nxb_ref = engine.tx_frames(cfg, F0 + NF, 700)
    # q is the row of the whole grid, not of the launch: rows 64..69 draw the noise streams 64..69, so they differ
    # from the rows 0..5 of a call on the same six SNR values (streams 0..5) in every noise-dependent sum
    set_cap(monkeypatch, None)
    alias = engine.rx_frames(cfg, tx_ref, bits_ref, F0, NF, SNR70[64:]).cpu().numpy()
    same = [64 + i for i in range(6) if alias[i, 7] == full[64 + i, 7] or alias[i, 9] == full[64 + i, 9]]
    assert not same, same
    for cap in (None, 4, 2):              # cap 4: S = 4, sub-blocks without an SNR point at small n
        set_cap(monkeypatch, cap)
        bad = []
        for n in (1, 3, 5, 16, 17, 63, 64, 65, 70):
            got = engine.rx_frames(cfg, tx_ref, bits_ref, F0, NF, SNR70[:n]).cpu().numpy()
            diff = np.argwhere(got != full[:n])
            if diff.size:
                bad.append((n, "rows", sorted(set(diff[:, 0].tolist()))))
        assert not bad, (cap, bad)
        # both batches built inside the first launch; the second launch (rows 64..69) reads the first one's
        tx, bits = engine.tx_buffers(NF)
        nx, nxb = engine.tx_buffers(700)
        for t in (tx, nx):
            t.fill_(-1.0)
        for t in (bits, nxb):
            t.fill_(-1)
        engine.set_next_tx(cfg, F0 + NF, 700, nx, nxb)
        _, _, cnt = engine.txrx_frames(cfg, F0, NF, SNR70, tx, bits)
        torch.cuda.synchronize()
        diff = np.argwhere(cnt.cpu().numpy() != full)
        assert diff.size == 0, (cap, diff[:8])
        assert _same_batch(torch, tx_ref, tx, bits_ref, bits, NF), cap
        assert _same_batch(torch, nx_ref, nx, nxb_ref, nxb, 700), cap
    # three chunks (128, 128, 37 frames) of two launches each, the next chunk's batch built in a chunk's first launch
    for cap in (None, 1):
        set_cap(monkeypatch, cap)
        got = engine.symbol_sweep(cfg, SNR70, NF, first_frame=F0, chunk_frames=128)
        diff = np.argwhere(got != full)
        assert diff.size == 0, (cap, diff[:8])


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("kw", CONFIGS, ids=_id)
def test_counters_vs_oracle_70_points(engine, oracle, pkg, monkeypatch, kw):
    """C: the non-dump receivers against the oracle, all counters, all 70 rows (A ties every other shape to this
    run exactly).  The allowance for near-threshold decisions is small and the rows are not trivial: asserted on
    the oracle's output alone."""
    o, N, NFq = oracle_rows(oracle, kw, SEED, F0, NF, SNR70)
    if kw["noise"] == "none":
        assert not o[:, 3].any() and not N.any()         # nothing to flip: every integer counter is exact
    else:
        assert np.count_nonzero(o[:, 3]) >= 30, np.count_nonzero(o[:, 3])
        if kw["channel"] == "awgn":
            assert np.count_nonzero(o[:, 3] == 0) >= 20
    g = gpu_rows(engine, pkg, monkeypatch, kw)
    check_vs_oracle(f"C {_id(kw)}", kw, g, o, N, NFq, NF)


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("kw", PACKED, ids=_id)
def test_dumps_across_the_slice_boundary(engine, oracle, pkg, monkeypatch, kw):
    """D: ofdm_rx_frames_dump on 70 points: each launch's offset into the dumps and the counters (rows 64..69:
    the second launch), with test_rx_chain_vs_oracle's assertions"""
    set_cap(monkeypatch, None)
    nf = 45
    cfg = pkg.make_cfg(**kw)
    tx, bits = engine.tx_frames(cfg, F0, nf)
    cnt, eq, db = engine.rx_frames_dump(cfg, tx, bits, F0, nf, SNR70)
    cnt = cnt.cpu().numpy(); eq = eq.cpu().numpy(); db = db.cpu().numpy().astype(np.uint32)
    plain = engine.rx_frames(cfg, tx, bits, F0, nf, SNR70).cpu().numpy()
    # reported, not asserted: the two launches are different template instantiations of the kernel
    same = np.array_equal(plain, cnt)
    cols = np.nonzero(np.any(plain != cnt, axis=0))[0]
    FIGURES[f"D {_id(kw)}"] = {"dump_counters_equal_non_dump": bool(same),
                               "rows_that_differ": int(np.count_nonzero(np.any(plain != cnt, axis=1))),
                               "columns_that_differ": cols.tolist(),
                               "largest_relative_difference": {int(k): float(np.max(
                                   np.abs(plain[:, k] - cnt[:, k]) / np.maximum(np.abs(plain[:, k]), 1))) for k in cols}}
    print(f"D {_id(kw)}: {FIGURES[f'D {_id(kw)}']}")
    ocnt, oeq, obits = oracle.symbol_sweep(oracle.cfg(**kw), SNR70, F0, nf, dumps=True)
    gbits = ((db[..., :, None] >> (31 - np.arange(32))) & 1).reshape(*db.shape[:-1], 96)
    near = np.repeat((np.abs(oeq.real) < DECISION_EPS) | (np.abs(oeq.imag) < DECISION_EPS), 2, axis=-1)
    for rows in (slice(0, 64), slice(64, 70)):
        err = np.abs(eq[rows] - oeq[rows]) / (1.0 + np.abs(oeq[rows]))
        assert np.quantile(err, 0.999) < 1e-4 and np.max(err) < 5e-3, (rows, np.max(err))
        assert not np.any((gbits[rows] != obits[rows]) & ~near[rows]), rows
        n_near = int(near[rows].sum())
        for k in (0, 1, 2, 6):
            assert np.array_equal(cnt[rows, k], ocnt[rows, k]), (rows, k)
        assert np.all(np.abs(cnt[rows, 3] - ocnt[rows, 3]) <= n_near), rows
        assert np.all(np.abs(cnt[rows, 4] - ocnt[rows, 4]) <= n_near), rows
        rel = np.abs(cnt[rows, 7] - ocnt[rows, 7]) / np.maximum(ocnt[rows, 7], 1)
        assert np.all(rel < 1e-4), (rows, rel)


# ---------------------------------------------------------------------------------------------- E
E_CONFIGS = [dict(est="ls", noise="real", channel="awgn", conv="c"),
             dict(est="ls", noise="real", channel="rayleigh4", conv="c"),
             dict(est="ideal", noise="real", channel="awgn", conv="c"),
             dict(est="ls", noise="complex", channel="awgn", conv="c")]
E_CASES = [(SEED, 2 ** 32 - 150), (SEED, 2 ** 31 - 150), (0x5EED00C0FFEE1234, 777)]


@pytest.mark.parametrize("seed,first", E_CASES, ids=["frame-2^32", "frame-2^31", "seed-64-bit"])
@pytest.mark.parametrize("kw", E_CONFIGS, ids=_id)
def test_32_bit_boundaries_and_64_bit_seed(engine, oracle, pkg, monkeypatch, kw, seed, first):
    """E: frames first .. first + 292 with the boundary (where there is one) between frame 149 and 150"""
    set_cap(monkeypatch, None)
    assert kw in CONFIGS
    cfg = pkg.make_cfg(seed=seed, **kw)
    g = engine.symbol_sweep(cfg, SNR3, NF, first_frame=first)
    o, N, NFq = oracle_rows(oracle, kw, seed, first, NF, SNR3)
    check_vs_oracle(f"E {_id(kw)} seed {seed:#x} first {first}", kw, g, o, N, NFq, NF)
    halves = engine.symbol_sweep(cfg, SNR3, 150, first_frame=first) + \
        engine.symbol_sweep(cfg, SNR3, NF - 150, first_frame=first + 150)
    assert np.array_equal(g, halves)


@pytest.mark.parametrize("seed,first", [(SEED, 2 ** 31 - 150), (0x5EED00C0FFEE1234, 2 ** 31 - 150)],
                         ids=["seed-32-bit", "seed-64-bit"])
def test_payload_words_across_symbol_2_to_32(engine, oracle, pkg, seed, first):
    """E: ofdm_tx_frames' payload words of the symbols either side of symbol index 2^32 (frame 2^31), as
    test_tx_symbols_vs_oracle: Philox counter word 1 is the symbol index's high word, key word 1 the seed's"""
    nf = 293
    tx, bits = engine.tx_frames(pkg.make_cfg(seed=seed), first, nf)
    seen = set()
    for s in (0, 298, 299, 300, 301, 2 * nf - 1):
        _, words = tile_symbol(tx, bits, s)
        gs = 2 * first + s
        seen.add(gs >> 32)
        ref = oracle.philox([gs & 0xffffffff, gs >> 32, 0, 0xB1750000], [seed & 0xffffffff, seed >> 32])[:3]
        assert np.array_equal(words, ref), (s, gs)
    assert seen == {0, 1}
