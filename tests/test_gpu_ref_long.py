"""The kernels on frames of 1 and 3..15 data symbols against the reference's own Transmitter stages and Receiver()
(tests/golden/ref_long_*.npz, ref_mc_curve_long.json; tests/ref_long.py rebuilds the captures): the transmitter, the
single-capture receiver, the batched receiver and the frame sweep, with the tolerances of the 2-symbol reference tests
(tests/test_gpu_frame.py, tests/test_gpu_captures.py).  1 is the smallest frame, 3 and 5 the long-capture kernel's small
end, 8 the benchmarked size, 9 / 13 / 15 the ring kernels' first, short-fifth-round and largest shapes.  Only the fixtures
and the oracle library (for the fixtures' Philox noise) are read.

Each test prints its figures before it asserts."""
import numpy as np
import pytest

import ref_long
from conftest import normwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


def set_frames(eng, nd: int) -> None:
    msg = ref_long.tx(nd)["msg"]
    assert (eng.set_long_message(msg) if len(msg) > 96 else eng.set_message(msg)) == nd
    assert eng.payload_frames("message") == nd


@pytest.fixture(scope="module")
def stage_caps(oracle):
    return {nd: ref_long.stage_captures(oracle, nd) for nd in ref_long.FRAMES}


# ---------------------------------------------------------------- A. transmitter
@pytest.mark.parametrize("nd", ref_long.FRAMES)
def test_transmitter_vs_reference(eng, pkg, nd):
    set_frames(eng, nd)
    w = eng.transmitter("c", "message")
    ref = ref_long.tx(nd)["wave"]
    e = normwise(w, ref)
    print(f"D={nd}: waveform normwise {e:.3g}")
    assert len(w) == pkg.abi.wave_len(nd) == len(ref)
    assert e < 2e-6


# ---------------------------------------------------------------- B. single-capture receiver
@pytest.mark.parametrize("nd", ref_long.FRAMES)
def test_receiver_vs_reference_stages(eng, pkg, stage_caps, nd):
    """test_gpu_frame.test_receiver_vs_reference_stages' assertions on the 8 cases of every frame size"""
    set_frames(eng, nd)
    g = ref_long.stages(nd)
    assert stage_caps[nd].shape == (8, pkg.abi.capture_len(nd))
    out = [eng.receiver(cap, "c", "message") for cap in stage_caps[nd]]
    print(f"D={nd}: packet_idx {[o['packet_idx'] for o in out]} reference {g['packet_idx'].tolist()}, worst eq "
          f"{max(normwise(o['eq'], g['nopilot'][k]) for k, o in enumerate(out)):.3g}, EVM_dB "
          f"{max(abs(float(o['res'][0]) - float(g['res'][k][0])) for k, o in enumerate(out)):.3g}")
    for k, o in enumerate(out):
        assert o["frames"] == nd and not o["oob"]
        assert o["packet_idx"] == int(g["packet_idx"][k]), k
        ref_eq = g["nopilot"][k]
        assert normwise(o["eq"], ref_eq) < 1e-4, k
        assert not np.any((o["bits"] != g["bits"][k]) & ~ref_long.near_pairs(ref_eq)), k
        assert o["res"][2] == pytest.approx(float(g["res"][k][2]), abs=1e-6)
        assert o["res"][0] == pytest.approx(float(g["res"][k][0]), abs=2e-3)


# ---------------------------------------------------------------- C. batched receiver
@pytest.mark.parametrize("nd", ref_long.FRAMES)
def test_reference_stages_in_one_batch(eng, stage_caps, nd):
    """test_gpu_captures.test_reference_stages_in_one_batch's assertions, one batch per frame size"""
    set_frames(eng, nd)
    g = ref_long.stages(nd)
    out = eng.receive_captures(stage_caps[nd], want_bits=True, want_eq=True)
    rec = out["records"]
    print(f"D={nd}: packet_idx {rec['packet_idx'].tolist()} reference {g['packet_idx'].tolist()}, worst eq "
          f"{max(normwise(out['eq'][k], g['nopilot'][k]) for k in range(8)):.3g}, EVM_dB "
          f"{np.max(np.abs(rec['evm_db_pre'] - g['res'][:, 0])):.3g}")
    assert len(rec) == 8 and out["bits"].shape == (8, 96 * nd) and out["eq"].shape == (8, 48 * nd)
    for k in range(8):
        assert int(rec["packet_idx"][k]) == int(g["packet_idx"][k]), k
        ref_eq = g["nopilot"][k]
        assert normwise(out["eq"][k], ref_eq) < 1e-4, k
        assert not np.any((out["bits"][k] != g["bits"][k]) & ~ref_long.near_pairs(ref_eq)), k
        assert float(rec["ber"][k]) == pytest.approx(float(g["res"][k][2]), abs=1e-6)
        assert float(rec["evm_db_pre"][k]) == pytest.approx(float(g["res"][k][0]), abs=2e-3)
        assert int(rec["flags"][k]) == int(g["packet_idx"][k] == 0)        # sync-fail bit alone: no late frame


@pytest.mark.parametrize("nd", ref_long.BULK_FRAMES)
def test_thousand_captures_vs_reference(eng, pkg, oracle, nd):
    """1,000 captures at 6..25 dB in one receive_captures call against the reference's Receiver() on each"""
    set_frames(eng, nd)
    b = ref_long.bulk(nd)
    caps = ref_long.bulk_captures(oracle, nd)
    rec = eng.receive_captures(caps, want_bits=False)["records"]
    gp, rp = rec["packet_idx"].astype(np.int64), b["packet_idx"].astype(np.int64)
    off = ~b["on_threshold"]
    same = gp == rp
    dev = np.abs(rec["bit_err"].astype(np.int64) - b["bit_err"])
    print(f"D={nd}: packet_idx differs on {int(np.sum(~same))} of 1000 ({int(np.sum(~same & off))} off the threshold), "
          f"{int(np.sum(rp == 0))} reference sync failures, bit-error counts differ on {int(np.sum(dev[same] > 0))} "
          f"captures (worst excess over `near`: {int(np.max((dev - b['near'])[same]))})")
    assert len(rec) == 1000 and off.sum() >= 995
    assert np.array_equal(gp[off], rp[off])
    assert np.all(dev[same] <= b["near"][same])
    assert np.array_equal((rec["flags"] & pkg.abi.CAPTURE_SYNC_FAIL) != 0, gp == 0)
    assert not np.any(rec["flags"] & pkg.abi.CAPTURE_OOB)


# ---------------------------------------------------------------- D. frame sweep against the reference's trial loop
@pytest.mark.parametrize("nd", [8, 15])
def test_frame_sweep_vs_reference_curve(eng, pkg, nd):
    """Engine.frame_sweep, 16 batches of 5,000 trials per point, against ref_mc_trials after set_message (20,000 trials
    per point).  BER: |z| < 5 with the GPU's standard error from its batch spread and the reference's from its
    per-trial BER variance plus a pseudo-count of one failed frame (test_reference_ber_curve_within_tenth_db).  Mean
    per-trial EVM_dB before the slicer: 5 standard errors of the difference plus 0.03 dB for the RNG difference; after
    it, finite against finite or -inf by the expected count of error-free trials (test_reference_evm_curve)."""
    set_frames(eng, nd)
    curve = ref_long.curve(nd)
    snr = np.array(sorted(curve))
    rows = [curve[s] for s in snr]
    cfg = pkg.make_cfg(payload="message")
    K, B = 16, 5000
    cnt = np.array([eng.frame_sweep(cfg, snr, B, first_trial=k * B) for k in range(K)])        # [K, n_snr, 16]
    assert np.all(cnt[:, :, 0] == B) and np.all(cnt[:, :, 2] == B * 96 * nd)
    ber_b = cnt[:, :, 3] / cnt[:, :, 2]
    pre_b = cnt[:, :, 9] / 2.0 ** 20 / cnt[:, :, 0]
    post_b = cnt[:, :, 10] / 2.0 ** 20 / np.maximum(cnt[:, :, 11], 1)
    fin, frames = cnt[:, :, 11].sum(axis=0), cnt[:, :, 0].sum(axis=0)
    checks = []
    for i, r in enumerate(rows):
        n_ref = float(r["trials"])
        ber = ber_b[:, i].mean()
        se_gpu = ber_b[:, i].std(ddof=1) / np.sqrt(K)
        se_ref = np.sqrt((r["ber_trial_var"] * n_ref + 0.25) / n_ref ** 2)
        z = (ber - r["ber"]) / np.hypot(se_gpu, se_ref)
        m = pre_b[:, i].mean()
        sd = pre_b[:, i].std(ddof=1)
        tol = 5 * np.hypot(sd / np.sqrt(K), sd * np.sqrt(B / n_ref)) + 0.03
        lam = (frames[i] - fin[i]) / frames[i] * n_ref     # error-free trials expected in the reference's sample
        print(f"D={nd} {r['snr_db']:5.1f} dB  BER GPU {ber:.4e} reference {r['ber']:.4e} z {z:+.2f}   EVM pre GPU {m:8.3f} "
              f"reference {r['mean_evm_db']:8.3f} diff {m - r['mean_evm_db']:+.3f} tol {tol:.3f}   post: reference "
              f"{r['mean_evm_agc_db']}, expected error-free trials {lam:.3g}")
        checks.append((r, z, m, tol, lam, i))
    for r, z, m, tol, lam, i in checks:
        assert abs(z) < 5, (r["snr_db"], z)
        assert abs(m - r["mean_evm_db"]) < tol, (r["snr_db"], m, r["mean_evm_db"], tol)
        ref_post = r["mean_evm_agc_db"]
        if np.isfinite(ref_post):
            assert lam < 5, (r["snr_db"], lam)
            mp, sp = post_b[:, i].mean(), post_b[:, i].std(ddof=1)
            tolp = 5 * np.hypot(sp / np.sqrt(K), sp * np.sqrt(B / r["trials"])) + 0.03
            print(f"D={nd} {r['snr_db']:5.1f} dB  EVM post: GPU {mp:8.3f}  reference {ref_post:8.3f}  tol {tolp:.3f}")
            assert abs(mp - ref_post) < tolp, (r["snr_db"], mp, ref_post)
        else:
            assert lam > 0.01, (r["snr_db"], lam)
