#!/usr/bin/env python3
"""Generate the committed golden fixtures from the COMPILED REFERENCE (oracle/_ref, built from the
unmodified /root/reference/src/OFDM.c) and from the reference's own data files.

Run in the build container (the GPU box has no /root/reference):
    python tests/golden/gen_golden.py [--only mc] [--mc-trials 48000 --mc-deep-trials 1000000]
    python tests/golden/gen_golden.py --only long [--procs 8]      (the four ref_long_* / ref_mc_curve_long files only)

Outputs (all plain data, loadable with numpy allow_pickle=False / json):
  fft_vectors.npz      200 random 64-pt inputs and the reference's fft()/ifft() outputs (OFDM.c:314-339)
  tx_waveform.npz      Transmitter() output (9800 cf32), Data bits, Data_Payload_Mod, Long_preamble_slot_Frequency,
                       RRC taps (OFDM.c:20-34, 467-618)
  rx_stages.npz        Receiver() intermediates for injected-noise captures (OFDM.c:941-1165)
  matlab_output.npz    the 96 KAT bits of data/Matlab_Output.txt (MATLAB Tester RX_Payload_1_demod)
  reference_data.json  the four data/Output_*.txt files of the reference run (format fixtures)
  ref_mc_curve.json    Monte-Carlo BER/EVM of the reference's own trial loop (TOA+Receiver) per SNR
  ref_genie_ls_curve.json  genie-timed symbol chain built from the reference's own ifft/fft/
                       Channel_Estimation (two separately noised LTF windows), real noise
                       sigma^2 = 0.4980 * 52/4096 / snr: pins symbol mode's LS estimator statistically
  ref_symbol_chain_curve.json  the same chain entirely from the reference's stage functions and its
                       gaussian_noise, 0..30 dB step 2, 2e6 frames at 8 / 10 dB and 1e7 at 12 dB (>= 1,000 bit
                       errors each) with per-frame error statistics (frame-clustered BER variance)
Frames of 1, 3, 5, 8, 9, 13 and 15 data symbols (--only long; RefLib.set_message builds the frame from the reference's
own stage functions, Receiver() then runs unmodified):
  ref_long_tx.npz      per frame size: the message, one period of the waveform (the ten are asserted identical), Data
                       bits, Data_Payload_Mod, dims
  ref_long_stages.npz  per frame size 8 injected-noise captures through Receiver(): packet_idx, H, equalised carriers,
                       bits, Res.  No noise is stored: a capture is rebuilt from (frames, case, rs, sigma, seed) by the
                       rule in the file's `rule` entry (Philox Gaussians of the oracle, stream tag 0xF1000000)
  ref_long_bulk.npz    1,000 captures each at 1, 8 and 15 symbols: packet_idx, bit errors, carriers near the slicer
                       threshold, and whether the sync decision sits on Packet_Selection's 0.75 threshold
  ref_mc_curve_long.json  ref_mc_curve.json's rows for 8 and 15 symbols: 20,000 trials at 6, 8, 10, 12, 14, 20 dB
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
from oracle import RefLib, build_ref  # noqa: E402

REF_DATA = Path("/root/reference/data")


def gen_fft(R: RefLib):
    rng = np.random.default_rng(802111)
    x = (rng.standard_normal((200, 64)) + 1j * rng.standard_normal((200, 64))).astype(np.complex64)
    # include structured vectors: impulses, constants, OFDM-like sparse spectra
    x[0] = 0; x[0, 0] = 1
    x[1] = 0; x[1, 17] = 1 - 2j
    x[2] = 1
    f = np.stack([R.fft(v) for v in x])
    i = np.stack([R.ifft(v) for v in x])
    np.savez_compressed(HERE / "fft_vectors.npz", x=x, fft=f, ifft=i)


def gen_tx(R: RefLib):
    g = R.globals()
    np.savez_compressed(HERE / "tx_waveform.npz", waveform=R.waveform(), bits=g["bits"],
                        payload_mod=g["payload_mod"], ltf_freq=g["ltf_freq"], dims=g["dims"],
                        rrc_taps=R.rrc_taps())


def gen_rx(R: RefLib):
    w = R.waveform()
    P = float(np.mean(np.abs(w.astype(np.complex128)) ** 2))
    cases = [(30.0, 0, 11), (20.0, 1234, 12), (14.0, 777, 13), (10.0, 3000, 14), (8.0, 50, 15),
             (6.0, 6000, 16), (12.0, 4321, 17), (100.0, 0, 18)]
    out = {"snr": [], "rx_start": [], "noise": [], "packet_idx": [], "corr": [], "rxframe": [],
           "coarse": [], "fine": [], "H": [], "Yf": [], "nopilot": [], "bits": [], "res": [], "res_receiver": []}
    for snr, rs, seed in cases:
        rng = np.random.default_rng(seed)
        sigma = np.sqrt(P / 10 ** (snr / 10))
        # injected real-only noise (D7) on the captured window only
        noise = np.zeros(len(w), np.float32)
        noise[rs:rs + 3008] = (sigma * rng.standard_normal(3008)).astype(np.float32)
        ota = (w + noise).astype(np.complex64)
        d = R.receiver_stages(ota, rs)
        rr = R.receiver(ota, rs)
        assert np.array_equal(np.nan_to_num(rr, neginf=-999), np.nan_to_num(d["res"], neginf=-999)), (rr, d["res"])
        out["snr"].append(snr); out["rx_start"].append(rs); out["noise"].append(noise[rs:rs + 3008])
        out["packet_idx"].append(d["packet_idx"]); out["res_receiver"].append(rr)
        for k in ("corr", "rxframe", "coarse", "fine", "H", "Yf", "nopilot", "bits", "res"):
            out[k].append(d[k])
    np.savez_compressed(HERE / "rx_stages.npz", **{k: np.array(v) for k, v in out.items()})


def gen_kat():
    kat = np.array([int(float(t)) for t in (REF_DATA / "Matlab_Output.txt").read_text().split()], np.int32)
    np.savez_compressed(HERE / "matlab_output.npz", bits=kat)
    files = {n: (REF_DATA / n).read_text() for n in
             ("Output_SNR.txt", "Output_EVM_AGC.txt", "Output_EVM_AGC_DB.txt", "Output_BER.txt")}
    (HERE / "reference_data.json").write_text(json.dumps(files, indent=1))


# fftshifted data bins / pilots of the subcarrier map (OFDM.c:523-548)
DATA_IDX = np.array([*range(6, 11), *range(12, 25), *range(26, 32), *range(33, 39), *range(40, 53), *range(54, 59)])
PILOTS = {11: 1.0, 25: 1.0, 39: 1.0, 53: -1.0}


def gen_genie(R: RefLib, frames: int = 20000, snrs=(0.0, 2.0, 4.0, 6.0)):
    rng = np.random.default_rng(80211)
    T = R.ifft(R.globals()["ltf_freq"])                       # long training symbol, C ifft (D5)
    ltf160 = np.concatenate([T[32:], T, T])
    s2 = 1 / np.sqrt(2)
    rows = []
    for snr in snrs:
        sigma = np.sqrt(0.4980 * 52 / 4096 / 10 ** (snr / 10))
        nbits = nerr = 0
        epre = 0.0
        for _ in range(frames):
            frame = np.zeros(480, np.complex64)
            frame[160:320] = ltf160
            bits = rng.integers(0, 2, (2, 96))
            for d in range(2):
                b0, b1 = bits[d, 0::2], bits[d, 1::2]
                # 00:(1+j) 01:(-1+j) 10:(-1-j) 11:(1-j), /sqrt2 (OFDM.c:423-430)
                q = (np.where(b0 == b1, 1.0, -1.0) + 1j * np.where(b0 == 1, -1.0, 1.0)) * s2
                X = np.zeros(64, np.complex64)
                X[DATA_IDX] = q
                for k, v in PILOTS.items():
                    X[k] = v
                x = R.ifft(X)
                frame[320 + 80 * d:400 + 80 * d] = np.concatenate([x[48:], x])
            rx = (frame + (sigma * rng.standard_normal(480)).astype(np.float32)).astype(np.complex64)  # D7
            H = R.channel_estimation(rx)
            for d in range(2):
                Y = R.fft(rx[336 + 80 * d:400 + 80 * d])
                z = Y[DATA_IDX].astype(np.complex128) / H[DATA_IDX]
                pr, pi = z.real > 0, z.imag > 0
                c0, c1 = (~pi).astype(int), (pr != pi).astype(int)
                nerr += int(np.sum(c0 != bits[d, 0::2]) + np.sum(c1 != bits[d, 1::2]))
                nbits += 96
                b0, b1 = bits[d, 0::2], bits[d, 1::2]
                ref = (np.where(b0 == b1, 1.0, -1.0) + 1j * np.where(b0 == 1, -1.0, 1.0)) * s2
                epre += float(np.sum(np.abs(z - ref) ** 2))
        rows.append({"snr_db": snr, "frames": frames, "bits": nbits, "bit_err": nerr, "evm_terms": nbits // 2,
                     "sum_evm_pre": epre})
    meta = {"generator": "tests/golden/gen_golden.py gen_genie",
            "source": "reference ifft/fft/Channel_Estimation (OFDM.c:314-339, 830-850), numpy real noise",
            "rows": rows}
    (HERE / "ref_genie_ls_curve.json").write_text(json.dumps(meta, indent=1))


CHAIN_SNRS = [float(x) for x in range(0, 31, 2)]            # bench.py's SNR grid
CHAIN_FRAMES = 200_000                                     # per point: EVM to ~0.001 dB, BER down to 4 dB
CHAIN_DEEP = {8.0: 2_000_000, 10.0: 2_000_000, 12.0: 10_000_000}   # >= 1,000 bit errors each
CHAIN_JOB = 100_000                                        # frames per job, seeded by job index


def _chain_worker(args):
    snr, n, seed = args
    return snr, RefLib().symbol_chain_stats(snr, n, seed).tolist()


def chain_jobs(snrs=CHAIN_SNRS) -> list:
    jobs = []
    for snr in snrs:
        n = CHAIN_DEEP.get(snr, CHAIN_FRAMES)
        jobs += [(snr, CHAIN_JOB, 3000017 * (j + 1) + int(snr)) for j in range(n // CHAIN_JOB)]
    return jobs


def chain_rows(res: list) -> list:
    """fixture rows from (snr, acc5) job results, summed in job order"""
    acc = {}
    for snr, a in res:
        acc[snr] = [x + y for x, y in zip(acc.get(snr, [0.0] * 5), a)]
    rows = []
    for snr in sorted(acc):
        be, nb, epre, be2, fe = acc[snr]
        rows.append({"snr_db": snr, "frames": int(nb) // 192, "bits": int(nb), "bit_err": int(be),
                     "evm_terms": int(nb) // 2, "sum_evm_pre": epre, "sum_frame_err_sq": int(be2),
                     "frames_with_err": int(fe)})
    return rows


def gen_chain(procs: int):
    """ref_symbol_chain_curve.json: the genie symbol chain built from the reference's own stage functions
    (ref_harness.c ref_time_symbol_chain: QPSK_Modulator, ifft, gaussian_noise, Channel_Estimation, fft,
    AGC_Receiver, QPSK_Demodulator -- OFDM.c:415-433, 320-339, 622-655, 830-850, 314-318, 852-908) over the
    bench's SNR grid, with the per-frame error statistics that give the frame-clustered BER variance.
    Jobs of CHAIN_JOB frames seeded 3000017 (j + 1) + snr, so the file does not depend on --procs."""
    with mp.Pool(procs) as pool:
        res = pool.map(_chain_worker, chain_jobs(), chunksize=1)     # job order: sums independent of --procs
    rows = chain_rows(res)
    meta = {"generator": f"tests/golden/gen_golden.py --only chain (jobs of {CHAIN_JOB} frames)",
            "source": "reference OFDM.c stage functions (gcc -O2) composed as the genie symbol chain "
                      "(oracle/ref_harness.c ref_time_symbol_chain, flags 4), real noise "
                      "sigma^2 = 0.4980 * 52/4096 / 10^(snr/10), LCG rand hook",
            "seeds": "job j of a point: noise 3000017 (j + 1) + snr, bits derived from it (RefLib.symbol_chain_stats)",
            "rows": rows}
    (HERE / "ref_symbol_chain_curve.json").write_text(json.dumps(meta, indent=1))


MC_SNRS = list(range(0, 17)) + [18, 20, 22, 24, 26, 28, 30]
MC_DEEP_SNRS = (11, 12, 13, 14, 15)     # the BER waterfall, where the curve is set by rare sync failures
MC_DEEP_SCALE = {13: 4, 14: 4, 15: 4}   # x --mc-deep-trials where the 1e-3.5 .. 1e-5 crossings are pinned
MC_DEEP_JOB = 25_000                    # trials per deep job (seeded by job index: independent of --procs)


def _mc_worker(args):
    snr, n, seed = args
    R = RefLib()
    t, acc = R.mc_trials(snr, n, seed)
    return snr, n, t, acc.tolist()


def mc_jobs(trials: int, procs: int, deep_trials: int, deep_snrs=MC_DEEP_SNRS):
    """(snr, trials, seed) jobs.  Shallow points: `procs` jobs of trials // procs each, seeded
    1000003 (p + 1) + snr (the round-2 fixture's seeds: 48000 = 8 x 6000 reproduces its rows).  Deep
    points: deep_trials (x MC_DEEP_SCALE) in jobs of MC_DEEP_JOB, seeded 2000003 (j + 1) + snr."""
    jobs = []
    for s in MC_SNRS:
        if deep_trials and s in deep_snrs:
            n_jobs = MC_DEEP_SCALE.get(s, 1) * deep_trials // MC_DEEP_JOB
            jobs += [(float(s), MC_DEEP_JOB, 2000003 * (j + 1) + s) for j in range(n_jobs)]
        else:
            per = max(1, trials // procs)
            jobs += [(float(s), per, 1000003 * (p + 1) + s) for p in range(procs)]
    return jobs


MC_KEYS = ("sum_evm_db", "sum_evm_agc_db", "sum_ber", "sum_ber2", "trials_ber_pos", "trials_ber_ge_quarter",
           "sum_evm_db2", "trials_evm_agc_finite")


def mc_rows(res) -> list:
    """fixture rows from (snr, trials, seconds, acc8) job results"""
    curve = {}
    keys = MC_KEYS
    for snr, n, t, acc in res:
        c = curve.setdefault(snr, {"trials": 0, "sec": 0.0, **{k: 0.0 for k in keys}})
        c["trials"] += n
        c["sec"] += t
        for k, v in zip(keys, acc):
            c[k] += v
    rows = []
    for snr in sorted(curve):
        c = curve[snr]
        n = c["trials"]
        var_ber = max(c["sum_ber2"] / n - (c["sum_ber"] / n) ** 2, 0.0)
        rows.append({"snr_db": snr, "trials": n, "ber": c["sum_ber"] / n,
                     "ber_trial_var": var_ber,                       # per-trial BER variance (frame-clustered)
                     "trials_ber_pos": int(c["trials_ber_pos"]),      # trials with any bit error
                     "trials_ber_ge_quarter": int(c["trials_ber_ge_quarter"]),   # failed frames (sync loss)
                     "mean_evm_db": c["sum_evm_db"] / n,
                     "evm_db_trial_var": max(c["sum_evm_db2"] / n - (c["sum_evm_db"] / n) ** 2, 0.0),
                     "mean_evm_agc_db": c["sum_evm_agc_db"] / n,
                     "trials_evm_agc_finite": int(c["trials_evm_agc_finite"]),
                     "sec_per_trial": c["sec"] / n})
    return rows


def gen_mc(trials: int, procs: int, deep_trials: int):
    jobs = mc_jobs(trials, procs, deep_trials)
    jobs.sort(key=lambda j: -j[1])                      # long jobs first
    with mp.Pool(procs) as pool:
        res = list(pool.imap_unordered(_mc_worker, jobs, chunksize=1))
    rows = mc_rows(res)
    meta = {"generator": f"tests/golden/gen_golden.py --only mc --mc-trials {trials} --procs {procs} "
                         f"--mc-deep-trials {deep_trials}",
            "source": "reference OFDM.c (gcc -O2) TOA+Receiver loop (ref_harness.c ref_mc_trials)",
            "rand": "64-bit LCG hook (oracle/ref_harness.c)",
            "seeds": "shallow points: 1000003 (p + 1) + snr per process p; deep points "
                     f"{list(MC_DEEP_SNRS)} (x {MC_DEEP_SCALE} trials): {MC_DEEP_JOB}-trial jobs seeded "
                     "2000003 (j + 1) + snr",
            "rows": rows}
    (HERE / "ref_mc_curve.json").write_text(json.dumps(meta, indent=1))


# ---------------------------------------------------------------- frames of 1 and 3..15 data symbols (--only long)
# Messages, typed in as data.  15 symbols: the reference's own second text (the commented alternative of OFDM.c:21, 171
# characters).  The other sizes: tests/test_gpu_long_frames.py's text cut as its text(n) cuts it (n - 1 characters and a
# full stop, so that no message ends in the blank the decoder strips) at 12, 30, 55, 96, 97 and 150 characters.
REF_LONG_MESSAGE = (b"The Supreme Lord Shree Krishna said: I taught this eternal science of Yog to the Sun God, Vivasvan, "
                    b"who passed it on to Manu; and Manu, in turn, instructed it to Ikshvaku.")
LONG_TEXT = (b"Long frames on the MI355X: the capture no longer fits one wave's share of the LDS, so the sync kernel keeps a "
             b"ring of it and detects a round at a time; fifteen data symbols is the cap!!")
LONG_CHARS = {1: 12, 3: 30, 5: 55, 8: 96, 9: 97, 13: 150, 15: 171}
LONG_D = tuple(LONG_CHARS)
FIXTURE_TAG = 0xF1000000                   # Philox counter word 3 of fixture noise (oracle/ofdm_oracle.c STREAM_FIXTURE)
STAGE_SNRS = (100.0, 30.0, 20.0, 14.0, 12.0, 10.0, 8.0, 6.0)
BULK_D = (1, 8, 15)
BULK_N = 1000
BULK_SNRS = (6.0, 8.0, 10.0, 12.0, 16.0, 25.0)
BULK_KEY = (0xB01C, 1)                     # Philox key of the bulk captures; a stages case has the key (seed, 0)
LONG_MC_D = (8, 15)
LONG_MC_SNRS = (6.0, 8.0, 10.0, 12.0, 14.0, 20.0)
LONG_MC_TRIALS = 20_000
LONG_MC_JOB = 2_500                        # trials per job, seeded by job index: the file does not depend on --procs
CAPTURE_RULE = ("capture = complex64(wave[rs:rs+L] + float32(sigma * z)), wave = the D-symbol period x 10 (complex64), "
                "L = int(0.307 * len(wave)), sigma a double, z = oracle.gauss_fill([case, D, 0xF1000000], key, L): the "
                "doubles of orc_gauss4 over the Philox blocks (b, case, D, 0xF1000000), b = 0, 1, .. -- real-only noise "
                "on the captured window.  key = (seed, 0) for a stages case; (0xB01C, 1) for a bulk capture, whose `case` is "
                "its index + 1000 x the noise draws that sat on the sync threshold before it.")


def long_message(nd: int) -> bytes:
    if nd == 15:
        assert len(REF_LONG_MESSAGE) == 171
        return REF_LONG_MESSAGE
    return LONG_TEXT[:LONG_CHARS[nd] - 1] + b"."


def long_capture(O, wave: np.ndarray, nd: int, case: int, rs: int, sigma: float, key) -> np.ndarray:
    """CAPTURE_RULE; `wave` is the complex64 waveform of ten periods."""
    L = int(len(wave) * 0.307)
    z = O.gauss_fill([case, nd, FIXTURE_TAG], key, L)
    return (wave[rs:rs + L] + (sigma * z).astype(np.float32)).astype(np.complex64)


def ref_long_decode(R: RefLib, wave: np.ndarray, cap: np.ndarray, rs: int) -> dict:
    """The reference's Receiver() on a capture laid at rs of the otherwise clean waveform (it reads nothing else)."""
    ota = wave.copy()
    ota[rs:rs + len(cap)] = cap
    return R.receiver_stages(ota, rs)


def threshold_decisions(corr: np.ndarray) -> set:
    """conftest.off_threshold_pidx_mismatches' rule: Packet_Selection's decisions with the 0.75 threshold moved by up to
    +-0.1 % in 21 steps (tests/test_lazy_rule.packet_selection, pinned to the compiled reference)."""
    sys.path.insert(0, str(ROOT / "tests"))
    from test_lazy_rule import packet_selection  # noqa: PLC0415
    return {packet_selection(corr, 0.75 * (1 + d)) for d in np.linspace(-1e-3, 1e-3, 21)}


def near_threshold(nopilot: np.ndarray) -> int:
    """components of the equalised carriers within 1e-4 of the slicer threshold (a decision there may differ)"""
    return int(np.sum(np.abs(nopilot.real) < 1e-4) + np.sum(np.abs(nopilot.imag) < 1e-4))


def stage_starts(n: int, L: int) -> list:
    """eight capture starts: both ends, the middle, one capture straddling a period boundary in its first quarter"""
    per = n // 10
    return [0, n - L - 1, (n - L) // 2, 3 * per - L // 4, 1234, per + 17, 5 * per - 1, (n - L) // 3]


def stages_case(R: RefLib, O, wave, P, nd: int, case: int, snr: float, rs: int, seed: int):
    """one ref_long_stages case, or None when a generator condition fails (the caller tries the next seed)"""
    sigma = float(np.sqrt(P / 10 ** (snr / 10)))
    cap = long_capture(O, wave, nd, case, rs, sigma, (seed, 0))
    d = ref_long_decode(R, wave, cap, rs)
    ota = wave.copy()
    ota[rs:rs + len(cap)] = cap
    rr = R.receiver(ota, rs)
    if not np.array_equal(np.nan_to_num(rr, neginf=-999), np.nan_to_num(d["res"], neginf=-999)):
        raise AssertionError(("Receiver() and receiver_stages differ", nd, case, rr, d["res"]))    # condition 1
    if d["ints"][3] != 0:                                                                           # condition 2
        return None
    if threshold_decisions(d["corr"]) != {d["packet_idx"]}:                                         # condition 3
        return None
    return dict(packet_idx=np.int32(d["packet_idx"]), H=d["H"], nopilot=d["nopilot"], bits=d["bits"].astype(np.int8),
                res=d["res"], ints=d["ints"], sigma=np.float64(sigma), rs=np.int32(rs), snr=np.float64(snr),
                seed=np.int64(seed))


def gen_long_tx(R: RefLib) -> dict:
    out, waves = {}, {}
    for nd in LONG_D:
        msg = long_message(nd)
        n = R.set_message(msg)
        g = R.globals()
        w = R.waveform()
        assert int(g["dims"][0]) == nd and n == len(w) == 10 * (2 * (320 + 80 * nd) + 20), (nd, n, g["dims"])
        per = w.reshape(10, -1)
        assert all(np.array_equal(per[k].view(np.uint32), per[0].view(np.uint32)) for k in range(10))
        out.update({f"d{nd}_msg": np.frombuffer(msg, np.uint8), f"d{nd}_period": per[0].copy(),
                    f"d{nd}_bits": g["bits"].astype(np.int8), f"d{nd}_payload_mod": g["payload_mod"],
                    f"d{nd}_dims": g["dims"]})
        waves[nd] = w
    np.savez_compressed(HERE / "ref_long_tx.npz", frames=np.array(LONG_D, np.int32), **out)
    return waves


def gen_long_stages(R: RefLib, O, waves: dict):
    out = {}
    for nd in LONG_D:
        R.set_message(long_message(nd))
        w = waves[nd]
        truth = R.globals()["bits"]
        P = float(np.mean(np.abs(w.astype(np.complex128)) ** 2))
        L = int(len(w) * 0.307)
        cases = []
        for case, (snr, rs) in enumerate(zip(STAGE_SNRS, stage_starts(len(w), L))):
            # condition 4 for every frame size: when no earlier case lost sync, the last (6 dB) one is one that does
            want_fail = case == len(STAGE_SNRS) - 1 and all(int(c["packet_idx"]) != 0 for c in cases)
            for seed in range(1000 * nd + 100 * case + 1, 1000 * nd + 100 * case + 100):
                c = stages_case(R, O, w, P, nd, case, snr, rs, seed)
                if c is not None and (not want_fail or int(c["packet_idx"]) == 0):
                    break
            else:
                raise AssertionError(("no seed gives a usable case", nd, case))
            cases.append(c)
        fails = sum(int(c["packet_idx"]) == 0 for c in cases)
        clean = sum(int(c["packet_idx"]) != 0 and np.array_equal(c["bits"], truth) for c in cases)
        assert fails > 0 and clean > 0, (nd, fails, clean)                                          # condition 4
        print(f"stages D={nd}: {fails} sync failures, {clean} error-free decodes, seeds {[int(c['seed']) for c in cases]}")
        for k in cases[0]:
            out[f"d{nd}_{k}"] = np.array([c[k] for c in cases])
    np.savez_compressed(HERE / "ref_long_stages.npz", frames=np.array(LONG_D, np.int32), rule=np.array(CAPTURE_RULE),
                        **out)


BULK_DRAWS = 3         # noise draws tried per bulk capture (see bulk_capture_row)


def bulk_capture_row(R: RefLib, O, wave, truth, nd: int, k: int, rs: int, sigma: float):
    """One bulk capture: (case, packet_idx, bit errors, near, on_threshold, draws on the threshold).  By the +-0.1 % rule
    about 4 % of uniformly drawn captures sit on Packet_Selection's threshold at every SNR (the metric climbs the
    plateau's edge by ~1/64 per sample, so 0.1 % of 0.75 moves the first crossing by a sample in that share of them);
    such a capture gets another noise draw, as a stages case gets another seed: case = k + BULK_N x draw, recorded."""
    moved = 0
    for draw in range(BULK_DRAWS):
        case = k + BULK_N * draw
        cap = long_capture(O, wave, nd, case, rs, sigma, BULK_KEY)
        d = ref_long_decode(R, wave, cap, rs)
        assert d["ints"][3] == 0, ("late frame read past the buffer", nd, case)
        on = len(threshold_decisions(d["corr"])) > 1
        if not on:
            break
        moved += 1
    return case, d["packet_idx"], int(np.sum(d["bits"] != truth)), near_threshold(d["nopilot"]), on, moved


def gen_long_bulk(R: RefLib, O, waves: dict):
    out = {}
    for nd in BULK_D:
        R.set_message(long_message(nd))
        w = waves[nd]
        truth = R.globals()["bits"]
        P = float(np.mean(np.abs(w.astype(np.complex128)) ** 2))
        L = int(len(w) * 0.307)
        rng = np.random.default_rng(802110 + nd)
        snr = rng.choice(BULK_SNRS, BULK_N)
        rs = rng.integers(0, len(w) - L, BULK_N).astype(np.int32)
        sigma = np.sqrt(P / 10 ** (snr / 10))
        rows = [bulk_capture_row(R, O, w, truth, nd, k, int(rs[k]), float(sigma[k])) for k in range(BULK_N)]
        case, pidx, err, near, on, moved = (np.array(v) for v in zip(*rows))
        print(f"bulk D={nd}: {int(np.sum(pidx == 0))} sync failures, {int(np.sum(on))} on the threshold "
              f"({int(np.sum(moved))} draws on it replaced), {int(np.sum(err == 0))} error-free, "
              f"{int(np.sum(near > 0))} with a carrier near the slicer threshold")
        assert np.sum(on) <= 0.005 * BULK_N, (nd, int(np.sum(on)))
        out.update({f"d{nd}_snr": snr, f"d{nd}_rs": rs, f"d{nd}_sigma": sigma, f"d{nd}_case": case.astype(np.int32),
                    f"d{nd}_packet_idx": pidx.astype(np.int32), f"d{nd}_bit_err": err.astype(np.int32),
                    f"d{nd}_near": near.astype(np.int16), f"d{nd}_on_threshold": on.astype(np.bool_)})
    np.savez_compressed(HERE / "ref_long_bulk.npz", frames=np.array(BULK_D, np.int32), rule=np.array(CAPTURE_RULE),
                        **out)


def _long_mc_worker(args):
    nd, snr, n, seed = args
    R = RefLib()
    R.set_message(long_message(nd))
    t, acc = R.mc_trials(snr, n, seed)
    return nd, snr, n, t, acc.tolist()


def long_mc_jobs(frames=LONG_MC_D, snrs=LONG_MC_SNRS, trials: int = LONG_MC_TRIALS) -> list:
    return [(nd, snr, LONG_MC_JOB, 3000029 * (j + 1) + 1000 * nd + int(snr))
            for nd in frames for snr in snrs for j in range(trials // LONG_MC_JOB)]


def gen_long_mc(procs: int):
    """ref_mc_curve_long.json: ref_mc_trials (Transmission_Over_Air + Receiver, OFDM.c:1206-1217) after set_message"""
    with mp.Pool(procs) as pool:
        res = pool.map(_long_mc_worker, long_mc_jobs(), chunksize=1)      # job order: sums independent of --procs
    rows = []
    for nd in LONG_MC_D:
        rows += [{"frames": nd, **r} for r in mc_rows([r[1:] for r in res if r[0] == nd])]
    meta = {"generator": f"tests/golden/gen_golden.py --only long (jobs of {LONG_MC_JOB} trials)",
            "source": "reference OFDM.c (gcc -O2) TOA+Receiver loop (ref_harness.c ref_mc_trials) on the frame "
                      "ref_set_message builds from the reference's stage functions",
            "rand": "64-bit LCG hook (oracle/ref_harness.c)",
            "messages": {str(nd): long_message(nd).decode() for nd in LONG_MC_D},
            "seeds": "job j of a point: 3000029 (j + 1) + 1000 frames + snr",
            "rows": rows}
    (HERE / "ref_mc_curve_long.json").write_text(json.dumps(meta, indent=1))


def gen_long(R: RefLib, procs: int, parts=("tx", "stages", "bulk", "mc")):
    from oracle import Oracle  # noqa: PLC0415  (only its Philox Gaussians: the noise rule needs no reference)
    O = Oracle()
    try:
        waves = gen_long_tx(R) if "tx" in parts else None
        if waves is None:
            waves = {}
            for nd in LONG_D:
                R.set_message(long_message(nd))
                waves[nd] = R.waveform()
        if "stages" in parts:
            gen_long_stages(R, O, waves)
        if "bulk" in parts:
            gen_long_bulk(R, O, waves)
    finally:
        R.set_message(R.DEFAULT_MESSAGE)
    if "mc" in parts:
        gen_long_mc(procs)


def main():
    ap = argparse.ArgumentParser()
    # the defaults reproduce the committed ref_mc_curve.json (48000 trials/point, 1e6 at 11, 12 dB, 4e6 at 13, 14, 15)
    ap.add_argument("--mc-trials", type=int, default=48000)
    ap.add_argument("--mc-deep-trials", type=int, default=1_000_000)
    ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--skip-mc", action="store_true")
    ap.add_argument("--only", choices=["genie", "mc", "chain", "long"], help="regenerate one fixture only")
    ap.add_argument("--long-parts", default="tx,stages,bulk,mc", help="--only long: which of its four files to write")
    a = ap.parse_args()
    build_ref()
    R = RefLib()
    if a.only == "genie":
        gen_genie(R)
        return
    if a.only == "mc":
        gen_mc(a.mc_trials, a.procs, a.mc_deep_trials)
        return
    if a.only == "chain":
        gen_chain(a.procs)
        return
    if a.only == "long":
        gen_long(R, a.procs, tuple(a.long_parts.split(",")))
        return
    gen_fft(R); gen_tx(R); gen_rx(R); gen_kat(); gen_genie(R); gen_chain(a.procs)
    if not a.skip_mc:
        gen_mc(a.mc_trials, a.procs, a.mc_deep_trials)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
