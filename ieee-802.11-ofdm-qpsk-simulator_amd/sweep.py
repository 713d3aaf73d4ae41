"""The reference's main() (src/OFDM.c:1187-1236) on the MI355X engine.

reference_main() sweeps SNR 6..40 dB step 1 (OFDM.c:18, 1195-1198) and writes the same four
files into out_dir (data/ by default): Output_SNR.txt, Output_EVM_AGC.txt (EVM before the slicer),
Output_EVM_AGC_DB.txt (EVM after the slicer) and Output_BER.txt, so scripts/OFDM_Plotting.py
runs unchanged.  The reference runs ONE trial per SNR point (frame mode, fixed message); here
`trials` is a parameter and the per-point values are pooled over them (BER = errors / bits,
EVM = 10 log10(sum|e|^2 / sum|d|^2)); with trials=1 they equal the reference's per-trial values.
`mode="symbol"` runs the per-symbol chain (genie timing, LTF LS estimate) instead.

Per-point values in the files.  Output_EVM_AGC.txt / Output_EVM_AGC_DB.txt hold, for trials > 1,
the MEAN over trials of the per-trial EVM_dB the reference writes for its one trial
(OFDM.c:1126,1150); the post-slicer mean is -inf as soon as one trial had no slicer error, as the
reference's own value for that trial is (ref_mc_curve.json's mean_evm_agc_db is the same
statistic).  evm="finite" keeps that pre-slicer file and writes, after the slicer, the mean over the trials
whose value is finite (trials with >= 1 slicer error; their count goes to the sidecar), so a many-trial
run stays plottable above ~3 dB.  evm="pooled" writes 10 log10(sum|e|^2 / sum|d|^2) over all trials
instead.  BER is errors / bits (= the mean per-trial BER: every trial carries the same bit count).

Multi-GPU: launched under torchrun, each rank takes a contiguous share of the trials
(dist.shard_range); reference_main() forms the process group (dist.init_from_env: RCCL, or gloo
with OFDM_DIST_BACKEND=gloo) and the counters are summed with one all-reduce before rank 0 writes.

link_sweep() / link_main() (`ofdm_pkg.py link`) sweep packets that each carry their own bits: transmitted once,
then impaired, received and scored per SNR point on the device (include/ofdm_mi355x_channel.h).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

from . import abi, dist
from .engine import Engine, SweepResult
from .fileio import write_reference_outputs

REF_SNR = np.arange(6.0, 41.0, 1.0)        # OFDM.c:18, 1197


def set_message(engine: Engine, message: str | bytes) -> int:
    """OFDM.c:20-21 `message`: up to 96 characters through the base entry, longer ones (up to 180 characters, 15 data
    symbols, frame mode) through the extension header's ofdm_set_long_message."""
    if len(message) > abi.MSG_MAX_CHARS:
        return engine.set_long_message(message)
    return engine.set_message(message)


def run_sweep(engine: Engine, snr_db, trials: int, mode: str = "frame", seed: int = 0x80211A,
              payload: str | None = None, est: str = "ls", noise: str = "real", channel: str = "awgn",
              conv: str = "c", rank: int = 0, world: int = 1, message: str | None = None) -> SweepResult:
    snr = np.asarray(snr_db, np.float64)
    if message is not None:
        set_message(engine, message)            # OFDM.c:20 `message`, framed by Data_Generator
    start, end = dist.shard_range(trials, rank, world)
    if mode == "frame":
        cfg = abi.make_cfg(seed=seed, conv=conv, payload=payload or "message", noise=noise)
        c = engine.frame_sweep(cfg, snr, end - start, first_trial=start, mode="c" if conv == "c" else "matlab")
    elif mode == "symbol":
        cfg = abi.make_cfg(seed=seed, conv=conv, payload=payload or "random", est=est, noise=noise, channel=channel)
        c = engine.symbol_sweep(cfg, snr, end - start, first_frame=start)
    else:
        raise ValueError(mode)
    if world > 1:
        c = dist.allreduce_counters_np(c, engine.device)
    return SweepResult(snr, c)


def reference_main(out_dir: str | Path = "data", trials: int = 1, mode: str = "frame", snr_db=REF_SNR,
                   seed: int = 0x80211A, device: int = 0, json_sidecar: bool = True, evm: str = "trial",
                   **kw) -> SweepResult:
    if evm not in ("trial", "finite", "pooled"):
        raise ValueError(evm)
    rank, world, local = dist.env_rank_world()
    if world > 1:
        dist.init_from_env()
    t0 = time.perf_counter()
    with Engine(local if world > 1 else device) as eng:
        res = run_sweep(eng, snr_db, trials, mode=mode, seed=seed, rank=rank, world=world, **kw)
    wall = time.perf_counter() - t0
    if rank == 0:
        pre, post = {"trial": (res.mean_frame_evm_db, res.mean_frame_evm_post_db),
                     "finite": (res.mean_frame_evm_db, res.mean_finite_frame_evm_post_db),
                     "pooled": (res.evm_pre_db, res.evm_post_db)}[evm]
        write_reference_outputs(out_dir, res.snr_db, pre, post, res.ber)
        if json_sidecar:
            side = {"mode": mode, "trials_per_snr": trials, "world": world, "seed": seed, "wall_s": wall,
                    "evm_files": evm, "snr_db": res.snr_db.tolist(), "ber": res.ber.tolist(),
                    "mean_trial_evm_db": res.mean_frame_evm_db.tolist(),
                    "mean_trial_evm_post_db": [float(v) for v in res.mean_frame_evm_post_db],
                    "mean_finite_trial_evm_post_db": [float(v) for v in res.mean_finite_frame_evm_post_db],
                    "post_finite_trials": res.counters[:, abi.C_EVMDB_POST_FINITE].tolist(),
                    "evm_pre_db": res.evm_pre_db.tolist(),
                    "evm_post_db": [float(v) for v in res.evm_post_db], "sync_fail_rate": res.sync_fail_rate.tolist(),
                    "counters": res.counters.tolist()}
            (Path(out_dir) / "ofdm_sweep.json").write_text(json.dumps(side, indent=1))
    return res


def impairment_sweep(engine: Engine, snr_db, cfo_hz, n_trials: int, taps=None, noise: str = "real",
                     seed: int = 0x80211A, payload: str = "message", mode: str = "c",
                     budget_bytes: int = 256 << 20) -> np.ndarray:
    """BER / EVM / sync counters against carrier frequency offset and SNR in the reference's own trial, sync and CFO
    estimation included: counters[n_cfo][n_snr][NCOUNTERS].  Every point runs n_trials captures through
    channel.make_captures (capture starts and noise from one torch generator seeded with `seed`) and
    Engine.receive_captures, in chunks whose captures stay below budget_bytes.  Single context: the counters are sums,
    so trials can be sharded over GPUs and added (dist.py)."""
    import torch  # noqa: PLC0415
    from .channel import make_captures  # noqa: PLC0415
    snr = np.atleast_1d(np.asarray(snr_db, np.float64))
    cfo = np.atleast_1d(np.asarray(cfo_hz, np.float64))
    dev = torch.device("cuda", engine.device)
    opts = abi.make_rx_opts(mode)
    L = opts.cap_len or abi.capture_len(engine.payload_frames(payload))
    wave = torch.from_numpy(engine.transmitter("c" if mode == "c" else "matlab", payload)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    chunk = max(1, int(budget_bytes) // (8 * L))
    out = torch.zeros((len(cfo), len(snr), abi.NCOUNTERS), dtype=torch.int64, device=dev)
    for ci, f in enumerate(cfo):
        for si, s in enumerate(snr):
            done = 0
            while done < n_trials:
                m = min(chunk, n_trials - done)
                starts = torch.randint(0, wave.shape[0] - L, (m,), generator=gen, device=dev)   # OFDM.c:949
                caps = make_captures(wave, starts, float(s), float(f), taps=taps, noise=noise, generator=gen, cap_len=L)
                engine.receive_captures(caps, mode=mode, payload=payload, want_bits=False, counters=out[ci, si])
                done += m
    return out.cpu().numpy()


def captures_main(argv=None):
    """`ofdm_pkg.py captures`: the reference's four Output_*.txt files per CFO value, from impairment_sweep."""
    from .channel import NOISE_KINDS, parse_taps  # noqa: PLC0415
    ap = argparse.ArgumentParser(description="BER / EVM against SNR under CFO, multipath and complex noise "
                                             "(batched receiver for caller-supplied captures)")
    ap.add_argument("--out", default="data")
    ap.add_argument("--trials", type=int, default=100, help="captures per (CFO, SNR) point")
    ap.add_argument("--snr", type=float, nargs="*", help="SNR grid in dB (default 6..40 step 1)")
    ap.add_argument("--cfo-hz", type=float, action="append", help="carrier frequency offset in Hz (repeatable; default 0)")
    ap.add_argument("--taps", help="multipath FIR at the oversampled rate, e.g. 1,0,0.4+0.3j")
    ap.add_argument("--noise", choices=list(NOISE_KINDS), default="real")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x80211A)
    ap.add_argument("--message", help="MESSAGE payload text (default: OFDM.c:20), up to 180 characters")
    a = ap.parse_args(argv)
    snr = np.array(a.snr) if a.snr else REF_SNR
    cfo = a.cfo_hz or [0.0]
    taps = parse_taps(a.taps) if a.taps else None
    out = Path(a.out)
    if not out.is_dir():
        raise FileNotFoundError(f"output directory {out} does not exist")
    t0 = time.perf_counter()
    with Engine(0) as eng:
        if a.message is not None:
            set_message(eng, a.message)
        c = impairment_sweep(eng, snr, cfo, a.trials, taps=taps, noise=a.noise, seed=a.seed)
    wall = time.perf_counter() - t0
    side = {"trials_per_point": a.trials, "seed": a.seed, "noise": a.noise, "wall_s": wall,
            "taps": None if taps is None else [[float(t.real), float(t.imag)] for t in taps],
            "snr_db": snr.tolist(), "cfo_hz": [float(f) for f in cfo], "counters": c.tolist(), "dirs": []}
    for ci, f in enumerate(cfo):
        res = SweepResult(snr, c[ci])
        d = out if len(cfo) == 1 else out / f"cfo_{f:g}"
        d.mkdir(exist_ok=True)
        write_reference_outputs(d, res.snr_db, res.mean_frame_evm_db, res.mean_frame_evm_post_db, res.ber)
        side["dirs"].append(str(d))
        for s, b, sf in zip(res.snr_db, res.ber, res.sync_fail_rate):
            print(f"CFO = {f:9.1f} Hz   SNR = {s:5.1f} dB   BER = {b:.3e}   sync fail = {sf:.3f}", file=sys.stderr)
    (out / "ofdm_captures.json").write_text(json.dumps(side, indent=1))
    return c


def link_sweep(engine: Engine, words, n_data: int, gap: int, snr_db, cfo_hz: float = 0.0, taps=None,
               noise: str = "real", seed: int = 0x80211A, trial: int = 0, window=None, fading=None,
               detector: str = "reference", threshold: float = 0.75, timing: str = "none",
               tracking: str = "none", branches: int = 1, code: str | None = None, rate="1/2", lengths=None,
               keep_packets: bool = False) -> dict:
    """Packet-error and bit-error counts against SNR for packets that each carry their own bits, the recording never
    leaving the device: the packets (words: uint32 [n, 3 n_data], each behind `gap` idle samples, and a closing gap)
    are transmitted once; per SNR point q the clean recording is impaired into a second buffer with the noise stream
    (seed, trial, q) (Engine.impair_stream), received (Engine.receive_stream_device) and scored
    (Engine.score_packets, offsets `window`) into row q of a device table that is read once at the end.  The SNR
    refers to the mean power of the packets' samples.  The context's MESSAGE payload is set to n_data symbols of
    blanks (the receiver takes its packet length from it).  window defaults to (8, 40).

    fading = dict(pdp=powers, index0=0): every packet goes through Rayleigh taps of its own (Engine.draw_taps with the
    sweep's seed, drawn once; Engine.transmit_faded), L = len(pdp) taps making it L - 1 samples longer.  The SNR then
    refers to the realised mean received power per nominal packet sample, sum |clean|^2 / (n P); the default window
    grows to (8, 40 + L - 1), since the detection front moves with the channel's delay, and `gap` must cover it.  The
    static taps, cfo_hz and the noise apply afterwards as they do without fading.

    detector, threshold: Engine.receive_stream_device's (include/ofdm_mi355x_detect.h).  The default window is the same
    for both detectors: the conjugate detector's fronts are the reference's on an unfaded link, and under a selective
    channel at low SNR a few of its detections can fall outside it and count as missed.
    timing: "none", or "ltf": every record's position is refined against the long training field before the decode
    (include/ofdm_mi355x_timing.h), which puts an unfaded packet's record at its first sample + 16.  "ltf-matlab" is accepted as well and is the same
    rule with the MATLAB convention's template; the sweep transmits C-convention packets, for which "ltf" is the
    right one.
    tracking: "none", or "pilots": every data symbol is turned back by its four pilots' common phase before the slicer
    (include/ofdm_mi355x_track.h).  For long packets; on 2-symbol packets it costs a little BER.
    branches: B = 1..4 receive antennas (include/ofdm_mi355x_diversity.h).  Branch b carries the same
    packets, through taps of its own when fading (Engine.draw_taps at index0 + b n), under the noise stream
    (seed, trial B + b, q); the B recordings are received together (Engine.receive_diversity_device).  power is then the
    mean of the branches' realised powers, and every branch gets the noise power it sets.  B > 1 needs
    detector="conjugate"; with B = 1 every call and every total is what it was without the argument.
    code: None, or "conv" (include/ofdm_mi355x_code.h): `words` are then information words
    [n, abi.code_info_words(n_data)], encoded once (Engine.encode_packets) into the payload words that are transmitted;
    per SNR point the receive call also returns d_eq, Engine.stream_csi forms the records' gains and Engine.decode_coded
    the information words, which are gathered by the scores' rx_index and compared with the sent ones on the device.
    The result then also holds info_totals (int64 [n_snr, 3]: information bits compared, information bit errors,
    matched packets with at least one of them); totals are those of the coded payload bits before the decoder.  The SNR
    axis stays per sample: at equal SNR a coded packet carries (48 D - 6) / 96 D of the bits.  With None every call and
    every total is what it was without the argument.
    rate: "1/2", or with code="conv" one of 802.11a's punctured rates "2/3" and "3/4" (include/ofdm_mi355x_punct.h,
    DESIGN.md K21): `words` are then [n, abi.punct_info_words(n_data, rate)], S D - 6 information bits per packet with
    S = 64 or 72, and the encoder and decoder are the punctured ones; info_totals keep their meaning.  With "1/2" every
    call is what it was without the argument.
    code="ppdu" (include/ofdm_mi355x_ppdu.h): self-describing packets of n_data symbols, the header's among
    them.  `words` are PSDU words [n, 31]; rate is one rate, a sequence of n rates, or "mixed" (packet i at rate code
    i mod 3); lengths gives the LENGTH values (the FCS's four bytes among them) and defaults to every packet's
    abi.ppdu_cap; packet i's scrambler seed is 1 + (i mod 127).  Engine.encode_ppdu makes the payload words once, and per
    SNR point Engine.decode_ppdu reads rate and LENGTH off every record's header, decodes, descrambles and checks the
    FCS.  The result then also holds ppdu_totals (int64 [n_snr, 3, 5]), counted on the device per rate of the sent
    packet among the matched ones: matched; header valid with the sent rate and LENGTH; FCS passed (status 0, what a
    receiver sees without knowing what was sent); FCS passed but the PSDU differs from the sent one; PSDU bit errors among
    the header-right packets.  keep_packets=True adds ppdu_packets, per SNR point (meta int32 [n, 4], psdu uint32
    [n, 31], matched bool [n]) of the record matched to every sent packet.  totals are those of the payload words, as
    with code=None on the same words.

    Returns snr_db, totals (int64 [n_snr, NSCORE]), power, packets, samples."""
    import torch  # noqa: PLC0415
    snr = np.atleast_1d(np.asarray(snr_db, np.float64))
    n, plen = int(len(words)), abi.packet_len(n_data)
    abi.timing_code(timing)                                          # ValueError before anything is set or launched
    abi.tracking_code(tracking)
    if isinstance(branches, bool) or not isinstance(branches, int) or not 1 <= branches <= abi.DIVERSITY_MAX_BRANCHES:
        raise ValueError(f"branches must be an integer in [1, {abi.DIVERSITY_MAX_BRANCHES}], got {branches!r}")
    if branches > 1 and detector != "conjugate":
        raise ValueError(f"branches={branches} needs detector='conjugate', got {detector!r}")
    pdp = None
    if fading is not None:
        if set(fading) - {"pdp", "index0"} or "pdp" not in fading:
            raise ValueError(f"fading is dict(pdp=..., index0=0), got keys {sorted(fading)}")
        pdp = np.asarray(fading["pdp"], np.float64).ravel()
        if not 1 <= len(pdp) <= abi.FADE_MAX_TAPS:
            raise ValueError(f"fading['pdp'] must hold 1 to {abi.FADE_MAX_TAPS} powers, got {len(pdp)}")
    if window is None:
        window = (8, 40 + (0 if pdp is None else len(pdp) - 1))
    if gap < 0:
        raise ValueError(f"gap must not be negative, got {gap}")
    if gap < window[1]:
        raise ValueError(f"gap {gap} is shorter than the scoring window {tuple(window)}: a record could serve two packets")
    if code not in (None, "conv", "ppdu"):
        raise ValueError(f"code must be None, 'conv' or 'ppdu', got {code!r}")
    if code == "ppdu":
        ppdu = _ppdu_plan(words, n_data, rate, lengths)              # ValueError before anything is set or launched
    else:
        if lengths is not None or keep_packets:
            raise ValueError("lengths and keep_packets need code='ppdu'")
        if abi.rate_code(rate) and not code:
            raise ValueError(f"rate {rate!r} needs code='conv'")
    set_message(engine, " " * (12 * n_data))
    dev = torch.device("cuda", engine.device)
    if code == "ppdu":
        w = engine.encode_ppdu(ppdu["psdu"], ppdu["lengths"], ppdu["rates"], ppdu["seeds"], n_data)["d_words"]
        sent = torch.from_numpy(ppdu["sent"].view(np.int32)).to(dev)
        sent_rate = torch.from_numpy(ppdu["rates"].astype(np.int64)).to(dev)
        sent_len = torch.from_numpy(ppdu["lengths"].astype(np.int32)).to(dev)
        popcount = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
        ppdu_totals = torch.zeros((len(snr), 3, 5), dtype=torch.int64, device=dev)
        kept = []
    else:
        w = words if torch.is_tensor(words) else torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)
    if code == "conv":
        # the sent information words without the last word's unused bits (the decoder writes them as 0), then the payload
        wi, kinfo = abi.punct_info_words(n_data, rate), abi.punct_info_bits(n_data, rate)
        if w.dim() != 2 or w.shape[1] != wi:
            raise ValueError(f"code='conv' takes information words [n, {wi}] for {n_data} data symbols"
                             f"{'' if rate == '1/2' else ' at rate ' + rate}, got {tuple(w.shape)}")
        info = w.clone()
        mask = (0xffffffff << (32 * wi - kinfo)) & 0xffffffff
        info[:, -1] &= mask - (1 << 32) if mask >> 31 else mask
        w = engine.encode_packets(info, n_data, rate=rate)
        popcount = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
        info_totals = torch.zeros((len(snr), 3), dtype=torch.int64, device=dev)
    nb = branches
    if pdp is None:
        stride = plen + gap
        n_out = n * stride + gap
        clean = [engine.transmit_packets(w, n_data, pos0=gap, stride=stride, n_out=n_out)] * nb
    else:
        stride = abi.faded_len(n_data, len(pdp)) + gap
        n_out = n * stride + gap
        clean = []
        for b in range(nb):
            h = engine.draw_taps(n, pdp, seed=seed, index0=fading.get("index0", 0) + b * n)
            clean.append(engine.transmit_faded(w, n_data, h, pos0=gap, stride=stride, n_out=n_out))
    # mean |w|^2 over the packets' samples: the gaps are zero
    # (unfaded branches share one clean recording; faded ones have a realised power each, and the sweep takes their mean)
    powers = [float((c.real.double() ** 2 + c.imag.double() ** 2).sum()) / max(n * plen, 1) for c in (clean if pdp is not None else clean[:1])]
    power = powers[0] if nb == 1 else float(np.mean(powers))
    rec = [torch.empty_like(clean[0]) for _ in range(nb)]
    totals = torch.zeros((len(snr), abi.NSCORE), dtype=torch.int64, device=dev)
    for q, s in enumerate(snr):
        for b in range(nb):
            engine.impair_stream(clean[b], power, float(s), cfo_hz, taps=taps, noise=noise, seed=seed, trial=trial * nb + b,
                                 snr_index=q, out=rec[b])
        if not code:
            if nb == 1:
                rx = engine.receive_stream_device(rec[0], detector=detector, threshold=threshold, timing=timing, tracking=tracking)
            else:
                rx = engine.receive_diversity_device(rec, detector=detector, threshold=threshold, timing=timing, tracking=tracking)
            engine.score_packets(w, n_data, rx, pos0=gap, stride=stride, window=window, totals=totals[q])
            continue
        if nb == 1:
            rx = engine.receive_stream_device(rec[0], detector=detector, threshold=threshold, timing=timing, tracking=tracking,
                                              want_eq=True)
        else:
            rx = engine.receive_diversity_device(rec, detector=detector, threshold=threshold, timing=timing, tracking=tracking,
                                                 want_eq=True)
        if code == "ppdu":
            dec = engine.decode_ppdu(rx, csi=engine.stream_csi(rec if nb > 1 else rec[0], rx))
            idx = engine.score_packets(w, n_data, rx, pos0=gap, stride=stride, window=window, totals=totals[q])["scores"][:, 0].long()
            matched = idx >= 0
            meta, got = dec["d_meta"][idx.clamp(min=0)], dec["d_psdu"][idx.clamp(min=0)]
            header_ok = matched & ((meta[:, 0] & abi.PPDU_BAD_HEADER) == 0) & (meta[:, 1] == sent_rate) & (meta[:, 2] == sent_len)
            fcs_ok = matched & (meta[:, 0] == 0)
            err = popcount[(got ^ sent).contiguous().view(torch.uint8).long()].sum(dim=1)
            cols = torch.stack([matched, header_ok, fcs_ok, fcs_ok & (err > 0)], dim=1).long()
            cols = torch.cat([cols, torch.where(header_ok, err, torch.zeros_like(err))[:, None]], dim=1)
            ppdu_totals[q].index_add_(0, sent_rate, cols)
            if keep_packets:
                kept.append((meta, got, matched))
            continue
        got = engine.decode_coded(rx, csi=engine.stream_csi(rec if nb > 1 else rec[0], rx), rate=rate)["d_info"]
        idx = engine.score_packets(w, n_data, rx, pos0=gap, stride=stride, window=window, totals=totals[q])["scores"][:, 0].long()
        matched = idx >= 0
        diff = (got[idx.clamp(min=0)] ^ info).contiguous().view(torch.uint8)
        err = torch.where(matched, popcount[diff.long()].sum(dim=1), torch.zeros_like(idx))
        info_totals[q] += torch.stack([matched.sum() * kinfo, err.sum(), (err > 0).sum()])
    out = dict(snr_db=snr, totals=totals.cpu().numpy(), power=power, packets=n, samples=n_out)
    if code == "conv":
        out.update(info_totals=info_totals.cpu().numpy())
    if code == "ppdu":
        out.update(ppdu_totals=ppdu_totals.cpu().numpy(), rates=ppdu["rates"], lengths=ppdu["lengths"])
        if keep_packets:
            out.update(ppdu_packets=[(m.cpu().numpy(), g.cpu().numpy().view(np.uint32), ok.cpu().numpy()) for m, g, ok in kept])
    return out


def _ppdu_plan(words, n_data: int, rate, lengths) -> dict:
    """link_sweep's packets with code="ppdu", checked on the host: psdu (uint32 [n, 31]), rates (int32 codes), lengths,
    seeds (1 + i mod 127) and sent (the PSDUs as they go out: the FCS in its place, zeros behind)."""
    from .stream import ppdu_fill  # noqa: PLC0415
    psdu = words.cpu().numpy() if hasattr(words, "cpu") else np.asarray(words)
    if psdu.ndim != 2 or psdu.shape[1] != abi.PPDU_PSDU_WORDS or psdu.dtype not in (np.uint32, np.int32):
        raise ValueError(f"code='ppdu' takes PSDU words uint32 [n, {abi.PPDU_PSDU_WORDS}], got {psdu.dtype} {psdu.shape}")
    psdu = np.ascontiguousarray(psdu).view(np.uint32)
    n = len(psdu)
    if not abi.PPDU_MIN_SYMBOLS <= n_data <= abi.LONG_MAX_DATA_SYMBOLS:
        raise ValueError(f"code='ppdu' needs n_data in [{abi.PPDU_MIN_SYMBOLS}, {abi.LONG_MAX_DATA_SYMBOLS}], got {n_data!r}")
    if isinstance(rate, str) and rate == "mixed":
        rates = np.arange(n, dtype=np.int32) % 3
    elif isinstance(rate, str) or rate is None:
        rates = np.full(n, abi.rate_code(rate), np.int32)
    else:
        rates = np.array([abi.rate_code(r) for r in rate], np.int32)
        if len(rates) != n:
            raise ValueError(f"rate must be one rate, 'mixed' or {n} rates, got {len(rates)}")
    caps = np.array([abi.ppdu_cap(n_data, r) for r in abi.RATE], np.int32)[rates]
    ln = caps if lengths is None else np.asarray(lengths).reshape(-1).astype(np.int32)
    if len(ln) != n:
        raise ValueError(f"lengths must hold {n} values, got {len(ln)}")
    bad = (ln < abi.PPDU_MIN_LENGTH) | (ln > caps)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"packet {k}: LENGTH must be in [{abi.PPDU_MIN_LENGTH}, {caps[k]}] for {n_data} symbols at rate "
                         f"{tuple(abi.RATE)[rates[k]]}, got {ln[k]}")
    return dict(psdu=psdu, rates=rates, lengths=ln, seeds=(1 + np.arange(n) % 127).astype(np.int32), sent=ppdu_fill(psdu, ln))


LINK_COLUMNS = ("snr_db", "transmitted", "matched", "missed", "false_alarms", "packet_err", "bit_err", "bits")
LINK_CODE_COLUMNS = ("info_bits", "info_bit_err", "info_packet_err")     # --code conv: three trailing columns
# --code ppdu: ppdu_totals' five counts per rate of the sent packet
LINK_PPDU_COLUMNS = tuple(f"{name}_{r}" for r in ("1of2", "2of3", "3of4")
                          for name in ("matched", "header_ok", "fcs_ok", "false_accept", "psdu_bit_err"))


def parse_snr_grid(text: str) -> np.ndarray:
    """'LO:HI:STEP' -> LO, LO + STEP, .. up to and including HI; a single number is one point"""
    parts = [float(t) for t in text.split(":")]
    if len(parts) == 1:
        return np.array(parts)
    if len(parts) != 3 or parts[2] <= 0 or parts[1] < parts[0]:
        raise ValueError(f"--snr takes LO:HI:STEP with STEP > 0 and HI >= LO, got {text!r}")
    lo, hi, step = parts
    return lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1)


def link_main(argv=None) -> int:
    """`ofdm_pkg.py link`: transmit -> channel -> receive -> score per SNR point on the device; writes the reference's
    Output_SNR.txt and Output_BER.txt (bit errors over bits compared, on matched packets) and link.csv under --out."""
    import csv  # noqa: PLC0415
    from .channel import NOISE_KINDS, parse_pdp, parse_taps  # noqa: PLC0415
    from .fileio import write_float_array_to_file  # noqa: PLC0415
    from .stream import pack_coded_messages, pack_messages, pack_ppdu_messages  # noqa: PLC0415
    ap = argparse.ArgumentParser(prog="ofdm_pkg.py link", description=link_main.__doc__)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--packets", type=int, help="packets of random payload bits (drawn from --seed)")
    src.add_argument("--messages", help="a text file, one packet per line (at most 180 characters)")
    ap.add_argument("--n-data", type=int, default=None, help="data symbols per packet (default 2, or what the longest line needs)")
    ap.add_argument("--gap", type=int, default=500, help="idle samples before every packet and after the last")
    ap.add_argument("--snr", default="6:40:1", help="SNR grid in dB, LO:HI:STEP")
    ap.add_argument("--cfo-hz", type=float, default=0.0)
    ap.add_argument("--taps", default=None, help="multipath FIR at the oversampled rate, e.g. 1,0,0.4+0.3j")
    ap.add_argument("--noise", choices=list(NOISE_KINDS), default="real")
    ap.add_argument("--fading", choices=["rayleigh"], default=None,
                    help="a Rayleigh channel of its own for every packet, drawn from --seed (alone: --pdp 1, flat)")
    ap.add_argument("--pdp", default=None, help="power delay profile of the fading channel: linear powers per 25 ns tap, "
                                                "e.g. 1,0.5,0.25,0.125 (normalised to sum 1; implies --fading rayleigh)")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x80211A)
    ap.add_argument("--detector", choices=tuple(abi.DETECTOR), default="reference",
                    help="the detection metric: the reference's, or delay-and-correlate with the conjugate at lag 32")
    ap.add_argument("--threshold", type=float, default=abi.DETECT_THRESHOLD, help="a crossing is M > threshold, inside (0, 1)")
    ap.add_argument("--timing", choices=tuple(abi.TIMING), default="none",
                    help="ltf: refine every packet's position against the long training field before the decode "
                         "(ltf-matlab: with the MATLAB convention's template)")
    ap.add_argument("--tracking", choices=tuple(abi.TRACKING), default="none",
                    help="pilots: turn every data symbol back by its four pilots' common phase before the slicer "
                         "(for long packets; costs a little BER on 2-symbol packets)")
    ap.add_argument("--branches", type=int, default=1,
                    help=f"receive antennas, 1 to {abi.DIVERSITY_MAX_BRANCHES}: independently faded and independently noisy "
                         "recordings of the same packets, combined in the receiver (more than 1 needs --detector conjugate)")
    ap.add_argument("--code", choices=["conv", "ppdu"], default=None,
                    help="conv: the packets carry 48 D - 6 information bits through 802.11a's K = 7 rate-1/2 code; the receiver's "
                         "equalised subcarriers go through a soft Viterbi decoder weighted with the channel's gains.  "
                         "ppdu: self-describing packets -- a header symbol names rate and length, the data is scrambled and "
                         "carries a CRC-32, and the receiver reports a packet error rate without knowing what was sent "
                         "(--n-data then counts the header's symbol, default 3)")
    ap.add_argument("--rate", choices=tuple(abi.RATE) + ("mixed",), default="1/2",
                    help="with --code conv: the code's rate; 2/3 and 3/4 are 802.11a's punctured rates, 64 D - 6 and 72 D - 6 "
                         "information bits per packet.  With --code ppdu also mixed: packet i at rate i mod 3 of the three")
    ap.add_argument("--out", default="data")
    a = ap.parse_args(argv)
    if not 0.0 < a.threshold < 1.0:
        raise SystemExit("--threshold must be inside (0, 1)")
    if a.rate != "1/2" and not a.code:
        raise SystemExit(f"--rate {a.rate} needs --code conv")
    if a.rate == "mixed" and a.code != "ppdu":
        raise SystemExit("--rate mixed needs --code ppdu")
    if not 1 <= a.branches <= abi.DIVERSITY_MAX_BRANCHES:
        raise SystemExit(f"--branches must be in [1, {abi.DIVERSITY_MAX_BRANCHES}]")
    if a.branches > 1 and a.detector != "conjugate":
        raise SystemExit("--branches above 1 needs --detector conjugate")
    snr = parse_snr_grid(a.snr)
    fading = None
    if a.fading or a.pdp:
        fading = dict(pdp=parse_pdp(a.pdp or "1"), index0=0)
    if a.messages:
        texts = [ln for ln in Path(a.messages).read_text(encoding="latin-1").splitlines() if ln]
        if not texts:
            raise SystemExit(f"{a.messages}: no lines")
        if a.code == "ppdu":
            rates = [tuple(abi.RATE)[i % 3] for i in range(len(texts))] if a.rate == "mixed" else [a.rate] * len(texts)
            try:
                words, lengths, d = pack_ppdu_messages(texts, a.n_data, rates)
            except ValueError as e:
                raise SystemExit(str(e)) from None
        else:
            words, d = pack_coded_messages(texts, a.n_data, a.rate) if a.code else pack_messages(texts, a.n_data)
    elif a.code == "ppdu":
        if a.packets < 0:
            raise SystemExit("--packets must not be negative")
        d = 3 if a.n_data is None else a.n_data
        if not abi.PPDU_MIN_SYMBOLS <= d <= abi.LONG_MAX_DATA_SYMBOLS:
            raise SystemExit(f"--n-data must be in [{abi.PPDU_MIN_SYMBOLS}, {abi.LONG_MAX_DATA_SYMBOLS}] with --code ppdu")
        words = np.random.default_rng(a.seed).integers(0, 1 << 32, (a.packets, abi.PPDU_PSDU_WORDS), dtype=np.uint64).astype(np.uint32)
        lengths = None
    else:
        if a.packets < 0:
            raise SystemExit("--packets must not be negative")
        d = 2 if a.n_data is None else a.n_data
        if not 1 <= d <= abi.LONG_MAX_DATA_SYMBOLS:
            raise SystemExit(f"--n-data must be in [1, {abi.LONG_MAX_DATA_SYMBOLS}]")
        nw = abi.punct_info_words(d, a.rate) if a.code else 3 * d
        words = np.random.default_rng(a.seed).integers(0, 1 << 32, (a.packets, nw), dtype=np.uint64).astype(np.uint32)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    t0 = time.perf_counter()
    with Engine(0) as eng:
        res = link_sweep(eng, words, d, a.gap, snr, cfo_hz=a.cfo_hz, taps=None if a.taps is None else parse_taps(a.taps),
                         noise=a.noise, seed=a.seed, fading=fading, detector=a.detector, threshold=a.threshold,
                         timing=a.timing, tracking=a.tracking, branches=a.branches, code=a.code, rate=a.rate,
                         **(dict(lengths=lengths, keep_packets=bool(a.messages)) if a.code == "ppdu" else {}))
    wall = time.perf_counter() - t0
    t = res["totals"]
    it = res.get("info_totals")
    ber = t[:, abi.S_BIT_ERR] / np.maximum(t[:, abi.S_BITS], 1)
    write_float_array_to_file(snr, out / "Output_SNR.txt")
    # with a code the file holds the information BER
    write_float_array_to_file(ber if it is None else it[:, 1] / np.maximum(it[:, 0], 1), out / "Output_BER.txt")
    with open(out / "link.csv", "w", newline="") as f:
        wr = csv.writer(f)
        pt = res.get("ppdu_totals")
        wr.writerow(LINK_COLUMNS + (() if it is None else LINK_CODE_COLUMNS) + (() if pt is None else LINK_PPDU_COLUMNS))
        for q, (s, r) in enumerate(zip(snr, t)):
            tx, matched, received = int(r[abi.S_TRANSMITTED]), int(r[abi.S_MATCHED]), int(r[abi.S_RECEIVED])
            row = [f"{s:g}", tx, matched, tx - matched, received - matched, int(r[abi.S_PACKET_ERR]),
                   int(r[abi.S_BIT_ERR]), int(r[abi.S_BITS])]
            line = (f"SNR = {s:5.1f} dB   matched {matched}/{tx}   false alarms {received - matched}   "
                    f"BER = {r[abi.S_BIT_ERR] / max(int(r[abi.S_BITS]), 1):.3e}")
            if it is not None:
                row += [int(v) for v in it[q]]
                line += f"   information BER = {it[q, 1] / max(int(it[q, 0]), 1):.3e}"
            if pt is not None:
                row += [int(v) for v in pt[q].ravel()]
                for name, c in zip(abi.RATE, pt[q]):
                    # blind: what the receiver sees (header invalid or FCS failed); true: the PSDU is not the sent one
                    m, blind = max(int(c[0]), 1), int(c[0] - c[2])
                    line += (f"\n    rate {name}: matched {c[0]}, header right {c[1]}, FCS passed {c[2]}, blind PER {blind / m:.3e}, "
                             f"true PER {(blind + int(c[3])) / m:.3e}, false accepts {c[3]}")
            wr.writerow(row)
            print(line, file=sys.stderr)
            if pt is not None and a.messages:
                meta, psdu, ok = res["ppdu_packets"][q]
                for k in np.nonzero(ok & (meta[:, 0] == 0))[0]:          # only texts whose FCS passed
                    body = psdu[k].astype(">u4").tobytes()[:int(meta[k, 2]) - 4]
                    print(f"SNR = {s:g} dB  packet {k}: {body.decode('latin-1')}")
    print(f"{res['packets']} packets of {d} data symbols, {res['samples']} samples, {len(snr)} SNR points in {wall:.2f} s "
          f"-> {out / 'link.csv'}", file=sys.stderr)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description="802.11a OFDM-QPSK Monte-Carlo sweep on MI355X (OFDM.c main())")
    ap.add_argument("--out", default="data")
    ap.add_argument("--trials", type=int, default=1, help="trials (frame mode) or frames (symbol mode) per SNR")
    ap.add_argument("--mode", choices=["frame", "symbol"], default="frame")
    ap.add_argument("--snr", type=float, nargs="*", help="SNR grid in dB (default 6..40 step 1)")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x80211A)
    ap.add_argument("--est", choices=["ls", "ideal"], default="ls")
    ap.add_argument("--noise", choices=["real", "complex", "none"], default="real")
    ap.add_argument("--channel", choices=["awgn", "rayleigh4"], default="awgn")
    ap.add_argument("--conv", choices=["c", "matlab"], default="c")
    ap.add_argument("--payload", choices=["random", "message", "tester"])
    ap.add_argument("--message", help="MESSAGE payload text (default: OFDM.c:20), up to 180 characters in frame mode (15 data "
                                      "symbols, e.g. the 171-character message of OFDM.c:21), up to 96 in symbol mode")
    ap.add_argument("--evm", choices=["trial", "finite", "pooled"], default="trial",
                    help="EVM files: mean of per-trial EVM_dB (the reference's statistic, -inf after the slicer "
                         "once one trial is clean), the same with the post-slicer mean over finite trials, or pooled")
    ap.add_argument("--print-messages", action="store_true",
                    help="as OFDM.c:1167-1182: receive one capture per SNR point and print the decoded text")
    a = ap.parse_args(argv)
    snr = np.array(a.snr) if a.snr else REF_SNR
    res = reference_main(a.out, a.trials, a.mode, snr, a.seed, est=a.est, noise=a.noise, channel=a.channel,
                         conv=a.conv, payload=a.payload, message=a.message, evm=a.evm)
    for s, b, e in zip(res.snr_db, res.ber, res.evm_pre_db):
        print(f"SNR = {s:5.1f} dB   BER = {b:.3e}   EVM = {e:7.2f} dB", file=sys.stderr)
    if a.print_messages:
        for line in received_messages(snr, a.message, a.seed):
            print(line)


def received_messages(snr_db, message: str | None = None, seed: int = 0x80211A, device: int = 0):
    """One reference trial per SNR point -- Transmission_Over_Air + capture + Receiver (OFDM.c:1202-1211)
    -- yielding the console text the reference prints (OFDM.c:1177-1181)."""
    with Engine(device) as eng:
        if message is not None:
            set_message(eng, message)
        nd = eng.payload_frames("message")
        w = eng.transmitter("c", "message")
        L = abi.capture_len(nd)
        rng = np.random.default_rng(seed)
        for i, s in enumerate(np.asarray(snr_db, np.float64)):
            ota = eng.transmission_over_air(w, float(s), seed=seed, trial=0, snr_index=i)
            rs = int(rng.integers(0, len(w) - L))               # rand() % (len - cap) (OFDM.c:949)
            o = eng.receiver(ota[rs:rs + L], "c", "message")
            yield f"SNR = {s:.0f} dB\nReceived Message: \n{o['message']}"


if __name__ == "__main__":
    main()
