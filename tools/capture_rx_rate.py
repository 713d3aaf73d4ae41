#!/usr/bin/env python3
"""Rate of the batched receiver for caller-supplied captures (ofdm_receive_captures) on one GPU.

bench.py has no workload for it, so this tool measures the shape a user with recorded captures runs: 2^17 captures of
3,008 samples resident on the device (channel.make_captures: 14 dB real-only noise, a 20 kHz offset), decoded by
Engine.receive_captures -- records only, and with the equalised subcarriers written as well -- each timed over
`--launches` launches between device events after a warm-up, the two variants interleaved.  Beside it, from the same
run:
  (a) the only path there was before: a loop of 200 Engine.receiver calls (one upload, launch and synchronise each),
      host clock;
  (b) the HBM floor: the n x pitch x 8 bytes the kernel must read over the measured time, as a fraction of 8 TB/s;
  (c) ofdm_frame_sweep's trials per second of kernel time on the same 2-symbol message (captures drawn in the kernel).
Writes one JSON record (default profiles/r08/captures/capture_rx_rate.json).

    python tools/capture_rx_rate.py [--captures N] [--launches K] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12
SNR_DB, CFO_HZ = 14.0, 20e3
SWEEP_SNR = np.arange(0.0, 31.0, 2.0)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--captures", type=int, default=1 << 17)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--receiver-calls", type=int, default=200)
    ap.add_argument("--sweep-trials", type=int, default=1 << 16)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08" / "captures" / "capture_rx_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.channel import make_captures  # noqa: PLC0415

    with pkg.Engine(0) as eng:
        nd = eng.payload_frames("message")
        L = abi.capture_len(nd)
        w = eng.transmitter("c", "message")
        wave = torch.from_numpy(w).cuda()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0xCA97)
        caps = torch.empty((a.captures, L), dtype=torch.complex64, device="cuda")
        for lo in range(0, a.captures, 8192):                       # the index and phase temporaries stay small
            m = min(8192, a.captures - lo)
            starts = torch.randint(0, len(w) - L, (m,), generator=gen, device="cuda")
            caps[lo:lo + m] = make_captures(wave, starts, SNR_DB, CFO_HZ, noise="real", generator=gen, cap_len=L)
        torch.cuda.synchronize()
        variants = {"records": dict(want_bits=False, want_eq=False), "records_eq": dict(want_bits=False, want_eq=True)}

        def launch(v):
            # records_eq runs the kernel variant that also parks the spectra and writes outputs (the bit words leave from
            # the same pass; their unpacking and decoding in Engine.receive_captures is host and torch work, not timed)
            return eng.receive_captures(caps, **variants[v])

        row = eng.new_counters(1)[0]
        eng.receive_captures(caps, want_bits=False, counters=row)   # warm-up, and the batch's own outcome
        for v in variants:
            launch(v)
        torch.cuda.synchronize()
        c = row.cpu().numpy()
        ms = {v: [] for v in variants}
        for _ in range(a.launches):
            for v in variants:                                      # interleaved
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(v)
                e1.record()
                e1.synchronize()
                ms[v].append(e0.elapsed_time(e1))
        # (a) the single-capture path
        host = caps[:a.receiver_calls].cpu().numpy()
        eng.receiver(host[0])
        t0 = time.perf_counter()
        for k in range(len(host)):
            eng.receiver(host[k])
        rx_s = time.perf_counter() - t0
        # (c) the in-kernel capture generator's sweep, kernel time
        cfg = pkg.make_cfg(payload="message")
        eng.frame_sweep(cfg, SWEEP_SNR, a.sweep_trials)
        eng.timing(True)
        sw_ms = []
        for _ in range(5):
            eng.timing_reset()
            eng.frame_sweep(cfg, SWEEP_SNR, a.sweep_trials)
            sw_ms.append(eng.timing_query(abi.K_FRAME)[0])
        eng.timing(False)

    def rate(v):
        return a.captures / (float(np.median(ms[v])) * 1e-3)

    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {x["name"]: {k: x.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")}
             for x in rows if "capture_rx_kernel" in x["name"]}
    single = len(host) / rx_s
    bytes_read = float(a.captures) * L * 8
    rec = {"captures": a.captures, "capture_samples": L, "data_symbols": nd, "launches": a.launches,
           "snr_db": SNR_DB, "cfo_hz": CFO_HZ, "unit": "captures/s (device events around one launch)",
           "batch": {v: {"ms": ms[v], "rate_median": rate(v), "rate_min": a.captures / (max(ms[v]) * 1e-3),
                         "rate_max": a.captures / (min(ms[v]) * 1e-3)} for v in variants},
           "batch_outcome": {"sync_fail": int(c[abi.C_SYNC_FAIL]), "frame_err": int(c[abi.C_FRAME_ERR]),
                             "ber": float(c[abi.C_BIT_ERR] / max(c[abi.C_BITS], 1))},
           "a_receiver_loop": {"calls": len(host), "seconds": rx_s, "captures_per_s": single},
           "batch_over_receiver_loop": rate("records") / single,
           "b_hbm_floor": {"bytes_read": bytes_read, "bytes_per_s": bytes_read / (float(np.median(ms["records"])) * 1e-3),
                           "fraction_of_8TBps": bytes_read / (float(np.median(ms["records"])) * 1e-3) / HBM_BYTES_PER_S},
           "c_frame_sweep": {"snr_points": len(SWEEP_SNR), "trials": a.sweep_trials, "ms": sw_ms,
                             "trials_per_s_kernel_time": a.sweep_trials * len(SWEEP_SNR) / (float(np.median(sw_ms)) * 1e-3)},
           "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"captures_per_s": rate("records"), "with_eq": rate("records_eq"),
                      "receiver_loop": single, "batch_over_loop": rec["batch_over_receiver_loop"],
                      "hbm_fraction": rec["b_hbm_floor"]["fraction_of_8TBps"],
                      "frame_sweep_trials_per_s": rec["c_frame_sweep"]["trials_per_s_kernel_time"]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
