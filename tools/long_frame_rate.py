#!/usr/bin/env python3
"""Rate of a long-message frame sweep (171 characters: 15 data symbols per frame, 9,394-sample captures) on one GPU.

bench.py has no workload for frames of more than 8 data symbols, so this tool measures the shape: a sweep over the
bench's 16 SNR points, the ring sync kernel (frame_ring_xl_kernel, the default route) and the whole-capture route
(frame_whole_xl_kernel, OFDM_FRAME_NO_LONG=1) interleaved on the same device after a warm-up of each, in symbol-SNR
evaluations per second of kernel time (ofdm_timing_query: sync + symbol kernels, as bench.py's frame workloads).
Writes one JSON record (default profiles/r07/long_frames/long_frame_rate.json) with both rates and the kernels'
resource usage from the build's report.

    python tools/long_frame_rate.py [--trials N] [--reps K] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MESSAGE = ("The reference ships a second, longer message next to its default one; this stand-in has that length, "
           "171 characters, and frames as fifteen data symbols of ninety-six bits.")
SNR_GRID = np.arange(0.0, 31.0, 2.0)
ROUTES = {"ring": None, "whole": "1"}            # OFDM_FRAME_NO_LONG per route


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trials", type=int, default=65536, help="trials per SNR point and sweep")
    ap.add_argument("--reps", type=int, default=5, help="timed sweeps per route, interleaved")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r07" / "long_frames" / "long_frame_rate.json"))
    a = ap.parse_args(argv)
    assert len(MESSAGE) == 171, len(MESSAGE)
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415

    def sweep(eng, route):
        if ROUTES[route]:
            os.environ["OFDM_FRAME_NO_LONG"] = ROUTES[route]
        else:
            os.environ.pop("OFDM_FRAME_NO_LONG", None)
        try:
            return eng.frame_sweep(cfg, SNR_GRID, a.trials)
        finally:
            os.environ.pop("OFDM_FRAME_NO_LONG", None)

    with pkg.Engine(0) as eng:
        nd = eng.set_long_message(MESSAGE)
        if nd != 15:
            raise SystemExit(f"set_long_message framed {nd} data symbols, expected 15")
        cfg = pkg.make_cfg(payload="message")
        ref = {r: sweep(eng, r) for r in ROUTES}                 # warm-up of each route (and the scratch allocation)
        if not np.array_equal(ref["ring"], ref["whole"]):
            raise SystemExit("the two routes disagree on the counters")
        eng.timing(True)
        ms = {r: [] for r in ROUTES}
        for _ in range(a.reps):
            for r in ROUTES:                                      # interleaved: ring, whole, ring, whole, ...
                eng.timing_reset()
                sweep(eng, r)
                ms[r].append(eng.timing_query(abi.K_FRAME)[0])
        eng.timing(False)
    units = float(a.trials) * nd * len(SNR_GRID)                  # symbol-SNR evaluations per sweep
    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {x["name"]: {k: x.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]",
                                               "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
             for x in rows if "_xl_kernel" in x["name"]}
    rec = {"message_chars": len(MESSAGE), "data_symbols": nd, "capture_samples": abi.capture_len(nd),
           "snr_points": len(SNR_GRID), "trials": a.trials, "reps": a.reps, "unit": "symbol-SNR evaluations/s (kernel time)",
           "routes": {r: {"kernel": "frame_ring_xl_kernel" if r == "ring" else "frame_whole_xl_kernel",
                          "ms": ms[r], "rate_median": units / (float(np.median(ms[r])) * 1e-3),
                          "rate_min": units / (max(ms[r]) * 1e-3), "rate_max": units / (min(ms[r]) * 1e-3)}
                      for r in ROUTES},
           "ber_30dB": float(ref["ring"][-1, abi.C_BIT_ERR] / max(ref["ring"][-1, abi.C_BITS], 1)),
           "resource_usage": usage}
    rec["ring_over_whole"] = rec["routes"]["ring"]["rate_median"] / rec["routes"]["whole"]["rate_median"]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: rec[k] for k in ("data_symbols", "snr_points", "trials", "ring_over_whole")} |
                     {r: rec["routes"][r]["rate_median"] for r in ROUTES}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
