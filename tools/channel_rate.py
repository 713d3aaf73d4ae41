#!/usr/bin/env python3
"""Rate of the device channel (ofdm_impair_stream) on one GPU, against the torch route it stands beside
(channel.impair_stream) and against a device copy of the same bytes, and the rate of the whole link sweep.

bench.py has no workload for it, so this tool measures the shape a link sweep runs: one device-resident recording of
2^26 and of 2^28 samples, impaired into a second buffer that is allocated beforehand, so a timed fused launch holds no
allocation and no host synchronisation.  Per size and case, interleaved and each timed between device events after a
warm-up:

  fused   Engine.impair_stream into a preallocated buffer: one kernel, 8 bytes read and 8 written per sample
  torch   channel.impair_stream on the same recording (one pass per tap, fp64 temporaries for the rotation,
          torch.randn for the noise); it allocates its result and its temporaries
  copy    the yardstick: torch's device-to-device copy of the recording (the same 16 bytes per sample)

Cases: real noise only; complex noise only; 3 taps; 32 taps; 3 taps with a 40 kHz offset and complex noise.
Also recorded: torch.cuda.max_memory_allocated over one call of either route (above what is allocated before it),
and the link sweep (sweep.link_sweep: transmit once, then impair, receive and score per SNR point) in packets per
second for 2^16 packets of D = 2 over 8 SNR points.  Writes one JSON record (default
profiles/r11/channel/channel_rate.json).

    python tools/channel_rate.py [--log2-samples 26,28] [--launches K] [--out FILE]
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
TAPS3 = np.array([1, 0, 0.4 + 0.3j], np.complex64)


def cases():
    r = np.random.default_rng(0xC4A)
    taps32 = ((r.standard_normal(32) + 1j * r.standard_normal(32)) * 0.25).astype(np.complex64)
    return {"noise_real": dict(noise="real"), "noise_complex": dict(noise="complex"),
            "taps3": dict(taps=TAPS3, noise="none"), "taps32": dict(taps=taps32, noise="none"),
            "taps3_cfo_complex": dict(taps=TAPS3, cfo_hz=40e3, noise="complex")}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--log2-samples", default="26,28")
    ap.add_argument("--launches", type=int, default=10, help="timed launches per route and case")
    ap.add_argument("--link-packets", type=int, default=1 << 16)
    ap.add_argument("--link-points", type=int, default=8)
    ap.add_argument("--link-repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11" / "channel" / "channel_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib, channel, sweep  # noqa: PLC0415

    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    sizes = {}
    with pkg.Engine(0) as eng:
        for lg in (int(t) for t in a.log2_samples.split(",")):
            n = 1 << lg
            x = torch.view_as_complex(torch.randn((n, 2), generator=gen, device="cuda", dtype=torch.float32))
            out = torch.empty_like(x)
            per_case = {}
            for name, kw in cases().items():
                routes = {"fused": lambda kw=kw: eng.impair_stream(x, 2.0, 20.0, out=out, **kw),
                          "torch": lambda kw=kw: channel.impair_stream(x, 2.0, 20.0, generator=gen, **kw),
                          "copy": lambda: out.copy_(x)}
                peak = {}
                for r, f in routes.items():                         # warm-up, and the peak memory of one call
                    f()
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    f()
                    torch.cuda.synchronize()
                    peak[r] = torch.cuda.max_memory_allocated() - base
                ms = {r: [] for r in routes}
                for _ in range(a.launches):
                    for r, f in routes.items():                     # interleaved
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ms[r].append(e0.elapsed_time(e1))
                med = {r: float(np.median(t)) for r, t in ms.items()}
                sps = {r: n / (med[r] * 1e-3) for r in ms}
                per_case[name] = {
                    "routes": {r: {"ms": ms[r], "ms_median": med[r], "ms_min": min(ms[r]), "ms_max": max(ms[r]),
                                   "samples_per_s": sps[r], "peak_bytes_above_inputs": peak[r]} for r in ms},
                    "fused_bytes_per_s": 16.0 * sps["fused"],
                    "fused_fraction_of_8TBps": 16.0 * sps["fused"] / HBM_BYTES_PER_S,
                    "fused_over_torch": sps["fused"] / sps["torch"], "fused_over_copy": sps["fused"] / sps["copy"]}
                torch.cuda.empty_cache()
            sizes[str(lg)] = {"samples": n, "cases": per_case}
            del x, out
            torch.cuda.empty_cache()

        # ---- the link sweep: transmit once; impair, receive and score per SNR point; one read-back at the end ----
        words = np.random.default_rng(7).integers(0, 1 << 32, (a.link_packets, 6), dtype=np.uint64).astype(np.uint32)
        snr = np.linspace(5.0, 40.0, a.link_points)
        kw = dict(cfo_hz=40e3, taps=TAPS3, noise="complex")
        sweep.link_sweep(eng, words[:256], 2, 500, snr, **kw)                  # warm-up
        sweep.link_sweep(eng, words, 2, 500, snr, **kw)
        wall = []
        for _ in range(a.link_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = sweep.link_sweep(eng, words, 2, 500, snr, **kw)              # ends in the totals' read-back
            wall.append(time.perf_counter() - t0)
        link = {"packets": a.link_packets, "n_data": 2, "gap": 500, "snr_db": snr.tolist(), "channel": "3 taps, 40 kHz, complex noise",
                "samples": res["samples"], "wall_s": wall, "wall_s_median": float(np.median(wall)),
                "packets_per_s": a.link_packets * a.link_points / float(np.median(wall)),
                "totals": res["totals"].tolist()}

    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {k: r.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                               "Occupancy [waves/SIMD]")} for r in rows if r.get("source") == "ofdm_channel.hip"}
    rec = {"launches": a.launches, "unit": "device events around one call; medians; link: host clock around the sweep",
           "yardsticks": {"hbm_bytes_per_s": HBM_BYTES_PER_S}, "sizes": sizes, "link": link, "resource_usage": usage,
           "tile": abi.CHANNEL_TILE}
    p = Path(a.out)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"sizes": {lg: {c: {"fused_samples_per_s": v["routes"]["fused"]["samples_per_s"],
                                         "torch_samples_per_s": v["routes"]["torch"]["samples_per_s"],
                                         "copy_samples_per_s": v["routes"]["copy"]["samples_per_s"],
                                         "fused_peak": v["routes"]["fused"]["peak_bytes_above_inputs"],
                                         "torch_peak": v["routes"]["torch"]["peak_bytes_above_inputs"]}
                                     for c, v in s["cases"].items()} for lg, s in sizes.items()},
                      "link_packets_per_s": link["packets_per_s"], "link_wall_s": link["wall_s"]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
