#!/usr/bin/env python3
"""Rate of the per-packet fading transmitter (ofdm_transmit_faded) on one GPU, against the unfaded transmitter on the
same buffers and against the host loop it replaces.

bench.py has no workload for it, so this tool measures the shape a fading link sweep runs: 2^16 packets of random
payloads and random taps, laid out densely (stride = faded packet length) in one device-resident recording, at D = 2
and D = 15 data symbols and L = 1, 4 and 32 taps, through the C ABI with every buffer allocated beforehand, so a timed
launch holds no allocation and no host synchronisation.  Per D, interleaved and each timed over `--launches` launches
between device events after a warm-up:

  unfaded_store / unfaded_accumulate     ofdm_transmit_packets into the same recording: the cost without the channel
  faded_L{1,4,32}_store / _accumulate    ofdm_transmit_faded

and once per (D, L), over `--baseline-packets` packets:

  host_loop     Engine.transmit_packets + Engine.impair_stream (noise none, the packet's taps), one packet at a time;
                its samples are compared with the batch's bit for bit

Reported per (D, L, mode): packets/s and output bytes/s, the ratio to the unfaded transmitter and to the host loop, and
the fp32 fused multiply-adds per second of the FIR alone (16 L per four outputs).  Also times ofdm_draw_taps for the
batch.  Writes one JSON record (default profiles/r12/fading/fading_rate.json).

    python tools/fading_rate.py [--packets N] [--launches K] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--baseline-packets", type=int, default=300)
    ap.add_argument("--data-symbols", default="2,15")
    ap.add_argument("--taps", default="1,4,32")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12" / "fading" / "fading_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415

    n = a.packets
    Ls = [int(t) for t in a.taps.split(",")]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    per_d = {}
    with pkg.Engine(0) as eng:
        for d in (int(t) for t in a.data_symbols.split(",")):
            plen = abi.packet_len(d)
            rng = np.random.default_rng(0xFA + d)
            words = torch.from_numpy(rng.integers(0, 1 << 32, (n, 3 * d), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
            taps = {L: torch.from_numpy((0.25 * (rng.standard_normal((n, L)) + 1j * rng.standard_normal((n, L))))
                                        .astype(np.complex64)).cuda() for L in Ls}
            rec = torch.zeros(n * abi.faded_len(d, max(Ls)), dtype=torch.complex64, device="cuda")

            def unfaded(flags: int):
                opts = abi.TxOpts(abi.CONV["c"], 1, d, flags)
                abi.check(eng.lib, eng.lib.ofdm_transmit_packets(
                    eng.ctx, C.byref(opts), ptr(words), n, None, 0, plen, None, None, ptr(rec), n * plen), "transmit_packets")

            def faded(L: int, flags: int):
                opts = abi.TxOpts(abi.CONV["c"], 1, d, flags)
                fl = abi.faded_len(d, L)
                abi.check(eng.lib, eng.lib.ofdm_transmit_faded(
                    eng.ctx, C.byref(opts), ptr(words), n, None, 0, fl, None, None, ptr(taps[L]), L, ptr(rec), n * fl),
                    "transmit_faded")

            variants = {"unfaded_store": lambda: unfaded(0), "unfaded_accumulate": lambda: unfaded(abi.TX_ACCUMULATE)}
            for L in Ls:
                variants[f"faded_L{L}_store"] = lambda L=L: faded(L, 0)
                variants[f"faded_L{L}_accumulate"] = lambda L=L: faded(L, abi.TX_ACCUMULATE)
            drawn = torch.zeros((n, max(Ls)), dtype=torch.complex64, device="cuda")
            pdp = np.full(max(Ls), 1.0 / max(Ls), np.float32)
            variants[f"draw_taps_L{max(Ls)}"] = lambda: abi.check(eng.lib, eng.lib.ofdm_draw_taps(
                eng.ctx, 0x80211A, 0, n, max(Ls), pdp.ctypes.data_as(C.c_void_p), ptr(drawn)), "draw_taps")
            for f in variants.values():                             # warm-up: code objects, allocator, clocks
                f()
                f()
            torch.cuda.synchronize()
            ms = {v: [] for v in variants}
            for _ in range(a.launches):
                for v, f in variants.items():                       # interleaved
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    ms[v].append(e0.elapsed_time(e1))
            med = {v: float(np.median(t)) for v, t in ms.items()}

            # ---- the route it replaces: one transmit_packets and one impair_stream per packet ----
            nb = min(a.baseline_packets, n)
            host = {}
            for L in Ls:
                fl = abi.faded_len(d, L)
                h = taps[L][:nb].cpu().numpy()
                tmp = torch.zeros(fl, dtype=torch.complex64, device="cuda")          # [w_k | L - 1 zeros]
                dst = torch.zeros(nb * fl, dtype=torch.complex64, device="cuda")

                def one(k):
                    eng.transmit_packets(words[k:k + 1], d, out=tmp[:plen])
                    eng.impair_stream(tmp, 1.0, 0.0, taps=h[k], noise="none", out=dst[k * fl:(k + 1) * fl])
                for k in range(3):                                  # warm-up
                    one(k)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(nb):
                    one(k)
                torch.cuda.synchronize()
                host_s = time.perf_counter() - t0
                faded(L, 0)
                torch.cuda.synchronize()
                same = bool(torch.equal(rec[:nb * fl].view(torch.float32).view(torch.int32),
                                        dst.view(torch.float32).view(torch.int32)))
                host[L] = {"packets": nb, "seconds": host_s, "packets_per_s": nb / host_s, "same_bits_as_the_batch": same}

            row = {"packet_samples": plen,
                   "unfaded": {m: {"ms": ms[f"unfaded_{m}"], "ms_median": med[f"unfaded_{m}"],
                                   "packets_per_s": n / (med[f"unfaded_{m}"] * 1e-3),
                                   "output_bytes_per_s": 8.0 * n * plen / (med[f"unfaded_{m}"] * 1e-3)}
                               for m in ("store", "accumulate")},
                   "draw_taps": {"n_taps": max(Ls), "ms": ms[f"draw_taps_L{max(Ls)}"],
                                 "ms_median": med[f"draw_taps_L{max(Ls)}"],
                                 "taps_per_s": n * max(Ls) / (med[f"draw_taps_L{max(Ls)}"] * 1e-3)},
                   "taps": {}}
            for L in Ls:
                fl = abi.faded_len(d, L)
                row["taps"][str(L)] = {"faded_samples": fl, "host_loop": host[L]}
                for m in ("store", "accumulate"):
                    t = med[f"faded_L{L}_{m}"] * 1e-3
                    row["taps"][str(L)][m] = {
                        "ms": ms[f"faded_L{L}_{m}"], "ms_median": med[f"faded_L{L}_{m}"], "packets_per_s": n / t,
                        "output_bytes_per_s": 8.0 * n * fl / t, "fir_fma_per_s": 4.0 * L * n * fl / t,
                        "time_over_unfaded": med[f"faded_L{L}_{m}"] / med[f"unfaded_{m}"],
                        "over_host_loop": (n / t) / host[L]["packets_per_s"]}
            per_d[str(d)] = row
            del rec, words, taps, drawn
            torch.cuda.empty_cache()

    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {k: r.get(k) for k in ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]",
                                               "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
             for r in rows if r.get("source") == "ofdm_fading.hip"}
    out_rec = {"packets": n, "launches": a.launches,
               "layout": "dense: pos0 = 0, stride = the (faded) packet length, conv c, no gain or carrier offset",
               "unit": "device events around one launch; medians", "data_symbols": per_d, "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(out_rec, indent=1) + "\n")
    brief = {}
    for d, r in per_d.items():
        brief[d] = {"unfaded_store_pps": r["unfaded"]["store"]["packets_per_s"],
                    "unfaded_accumulate_pps": r["unfaded"]["accumulate"]["packets_per_s"],
                    "draw_taps_per_s": r["draw_taps"]["taps_per_s"]}
        for L, t in r["taps"].items():
            brief[d][f"L{L}"] = {"store_pps": t["store"]["packets_per_s"], "accumulate_pps": t["accumulate"]["packets_per_s"],
                                 "store_time_over_unfaded": t["store"]["time_over_unfaded"],
                                 "accumulate_time_over_unfaded": t["accumulate"]["time_over_unfaded"],
                                 "store_fir_fma_per_s": t["store"]["fir_fma_per_s"],
                                 "host_loop_pps": t["host_loop"]["packets_per_s"],
                                 "store_over_host_loop": t["store"]["over_host_loop"],
                                 "host_loop_same_bits": t["host_loop"]["same_bits_as_the_batch"]}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
