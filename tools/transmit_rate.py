#!/usr/bin/env python3
"""Rate of the batched packet transmitter (ofdm_transmit_packets) on one GPU, against a device copy of the same bytes
and against the only route there was before it.

bench.py has no workload for it, so this tool measures the shape a traffic generator runs: 2^16 packets of random
payloads, laid out densely (stride = packet length) in one device-resident recording, at D = 2 and D = 15 data symbols,
through the C ABI with every buffer allocated beforehand, so a timed launch holds no allocation and no host
synchronisation.  Per D, interleaved and each timed over `--launches` launches between device events after a warm-up:

  store         plain stores into the recording
  accumulate    OFDM_TX_ACCUMULATE: fp32 atomic adds onto the recording
  store_impaired  store mode with a per-packet gain and carrier offset (the fp64 phase and the sine / cosine per sample)
  copy          the yardstick: torch's device-to-device copy of as many bytes as the transmitter writes (it also
                reads them, which the transmitter does not)

and once, over `--baseline-packets` packets:

  host_loop     the parent route: set_long_message + transmitter() + upload of the first period, one packet at a time

Reported per D: packets/s and output bytes/s, the fraction of the 8 TB/s HBM peak (store), the fraction of the
~1.3 TB/s the memory side adds float atomics at (accumulate), the ratio to the copy and the ratio to the host loop.
Writes one JSON record (default profiles/r10/transmit/transmit_rate.json).

    python tools/transmit_rate.py [--packets N] [--launches K] [--out FILE]
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

HBM_BYTES_PER_S = 8e12
ATOMIC_BYTES_PER_S = 1.3e12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--baseline-packets", type=int, default=300)
    ap.add_argument("--data-symbols", default="2,15")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10" / "transmit" / "transmit_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.fileio import decode_message  # noqa: PLC0415

    n = a.packets
    ptr = lambda t: C.c_void_p(t.data_ptr())
    per_d = {}
    with pkg.Engine(0) as eng:
        for d in (int(t) for t in a.data_symbols.split(",")):
            plen = abi.packet_len(d)
            n_out = n * plen
            rng = np.random.default_rng(0x7A + d)
            words = torch.from_numpy(rng.integers(0, 1 << 32, (n, 3 * d), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
            gains = torch.from_numpy((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)).cuda()
            cfos = torch.from_numpy(rng.uniform(-110e3, 110e3, n).astype(np.float32)).cuda()
            rec = torch.zeros(n_out, dtype=torch.complex64, device="cuda")
            src = torch.zeros(n_out, dtype=torch.complex64, device="cuda")

            def launch(flags: int, impaired: bool):
                opts = abi.TxOpts(abi.CONV["c"], 1, d, flags)
                abi.check(eng.lib, eng.lib.ofdm_transmit_packets(
                    eng.ctx, C.byref(opts), ptr(words), n, None, 0, plen, ptr(gains) if impaired else None,
                    ptr(cfos) if impaired else None, ptr(rec), n_out), "transmit_packets")

            variants = {"store": lambda: launch(0, False), "accumulate": lambda: launch(abi.TX_ACCUMULATE, False),
                        "store_impaired": lambda: launch(0, True), "copy": lambda: rec.copy_(src)}
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

            # ---- the parent route: one message, one waveform, one upload per packet ----
            nb = min(a.baseline_packets, n)
            host_words = words[:nb].cpu().numpy().view(np.uint32)
            bits = ((host_words[..., None] >> np.arange(31, -1, -1, dtype=np.uint32)) & 1).reshape(nb, -1)
            texts = [decode_message(row).encode("latin-1") for row in bits]      # any 12 D bytes are a message
            dst = torch.zeros(nb * plen, dtype=torch.complex64, device="cuda")
            for k in range(3):                                      # warm-up
                eng.set_long_message(texts[k])
                dst[:plen] = torch.from_numpy(eng.transmitter("c", "message")[:plen]).cuda()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(nb):
                eng.set_long_message(texts[k])
                dst[k * plen:(k + 1) * plen] = torch.from_numpy(eng.transmitter("c", "message")[:plen]).cuda()
            torch.cuda.synchronize()
            host_s = time.perf_counter() - t0
            # the two routes build the same packets
            launch(0, False)
            torch.cuda.synchronize()
            dev = float((rec[:nb * plen] - dst).abs().max() / dst.abs().max())

            med = {v: float(np.median(t)) for v, t in ms.items()}
            pps = {v: n / (med[v] * 1e-3) for v in ms}
            bps = {v: 8.0 * n_out / (med[v] * 1e-3) for v in ms}
            host_pps = nb / host_s
            per_d[str(d)] = {
                "packet_samples": plen, "output_bytes": 8 * n_out,
                "variants": {v: {"ms": ms[v], "ms_median": med[v], "ms_min": min(ms[v]), "ms_max": max(ms[v]),
                                 "packets_per_s": pps[v], "output_bytes_per_s": bps[v]} for v in ms},
                "store_fraction_of_8TBps": bps["store"] / HBM_BYTES_PER_S,
                "accumulate_fraction_of_1p3TBps": bps["accumulate"] / ATOMIC_BYTES_PER_S,
                "store_over_copy": bps["store"] / bps["copy"],
                "accumulate_over_copy": bps["accumulate"] / bps["copy"],
                "store_impaired_over_store": bps["store_impaired"] / bps["store"],
                "host_loop": {"packets": nb, "seconds": host_s, "packets_per_s": host_pps,
                              "normwise_against_the_batch": dev},
                "store_over_host_loop": pps["store"] / host_pps,
                "accumulate_over_host_loop": pps["accumulate"] / host_pps}
            del rec, src, words, gains, cfos, dst
            torch.cuda.empty_cache()

    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {k: r.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                               "Occupancy [waves/SIMD]")} for r in rows if r.get("source") == "ofdm_transmit.hip"}
    out_rec = {"packets": n, "launches": a.launches, "layout": "dense: pos0 = 0, stride = packet length, conv c",
               "unit": "device events around one launch; medians",
               "yardsticks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "float_atomic_bytes_per_s": ATOMIC_BYTES_PER_S},
               "data_symbols": per_d, "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(out_rec, indent=1) + "\n")
    print(json.dumps({d: {"store_packets_per_s": r["variants"]["store"]["packets_per_s"],
                          "store_bytes_per_s": r["variants"]["store"]["output_bytes_per_s"],
                          "accumulate_bytes_per_s": r["variants"]["accumulate"]["output_bytes_per_s"],
                          "impaired_bytes_per_s": r["variants"]["store_impaired"]["output_bytes_per_s"],
                          "copy_bytes_per_s": r["variants"]["copy"]["output_bytes_per_s"],
                          "store_over_copy": r["store_over_copy"], "host_loop_packets_per_s": r["host_loop"]["packets_per_s"],
                          "store_over_host_loop": r["store_over_host_loop"],
                          "host_loop_normwise": r["host_loop"]["normwise_against_the_batch"]} for d, r in per_d.items()}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
