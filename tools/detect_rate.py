#!/usr/bin/env python3
"""Rate of the stream receiver's optional detection kernels (ofdm_receive_stream_ex, csrc/ofdm_stream_conj.hip) on one
GPU, against stream_detect_kernel on the same buffers.

The recording is tools/stream_rx_rate.py's: one stream of 2^28 samples (2 GiB) resident on the device -- back-to-back
2-symbol frames behind 500-sample idle gaps, 14 dB real-only noise over all of it, a 20 kHz offset.  Every variant is the
detection and selection of one call with max_packets = 0 (no decode launch), outputs preallocated:

  reference       ofdm_receive_stream: stream_detect_kernel<false>, the yardstick (the parent's code object, unchanged)
  conjugate       ofdm_receive_stream_ex {CONJUGATE, 0.75}: stream_detect_conj_kernel<false>
  reference_thr   ofdm_receive_stream_ex {REFERENCE, 0.6}: stream_detect_thr_kernel<false>

`--launches` launches per variant, interleaved, after a warm-up.  A launch is timed twice: the whole call between
device events of the caller, and the detection kernel alone between the library's own events (ofdm_timing_query, reset
before and read after every launch); the ratio the record leads with is of the kernels' medians.
Writes one JSON record (default profiles/r13/detect/detect_rate.json).

    python tools/detect_rate.py [--samples N] [--launches K] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12
SNR_DB, CFO_HZ, GAP = 14.0, 20e3, 500
UNITS_PER_CHUNK = 2048


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13" / "detect" / "detect_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.channel import make_stream  # noqa: PLC0415
    from ofdm_amd.stream import synthetic_segments  # noqa: PLC0415

    n = a.samples
    with pkg.Engine(0) as eng:
        w = eng.transmitter("c", "message")
        period = len(w) // 10
        wave = torch.from_numpy(w).cuda()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x57EA)
        x = torch.empty(n, dtype=torch.complex64, device="cuda")
        seg = synthetic_segments(period, UNITS_PER_CHUNK, GAP)[:-1]     # whole gap + frame units
        chunk = UNITS_PER_CHUNK * (GAP + period)
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            x[lo:lo + m] = make_stream(wave, seg, SNR_DB, CFO_HZ, noise="real", generator=gen)[:m]
        torch.cuda.synchronize()

        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        opts = abi.make_rx_opts("c")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        tail = (abi.PAYLOAD["message"], 0, None, ptr(cnt), None, None, None, None, None)
        conj, thr = abi.make_stream_opts("conjugate", 0.75), abi.make_stream_opts("reference", 0.6)

        def reference():
            abi.check(eng.lib, eng.lib.ofdm_receive_stream(eng.ctx, ptr(x), n, C.byref(opts), *tail), "receive_stream")

        def extended(so):
            abi.check(eng.lib, eng.lib.ofdm_receive_stream_ex(eng.ctx, ptr(x), n, C.byref(opts), C.byref(so), *tail),
                      "receive_stream_ex")

        variants = {"reference": (reference, abi.K_STREAM_DETECT, "stream_detect_kernel<false>"),
                    "conjugate": (lambda: extended(conj), abi.K_STREAM_DETECT_CONJ, "stream_detect_conj_kernel<false>"),
                    "reference_thr": (lambda: extended(thr), abi.K_STREAM_DETECT, "stream_detect_thr_kernel<false>")}
        found = {}
        for v, (f, _, _) in variants.items():                       # warm-up: code objects, scratch
            f()
            torch.cuda.synchronize()
            found[v] = int(cnt.cpu()[0])
        call_ms = {v: [] for v in variants}
        kernel_ms = {v: [] for v in variants}
        eng.timing(True)
        for _ in range(a.launches):
            for v, (f, kid, _) in variants.items():                 # interleaved
                eng.timing_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                call_ms[v].append(e0.elapsed_time(e1))
                ms, launches = eng.timing_query(kid)
                assert launches == 1
                kernel_ms[v].append(ms)
        eng.timing(False)
        scratch = eng.scratch_bytes()

    med = {v: float(np.median(t)) for v, t in kernel_ms.items()}
    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {k: r.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                               "Occupancy [waves/SIMD]")}
             for r in rows if "stream_detect" in r.get("name", "")}
    rec = {"samples": n, "stream_bytes": 8 * n, "gap": GAP, "snr_db": SNR_DB, "cfo_hz": CFO_HZ, "launches": a.launches,
           "unit": "milliseconds of the detection kernel alone (the library's device events around its launch)",
           "yardstick": "stream_detect_kernel<false> on the same buffers",
           "kernel_ms_median_over_reference": {v: med[v] / med["reference"] for v in med},
           "variants": {v: {"kernel": variants[v][2], "packets_found": found[v], "kernel_ms": kernel_ms[v],
                            "kernel_ms_median": med[v], "kernel_ms_min": min(kernel_ms[v]), "kernel_ms_max": max(kernel_ms[v]),
                            "samples_per_s": n / (med[v] * 1e-3),
                            "fraction_of_8TBps": 8 * n / (med[v] * 1e-3) / HBM_BYTES_PER_S,
                            "call_ms_detect_and_select": call_ms[v],
                            "call_ms_detect_and_select_median": float(np.median(call_ms[v]))} for v in variants},
           "scratch_bytes": scratch, "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"kernel_ms_median": med, "over_reference": rec["kernel_ms_median_over_reference"], "found": found}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
