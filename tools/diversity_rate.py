#!/usr/bin/env python3
"""Rate of the stream receiver's diversity path (ofdm_receive_stream_diversity, csrc/ofdm_stream_div.hip) on one GPU for
B = 1, 2 and 4 branches, against B x the single-branch call (ofdm_receive_stream_tracked) on the same buffers -- of this
library and, with --parent-lib, of the parent commit's library.

The recordings are tools/stream_rx_rate.py's stream, once per branch: back-to-back frames behind 500-sample idle gaps, a
20 kHz offset, each branch with a complex gain of its own and 14 dB complex noise of its own, resident on the device.
--n-data D sets the message to D data symbols of blanks.  Every variant is one whole call with the conjugate detector,
OFDM_TIMING_LTF and OFDM_TRACK_PILOTS with d_bits -- detection, selection, fine timing, decode of every packet found --
with outputs preallocated:

  single        ofdm_receive_stream_tracked on branch 0
  parent        the same call into the library at --parent-lib, a context of its own on the same stream
  b1, b2, b4    ofdm_receive_stream_diversity on the first 1, 2 and 4 branches (b1 dispatches to the single-branch call)

`--launches` launches per variant, interleaved, after a warm-up.  A launch is timed as a whole between device events of
the caller, and per kernel between the library's own events (ofdm_timing_query, reset before and read after every
launch): detection (id 12 or 15), selection (5), fine timing (13 or 16), decode (14 or 17).
Writes one JSON record under profiles/r19/diversity/.

    python tools/diversity_rate.py [--samples N] [--launches K] [--n-data D] [--parent-lib FILE] [--out FILE]
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

SNR_DB, CFO_HZ, GAP = 14.0, 20e3, 500
UNITS_PER_CHUNK = 2048
GAINS = (1.0, 0.6 + 0.5j, -0.3 + 0.9j, 0.8j)       # one complex gain per branch


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--n-data", type=int, default=2, help="data symbols per packet (blanks)")
    ap.add_argument("--parent-lib", default=None, help="libofdm_mi355x.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    log2 = int(np.log2(a.samples))
    out = Path(a.out) if a.out else ROOT / "profiles" / "r19" / "diversity" / f"diversity_rate_2p{log2}_d{a.n_data}.json"
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.channel import make_stream  # noqa: PLC0415
    from ofdm_amd.stream import synthetic_segments  # noqa: PLC0415
    from tools.track_rate import ParentLib  # noqa: PLC0415

    n, nb_max = a.samples, len(GAINS)
    message = b" " * (12 * a.n_data)
    with pkg.Engine(0) as eng:
        eng.set_long_message(message)
        nd = eng.payload_frames("message")
        w = eng.transmitter("c", "message")
        period = len(w) // 10
        seg = synthetic_segments(period, UNITS_PER_CHUNK, GAP)[:-1]     # whole gap + frame units
        chunk = UNITS_PER_CHUNK * (GAP + period)
        xs = []
        for b, g in enumerate(GAINS):
            wave = torch.from_numpy((w * np.complex64(g)).astype(np.complex64)).cuda()
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0x57EA + b)
            x = torch.empty(n, dtype=torch.complex64, device="cuda")
            for lo in range(0, n, chunk):
                m = min(chunk, n - lo)
                x[lo:lo + m] = make_stream(wave, seg, SNR_DB, CFO_HZ, noise="complex", generator=gen)[:m]
            xs.append(x)
        torch.cuda.synchronize()
        parent = ParentLib(a.parent_lib, abi, torch.cuda.current_stream().cuda_stream, message) if a.parent_lib else None

        rows = n // 301 + 1
        pk = torch.empty((rows, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device="cuda")
        words = torch.empty((rows, 3 * nd), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        opts = abi.make_rx_opts("c")
        conj = abi.make_stream_opts("conjugate", 0.75)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        ltf, pilots = abi.TIMING["ltf"], abi.TRACKING["pilots"]
        tail = (abi.PAYLOAD["message"], rows, ptr(pk), ptr(cnt), ptr(words), None, None, None, None, None, None)

        def single(who=eng):
            abi.check(who.lib, who.lib.ofdm_receive_stream_tracked(who.ctx, ptr(xs[0]), n, C.byref(opts), C.byref(conj), ltf,
                                                                   pilots, *tail), "receive_stream_tracked")

        def diversity(nb):
            table = (C.c_void_p * nb)(*[x.data_ptr() for x in xs[:nb]])
            abi.check(eng.lib, eng.lib.ofdm_receive_stream_diversity(eng.ctx, table, nb, n, C.byref(opts), C.byref(conj), ltf,
                                                                     pilots, *tail, None), "receive_stream_diversity")

        one = dict(detect=abi.K_STREAM_DETECT_CONJ, select=abi.K_STREAM_SELECT, timing=abi.K_STREAM_TIMING,
                   decode=abi.K_STREAM_DECODE_TRACK)
        div = dict(detect=abi.K_STREAM_DETECT_DIV, select=abi.K_STREAM_SELECT, timing=abi.K_STREAM_TIMING_DIV,
                   decode=abi.K_STREAM_DECODE_DIV)
        # name -> (launch, who answers ofdm_timing_query, the kernels' ids)
        variants = {"single": (single, eng, one), "b1": (lambda: diversity(1), eng, one), "b2": (lambda: diversity(2), eng, div),
                    "b4": (lambda: diversity(nb_max), eng, div)}
        if parent:
            variants["parent"] = (lambda: single(parent), parent, one)
        found, errs = {}, {}
        for v, (f, _, _) in variants.items():                       # warm-up: code objects, scratch, the template
            f()
            torch.cuda.synchronize()
            found[v] = [int(c) for c in cnt.cpu()]
            rec = pk[:found[v][1]].cpu().numpy().view(abi.stream_packet_dtype())
            errs[v] = int(rec["bit_err"].astype(np.int64).sum())
        call_ms = {v: [] for v in variants}
        kernel_ms = {v: {k: [] for k in one} for v in variants}
        eng.timing(True)
        if parent:
            parent.timing(True)
        for _ in range(a.launches):
            for v, (f, who, ids) in variants.items():               # interleaved
                who.timing_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                call_ms[v].append(e0.elapsed_time(e1))
                for k, kid in ids.items():
                    kernel_ms[v][k].append(who.timing_query(kid)[0])
        eng.timing(False)
        if parent:
            parent.timing(False)
            parent.close()

    med = lambda t: float(np.median(t))
    report = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {key: r.get(key) for key in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                                     "Occupancy [waves/SIMD]")}
             for r in report if r.get("source") == "ofdm_stream_div.hip"}
    cm = {v: med(t) for v, t in call_ms.items()}
    km = {v: {k: med(t) for k, t in d.items()} for v, d in kernel_ms.items()}
    base = "parent" if parent else "single"
    ratios = {"baseline": f"B x {base}" + (" (the parent commit's library)" if parent else " (this library's single-branch call)")}
    for v, nb in (("b1", 1), ("b2", 2), ("b4", nb_max)):
        ratios[f"call_{v}_over_B_x_{base}"] = cm[v] / (nb * cm[base])
        for k in one:
            ratios[f"{k}_{v}_over_B_x_{base}"] = km[v][k] / (nb * km[base][k])
    rec = {"samples": n, "stream_bytes_per_branch": 8 * n, "data_symbols": nd, "gap": GAP, "snr_db": SNR_DB, "cfo_hz": CFO_HZ,
           "branch_gains": [str(g) for g in GAINS], "launches": a.launches, "detector": "conjugate", "timing": "ltf",
           "tracking": "pilots", "max_packets": rows, "packets_found_and_written": found, "bit_errors_of_the_records": errs,
           "unit": "milliseconds; a kernel between the library's device events around its launches, the call between the caller's",
           "kernel_ms_median": km, "call_ms_median": cm, "ratios": ratios,
           "detect_GBps_read": {v: nb * 8 * n / (km[v]["detect"] * 1e-3) / 1e9 for v, nb in (("single", 1), ("b1", 1), ("b2", 2), ("b4", nb_max))},
           "kernel_ms": kernel_ms, "call_ms": call_ms, "resource_usage": usage}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({key: rec[key] for key in ("samples", "data_symbols", "kernel_ms_median", "call_ms_median", "ratios",
                                                "packets_found_and_written", "bit_errors_of_the_records")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
