#!/usr/bin/env python3
"""Rate of the stream receiver (ofdm_receive_stream) on one GPU, against the only route there was before it.

bench.py has no workload for it, so this tool measures the shape a user with a recording runs: one stream of 2^28
samples (2 GiB) resident on the device -- back-to-back 2-symbol frames behind 500-sample idle gaps, 14 dB real-only
noise over all of it, a 20 kHz offset (channel.make_stream, laid out in chunks of whole gap + frame units) -- decoded by
ofdm_receive_stream through the C ABI with preallocated outputs, so a timed launch holds no allocation and no host
synchronisation.  Two variants (records only; records, bits and equalised subcarriers), each timed over `--launches`
launches between device events after a warm-up, interleaved with the baseline:

  the parent route: ofdm_receive_captures over 3,008-sample windows hopped by one 980-sample frame.  The entry point
  takes no overlapping rows (pitch >= cap_len), so the windows are four strided views of the stream, hop 3,920 at
  offsets 0, 980, 1,960 and 2,940, no copy; one timed "launch" is the four calls.  Its packets (packet_idx - 11 +
  window start of every capture that synchronised, deduplicated on the host afterwards) are compared with the stream
  receiver's.

Beside the rates: the three kernels' milliseconds from ofdm_timing_query (a separate pass with timing on) and the
fraction of the 8 TB/s HBM peak that the 8 bytes per sample the detection must read represent.
Writes one JSON record (default profiles/r09/stream/stream_rx_rate.json).

    python tools/stream_rx_rate.py [--samples N] [--launches K] [--out FILE]
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09" / "stream" / "stream_rx_rate.json"))
    a = ap.parse_args(argv)
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.channel import make_stream  # noqa: PLC0415
    from ofdm_amd.stream import synthetic_segments  # noqa: PLC0415

    n = a.samples
    with pkg.Engine(0) as eng:
        nd = eng.payload_frames("message")
        L = abi.capture_len(nd)
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
        sent = (n + GAP + period - 1) // (GAP + period)

        # ---- the stream receiver through the C ABI: outputs allocated once ----
        maxp = n // 301 + 1
        pk = torch.empty((maxp, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        words = torch.empty((maxp, 3 * nd), dtype=torch.int32, device="cuda")
        eq = torch.empty((maxp, 48 * nd), dtype=torch.complex64, device="cuda")
        opts = abi.make_rx_opts("c")
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def stream_launch(full: bool):
            abi.check(eng.lib, eng.lib.ofdm_receive_stream(
                eng.ctx, ptr(x), n, C.byref(opts), abi.PAYLOAD["message"], maxp, ptr(pk), ptr(cnt),
                ptr(words) if full else None, ptr(eq) if full else None, None, None, None), "receive_stream")

        # ---- the parent route: four strided views, windows hopped by one frame ----
        hop = 4 * period
        views = []
        for off in range(0, hop, period):
            nw = (n - off - L) // hop + 1 if n - off >= L else 0
            if nw > 0:
                views.append((off, x[off:].as_strided((nw, L), (hop, 1))))

        def windows_launch():
            return [eng.receive_captures(v, want_bits=False) for _, v in views]

        variants = {"stream_records": lambda: stream_launch(False), "stream_records_bits_eq": lambda: stream_launch(True),
                    "windows_hop_980": windows_launch}
        for f in variants.values():                                 # warm-up: code objects, scratch, allocator
            f()
        torch.cuda.synchronize()
        found, written = (int(v) for v in cnt.cpu())
        pos = pk[:written].cpu().numpy().view(abi.stream_packet_dtype())["packet_pos"].copy()
        base_pos = []
        for (off, v), out in zip(views, windows_launch()):
            r = out["records"]
            ok = (r["flags"] & abi.CAPTURE_SYNC_FAIL) == 0
            start = off + hop * torch.arange(v.shape[0], device="cuda", dtype=torch.int64)
            base_pos.append((r["packet_idx"].to(torch.int64) + start)[ok].cpu().numpy())
        base_pos = np.unique(np.concatenate(base_pos)) if base_pos else np.zeros(0, np.int64)
        recovered = int(np.isin(pos, base_pos).sum())
        window_samples = int(sum(v.shape[0] for _, v in views)) * L

        ms = {v: [] for v in variants}
        for _ in range(a.launches):
            for v, f in variants.items():                           # interleaved
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[v].append(e0.elapsed_time(e1))
        # ---- per-kernel milliseconds (a pass of its own: the events of the timing hooks stay out of the rates) ----
        eng.timing(True)
        eng.timing_reset()
        reps = 5
        for _ in range(reps):
            stream_launch(False)
        eng.synchronize()
        kernels = {name: eng.timing_query(k)[0] / reps for name, k in
                   (("stream_detect_kernel", abi.K_STREAM_DETECT), ("stream_select_kernel (three launches)", abi.K_STREAM_SELECT),
                    ("stream_decode_kernel<false>", abi.K_STREAM_DECODE))}
        eng.timing(False)
        scratch = eng.scratch_bytes()

    med = {v: float(np.median(t)) for v, t in ms.items()}
    rate = {v: n / (med[v] * 1e-3) for v in ms}
    rows = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {k: r.get(k) for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                               "Occupancy [waves/SIMD]")} for r in rows if r.get("source") == "ofdm_stream.hip"}
    rec = {"samples": n, "stream_bytes": 8 * n, "data_symbols": nd, "gap": GAP, "snr_db": SNR_DB, "cfo_hz": CFO_HZ,
           "launches": a.launches, "unit": "samples/s of the stream (device events around one launch)",
           "packets": {"transmitted_whole_or_cut": sent, "found": found, "decoded": written},
           "variants": {v: {"ms": ms[v], "ms_median": med[v], "samples_per_s": rate[v],
                            "samples_per_s_min": n / (max(ms[v]) * 1e-3), "samples_per_s_max": n / (min(ms[v]) * 1e-3)}
                        for v in ms},
           "packets_per_s": {v: found / (med[v] * 1e-3) for v in ("stream_records", "stream_records_bits_eq")},
           "kernel_ms": kernels,
           "hbm": {"bytes_per_sample": 8, "fraction_of_8TBps_whole_call": 8 * rate["stream_records"] / HBM_BYTES_PER_S,
                   "fraction_of_8TBps_detect_kernel": 8 * n / (kernels["stream_detect_kernel"] * 1e-3) / HBM_BYTES_PER_S},
           "baseline": {"route": "ofdm_receive_captures, 3008-sample windows hopped by 980 (four strided views, hop 3920)",
                        "windows": int(sum(v.shape[0] for _, v in views)), "samples_staged": window_samples,
                        "samples_staged_per_stream_sample": window_samples / n, "packets": int(len(base_pos)),
                        "stream_packets_recovered": recovered, "stream_packets": int(len(pos)),
                        "host_dedup_timed": False},
           "stream_over_baseline": rate["stream_records"] / rate["windows_hop_980"],
           "scratch_bytes": scratch, "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({"samples_per_s": rate["stream_records"], "with_bits_eq": rate["stream_records_bits_eq"],
                      "baseline_samples_per_s": rate["windows_hop_980"], "stream_over_baseline": rec["stream_over_baseline"],
                      "found": found, "baseline_recovers": recovered, "kernel_ms": kernels,
                      "hbm_fraction_detect": rec["hbm"]["fraction_of_8TBps_detect_kernel"]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
