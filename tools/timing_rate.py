#!/usr/bin/env python3
"""Rate of the stream receiver's fine timing kernel (ofdm_receive_stream_timed, csrc/ofdm_stream_timing.hip) on one GPU,
against the same call without timing on the same buffers.

The recording is tools/stream_rx_rate.py's: one stream of 2^28 samples (2 GiB) resident on the device -- back-to-back
2-symbol frames behind 500-sample idle gaps, 14 dB real-only noise over all of it, a 20 kHz offset.  Both variants are
one whole call with the conjugate detector -- detection, selection, decode of every packet found, payload words
written -- with outputs preallocated:

  none   ofdm_receive_stream_timed, OFDM_TIMING_NONE: ofdm_receive_stream_ex itself, the yardstick (the kernels the
         library had before the timing option, unchanged)
  ltf    ofdm_receive_stream_timed, OFDM_TIMING_LTF: stream_timing_kernel between the selection and the decode

`--launches` launches per variant, interleaved, after a warm-up.  A launch is timed twice: the whole call between
device events of the caller, and every kernel of it between the library's own events (ofdm_timing_query, reset before
and read after every launch): the timing kernel under id 13 beside the decode kernel under id 6.
Writes one JSON record (default profiles/r14/timing/timing_rate.json).

    python tools/timing_rate.py [--samples N] [--launches K] [--out FILE]
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14" / "timing" / "timing_rate.json"))
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

        rows = n // 301 + 1
        pk = torch.empty((rows, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device="cuda")
        words = torch.empty((rows, 3 * nd), dtype=torch.int32, device="cuda")
        tim = torch.empty((rows, C.sizeof(abi.StreamTiming)), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        opts = abi.make_rx_opts("c")
        conj = abi.make_stream_opts("conjugate", 0.75)
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def call(timing, d_timing):
            abi.check(eng.lib, eng.lib.ofdm_receive_stream_timed(
                eng.ctx, ptr(x), n, C.byref(opts), C.byref(conj), timing, abi.PAYLOAD["message"], rows, ptr(pk), ptr(cnt),
                ptr(words), None, None, None, None, d_timing), "receive_stream_timed")

        variants = {"none": lambda: call(abi.TIMING["none"], None), "ltf": lambda: call(abi.TIMING["ltf"], ptr(tim))}
        kernels = {"detect_conj": abi.K_STREAM_DETECT_CONJ, "select": abi.K_STREAM_SELECT, "timing": abi.K_STREAM_TIMING,
                   "decode": abi.K_STREAM_DECODE}
        found, moved = {}, None
        for v, f in variants.items():                               # warm-up: code objects, scratch, the template
            f()
            torch.cuda.synchronize()
            found[v] = [int(c) for c in cnt.cpu()]
        k = found["ltf"][1]
        t = tim[:k].cpu().numpy().view(abi.stream_timing_dtype()).reshape(k)
        moved = {"records": k, "shifted": int((t["shift"] != 0).sum()), "shift_min": int(t["shift"].min()),
                 "shift_max": int(t["shift"].max()), "not_refined": int((t["quality"] == 0).sum()),
                 "quality_median": float(np.median(t["quality"]))}
        call_ms = {v: [] for v in variants}
        kernel_ms = {v: {name: [] for name in kernels} for v in variants}
        eng.timing(True)
        for _ in range(a.launches):
            for v, f in variants.items():                           # interleaved
                eng.timing_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                call_ms[v].append(e0.elapsed_time(e1))
                for name, kid in kernels.items():
                    ms, launches = eng.timing_query(kid)
                    assert launches == (0 if name == "timing" and v == "none" else 1), (v, name, launches)
                    kernel_ms[v][name].append(ms)
        eng.timing(False)
        scratch = eng.scratch_bytes()

    med = lambda t: float(np.median(t))
    report = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {key: r.get(key) for key in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                                     "Occupancy [waves/SIMD]")}
             for r in report if r.get("name", "") in ("ofdm::stream_timing_kernel", "ofdm::stream_decode_kernel<true>")}
    timing_ms, decode_ms = med(kernel_ms["ltf"]["timing"]), med(kernel_ms["ltf"]["decode"])
    rec = {"samples": n, "stream_bytes": 8 * n, "gap": GAP, "snr_db": SNR_DB, "cfo_hz": CFO_HZ, "launches": a.launches,
           "detector": "conjugate", "max_packets": rows, "packets_found_and_written": found, "timing_rows": moved,
           "unit": "milliseconds; kernels between the library's device events around their launches (ids 12, 5, 13, 6), the "
                   "call between the caller's",
           "yardstick": "the same call with OFDM_TIMING_NONE on the same buffers (ofdm_receive_stream_ex's launches)",
           "timing_kernel_ms_median_id13": timing_ms, "decode_kernel_ms_median_id6": decode_ms,
           "timing_over_decode": timing_ms / decode_ms,
           "packets_per_s_timing_kernel": found["ltf"][1] / (timing_ms * 1e-3),
           "call_ms_median": {v: med(call_ms[v]) for v in variants},
           "call_ltf_over_none": med(call_ms["ltf"]) / med(call_ms["none"]),
           "kernel_ms_median": {v: {name: med(t) for name, t in kernel_ms[v].items()} for v in variants},
           "call_ms": call_ms, "kernel_ms": kernel_ms, "scratch_bytes": scratch, "resource_usage": usage}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({key: rec[key] for key in ("timing_kernel_ms_median_id13", "decode_kernel_ms_median_id6", "timing_over_decode",
                                                "call_ms_median", "call_ltf_over_none", "packets_found_and_written", "timing_rows")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
