#!/usr/bin/env python3
"""Rate of the stream receiver's pilot-tracking decode (ofdm_receive_stream_tracked, csrc/ofdm_stream_track.hip) on one
GPU, against the untracked decode of this library and -- with --parent-lib -- of the parent commit's library, on the
same buffers.

The recording is tools/stream_rx_rate.py's: one stream of 2^28 samples (2 GiB) resident on the device -- back-to-back
frames behind 500-sample idle gaps, 14 dB real-only noise over all of it, a 20 kHz offset.  --n-data D sets the message
to D data symbols of blanks (default: the context's own 2-symbol message).  Every variant is one whole call with the
conjugate detector and OFDM_TIMING_LTF -- detection, selection, fine timing, decode of every packet found -- with
outputs preallocated:

  none_bits     OFDM_TRACK_NONE with d_bits: stream_decode_kernel<true>, which parks and re-reads the spectra as the
                tracked decode does -- the fair baseline
  none_plain    OFDM_TRACK_NONE without any optional output: stream_decode_kernel<false>
  pilots_bits   OFDM_TRACK_PILOTS with d_bits
  pilots_plain  OFDM_TRACK_PILOTS without any optional output (no d_phase either)
  parent_bits, parent_plain, parent_pilots_bits, parent_pilots_plain   the same four calls into the library at
                --parent-lib (built from the parent commit), loaded beside this one in the same process, a context of
                its own on the same stream

`--launches` launches per variant, interleaved, after a warm-up.  A launch is timed twice: the whole call between
device events of the caller, and the decode kernel between the library's own events (ofdm_timing_query, reset before
and read after every launch): id 6 for the untracked decode, id 14 for the tracked one.
Writes one JSON record (default profiles/r15/track/track_rate.json, track_rate_d15.json with --n-data 15).

    python tools/track_rate.py [--samples N] [--launches K] [--n-data D] [--parent-lib FILE] [--out FILE]
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


class ParentLib:
    """The parent commit's library through ctypes alone: the entry points this tool needs, and a context of its own"""

    def __init__(self, path, abi, stream_handle, message):
        self.lib = C.CDLL(str(path))
        for name, (res, args) in {**abi._SIGS, **abi._LONG_SIGS, **abi._TRACK_SIGS}.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.abi = abi
        self.ctx = C.c_void_p()
        abi.check(self.lib, self.lib.ofdm_ctx_create(0, C.byref(self.ctx)), "parent ctx_create")
        abi.check(self.lib, self.lib.ofdm_ctx_set_stream(self.ctx, C.c_void_p(stream_handle or None)), "parent ctx_set_stream")
        if message is not None:
            frames = C.c_int32()
            abi.check(self.lib, self.lib.ofdm_set_long_message(self.ctx, message, len(message), C.byref(frames)), "parent set_long_message")

    def timing(self, on):
        self.abi.check(self.lib, self.lib.ofdm_timing_enable(self.ctx, int(on)), "parent timing_enable")

    def timing_reset(self):
        self.abi.check(self.lib, self.lib.ofdm_timing_reset(self.ctx), "parent timing_reset")

    def timing_query(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        self.abi.check(self.lib, self.lib.ofdm_timing_query(self.ctx, kernel, C.byref(ms), C.byref(n)), "parent timing_query")
        return ms.value, n.value

    def close(self):
        self.lib.ofdm_ctx_destroy(self.ctx)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=1 << 28)
    ap.add_argument("--launches", type=int, default=20, help="timed launches per variant (at least 20 for a record)")
    ap.add_argument("--n-data", type=int, default=None, help="data symbols per packet (blanks); default the context's 2-symbol message")
    ap.add_argument("--parent-lib", default=None, help="libofdm_mi355x.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    out = Path(a.out) if a.out else ROOT / "profiles" / "r15" / "track" / (f"track_rate_d{a.n_data}.json" if a.n_data else "track_rate.json")
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415
    from ofdm_amd.channel import make_stream  # noqa: PLC0415
    from ofdm_amd.stream import synthetic_segments  # noqa: PLC0415

    n = a.samples
    message = None if a.n_data is None else b" " * (12 * a.n_data)
    with pkg.Engine(0) as eng:
        if message is not None:
            eng.set_long_message(message)
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
        parent = ParentLib(a.parent_lib, abi, torch.cuda.current_stream().cuda_stream, message) if a.parent_lib else None

        rows = n // 301 + 1
        pk = torch.empty((rows, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device="cuda")
        words = torch.empty((rows, 3 * nd), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        opts = abi.make_rx_opts("c")
        conj = abi.make_stream_opts("conjugate", 0.75)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        ltf = abi.TIMING["ltf"]

        def call(tracking, bits, who=eng):
            abi.check(who.lib, who.lib.ofdm_receive_stream_tracked(
                who.ctx, ptr(x), n, C.byref(opts), C.byref(conj), ltf, tracking, abi.PAYLOAD["message"], rows, ptr(pk), ptr(cnt),
                ptr(words) if bits else None, None, None, None, None, None, None), "receive_stream_tracked")

        none, pilots = abi.TRACKING["none"], abi.TRACKING["pilots"]
        # name -> (launch, who answers ofdm_timing_query, the decode kernel's id)
        variants = {"none_bits": (lambda: call(none, True), eng, abi.K_STREAM_DECODE),
                    "none_plain": (lambda: call(none, False), eng, abi.K_STREAM_DECODE),
                    "pilots_bits": (lambda: call(pilots, True), eng, abi.K_STREAM_DECODE_TRACK),
                    "pilots_plain": (lambda: call(pilots, False), eng, abi.K_STREAM_DECODE_TRACK)}
        if parent:
            variants["parent_bits"] = (lambda: call(none, True, parent), parent, abi.K_STREAM_DECODE)
            variants["parent_plain"] = (lambda: call(none, False, parent), parent, abi.K_STREAM_DECODE)
            variants["parent_pilots_bits"] = (lambda: call(pilots, True, parent), parent, abi.K_STREAM_DECODE_TRACK)
            variants["parent_pilots_plain"] = (lambda: call(pilots, False, parent), parent, abi.K_STREAM_DECODE_TRACK)
        found, errs = {}, {}
        for v, (f, _, _) in variants.items():                       # warm-up: code objects, scratch, the template
            f()
            torch.cuda.synchronize()
            found[v] = [int(c) for c in cnt.cpu()]
            rec = pk[:found[v][1]].cpu().numpy().view(abi.stream_packet_dtype())
            errs[v] = int(rec["bit_err"].astype(np.int64).sum())
        call_ms = {v: [] for v in variants}
        decode_ms = {v: [] for v in variants}
        eng.timing(True)
        if parent:
            parent.timing(True)
        for _ in range(a.launches):
            for v, (f, who, kid) in variants.items():               # interleaved
                who.timing_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                call_ms[v].append(e0.elapsed_time(e1))
                ms, launches = who.timing_query(kid)
                assert launches == 1, (v, launches)
                decode_ms[v].append(ms)
        eng.timing(False)
        if parent:
            parent.timing(False)
            parent.close()

    med = lambda t: float(np.median(t))
    report = json.loads(build_lib.RESOURCE_REPORT.read_text()) if build_lib.RESOURCE_REPORT.exists() else []
    usage = {r["name"]: {key: r.get(key) for key in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
                                                     "Occupancy [waves/SIMD]")}
             for r in report if r.get("name", "").startswith("ofdm::stream_decode")}
    dm, cm = {v: med(t) for v, t in decode_ms.items()}, {v: med(t) for v, t in call_ms.items()}
    base = "parent" if parent else "none"
    ratios = {"baseline": f"{base}_bits / {base}_plain" + (" (the parent commit's library)" if parent else " (this library, OFDM_TRACK_NONE)"),
              "decode_pilots_bits_over_baseline_bits": dm["pilots_bits"] / dm[f"{base}_bits"],
              "decode_pilots_plain_over_baseline_plain": dm["pilots_plain"] / dm[f"{base}_plain"],
              "decode_pilots_plain_over_baseline_bits": dm["pilots_plain"] / dm[f"{base}_bits"],
              "call_pilots_bits_over_baseline_bits": cm["pilots_bits"] / cm[f"{base}_bits"],
              "call_pilots_plain_over_baseline_plain": cm["pilots_plain"] / cm[f"{base}_plain"]}
    if parent:                                                      # every decode variant of this library over the parent's own
        for v, pv in (("none_bits", "parent_bits"), ("none_plain", "parent_plain"), ("pilots_bits", "parent_pilots_bits"),
                      ("pilots_plain", "parent_pilots_plain")):
            ratios[f"decode_{v}_over_{pv}"] = dm[v] / dm[pv]
    rec = {"samples": n, "stream_bytes": 8 * n, "data_symbols": nd, "gap": GAP, "snr_db": SNR_DB, "cfo_hz": CFO_HZ,
           "launches": a.launches, "detector": "conjugate", "timing": "ltf", "max_packets": rows,
           "packets_found_and_written": found, "bit_errors_of_the_records": errs,
           "unit": "milliseconds; the decode kernel between the library's device events around its launch (id 6 untracked, 14 "
                   "tracked), the call between the caller's",
           "decode_kernel_ms_median": dm, "call_ms_median": cm, "ratios": ratios,
           "packets_per_s_decode_kernel": {v: found[v][1] / (dm[v] * 1e-3) for v in variants},
           "decode_kernel_ms": decode_ms, "call_ms": call_ms, "resource_usage": usage}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({key: rec[key] for key in ("data_symbols", "decode_kernel_ms_median", "call_ms_median", "ratios",
                                                "packets_found_and_written", "bit_errors_of_the_records")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
