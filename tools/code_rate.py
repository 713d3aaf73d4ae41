#!/usr/bin/env python3
"""Times of the coded link's three kernels (include/ofdm_mi355x_code.h, csrc/ofdm_code.hip) on one GPU: the encoder, the
gains kernel and the Viterbi decoder, for 2^16 packets of D = 2 and D = 15 data symbols on B = 1 and 2 branches.

Per case: random information words are encoded and transmitted behind 500-sample idle gaps, every branch gets 20 dB of
complex noise of its own, and `--launches` rounds of receive (conjugate detector, OFDM_TIMING_LTF, with d_eq; pilot
tracking for D = 15) -> ofdm_stream_csi -> ofdm_code_decode run after a warm-up round.  Times are the library's own
events (ofdm_timing_query), reset before and read after the rounds: per launch for ids 18 (encode), 19 (gains), 20
(decode) and for the stream decode kernel of the same receive call (6, 14 or 17); the gains and the Viterbi decoder
are also given as ratios to that kernel.  Writes one JSON record under profiles/r20/code/.

--rate 2/3 or 3/4 times the punctured rates' encoder and decoder instead (include/ofdm_mi355x_punct.h,
csrc/ofdm_punct.hip), which are timed under the same ids 18 and 20; the record, under profiles/r21/punct/, then also
holds the decoder's time per trellis step, to set against the rate-1/2 record of the same session.

--ppdu times the two calls of the self-describing packets instead (include/ofdm_mi355x_ppdu.h, csrc/ofdm_ppdu.hip), also
under ids 18 and 20: for D = 2 and D = 15 symbols and each of the three rates, and for packets of mixed rates, 2^16
packets of the largest LENGTH are encoded (ofdm_ppdu_encode, both launches under one id; ofdm_punct_encode of the same
number of payload words beside it), mapped to noise-free subcarriers with 10 dB of complex noise on the device, and decoded
by the fused kernel and, the same rows at the same rate and D, by ofdm_punct_decode; both as time per row and trellis step
(48 + S (D - 1) against S D).  The record goes under profiles/r22/ppdu/.

    python tools/code_rate.py [--packets N] [--launches K] [--rate {1/2,2/3,3/4}] [--ppdu] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SNR_DB, GAP = 20.0, 500
CASES = ((2, 1), (2, 2), (15, 1), (15, 2))      # (D, B)


def ppdu_main(a) -> int:
    """--ppdu: the encoder's and the fused decoder's times beside the punctured calls' on the same rows"""
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415

    n = a.packets
    out = Path(a.out) if a.out else ROOT / "profiles" / "r22" / "ppdu" / f"ppdu_rate_{n}.json"
    record = dict(tool="tools/code_rate.py --ppdu", device=torch.cuda.get_device_name(0), packets=n, launches=a.launches,
                  snr_db=10.0, cases=[])
    rng = np.random.default_rng(0xC0DE)
    rates = tuple(abi.RATE)
    with pkg.Engine(0) as eng:
        eng.timing(True)

        def timed(kernel, call):
            call()                                                    # warm-up
            eng.timing_reset()
            for _ in range(a.launches):
                res = call()
            eng.synchronize()
            ms, cnt = eng.timing_query(kernel)
            assert cnt == a.launches, (kernel, cnt)
            return ms / cnt, res
        for d in (2, 15):
            psdu = torch.from_numpy(rng.integers(0, 1 << 32, (n, abi.PPDU_PSDU_WORDS), dtype=np.uint64).astype(np.uint32)
                                    .view(np.int32)).cuda()
            seeds = torch.from_numpy((1 + np.arange(n) % 127).astype(np.int32)).cuda()
            for name in rates + ("mixed",):
                codes = np.arange(n) % 3 if name == "mixed" else np.full(n, abi.rate_code(name))
                lens = np.array([abi.ppdu_cap(d, r) for r in rates])[codes]
                tl, tr = (torch.from_numpy(v.astype(np.int32)).cuda() for v in (lens, codes))
                enc_ms, enc = timed(abi.K_CODE_ENCODE, lambda: eng.encode_ppdu(psdu, tl, tr, seeds, d))
                # payload bits -> the reference's QPSK map (re > 0 iff b0 == b1, im > 0 iff b0 == 0) -> 10 dB of noise
                w = enc["d_words"]
                bits = (w[:, :, None] >> torch.arange(31, -1, -1, device=w.device, dtype=torch.int32)) & 1
                b = bits.reshape(n, 48 * d, 2)
                re = torch.where(b[:, :, 0] == b[:, :, 1], 1.0, -1.0)
                im = torch.where(b[:, :, 0] == 0, 1.0, -1.0)
                g = torch.Generator(device="cuda").manual_seed(d)
                eq = torch.complex(re, im).to(torch.complex64) / 2 ** 0.5
                sigma = (10 ** -1.0 / 2) ** 0.5
                eq = (eq + sigma * torch.view_as_complex(torch.randn((n, 48 * d, 2), generator=g, device="cuda"))).contiguous()
                del bits, b, re, im
                dec_ms, dec = timed(abi.K_CODE_DECODE, lambda: eng.decode_ppdu(eq))
                status = dec["d_meta"][:, 0]
                case = dict(n_data=d, rate=name, encode_ms=enc_ms, decode_ms=dec_ms,
                            header_valid=int((status & abi.PPDU_BAD_HEADER == 0).sum()), fcs_passed=int((status == 0).sum()))
                if name != "mixed":
                    s_ = abi.PUNCT_STEPS[abi.rate_code(name)]
                    info = torch.zeros((n, abi.punct_info_words(d, name)), dtype=torch.int32, device="cuda")
                    case["punct_encode_ms"], _ = timed(abi.K_CODE_ENCODE, lambda: eng.encode_packets(info, d, rate=name))
                    case["punct_decode_ms"], _ = timed(abi.K_CODE_DECODE, lambda: eng.decode_coded(eq, rate=name))
                    # a D = 2 packet at rate 1/2 holds no LENGTH: every header is refused and the data part is not decoded
                    steps = 48 + s_ * (d - 1) if case["header_valid"] else 48
                    case.update(trellis_steps=steps, punct_trellis_steps=s_ * d,
                                decode_ns_per_row_step=1e6 * dec_ms / (n * steps),
                                punct_decode_ns_per_row_step=1e6 * case["punct_decode_ms"] / (n * s_ * d))
                    case["per_step_ratio"] = case["decode_ns_per_row_step"] / case["punct_decode_ns_per_row_step"]
                record["cases"].append(case)
                print(json.dumps(case), file=sys.stderr)
                del eq, dec, enc
                torch.cuda.empty_cache()
            single = [c["decode_ms"] for c in record["cases"] if c["n_data"] == d and c["rate"] != "mixed"]
            mixed = next(c for c in record["cases"] if c["n_data"] == d and c["rate"] == "mixed")
            mixed["mean_of_single_rate_decode_ms"] = float(np.mean(single))
            mixed["mixed_over_mean"] = mixed["decode_ms"] / mixed["mean_of_single_rate_decode_ms"]
        eng.timing(False)
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    record["resources"] = {r["name"]: {k: r[k] for k in ("VGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
                           for r in report if r.get("source") in ("ofdm_punct.hip", "ofdm_ppdu.hip")}
    record["ppdu_flags"] = build_lib.SOURCE_FLAGS["ofdm_ppdu.hip"]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1))
    print(f"-> {out}", file=sys.stderr)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rate", choices=("1/2", "2/3", "3/4"), default="1/2")
    ap.add_argument("--branches", type=int, nargs="+", default=[1, 2], choices=(1, 2), help="the cases' B to run (default both)")
    ap.add_argument("--ppdu", action="store_true", help="time ofdm_ppdu_encode and ofdm_ppdu_decode instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.ppdu:
        return ppdu_main(a)
    if a.out:
        out = Path(a.out)
    elif a.rate == "1/2":
        out = ROOT / "profiles" / "r20" / "code" / f"code_rate_{a.packets}.json"
    else:
        out = ROOT / "profiles" / "r21" / "punct" / f"code_rate_{a.rate.replace('/', 'of')}_{a.packets}.json"
    import torch  # noqa: PLC0415
    import ofdm_pkg  # noqa: PLC0415
    pkg = ofdm_pkg.load()
    from ofdm_amd import abi, build_lib  # noqa: PLC0415

    n = a.packets
    record = dict(tool="tools/code_rate.py", device=torch.cuda.get_device_name(0), packets=n, launches=a.launches,
                  rate=a.rate, snr_db=SNR_DB, gap=GAP, cases=[])
    rng = np.random.default_rng(0xC0DE)
    with pkg.Engine(0) as eng:
        for d, nb in (c for c in CASES if c[1] in a.branches):
            eng.set_long_message(" " * (12 * d))
            info = rng.integers(0, 1 << 32, (n, abi.punct_info_words(d, a.rate)), dtype=np.uint64).astype(np.uint32)
            tinfo = torch.from_numpy(info.view(np.int32)).cuda()
            stride = abi.packet_len(d) + GAP
            eng.timing(True)
            eng.timing_reset()
            for _ in range(a.launches + 1):
                words = eng.encode_packets(tinfo, d, rate=a.rate)
            enc_ms, enc_n = eng.timing_query(abi.K_CODE_ENCODE)
            clean = eng.transmit_packets(words, d, pos0=GAP, stride=stride, n_out=n * stride + GAP)
            power = float((clean.real.double() ** 2 + clean.imag.double() ** 2).sum()) / (n * abi.packet_len(d))
            rec = [eng.impair_stream(clean, power, SNR_DB, noise="complex", trial=b) for b in range(nb)]
            del clean
            tracking = "pilots" if d == 15 else "none"
            dec_id = abi.K_STREAM_DECODE_DIV if nb > 1 else abi.K_STREAM_DECODE_TRACK if d == 15 else abi.K_STREAM_DECODE

            def round_():
                if nb == 1:
                    rx = eng.receive_stream_device(rec[0], detector="conjugate", timing="ltf", tracking=tracking, want_eq=True)
                else:
                    rx = eng.receive_diversity_device(rec, detector="conjugate", timing="ltf", tracking=tracking, want_eq=True)
                csi = eng.stream_csi(rec if nb > 1 else rec[0], rx)
                return rx, eng.decode_coded(rx, csi=csi, rate=a.rate)
            round_()                                                  # warm-up
            eng.timing_reset()
            for _ in range(a.launches):
                rx, dec = round_()
            eng.synchronize()
            per = {}
            for name, k in (("stream_decode", dec_id), ("stream_csi", abi.K_STREAM_CSI), ("code_decode", abi.K_CODE_DECODE)):
                ms, cnt = eng.timing_query(k)
                assert cnt == a.launches, (name, cnt)
                per[name] = ms / cnt
            eng.timing(False)
            count = int(rx["d_count"].cpu()[1])
            steps = abi.PUNCT_STEPS[abi.rate_code(a.rate)] * d
            case = dict(n_data=d, branches=nb, samples=n * stride + GAP, received=count, trellis_steps=steps,
                        code_decode_ns_per_row_step=1e6 * per["code_decode"] / (max(count, 1) * steps),
                        encode_ms=enc_ms / enc_n, stream_decode_kernel=dec_id, stream_decode_ms=per["stream_decode"],
                        stream_csi_ms=per["stream_csi"], code_decode_ms=per["code_decode"],
                        csi_over_stream_decode=per["stream_csi"] / per["stream_decode"],
                        code_decode_over_stream_decode=per["code_decode"] / per["stream_decode"])
            record["cases"].append(case)
            print(json.dumps(case), file=sys.stderr)
            del rec, rx, dec
            torch.cuda.empty_cache()
    report = json.loads(build_lib.RESOURCE_REPORT.read_text())
    record["resources"] = {r["name"]: {k: r[k] for k in ("VGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
                           for r in report if r.get("source") in ("ofdm_code.hip", "ofdm_punct.hip")}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1))
    print(f"-> {out}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
