"""Host-side engine: one ofdm_ctx per GPU, device buffers from PyTorch (plumbing only).

Mirrors the reference's three hot-path functions (src/OFDM.c):
    Transmitter()            OFDM.c:467-618   -> Engine.transmitter() / Engine.tx_frames()
    Transmission_Over_Air()  OFDM.c:635-655   -> Engine.transmission_over_air() / Engine.impair_stream() (a device
                                                 recording: multipath, carrier offset, reproducible noise)
    Receiver()               OFDM.c:941-1165  -> Engine.receiver() / Engine.rx_frames() / Engine.receive_captures() /
                                                 Engine.receive_stream() (every packet of one recording)
and main()'s SNR loop (OFDM.c:1187-1222) -> Engine.symbol_sweep() / Engine.frame_sweep().
All arithmetic happens in the HIP kernels of libofdm_mi355x.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from .abi import Cfg, RxOpts, check, load_library, make_cfg, make_rx_opts
from .fileio import decode_message


def _torch():
    import torch  # noqa: PLC0415  (device memory / streams only)
    return torch


def _ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


class Engine:
    """A context bound to one MI355X (gfx950).  Use as a context manager or call close()."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        self.lib = load_library()
        self.device = device
        torch = _torch()
        if not torch.cuda.is_available():
            raise abi.OfdmError("no GPU visible: the OFDM engine runs only on gfx950")
        torch.cuda.set_device(device)
        h = C.c_void_p()
        check(self.lib, self.lib.ofdm_ctx_create(device, C.byref(h)), "ofdm_ctx_create")
        self.ctx = h
        if use_torch_stream:
            self.set_stream(torch.cuda.current_stream(device).cuda_stream)

    # ---- lifecycle -------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ofdm_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int | None):
        """Enqueue on this hipStream_t handle (0 / None = the null stream, PyTorch's default)."""
        check(self.lib, self.lib.ofdm_ctx_set_stream(self.ctx, C.c_void_p(stream_handle or None)), "set_stream")

    def synchronize(self):
        check(self.lib, self.lib.ofdm_ctx_synchronize(self.ctx), "synchronize")

    def trim(self) -> int:
        """Free the context's sweep scratch (ofdm_ctx_trim: up to 12 GiB of frame-sweep hand-off buffer); returns
        the bytes released.  Later sweeps allocate it again."""
        n = C.c_int64()
        check(self.lib, self.lib.ofdm_ctx_trim(self.ctx, C.byref(n)), "ctx_trim")
        return n.value

    def scratch_bytes(self) -> int:
        n = C.c_int64()
        check(self.lib, self.lib.ofdm_ctx_scratch_bytes(self.ctx, C.byref(n)), "ctx_scratch_bytes")
        return n.value

    # ---- timing ----------------------------------------------------------------------
    def timing(self, enable: bool = True):
        check(self.lib, self.lib.ofdm_timing_enable(self.ctx, int(enable)), "timing_enable")

    def timing_reset(self):
        check(self.lib, self.lib.ofdm_timing_reset(self.ctx), "timing_reset")

    def timing_query(self, kernel: int) -> tuple[float, int]:
        ms = C.c_double(); n = C.c_int64()
        check(self.lib, self.lib.ofdm_timing_query(self.ctx, kernel, C.byref(ms), C.byref(n)), "timing_query")
        return ms.value, n.value

    # ---- K1: batched 64-point transforms (device tensors, complex64 [n, 64]) -----------
    def fft64(self, x, inverse: bool = False, conv: str = "c"):
        torch = _torch()
        x = x.contiguous()
        assert x.dtype == torch.complex64 and x.shape[-1] == 64 and x.is_cuda
        out = torch.empty_like(x)
        n = x.numel() // 64
        check(self.lib, self.lib.ofdm_fft64(self.ctx, _ptr(x), _ptr(out), n, int(inverse), abi.CONV[conv]), "fft64")
        return out

    def fft64_into(self, x, out, inverse: bool = False, conv: str = "c"):
        """fft64 into a preallocated complex64 [n, 64] device tensor (no allocation; in place allowed)."""
        torch = _torch()
        assert x.dtype == torch.complex64 and out.dtype == torch.complex64 and x.is_contiguous() and out.is_contiguous()
        assert x.shape == out.shape and x.shape[-1] == 64 and x.is_cuda and out.is_cuda
        check(self.lib, self.lib.ofdm_fft64(self.ctx, _ptr(x), _ptr(out), x.numel() // 64, int(inverse), abi.CONV[conv]),
              "fft64")
        return out

    # ---- symbol mode (the per-symbol chain) ---------------------------------------------
    def tx_buffers(self, n_frames: int):
        torch = _torch()
        tb = C.c_int64(); bb = C.c_int64()
        check(self.lib, self.lib.ofdm_tx_bytes(n_frames, C.byref(tb), C.byref(bb)), "tx_bytes")
        tx = torch.empty(tb.value // 8, dtype=torch.complex64, device=f"cuda:{self.device}")
        bits = torch.empty(bb.value // 4, dtype=torch.int32, device=f"cuda:{self.device}")
        return tx, bits

    def tx_frames(self, cfg: Cfg, first_frame: int, n_frames: int, tx=None, bits=None):
        if tx is None or bits is None:
            tx, bits = self.tx_buffers(n_frames)
        check(self.lib, self.lib.ofdm_tx_frames(self.ctx, C.byref(cfg), first_frame, n_frames, _ptr(tx), _ptr(bits)),
              "tx_frames")
        return tx, bits

    def set_next_tx(self, cfg: Cfg, first_frame: int, n_frames: int, tx, bits):
        """The next rx_frames call also builds this Tx batch (ofdm_set_next_tx: fused into the packed
        receiver, else a Tx launch ahead of it on the same stream)."""
        check(self.lib, self.lib.ofdm_set_next_tx(self.ctx, C.byref(cfg), first_frame, n_frames, _ptr(tx), _ptr(bits)),
              "set_next_tx")

    def new_counters(self, n_snr: int):
        torch = _torch()
        return torch.zeros((n_snr, abi.NCOUNTERS), dtype=torch.int64, device=f"cuda:{self.device}")

    def rx_frames(self, cfg: Cfg, tx, bits, first_frame: int, n_frames: int, snr_db, counters=None):
        snr = np.ascontiguousarray(snr_db, np.float64)
        if counters is None:
            counters = self.new_counters(len(snr))
        check(self.lib, self.lib.ofdm_rx_frames(self.ctx, C.byref(cfg), _ptr(tx), _ptr(bits), first_frame, n_frames,
                                                snr.ctypes.data_as(C.c_void_p), len(snr), _ptr(counters)), "rx_frames")
        return counters

    def txrx_frames(self, cfg: Cfg, first_frame: int, n_frames: int, snr_db, tx=None, bits=None, counters=None):
        """ofdm_txrx_frames: the Tx batch (written to tx / bits) and its receiver pass in one call (one launch
        for the packed real-noise receivers)."""
        snr = np.ascontiguousarray(snr_db, np.float64)
        if tx is None or bits is None:
            tx, bits = self.tx_buffers(n_frames)
        if counters is None:
            counters = self.new_counters(len(snr))
        check(self.lib, self.lib.ofdm_txrx_frames(self.ctx, C.byref(cfg), first_frame, n_frames, _ptr(tx), _ptr(bits),
                                                  snr.ctypes.data_as(C.c_void_p), len(snr), _ptr(counters)),
              "txrx_frames")
        return tx, bits, counters

    def rx_frames_dump(self, cfg: Cfg, tx, bits, first_frame: int, n_frames: int, snr_db):
        torch = _torch()
        snr = np.ascontiguousarray(snr_db, np.float64)
        counters = self.new_counters(len(snr))
        eq = torch.zeros((len(snr), n_frames, 2, 48), dtype=torch.complex64, device=f"cuda:{self.device}")
        db = torch.zeros((len(snr), n_frames, 2, 3), dtype=torch.int32, device=f"cuda:{self.device}")
        check(self.lib, self.lib.ofdm_rx_frames_dump(self.ctx, C.byref(cfg), _ptr(tx), _ptr(bits), first_frame,
                                                     n_frames, snr.ctypes.data_as(C.c_void_p), len(snr),
                                                     _ptr(counters), _ptr(eq), _ptr(db)), "rx_frames_dump")
        return counters, eq, db

    def symbol_sweep(self, cfg: Cfg, snr_db, n_frames: int, first_frame: int = 0, chunk_frames: int = 0) -> np.ndarray:
        snr = np.ascontiguousarray(snr_db, np.float64)
        out = np.zeros((len(snr), abi.NCOUNTERS), np.int64)
        check(self.lib, self.lib.ofdm_symbol_sweep(self.ctx, C.byref(cfg), snr.ctypes.data_as(C.c_void_p), len(snr),
                                                   first_frame, n_frames, chunk_frames,
                                                   out.ctypes.data_as(C.c_void_p)), "symbol_sweep")
        return out

    # ---- frame mode (the reference's own trial) -----------------------------------------
    def set_message(self, message: str | bytes) -> int:
        """MESSAGE payload text (OFDM.c:20); returns the data symbols per frame, ceil(8 len / 96)."""
        b = message.encode("latin-1") if isinstance(message, str) else bytes(message)
        n = C.c_int32()
        check(self.lib, self.lib.ofdm_set_message(self.ctx, b, len(b), C.byref(n)), "set_message")
        return n.value

    def set_long_message(self, message: str | bytes) -> int:
        """MESSAGE payload text of up to 180 characters (15 data symbols; ofdm_set_long_message, frame mode only for
        more than 96); up to 96 characters it is set_message itself.  Returns the data symbols per frame."""
        b = message.encode("latin-1") if isinstance(message, str) else bytes(message)
        n = C.c_int32()
        check(self.lib, self.lib.ofdm_set_long_message(self.ctx, b, len(b), C.byref(n)), "set_long_message")
        return n.value

    def payload_frames(self, payload: str = "message") -> int:
        n = C.c_int32()
        check(self.lib, self.lib.ofdm_payload_frames(self.ctx, abi.PAYLOAD[payload], C.byref(n)), "payload_frames")
        return n.value

    def transmitter(self, conv: str = "c", payload: str = "message", float_taps: bool = True) -> np.ndarray:
        cap = abi.wave_len(self.payload_frames(payload))
        buf = np.zeros(2 * cap, np.float32)
        n = C.c_int32()
        check(self.lib, self.lib.ofdm_transmitter(self.ctx, abi.CONV[conv], abi.PAYLOAD[payload], int(float_taps),
                                                  buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "transmitter")
        return buf[:2 * n.value].view(np.complex64).copy()

    def transmit_packets(self, words, n_data: int, positions=None, pos0: int = 0, stride: int | None = None,
                         gains=None, cfo_hz=None, out=None, n_out: int | None = None, accumulate: bool = False,
                         conv: str = "c", float_taps: bool = True):
        """Transmitter() over a batch of per-packet payloads, written into one device-resident recording
        (ofdm_transmit_packets, include/ofdm_mi355x_tx.h); returns the recording, a torch complex64 device tensor.

        words: uint32 / int32 [n, 3 n_data] payload words (stream.pack_messages; the `words` layout behind
        receive_stream's bits), a torch tensor on this engine's device used in place, or a numpy array, uploaded.
        Packet k starts at positions[k] (int64 [n], torch on the device or numpy) or at pos0 + k stride, stride
        defaulting to the packet length P = abi.packet_len(n_data); samples outside the recording are dropped.
        gains (complex64 [n]) and cfo_hz (float32 [n]) are optional, torch on the device or numpy.  out: the recording
        to write into, a contiguous complex64 device tensor, used in place; otherwise a zero-filled one of n_out
        samples is allocated, by default just large enough for the dense layout pos0 + n stride (pos0 >= 0), or for the
        furthest packet when positions is a numpy array.  accumulate adds to the recording (fp32 atomic adds) instead
        of storing.  Anything malformed raises ValueError before any launch.  The call waits for the device only when it
        uploaded numpy inputs (their device copies are released on return)."""
        return self._transmit(words, n_data, None, positions, pos0, stride, gains, cfo_hz, out, n_out, accumulate, conv,
                              float_taps)

    def _transmit(self, words, n_data, taps, positions, pos0, stride, gains, cfo_hz, out, n_out, accumulate, conv,
                  float_taps):
        """transmit_packets (taps None) and transmit_faded: the argument checks and the launch"""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if int(n_data) != n_data or not 1 <= n_data <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"n_data must be an integer in [1, {abi.LONG_MAX_DATA_SYMBOLS}], got {n_data!r}")
        n_data = int(n_data)
        if conv not in abi.CONV:
            raise ValueError(f"conv must be one of {tuple(abi.CONV)}, got {conv!r}")

        uploaded = []

        def device_array(x, name, np_dtypes, torch_dtypes, shape_text, ndim):
            if isinstance(x, np.ndarray):
                if x.dtype not in np_dtypes or x.ndim != ndim:
                    raise ValueError(f"{name} must be {shape_text}, got {x.dtype} {x.shape}")
                uploaded.append(name)
                return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            if not torch.is_tensor(x):
                raise ValueError(f"{name} must be a torch tensor or a numpy array, got {type(x).__name__}")
            if x.dtype not in torch_dtypes or x.dim() != ndim:
                raise ValueError(f"{name} must be {shape_text}, got {x.dtype} {tuple(x.shape)}")
            if x.device != dev:
                raise ValueError(f"{name} is on {x.device}, the engine runs on {dev}")
            if not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous, got strides {x.stride()}")
            return x

        if isinstance(words, np.ndarray) and words.dtype == np.uint32:
            words = words.view(np.int32)                                  # torch has no uint32 arithmetic; same bits
        w = device_array(words, "words", (np.dtype(np.int32),), (torch.int32, getattr(torch, "uint32", torch.int32)),
                         f"uint32 / int32 [n, {3 * n_data}]", 2)
        if w.shape[1] != 3 * n_data:
            raise ValueError(f"words must be uint32 / int32 [n, {3 * n_data}], got {tuple(w.shape)}")
        n = int(w.shape[0])
        h, L = None, 1
        if taps is not None:
            h = device_array(taps, "taps", (np.dtype(np.complex64),), (torch.complex64,), "complex64 [n, L]", 2)
            L = int(h.shape[1])
            if int(h.shape[0]) != n or not 1 <= L <= abi.FADE_MAX_TAPS:
                raise ValueError(f"taps must be complex64 [n = {n}, L] with 1 <= L <= {abi.FADE_MAX_TAPS}, "
                                 f"got {tuple(h.shape)}")
        plen = abi.faded_len(n_data, L)                                   # L = 1: the packet length itself
        per_packet = (("positions", positions, (np.dtype(np.int64),), (torch.int64,), "int64 [n]"),
                      ("gains", gains, (np.dtype(np.complex64),), (torch.complex64,), "complex64 [n]"),
                      ("cfo_hz", cfo_hz, (np.dtype(np.float32),), (torch.float32,), "float32 [n]"))
        dv = {}
        for name, x, npd, td, text in per_packet:
            dv[name] = None if x is None else device_array(x, name, npd, td, text, 1)
            if dv[name] is not None and int(dv[name].shape[0]) != n:
                raise ValueError(f"{name} must be {text} with n = {n}, got {tuple(dv[name].shape)}")
        if stride is None:
            stride = plen
        if int(pos0) != pos0 or int(stride) != stride:
            raise ValueError(f"pos0 and stride must be integers, got {pos0!r}, {stride!r}")
        pos0, stride = int(pos0), int(stride)
        if out is not None:
            if not (torch.is_tensor(out) and out.dtype == torch.complex64 and out.dim() == 1):
                raise ValueError("out must be a one-dimensional torch complex64 tensor")
            if out.device != dev:
                raise ValueError(f"out is on {out.device}, the engine runs on {dev}")
            if out.shape[0] > 1 and out.stride(0) != 1:
                raise ValueError(f"out needs a unit stride, got {out.stride(0)}")
            if n_out is not None and int(n_out) != int(out.shape[0]):
                raise ValueError(f"n_out {n_out!r} does not match out's {int(out.shape[0])} samples")
            rec = out
        else:
            if n_out is None:
                if positions is None:
                    n_out = max(pos0 + (n - 1) * stride, pos0) + plen if n else 0
                elif isinstance(positions, np.ndarray):
                    n_out = int(positions.max()) + plen if n else 0
                else:
                    raise ValueError("n_out or out is required when positions is a device tensor")
            if int(n_out) != n_out or n_out < 0:
                raise ValueError(f"n_out must be a non-negative integer, got {n_out!r}")
            rec = torch.zeros(int(n_out), dtype=torch.complex64, device=dev)
        opts = abi.TxOpts(abi.CONV[conv], int(bool(float_taps)), n_data, abi.TX_ACCUMULATE if accumulate else 0)
        opt = lambda x: None if x is None else _ptr(x)
        n_rec = int(rec.shape[0])
        if h is None:
            check(self.lib, self.lib.ofdm_transmit_packets(
                self.ctx, C.byref(opts), _ptr(w) if n else None, n, opt(dv["positions"]), pos0, stride, opt(dv["gains"]),
                opt(dv["cfo_hz"]), _ptr(rec) if n_rec else None, n_rec), "transmit_packets")
        else:
            check(self.lib, self.lib.ofdm_transmit_faded(
                self.ctx, C.byref(opts), _ptr(w) if n else None, n, opt(dv["positions"]), pos0, stride, opt(dv["gains"]),
                opt(dv["cfo_hz"]), _ptr(h) if n else None, L, _ptr(rec) if n_rec else None, n_rec), "transmit_faded")
        if uploaded:
            self.synchronize()
        return rec

    def draw_taps(self, n: int, pdp, seed: int = 0x80211A, index0: int = 0, out=None):
        """Rayleigh taps for n packets on the device (ofdm_draw_taps, include/ofdm_mi355x_fading.h): a torch complex64
        device tensor [n, len(pdp)], tap l of packet k a complex Gaussian of power pdp[l], a function of
        (seed, index0 + k, l) alone.  pdp: at most 32 finite powers >= 0, used as they are (channel.parse_pdp
        normalises a text).  out: the tensor to fill, used in place.  Anything malformed raises ValueError before any
        launch; the call does not wait for the device."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        for name, v in (("n", n), ("seed", seed), ("index0", index0)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
        n, seed, index0 = int(n), int(seed), int(index0)
        if n < 0:
            raise ValueError(f"n must not be negative, got {n}")
        if not 0 <= seed < 1 << 64 or not 0 <= index0 < 1 << 64:
            raise ValueError("seed and index0 must fit 64 unsigned bits")
        p = np.ascontiguousarray(np.asarray(pdp, np.float64).ravel(), np.float32)
        if not 1 <= len(p) <= abi.FADE_MAX_TAPS:
            raise ValueError(f"pdp must hold 1 to {abi.FADE_MAX_TAPS} powers, got {len(p)}")
        if not np.isfinite(p).all() or (p < 0).any():
            raise ValueError("pdp must be finite and not negative")
        if out is None:
            out = torch.empty((n, len(p)), dtype=torch.complex64, device=dev)
        elif not (torch.is_tensor(out) and out.dtype == torch.complex64 and tuple(out.shape) == (n, len(p))
                  and out.device == dev and out.is_contiguous()):
            raise ValueError(f"out must be a contiguous torch complex64 tensor [{n}, {len(p)}] on {dev}")
        check(self.lib, self.lib.ofdm_draw_taps(self.ctx, seed, index0, n, len(p), p.ctypes.data_as(C.c_void_p),
                                                _ptr(out) if n else None), "draw_taps")
        return out

    def transmit_faded(self, words, n_data: int, taps, positions=None, pos0: int = 0, stride: int | None = None,
                       gains=None, cfo_hz=None, out=None, n_out: int | None = None, accumulate: bool = False,
                       conv: str = "c", float_taps: bool = True):
        """transmit_packets through a channel of its own per packet (ofdm_transmit_faded,
        include/ofdm_mi355x_fading.h): packet k is its transmit_packets samples convolved with taps[k] -- complex64
        [n, L], L at most 32, a torch tensor on this engine's device (Engine.draw_taps) or a numpy array, uploaded -- and
        then takes its gain and carrier offset; it is abi.faded_len(n_data, L) = P + L - 1 samples long, which is also
        the default stride.  Every other argument is transmit_packets'."""
        if taps is None:
            raise ValueError("taps is required")
        return self._transmit(words, n_data, taps, positions, pos0, stride, gains, cfo_hz, out, n_out, accumulate, conv,
                              float_taps)

    def transmission_over_air(self, tx: np.ndarray, snr_db: float, seed: int = 0x80211A, trial: int = 0,
                              snr_index: int = 0) -> np.ndarray:
        tx = np.ascontiguousarray(tx, np.complex64)
        out = np.zeros_like(tx)
        check(self.lib, self.lib.ofdm_transmission_over_air(self.ctx, tx.ctypes.data_as(C.c_void_p),
                                                            out.ctypes.data_as(C.c_void_p), len(tx), snr_db, seed,
                                                            trial, snr_index), "transmission_over_air")
        return out

    def receiver(self, capture: np.ndarray, mode: str = "c", payload: str = "message", opts: dict | None = None):
        """Receiver() on one capture (OFDM.c:941-1182): metrics, packet_idx, bits, equalised
        subcarriers and the decoded text (Message_Generator, OFDM.c:921-939).  opts: single fields of ofdm_rx_opts
        over the mode's (abi.make_rx_opts), e.g. {"cap_len": 1100} for a capture shorter than its packet."""
        opts = make_rx_opts(mode, opts=opts)
        nd = self.payload_frames(payload)
        L = opts.cap_len or abi.capture_len(nd)
        cap = np.ascontiguousarray(capture[:L], np.complex64)
        if len(cap) != L:
            raise ValueError(f"capture must hold {L} samples")
        res = np.zeros(3, np.float32); ints = np.zeros(4, np.int32)
        bits = np.zeros(96 * nd, np.int32); eq = np.zeros(2 * 48 * nd, np.float32)
        check(self.lib, self.lib.ofdm_receiver(self.ctx, cap.ctypes.data_as(C.c_void_p), C.byref(opts),
                                               abi.PAYLOAD[payload], res.ctypes.data_as(C.c_void_p),
                                               ints.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p),
                                               eq.ctypes.data_as(C.c_void_p)), "receiver")
        return dict(res=res, packet_idx=int(ints[0]), sync_fail=int(ints[1]), oob=int(ints[2]), frames=nd,
                    bits=bits, eq=eq.view(np.complex64).copy(), message=decode_message(bits))

    def receive_captures(self, captures, mode: str = "c", payload: str = "message", want_bits: bool = True,
                         want_eq: bool = False, counters=None, opts: dict | None = None) -> dict:
        """Receiver() over a batch of caller-supplied captures (ofdm_receive_captures, include/ofdm_mi355x_captures.h):
        one record per capture, the two CFO estimates included.  opts: single fields of ofdm_rx_opts over the mode's
        (abi.make_rx_opts), e.g. {"cap_len": 1100} for captures shorter than their packet.

        captures: a torch complex64 tensor [n, L >= cap_len] on this engine's device, used in place (its row stride
        is the pitch; it is never written), or a numpy complex64 array of that shape, uploaded once.  Anything else
        raises ValueError before any launch.  counters: an int64 device tensor of NCOUNTERS elements, added to.
        Returns records (a structured array, abi.capture_result_dtype(); for torch input a dict of device tensors per
        field), bits ([n, 96 D] int32), eq ([n, 48 D] complex64), messages (decode_message per row) -- bits, eq and
        messages None when not asked for.  Outputs are allocated by torch on the current stream; only `messages`
        (want_bits) and numpy results wait for the device."""
        torch = _torch()
        opts = make_rx_opts(mode, opts=opts)
        nd = self.payload_frames(payload)
        L = opts.cap_len or abi.capture_len(nd)
        dev = torch.device("cuda", self.device)
        from_numpy = isinstance(captures, np.ndarray)
        if from_numpy:
            if captures.dtype != np.complex64 or captures.ndim != 2:
                raise ValueError(f"captures must be complex64 [n, L], got {captures.dtype} {captures.shape}")
            if captures.shape[1] < L:
                raise ValueError(f"captures hold {captures.shape[1]} samples, the receiver needs {L}")
            t = torch.from_numpy(np.ascontiguousarray(captures)).to(dev)
        elif torch.is_tensor(captures):
            t = captures
        else:
            raise ValueError(f"captures must be a torch tensor or a numpy array, got {type(captures).__name__}")
        if t.dtype != torch.complex64 or t.dim() != 2:
            raise ValueError(f"captures must be complex64 [n, L], got {t.dtype} {tuple(t.shape)}")
        if t.shape[1] < L:
            raise ValueError(f"captures hold {t.shape[1]} samples, the receiver needs {L}")
        if t.device != dev:
            raise ValueError(f"captures are on {t.device}, the engine runs on {dev}")
        n = int(t.shape[0])
        if t.stride(1) != 1 or (n > 1 and t.stride(0) < L):
            raise ValueError(f"captures need a unit inner stride and a row stride >= {L}, got strides {t.stride()}")
        pitch = int(t.stride(0)) if n > 1 else max(int(t.shape[1]), L)
        if counters is not None:
            if not (torch.is_tensor(counters) and counters.dtype == torch.int64 and counters.device == dev
                    and counters.numel() == abi.NCOUNTERS and counters.is_contiguous()):
                raise ValueError("counters must be a contiguous int64 device tensor of NCOUNTERS elements")
        rec = torch.empty((n, C.sizeof(abi.CaptureResult)), dtype=torch.uint8, device=dev)
        words = torch.empty((n, 3 * nd), dtype=torch.int32, device=dev) if want_bits else None
        eq = torch.empty((n, 48 * nd), dtype=torch.complex64, device=dev) if want_eq else None
        if n:
            check(self.lib, self.lib.ofdm_receive_captures(
                self.ctx, _ptr(t), n, pitch, C.byref(opts), abi.PAYLOAD[payload], _ptr(rec),
                None if words is None else _ptr(words), None if eq is None else _ptr(eq),
                None if counters is None else _ptr(counters)), "receive_captures")
        bits = None
        if want_bits:
            sh = torch.arange(31, -1, -1, dtype=torch.int32, device=dev)
            bits = ((words.unsqueeze(-1) >> sh) & 1).reshape(n, 96 * nd)              # MSB first
        dt = abi.capture_result_dtype()
        if from_numpy:
            records = rec.cpu().numpy().view(dt).reshape(n)
            bits = None if bits is None else bits.cpu().numpy()
            eq = None if eq is None else eq.cpu().numpy()
        else:
            w = rec.view(torch.int32)                                                 # [n, 12]
            records = {name: (w[:, k] if dt[name].kind == "i" else w[:, k].view(torch.float32))
                       for k, name in enumerate(dt.names[:10])}
        messages = None
        if want_bits:
            host = bits if from_numpy else bits.cpu().numpy()
            messages = [decode_message(row) for row in host]
        return dict(records=records, bits=bits, eq=eq, messages=messages, frames=nd, cap_len=L)

    def receive_stream(self, samples, mode: str = "c", payload: str = "message", max_packets: int | None = None,
                       want_bits: bool = True, want_eq: bool = False, want_metric: bool = False,
                       want_cross: bool = False, counters=None, keep_device: bool = False,
                       opts: dict | None = None, detector: str = "reference", threshold: float = 0.75,
                       timing: str = "none", tracking: str = "none") -> dict:
        """Every packet of one recording of any length (ofdm_receive_stream, include/ofdm_mi355x_stream.h): the
        reference's detection rule once over the whole recording, then the receiver chain on every packet found.
        opts: single fields of ofdm_rx_opts over the mode's (abi.make_rx_opts; a stream has no cap_len to set).
        detector, threshold: ofdm_receive_stream_ex's options (include/ofdm_mi355x_detect.h): "reference", the metric
        above over Lc = n - 47 positions, or "conjugate", the lag-32 delay-and-correlate metric with the conjugate over
        Lc = n - 63; a crossing is M > threshold, 0 < threshold < 1.  The defaults are ofdm_receive_stream itself.
        timing: "none", or "ltf" (ofdm_receive_stream_timed, include/ofdm_mi355x_timing.h): every packet_pos is refined
        against the long training field before the decode (stream.refine_timing is the rule); "ltf-matlab" is the same
        with the template of a MATLAB-convention waveform, for recordings made with conv="matlab" -- the recording's
        convention decides, not mode=, which decodes either.  The result then also
        holds coarse_pos (int64 [count], front + 11), shift (int32, packet_pos - coarse_pos) and quality (float32,
        in [0, 1], 0 for a packet that was not refined) -- all three None with "none".
        tracking: "none", or "pilots" (ofdm_receive_stream_tracked, include/ofdm_mi355x_track.h): every data symbol is
        turned back by the common phase of its four pilots before the slicer (stream.track_pilots is the rule), and
        records, bits and eq are those of the corrected subcarriers.  For long packets: on 2-symbol packets it costs a
        little BER.  The result then also holds phase (float32 [count, D], radians, 0 where the rule
        fell back to no correction) -- None with "none".

        samples: a one-dimensional contiguous torch complex64 tensor on this engine's device, used in place (never
        written), or a numpy complex64 array, uploaded once.  Anything else raises ValueError before any launch.
        max_packets: records to decode at most, default n // 301 + 1 (no stream holds more fronts).  counters: an int64
        device tensor of NCOUNTERS elements, added to.
        Returns count (records written), found (packets in the stream), positions (int64 [count]), records (a
        structured host array, abi.stream_packet_dtype()), bits ([count, 96 D] int32), eq ([count, 48 D] complex64),
        messages, metric (float32 [Lc]) and cross (uint32 words, stream.unpack_cross) -- those not asked for None;
        bits, eq, metric and cross stay on the device for torch input.  The call reads the packet count back, so it
        waits for the device.  keep_device: also return d_packets (uint8 [rows, 64]), d_count (int64 [2]) and d_words
        (int32 [rows, 3 D], None without want_bits), the device tensors the kernels wrote, for score_packets, d_timing
        and d_phase (float32 [rows, D], None without tracking)."""
        torch = _torch()
        opts = make_rx_opts(mode, opts=opts)
        nd = self.payload_frames(payload)
        dev = torch.device("cuda", self.device)
        from_numpy = isinstance(samples, np.ndarray)
        if from_numpy:
            if samples.dtype != np.complex64 or samples.ndim != 1:
                raise ValueError(f"samples must be complex64 [n], got {samples.dtype} {samples.shape}")
            t = torch.from_numpy(np.ascontiguousarray(samples)).to(dev)
        elif torch.is_tensor(samples):
            t = samples
        else:
            raise ValueError(f"samples must be a torch tensor or a numpy array, got {type(samples).__name__}")
        if t.dtype != torch.complex64 or t.dim() != 1:
            raise ValueError(f"samples must be complex64 [n], got {t.dtype} {tuple(t.shape)}")
        if t.device != dev:
            raise ValueError(f"samples are on {t.device}, the engine runs on {dev}")
        n = int(t.shape[0])
        if n > 1 and t.stride(0) != 1:
            raise ValueError(f"samples need a unit stride, got {t.stride(0)}")
        if max_packets is None:
            max_packets = n // 301 + 1
        if int(max_packets) != max_packets or max_packets < 0:
            raise ValueError(f"max_packets must be a non-negative integer, got {max_packets!r}")
        max_packets = int(max_packets)
        if counters is not None:
            if not (torch.is_tensor(counters) and counters.dtype == torch.int64 and counters.device == dev
                    and counters.numel() == abi.NCOUNTERS and counters.is_contiguous()):
                raise ValueError("counters must be a contiguous int64 device tensor of NCOUNTERS elements")
        sopts = abi.make_stream_opts(detector, threshold)
        tcode, kcode = abi.timing_code(timing), abi.tracking_code(tracking)
        lc = abi.stream_positions(n, detector)
        pk, cnt, words, eq, metric, cross, tim, ph = self._launch_receive_stream(
            t, opts, payload, nd, max_packets, want_bits, want_eq, want_metric, want_cross, counters, sopts, tcode, kcode)
        found, count = (int(v) for v in cnt.cpu())
        records = pk[:count].cpu().numpy().view(abi.stream_packet_dtype()).reshape(count)
        bits = None
        if want_bits:
            sh = torch.arange(31, -1, -1, dtype=torch.int32, device=dev)
            bits = ((words[:count].unsqueeze(-1) >> sh) & 1).reshape(count, 96 * nd)          # MSB first
        eq = None if eq is None else eq[:count]
        metric = None if metric is None else metric[:lc]
        cross = None if cross is None else cross[:(lc + 31) // 32]
        messages = None
        if want_bits:
            host = bits.cpu().numpy()
            messages = [decode_message(row) for row in host]
            if from_numpy:
                bits = host
        if from_numpy:
            eq = None if eq is None else eq.cpu().numpy()
            metric = None if metric is None else metric.cpu().numpy()
            cross = None if cross is None else cross.cpu().numpy().view(np.uint32)
        out = dict(count=count, found=found, positions=records["packet_pos"].copy(), records=records, bits=bits,
                   eq=eq, messages=messages, metric=metric, cross=cross, frames=nd, coarse_pos=None, shift=None,
                   quality=None, phase=None)
        if ph is not None:
            out.update(phase=ph[:count].cpu().numpy())
        if tim is not None:
            rows = tim[:count].cpu().numpy().view(abi.stream_timing_dtype()).reshape(count)
            out.update(coarse_pos=rows["coarse_pos"].copy(), shift=rows["shift"].copy(), quality=rows["quality"].copy())
        if keep_device:
            out.update(d_packets=pk, d_count=cnt, d_words=words, d_timing=tim, d_phase=ph)
        return out

    def receive_stream_device(self, samples, mode: str = "c", payload: str = "message", max_packets: int | None = None,
                              counters=None, detector: str = "reference", threshold: float = 0.75,
                              timing: str = "none", tracking: str = "none", want_eq: bool = False) -> dict:
        """receive_stream for a device recording without the read-back: nothing waits for the device.  samples: a
        one-dimensional contiguous torch complex64 tensor on this engine's device.  Returns d_packets (uint8
        [rows, 64], ofdm_stream_packet), d_count (int64 [2]: found, written) and d_words (int32 [rows, 3 D]), of which
        the first d_count[1] rows are written, and frames -- what score_packets takes.  detector, threshold: as
        receive_stream's.  timing: as receive_stream's; d_timing (uint8 [rows, 16], ofdm_stream_timing) with "ltf" or "ltf-matlab", else
        None.  tracking: as receive_stream's; d_phase (float32 [rows, D]) with "pilots", else None.  want_eq: the
        result also holds d_eq (complex64 [rows, 48 D], the equalised subcarriers), what decode_coded takes."""
        torch = _torch()
        opts = make_rx_opts(mode)
        nd = self.payload_frames(payload)
        dev = torch.device("cuda", self.device)
        if not torch.is_tensor(samples) or samples.dtype != torch.complex64 or samples.dim() != 1:
            raise ValueError("samples must be a one-dimensional torch complex64 tensor")
        if samples.device != dev:
            raise ValueError(f"samples are on {samples.device}, the engine runs on {dev}")
        n = int(samples.shape[0])
        if n > 1 and samples.stride(0) != 1:
            raise ValueError(f"samples need a unit stride, got {samples.stride(0)}")
        if max_packets is None:
            max_packets = n // 301 + 1
        if int(max_packets) != max_packets or max_packets < 0:
            raise ValueError(f"max_packets must be a non-negative integer, got {max_packets!r}")
        sopts = abi.make_stream_opts(detector, threshold)
        out = self._launch_receive_stream(samples, opts, payload, nd, int(max_packets), True, bool(want_eq), False, False,
                                          counters, sopts, abi.timing_code(timing), abi.tracking_code(tracking))
        res = dict(d_packets=out[0], d_count=out[1], d_words=out[2], frames=nd, d_timing=out[6], d_phase=out[7])
        if want_eq:
            res.update(d_eq=out[3])
        return res

    def _launch_receive_stream(self, t, opts, payload, nd, max_packets, want_bits, want_eq, want_metric, want_cross,
                               counters, sopts=None, timing=0, tracking=0):
        """Allocates ofdm_receive_stream's outputs and enqueues it: (packets, count, words, eq, metric, cross, timing,
        phase).
        sopts (abi.StreamOpts) other than the defaults goes through ofdm_receive_stream_ex, its outputs sized by its Lc;
        a timing other than OFDM_TIMING_NONE through ofdm_receive_stream_timed, with its rows (uint8 [rows, 16]); a
        tracking other than OFDM_TRACK_NONE through ofdm_receive_stream_tracked, with its phases (float32 [rows, D])."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        n = int(t.shape[0])
        conj = sopts is not None and sopts.detector == abi.DETECTOR["conjugate"]
        default = sopts is None or (not conj and sopts.threshold == abi.DETECT_THRESHOLD)
        lc = abi.stream_positions(n, "conjugate" if conj else "reference")
        rows = max(max_packets, 1)                                    # a pointer even when nothing may be written
        pk = torch.empty((rows, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        words = torch.empty((rows, 3 * nd), dtype=torch.int32, device=dev) if want_bits else None
        eq = torch.empty((rows, 48 * nd), dtype=torch.complex64, device=dev) if want_eq else None
        metric = torch.empty(max(lc, 1), dtype=torch.float32, device=dev) if want_metric else None
        cross = torch.empty(max((lc + 31) // 32, 1), dtype=torch.int32, device=dev) if want_cross else None
        opt = lambda x: None if x is None else _ptr(x)
        tim = ph = None
        if tracking != abi.TRACKING["none"]:
            if timing != abi.TIMING["none"]:
                tim = torch.empty((rows, C.sizeof(abi.StreamTiming)), dtype=torch.uint8, device=dev)
            ph = torch.empty((rows, nd), dtype=torch.float32, device=dev)
            check(self.lib, self.lib.ofdm_receive_stream_tracked(
                self.ctx, _ptr(t) if n else None, n, C.byref(opts), None if sopts is None else C.byref(sopts), timing,
                tracking, abi.PAYLOAD[payload], max_packets, _ptr(pk), _ptr(cnt), opt(words), opt(eq), opt(counters),
                opt(metric), opt(cross), opt(tim), _ptr(ph)), "receive_stream_tracked")
        elif timing != abi.TIMING["none"]:
            tim = torch.empty((rows, C.sizeof(abi.StreamTiming)), dtype=torch.uint8, device=dev)
            check(self.lib, self.lib.ofdm_receive_stream_timed(
                self.ctx, _ptr(t) if n else None, n, C.byref(opts), None if sopts is None else C.byref(sopts), timing,
                abi.PAYLOAD[payload], max_packets, _ptr(pk), _ptr(cnt), opt(words), opt(eq), opt(counters), opt(metric),
                opt(cross), _ptr(tim)), "receive_stream_timed")
        elif default:
            check(self.lib, self.lib.ofdm_receive_stream(
                self.ctx, _ptr(t) if n else None, n, C.byref(opts), abi.PAYLOAD[payload], max_packets, _ptr(pk), _ptr(cnt),
                opt(words), opt(eq), opt(counters), opt(metric), opt(cross)), "receive_stream")
        else:
            check(self.lib, self.lib.ofdm_receive_stream_ex(
                self.ctx, _ptr(t) if n else None, n, C.byref(opts), C.byref(sopts), abi.PAYLOAD[payload], max_packets,
                _ptr(pk), _ptr(cnt), opt(words), opt(eq), opt(counters), opt(metric), opt(cross)), "receive_stream_ex")
        return pk, cnt, words, eq, metric, cross, tim, ph

    def _branch_tensors(self, branches) -> list:
        """The B recordings of receive_diversity as one-dimensional complex64 device tensors of one length: a [B, n]
        complex64 tensor with unit stride along n and 8-byte-aligned rows, a sequence of B one-dimensional tensors, or
        a numpy [B, n] array (uploaded once).  ValueError for anything else, before any launch."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(branches, np.ndarray):
            if branches.dtype != np.complex64 or branches.ndim != 2:
                raise ValueError(f"branches must be complex64 [B, n], got {branches.dtype} {branches.shape}")
            branches = torch.from_numpy(np.ascontiguousarray(branches)).to(dev)
        if torch.is_tensor(branches):
            if branches.dim() != 2:
                raise ValueError(f"branches must be complex64 [B, n], got {tuple(branches.shape)}")
            rows = list(branches.unbind(0))
        elif isinstance(branches, (list, tuple)) and all(torch.is_tensor(r) for r in branches):
            rows = list(branches)
            if any(r.dim() != 1 for r in rows):
                raise ValueError("a sequence of one-dimensional tensors expected")
        else:
            raise ValueError(f"branches must be a [B, n] tensor, a sequence of tensors or a numpy array, got "
                             f"{type(branches).__name__}")
        if not 1 <= len(rows) <= abi.DIVERSITY_MAX_BRANCHES:
            raise ValueError(f"1 to {abi.DIVERSITY_MAX_BRANCHES} branches expected, got {len(rows)}")
        n = int(rows[0].shape[0])
        for b, r in enumerate(rows):
            if r.dtype != torch.complex64:
                raise ValueError(f"branch {b} must be complex64, got {r.dtype}")
            if r.device != dev:
                raise ValueError(f"branch {b} is on {r.device}, the engine runs on {dev}")
            if int(r.shape[0]) != n:
                raise ValueError(f"branches of one length expected, branch {b} has {int(r.shape[0])} samples, branch 0 {n}")
            if n > 1 and r.stride(0) != 1:
                raise ValueError(f"branch {b} needs a unit stride along its samples, got {r.stride(0)}")
            if n and r.data_ptr() % 8:
                raise ValueError(f"branch {b} must be 8-byte aligned")
        return rows

    def receive_diversity(self, branches, mode: str = "c", payload: str = "message", max_packets: int | None = None,
                          want_bits: bool = True, want_eq: bool = False, want_metric: bool = False,
                          want_cross: bool = False, counters=None, keep_device: bool = False,
                          opts: dict | None = None, detector: str = "reference", threshold: float = 0.75,
                          timing: str = "none", tracking: str = "none") -> dict:
        """receive_stream over B = 1..4 recordings of the same packets, one per antenna, on a common sample clock and
        oscillator (ofdm_receive_stream_diversity, include/ofdm_mi355x_diversity.h): the conjugate detector's sums, the
        fine timing metric and the carrier offset correlations are summed over the branches, and the branches'
        spectra are combined with maximal-ratio weights before the slicer (stream.diversity_metric,
        stream.refine_timing_branches and stream.combine_branches are the rules).  With one branch the call is
        receive_stream's on that recording.
        branches: a [B, n] complex64 tensor on this engine's device with unit stride along n and 8-byte-aligned rows, a
        sequence of B one-dimensional such tensors of equal length, or a numpy complex64 [B, n] array, uploaded once.
        Anything else raises ValueError before any launch, as does B > 1 with a detector other than "conjugate" (the
        reference's metric carries the channel's phase: its branch sums would cancel).  The other arguments and the result are receive_stream's, plus gain (float32 [count, B]: every
        branch's mean |H|^2 over the 52 used subcarriers; None for B = 1) and, with keep_device, d_gain."""
        torch = _torch()
        opts = make_rx_opts(mode, opts=opts)
        nd = self.payload_frames(payload)
        dev = torch.device("cuda", self.device)
        from_numpy = isinstance(branches, np.ndarray)
        rows = self._branch_tensors(branches)
        n = int(rows[0].shape[0])
        max_packets = self._div_max_packets(n, max_packets)
        if counters is not None:
            if not (torch.is_tensor(counters) and counters.dtype == torch.int64 and counters.device == dev
                    and counters.numel() == abi.NCOUNTERS and counters.is_contiguous()):
                raise ValueError("counters must be a contiguous int64 device tensor of NCOUNTERS elements")
        sopts = abi.make_stream_opts(detector, threshold)
        tcode, kcode = abi.timing_code(timing), abi.tracking_code(tracking)
        if len(rows) > 1 and detector != "conjugate":
            raise ValueError(f"{len(rows)} branches need detector='conjugate', got {detector!r}")
        lc = abi.stream_positions(n, detector)
        pk, cnt, words, eq, metric, cross, tim, ph, gain = self._launch_receive_diversity(
            rows, opts, payload, nd, max_packets, want_bits, want_eq, want_metric, want_cross, counters, sopts, tcode, kcode)
        found, count = (int(v) for v in cnt.cpu())
        records = pk[:count].cpu().numpy().view(abi.stream_packet_dtype()).reshape(count)
        bits = messages = None
        if want_bits:
            sh = torch.arange(31, -1, -1, dtype=torch.int32, device=dev)
            bits = ((words[:count].unsqueeze(-1) >> sh) & 1).reshape(count, 96 * nd)          # MSB first
            host = bits.cpu().numpy()
            messages = [decode_message(row) for row in host]
            if from_numpy:
                bits = host
        eq = None if eq is None else eq[:count]
        metric = None if metric is None else metric[:lc]
        cross = None if cross is None else cross[:(lc + 31) // 32]
        if from_numpy:
            eq = None if eq is None else eq.cpu().numpy()
            metric = None if metric is None else metric.cpu().numpy()
            cross = None if cross is None else cross.cpu().numpy().view(np.uint32)
        out = dict(count=count, found=found, positions=records["packet_pos"].copy(), records=records, bits=bits,
                   eq=eq, messages=messages, metric=metric, cross=cross, frames=nd, coarse_pos=None, shift=None,
                   quality=None, phase=None, gain=None, branches=len(rows))
        if ph is not None:
            out.update(phase=ph[:count].cpu().numpy())
        if gain is not None:
            out.update(gain=gain[:count].cpu().numpy())
        if tim is not None:
            trows = tim[:count].cpu().numpy().view(abi.stream_timing_dtype()).reshape(count)
            out.update(coarse_pos=trows["coarse_pos"].copy(), shift=trows["shift"].copy(), quality=trows["quality"].copy())
        if keep_device:
            out.update(d_packets=pk, d_count=cnt, d_words=words, d_timing=tim, d_phase=ph, d_gain=gain)
        return out

    def receive_diversity_device(self, branches, mode: str = "c", payload: str = "message",
                                 max_packets: int | None = None, counters=None, detector: str = "reference",
                                 threshold: float = 0.75, timing: str = "none", tracking: str = "none",
                                 want_eq: bool = False) -> dict:
        """receive_diversity for device recordings without the read-back: nothing waits for the device.  Returns what
        receive_stream_device returns -- d_packets, d_count, d_words, frames, d_timing, d_phase -- and d_gain (float32
        [rows, B], None for B = 1); with want_eq also d_eq (complex64 [rows, 48 D])."""
        opts = make_rx_opts(mode)
        nd = self.payload_frames(payload)
        if isinstance(branches, np.ndarray):
            raise ValueError("branches must be device tensors")
        rows = self._branch_tensors(branches)
        max_packets = self._div_max_packets(int(rows[0].shape[0]), max_packets)
        sopts = abi.make_stream_opts(detector, threshold)
        tcode, kcode = abi.timing_code(timing), abi.tracking_code(tracking)
        if len(rows) > 1 and detector != "conjugate":
            raise ValueError(f"{len(rows)} branches need detector='conjugate', got {detector!r}")
        out = self._launch_receive_diversity(rows, opts, payload, nd, max_packets, True, bool(want_eq), False, False, counters,
                                             sopts, tcode, kcode)
        res = dict(d_packets=out[0], d_count=out[1], d_words=out[2], frames=nd, d_timing=out[6], d_phase=out[7],
                   d_gain=out[8])
        if want_eq:
            res.update(d_eq=out[3])
        return res

    # ---- the coded link (include/ofdm_mi355x_code.h) ------------------------------------
    def encode_packets(self, info, n_data: int, rate: str = "1/2"):
        """Information words -> payload words on the device (ofdm_code_encode; stream.conv_encode is the rule): the
        K = 7 rate-1/2 code, the per-symbol interleaver and the precoding for the reference's QPSK map.  info: uint32
        or int32 [n, W_i] (abi.code_info_words(n_data)), a numpy array (uploaded) or a contiguous tensor on this engine's
        device.  Returns an int32 device tensor [n, 3 n_data], what transmit_packets and transmit_faded take.
        rate: "1/2", or "2/3" or "3/4" (include/ofdm_mi355x_punct.h: ofdm_punct_encode; stream.conv_encode_rate is the
        rule); W_i is then abi.punct_info_words(n_data, rate)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        rcode = abi.rate_code(rate)
        nd = int(n_data)
        if nd != n_data or not 1 <= nd <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"n_data must be in [1, {abi.LONG_MAX_DATA_SYMBOLS}], got {n_data!r}")
        wi = abi.punct_info_words(nd, rate)
        if isinstance(info, np.ndarray):
            if info.dtype not in (np.uint32, np.int32) or info.ndim != 2:
                raise ValueError(f"info must be uint32 [n, {wi}], got {info.dtype} {info.shape}")
            info = torch.from_numpy(np.ascontiguousarray(info).view(np.int32)).to(dev)
        if not torch.is_tensor(info) or info.dtype != torch.int32 or info.dim() != 2 or info.shape[1] != wi:
            raise ValueError(f"info must be 32-bit integers [n, {wi}] for {nd} data symbols")
        if info.device != dev or not info.is_contiguous():
            raise ValueError(f"info must be contiguous on {dev}")
        n = int(info.shape[0])
        words = torch.empty((n, 3 * nd), dtype=torch.int32, device=dev)
        if n and rcode == 0:
            check(self.lib, self.lib.ofdm_code_encode(self.ctx, nd, _ptr(info), n, _ptr(words)), "code_encode")
        elif n:
            check(self.lib, self.lib.ofdm_punct_encode(self.ctx, rcode, nd, _ptr(info), n, _ptr(words)), "punct_encode")
        return words

    def stream_csi(self, branches_or_samples, rx: dict):
        """The per-subcarrier gains of the records of a finished receive call (ofdm_stream_csi; stream.channel_gain is
        the rule): csi[i][m] = sum over the branches of |H_b|^2 at data subcarrier m, d_eq's order.
        branches_or_samples: the recording the call ran on, a one-dimensional complex64 device tensor, or its branches
        as receive_diversity takes them.  rx: the call's result with d_packets and d_count (receive_stream_device,
        receive_diversity_device, or receive_stream(keep_device=True)).  Returns a float32 device tensor [rows, 48] of
        which the first d_count[1] rows are written.  Nothing waits for the device."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if torch.is_tensor(branches_or_samples) and branches_or_samples.dim() == 1:
            branches_or_samples = [branches_or_samples]
        rows = self._branch_tensors(branches_or_samples)
        nb, n = len(rows), int(rows[0].shape[0])
        pk, cnt = rx["d_packets"], rx["d_count"]
        max_packets = int(pk.shape[0])
        csi = torch.empty((max_packets, 48), dtype=torch.float32, device=dev)
        table = (C.c_void_p * nb)(*[r.data_ptr() if n else None for r in rows])
        check(self.lib, self.lib.ofdm_stream_csi(self.ctx, table, nb, n, _ptr(pk), _ptr(cnt), max_packets, _ptr(csi)),
              "stream_csi")
        return csi

    def decode_coded(self, rx, csi=None, want_path: bool = False, n_data: int | None = None, rate: str = "1/2") -> dict:
        """The soft Viterbi decoder over equalised subcarriers (ofdm_code_decode; stream.conv_soft and
        stream.viterbi_decode are the rule, bit for bit).  rx: a receive call's result with d_eq and d_count
        (want_eq=True), or a complex64 device tensor [n, 48 D] to decode whole.  csi: stream_csi's tensor, or None for
        unweighted soft values.  Returns d_info (int32 [rows, W_i], MSB first; with rx a result, the first d_count[1]
        rows are written) and d_path (float32 [rows], the path metric; None without want_path).  Nothing waits for the
        device.  rate: "1/2", or "2/3" or "3/4" (include/ofdm_mi355x_punct.h: ofdm_punct_decode; stream.conv_soft_rate and
        stream.viterbi_decode_rate are the rule, bit for bit); W_i is then abi.punct_info_words(D, rate)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        rcode = abi.rate_code(rate)
        if isinstance(rx, dict):
            eq, cnt = rx.get("d_eq"), rx["d_count"]
            if eq is None:
                raise ValueError("the receive call must be made with want_eq=True")
        else:
            eq, cnt = rx, None
        if not torch.is_tensor(eq) or eq.dtype != torch.complex64 or eq.dim() != 2 or eq.shape[1] % 48:
            raise ValueError("d_eq must be a complex64 tensor [n, 48 D]")
        if eq.device != dev or not eq.is_contiguous():
            raise ValueError(f"d_eq must be contiguous on {dev}")
        n, nd = int(eq.shape[0]), int(eq.shape[1]) // 48
        if n_data is not None and int(n_data) != nd:
            raise ValueError(f"d_eq holds {nd} data symbols per row, n_data is {n_data}")
        if not 1 <= nd <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"1 to {abi.LONG_MAX_DATA_SYMBOLS} data symbols per row expected, got {nd}")
        if csi is not None:
            if not (torch.is_tensor(csi) and csi.dtype == torch.float32 and csi.device == dev and csi.is_contiguous()
                    and tuple(csi.shape) == (n, 48)):
                raise ValueError(f"csi must be a contiguous float32 device tensor [{n}, 48]")
        info = torch.empty((n, abi.punct_info_words(nd, rate)), dtype=torch.int32, device=dev)
        path = torch.empty(n, dtype=torch.float32, device=dev) if want_path else None
        opt = lambda x: None if x is None else _ptr(x)
        if n and rcode == 0:
            check(self.lib, self.lib.ofdm_code_decode(self.ctx, nd, _ptr(eq), opt(csi), opt(cnt), n, _ptr(info), opt(path)),
                  "code_decode")
        elif n:
            check(self.lib, self.lib.ofdm_punct_decode(self.ctx, rcode, nd, _ptr(eq), opt(csi), opt(cnt), n, _ptr(info),
                                                       opt(path)), "punct_decode")
        return dict(d_info=info, d_path=path, frames=nd)

    # ---- self-describing packets (include/ofdm_mi355x_ppdu.h) -----------------------------
    def encode_ppdu(self, psdu, lengths, rates, seeds, n_data: int) -> dict:
        """PSDUs -> payload words on the device (ofdm_ppdu_encode; stream.ppdu_encode is the rule): per packet a header
        symbol that names rate and LENGTH, the FCS over the first LENGTH - 4 bytes written behind them, the scrambler
        from the packet's seed, and the K = 7 code at the packet's rate.  psdu: 32-bit words [n, 31]; lengths, rates
        (codes 0, 1, 2 for "1/2", "2/3", "3/4") and seeds (1 .. 127): integers [n]; each a numpy array (uploaded) or a
        contiguous int32 tensor on this engine's device.  n_data: D symbols per packet, the header's among them, 2 .. 15.
        Host arrays are checked here: ValueError for a rate outside 0 .. 2, a LENGTH outside [4, abi.ppdu_cap(D, rate)]
        or a seed outside [1, 127].  Device tensors cannot be checked without a synchronisation: the kernel sends such a
        packet with a header that no receiver accepts (LENGTH 0 under a RATE field of 0).  Returns d_words (int32
        [n, 3 D], what transmit_packets and transmit_faded take) and d_info (int32 [n, 36], the header words and the
        scrambled information words).  Nothing waits for the device."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        nd = int(n_data)
        if nd != n_data or not abi.PPDU_MIN_SYMBOLS <= nd <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"n_data must be in [{abi.PPDU_MIN_SYMBOLS}, {abi.LONG_MAX_DATA_SYMBOLS}], got {n_data!r}")
        host = [np.asarray(x).reshape(-1) for x in (lengths, rates, seeds) if not torch.is_tensor(x)]
        if len(host) == 3:
            ln, rt, sd = (x.astype(np.int64) for x in host)
            if not (len(ln) == len(rt) == len(sd)):
                raise ValueError(f"lengths, rates and seeds must have one entry per packet, got {len(ln)}, {len(rt)}, {len(sd)}")
            if ((rt < 0) | (rt > 2)).any():
                raise ValueError(f"a rate code must be 0, 1 or 2, got {rt[(rt < 0) | (rt > 2)][0]}")
            caps = np.array([abi.ppdu_cap(nd, r) for r in abi.RATE])[rt]
            bad = (ln < abi.PPDU_MIN_LENGTH) | (ln > caps)
            if bad.any():
                k = int(np.nonzero(bad)[0][0])
                raise ValueError(f"packet {k}: LENGTH must be in [{abi.PPDU_MIN_LENGTH}, {caps[k]}] for {nd} symbols at rate "
                                 f"{tuple(abi.RATE)[rt[k]]}, got {ln[k]}")
            if ((sd < 1) | (sd > 127)).any():
                raise ValueError(f"a seed must be in [1, 127], got {sd[(sd < 1) | (sd > 127)][0]}")
        if isinstance(psdu, np.ndarray):
            if psdu.dtype not in (np.uint32, np.int32) or psdu.ndim != 2:
                raise ValueError(f"psdu must be uint32 [n, {abi.PPDU_PSDU_WORDS}], got {psdu.dtype} {psdu.shape}")
            psdu = torch.from_numpy(np.ascontiguousarray(psdu).view(np.int32)).to(dev)
        if not torch.is_tensor(psdu) or psdu.dtype != torch.int32 or psdu.dim() != 2 or psdu.shape[1] != abi.PPDU_PSDU_WORDS:
            raise ValueError(f"psdu must be 32-bit integers [n, {abi.PPDU_PSDU_WORDS}]")
        n = int(psdu.shape[0])
        per = []
        for name, x in (("lengths", lengths), ("rates", rates), ("seeds", seeds)):
            if not torch.is_tensor(x):
                x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1).astype(np.int32))).to(dev)
            if x.dtype != torch.int32 or tuple(x.shape) != (n,):
                raise ValueError(f"{name} must be int32 [{n}]")
            per.append(x)
        for x in (psdu, *per):
            if x.device != dev or not x.is_contiguous():
                raise ValueError(f"psdu, lengths, rates and seeds must be contiguous on {dev}")
        info = torch.empty((n, abi.PPDU_INFO_WORDS), dtype=torch.int32, device=dev)
        words = torch.empty((n, 3 * nd), dtype=torch.int32, device=dev)
        if n:
            check(self.lib, self.lib.ofdm_ppdu_encode(self.ctx, nd, _ptr(psdu), _ptr(per[0]), _ptr(per[1]), _ptr(per[2]), n,
                                                      _ptr(info), _ptr(words)), "ppdu_encode")
        return dict(d_words=words, d_info=info, frames=nd)

    def decode_ppdu(self, rx, csi=None, want_path: bool = False, n_data: int | None = None) -> dict:
        """The fused decoder of self-describing packets (ofdm_ppdu_decode; stream.ppdu_decode is the rule, bit for bit):
        per row the header symbol, then the data symbols at the rate the header names, the descrambling and the FCS.
        rx, csi, n_data: decode_coded's.  Returns d_meta (int32 [rows, 4]: status -- 0 for a packet whose FCS passed,
        else abi.PPDU_BAD_* bits --, the rate's code or -1, LENGTH, seed), d_psdu (int32 [rows, 31], MSB first: the LENGTH
        bytes, zeros behind) and d_path (float32 [rows, 2], the header's and the data part's path metric; None without
        want_path).  With rx a result, the first d_count[1] rows are written.  Nothing waits for the device."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(rx, dict):
            eq, cnt = rx.get("d_eq"), rx["d_count"]
            if eq is None:
                raise ValueError("the receive call must be made with want_eq=True")
        else:
            eq, cnt = rx, None
        if not torch.is_tensor(eq) or eq.dtype != torch.complex64 or eq.dim() != 2 or eq.shape[1] % 48:
            raise ValueError("d_eq must be a complex64 tensor [n, 48 D]")
        if eq.device != dev or not eq.is_contiguous():
            raise ValueError(f"d_eq must be contiguous on {dev}")
        n, nd = int(eq.shape[0]), int(eq.shape[1]) // 48
        if n_data is not None and int(n_data) != nd:
            raise ValueError(f"d_eq holds {nd} symbols per row, n_data is {n_data}")
        if not abi.PPDU_MIN_SYMBOLS <= nd <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"{abi.PPDU_MIN_SYMBOLS} to {abi.LONG_MAX_DATA_SYMBOLS} symbols per row expected, got {nd}")
        if csi is not None:
            if not (torch.is_tensor(csi) and csi.dtype == torch.float32 and csi.device == dev and csi.is_contiguous()
                    and tuple(csi.shape) == (n, 48)):
                raise ValueError(f"csi must be a contiguous float32 device tensor [{n}, 48]")
        meta = torch.empty((n, 4), dtype=torch.int32, device=dev)
        psdu = torch.empty((n, abi.PPDU_PSDU_WORDS), dtype=torch.int32, device=dev)
        path = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_path else None
        opt = lambda x: None if x is None else _ptr(x)
        if n:
            check(self.lib, self.lib.ofdm_ppdu_decode(self.ctx, nd, _ptr(eq), opt(csi), opt(cnt), n, _ptr(meta), _ptr(psdu),
                                                      opt(path)), "ppdu_decode")
        return dict(d_meta=meta, d_psdu=psdu, d_path=path, frames=nd)

    @staticmethod
    def _div_max_packets(n: int, max_packets) -> int:
        if max_packets is None:
            max_packets = n // 301 + 1
        if int(max_packets) != max_packets or max_packets < 0:
            raise ValueError(f"max_packets must be a non-negative integer, got {max_packets!r}")
        return int(max_packets)

    def _launch_receive_diversity(self, rows, opts, payload, nd, max_packets, want_bits, want_eq, want_metric, want_cross,
                                  counters, sopts, timing, tracking):
        """Allocates ofdm_receive_stream_diversity's outputs and enqueues it: _launch_receive_stream's tuple and the
        gains (float32 [rows, B], None for one branch)."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        nb, n = len(rows), int(rows[0].shape[0])
        conj = sopts.detector == abi.DETECTOR["conjugate"]
        lc = abi.stream_positions(n, "conjugate" if conj else "reference")
        nrows = max(max_packets, 1)                                   # a pointer even when nothing may be written
        pk = torch.empty((nrows, C.sizeof(abi.StreamPacket)), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        words = torch.empty((nrows, 3 * nd), dtype=torch.int32, device=dev) if want_bits else None
        eq = torch.empty((nrows, 48 * nd), dtype=torch.complex64, device=dev) if want_eq else None
        metric = torch.empty(max(lc, 1), dtype=torch.float32, device=dev) if want_metric else None
        cross = torch.empty(max((lc + 31) // 32, 1), dtype=torch.int32, device=dev) if want_cross else None
        tim = torch.empty((nrows, C.sizeof(abi.StreamTiming)), dtype=torch.uint8, device=dev) \
            if timing != abi.TIMING["none"] else None
        ph = torch.empty((nrows, nd), dtype=torch.float32, device=dev) if tracking != abi.TRACKING["none"] else None
        gain = torch.empty((nrows, nb), dtype=torch.float32, device=dev) if nb > 1 else None
        opt = lambda x: None if x is None else _ptr(x)
        table = (C.c_void_p * nb)(*[r.data_ptr() if n else None for r in rows])
        check(self.lib, self.lib.ofdm_receive_stream_diversity(
            self.ctx, table, nb, n, C.byref(opts), C.byref(sopts), timing, tracking, abi.PAYLOAD[payload], max_packets,
            _ptr(pk), _ptr(cnt), opt(words), opt(eq), opt(counters), opt(metric), opt(cross), opt(tim), opt(ph), opt(gain)),
              "receive_stream_diversity")
        return pk, cnt, words, eq, metric, cross, tim, ph, gain

    def impair_stream(self, x, power: float, snr_db: float, cfo_hz: float = 0.0, taps=None, noise: str = "real",
                      seed: int = 0x80211A, trial: int = 0, snr_index: int = 0, index0: int = 0, lead: int = 0,
                      out=None):
        """The channel over a device-resident recording (ofdm_impair_stream, include/ofdm_mi355x_channel.h): the
        multipath FIR `taps` (complex, at most 32), the rotation exp(j 2 pi cfo_hz k 25e-9) by the absolute index
        k = index0 + i, then noise of variance power / 10^(snr_db / 10) from the Philox stream (seed, trial, snr_index)
        at index k ("real": all of it in the real part, "complex": split across both axes, "none").

        x: a contiguous one-dimensional torch complex64 tensor on this engine's device, or a numpy complex64 array,
        uploaded once.  Its first `lead` samples are history for the filter and give no output: the result has
        len(x) - lead samples.  out: the tensor to write, used in place; `out is x` (lead 0, at most one tap) is the
        in-place case.  Returns the device tensor.  Anything malformed raises ValueError before any launch; the call
        does not wait for the device."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if noise not in abi.NOISE:
            raise ValueError(f"noise must be one of {tuple(abi.NOISE)}, got {noise!r}")
        if isinstance(x, np.ndarray):
            if x.dtype != np.complex64 or x.ndim != 1:
                raise ValueError(f"x must be complex64 [n], got {x.dtype} {x.shape}")
            x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        elif not torch.is_tensor(x):
            raise ValueError(f"x must be a torch tensor or a numpy array, got {type(x).__name__}")
        for name, t in (("x", x), ("out", out)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.complex64 or t.dim() != 1:
                raise ValueError(f"{name} must be a one-dimensional torch complex64 tensor")
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, the engine runs on {dev}")
            if t.shape[0] > 1 and t.stride(0) != 1:
                raise ValueError(f"{name} needs a unit stride, got {t.stride(0)}")
        for name, v in (("trial", trial), ("seed", seed), ("snr_index", snr_index), ("index0", index0), ("lead", lead)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"{name} must be an integer, got {v!r}")
        seed, trial, snr_index, index0, lead = int(seed), int(trial), int(snr_index), int(index0), int(lead)
        if not 0 <= seed < 1 << 64 or not 0 <= trial < 1 << 64:
            raise ValueError("seed and trial must fit 64 unsigned bits")
        if not 0 <= snr_index < 1 << 24:
            raise ValueError(f"snr_index must be in [0, 2^24), got {snr_index}")
        if index0 < 0 or index0 >= 1 << 62:
            raise ValueError(f"index0 must be a non-negative stream index, got {index0}")
        if not 0 <= lead <= int(x.shape[0]):
            raise ValueError(f"lead must be in [0, len(x) = {int(x.shape[0])}], got {lead}")
        for name, v in (("power", power), ("snr_db", snr_db), ("cfo_hz", cfo_hz)):
            if not np.isfinite(float(v)):
                raise ValueError(f"{name} must be finite, got {v!r}")
        if float(power) < 0:
            raise ValueError(f"power must not be negative, got {power!r}")
        h = np.zeros(0, np.complex64) if taps is None else np.ascontiguousarray(np.asarray(taps).ravel(), np.complex64)
        if len(h) > abi.CHANNEL_MAX_TAPS:
            raise ValueError(f"at most {abi.CHANNEL_MAX_TAPS} taps, got {len(h)}")
        if not np.isfinite(h.view(np.float32)).all():
            raise ValueError("taps must be finite")
        n = int(x.shape[0]) - lead
        if out is None:
            out = torch.empty(n, dtype=torch.complex64, device=dev)
        elif int(out.shape[0]) != n:
            raise ValueError(f"out must hold len(x) - lead = {n} samples, got {int(out.shape[0])}")
        if noise != "none" and index0 + n > 1 << (34 if noise == "real" else 33):
            raise ValueError(f"index0 + n = {index0 + n} exceeds the {noise} noise stream's 2^{34 if noise == 'real' else 33} samples")
        if n:
            a0, a1 = x.data_ptr(), x.data_ptr() + 8 * (lead + n)
            b0, b1 = out.data_ptr(), out.data_ptr() + 8 * n
            if b0 < a1 and a0 < b1 and not (b0 == a0 and lead == 0 and len(h) <= 1):
                raise ValueError("out overlaps x: in place needs out to start where x starts, lead 0 and at most one tap")
        opts = abi.ChannelOpts(float(power), float(snr_db), float(cfo_hz), seed, trial, index0, abi.NOISE[noise],
                               snr_index, len(h), lead)
        try:
            check(self.lib, self.lib.ofdm_impair_stream(
                self.ctx, C.byref(opts), h.ctypes.data_as(C.c_void_p) if len(h) else None, _ptr(x) if n else None,
                _ptr(out) if n else None, n), "impair_stream")
        except abi.OfdmError as e:
            if "(-1)" in str(e):
                raise ValueError(str(e)) from None
            raise
        return out

    def score_packets(self, words, n_data: int, rx, positions=None, pos0: int = 0, stride: int | None = None,
                      window=(8, 40), totals=None) -> dict:
        """Scores received records against the transmitted packets on the device (ofdm_score_packets,
        include/ofdm_mi355x_channel.h; stream.score_packets is the rule in numpy).

        words, positions, pos0, stride: what transmit_packets was given (device tensors used in place, numpy arrays
        uploaded).  rx: receive_stream's result with keep_device=True, receive_stream_device's result, or the tuple
        (d_packets, d_count, d_words).  window: (off_lo, off_hi), the offsets packet_pos - position that count as a
        match.  totals: an int64 device tensor of NSCORE elements, added to; otherwise a zeroed one is made.
        Returns scores (int32 [n, 2] device tensor: rx_index, bit_err) and totals (the device tensor); nothing waits
        for the device unless numpy inputs were uploaded."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(n_data, bool) or int(n_data) != n_data or not 1 <= n_data <= abi.LONG_MAX_DATA_SYMBOLS:
            raise ValueError(f"n_data must be an integer in [1, {abi.LONG_MAX_DATA_SYMBOLS}], got {n_data!r}")
        n_data = int(n_data)
        try:
            lo, hi = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError(f"window must be (off_lo, off_hi), got {window!r}") from None
        if not (0 <= lo <= hi and hi - lo <= abi.SCORE_MAX_WINDOW):
            raise ValueError(f"window needs 0 <= off_lo <= off_hi and off_hi - off_lo <= {abi.SCORE_MAX_WINDOW}, got {window!r}")
        uploaded = False

        def device_array(x, name, np_dtype, torch_dtypes, ndim):
            nonlocal uploaded
            if isinstance(x, np.ndarray):
                if x.dtype != np_dtype or x.ndim != ndim:
                    raise ValueError(f"{name} must be {np_dtype} with {ndim} dimensions, got {x.dtype} {x.shape}")
                uploaded = True
                return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            if not torch.is_tensor(x) or x.dtype not in torch_dtypes or x.dim() != ndim:
                raise ValueError(f"{name} must be a torch tensor or a numpy array of {np_dtype} with {ndim} dimensions")
            if x.device != dev or not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous on {dev}")
            return x

        if isinstance(words, np.ndarray) and words.dtype == np.uint32:
            words = words.view(np.int32)
        w = device_array(words, "words", np.dtype(np.int32), (torch.int32, getattr(torch, "uint32", torch.int32)), 2)
        if w.shape[1] != 3 * n_data:
            raise ValueError(f"words must be uint32 / int32 [n, {3 * n_data}], got {tuple(w.shape)}")
        n = int(w.shape[0])
        pos = None
        if positions is not None:
            pos = device_array(positions, "positions", np.dtype(np.int64), (torch.int64,), 1)
            if int(pos.shape[0]) != n:
                raise ValueError(f"positions must be int64 [n] with n = {n}, got {tuple(pos.shape)}")
        if stride is None:
            stride = abi.packet_len(n_data)
        if int(pos0) != pos0 or int(stride) != stride:
            raise ValueError(f"pos0 and stride must be integers, got {pos0!r}, {stride!r}")
        if isinstance(rx, dict):
            if any(rx.get(k) is None for k in ("d_packets", "d_count", "d_words")):
                raise ValueError("rx needs d_packets, d_count and d_words: receive_stream(..., keep_device=True)")
            if rx.get("frames", n_data) != n_data:
                raise ValueError(f"rx holds packets of {rx['frames']} data symbols, n_data is {n_data}")
            pk, cnt, rw = rx["d_packets"], rx["d_count"], rx["d_words"]
        else:
            try:
                pk, cnt, rw = rx
            except (TypeError, ValueError):
                raise ValueError("rx must be receive_stream's result or (d_packets, d_count, d_words)") from None
        for name, t, dt in (("d_packets", pk, torch.uint8), ("d_count", cnt, torch.int64), ("d_words", rw, torch.int32)):
            if not (torch.is_tensor(t) and t.dtype == dt and t.device == dev and t.is_contiguous()):
                raise ValueError(f"rx {name} must be a contiguous {dt} tensor on {dev}")
        rows = int(pk.shape[0]) if pk.dim() == 2 else -1
        if pk.dim() != 2 or pk.shape[1] != C.sizeof(abi.StreamPacket) or cnt.numel() != 2 \
                or tuple(rw.shape) != (rows, 3 * n_data):
            raise ValueError(f"rx needs d_packets [rows, 64], d_count [2] and d_words [rows, {3 * n_data}]")
        if totals is None:
            totals = torch.zeros(abi.NSCORE, dtype=torch.int64, device=dev)
        elif not (torch.is_tensor(totals) and totals.dtype == torch.int64 and totals.device == dev
                  and totals.numel() == abi.NSCORE and totals.is_contiguous()):
            raise ValueError("totals must be a contiguous int64 device tensor of NSCORE elements")
        scores = torch.empty((n, 2), dtype=torch.int32, device=dev)
        check(self.lib, self.lib.ofdm_score_packets(
            self.ctx, n_data, _ptr(w) if n else None, n, None if pos is None else _ptr(pos), int(pos0), int(stride),
            _ptr(pk), _ptr(cnt), _ptr(rw), lo, hi, _ptr(scores) if n else None, _ptr(totals)), "score_packets")
        if uploaded:
            self.synchronize()
        return dict(scores=scores, totals=totals)

    def word_length_report(self, capture: np.ndarray) -> dict:
        """Word_Optimization_Analysis (OFDM.c:38-73) of the capture's RRC matched-filter output."""
        cap = np.ascontiguousarray(capture, np.complex64)
        out = np.zeros(3, np.float32)
        bits = C.c_int32()
        check(self.lib, self.lib.ofdm_word_length_report(self.ctx, cap.ctypes.data_as(C.c_void_p), len(cap),
                                                         out.ctypes.data_as(C.c_void_p), C.byref(bits)),
              "word_length_report")
        return dict(min=float(out[0]), max=float(out[1]), max_abs=float(out[2]), bits=bits.value)

    def frame_sweep(self, cfg: Cfg, snr_db, n_trials: int, first_trial: int = 0, mode: str = "c",
                    fixed_start: int = -1, want_packet_idx: bool = False, word_stats: bool = False,
                    cap_len: int = 0):
        """cap_len 0: the mode's capture (int(0.307 len), OFDM.c:945; 3000 for 'matlab')."""
        snr = np.ascontiguousarray(snr_db, np.float64)
        out = np.zeros((len(snr), abi.NCOUNTERS), np.int64)
        pidx = np.zeros((len(snr), n_trials), np.int32) if want_packet_idx else None
        opts = make_rx_opts(mode, fixed_start)
        opts.word_stats = int(word_stats)
        if cap_len:
            opts.cap_len = int(cap_len)
        check(self.lib, self.lib.ofdm_frame_sweep(self.ctx, C.byref(cfg), C.byref(opts), snr.ctypes.data_as(C.c_void_p),
                                                  len(snr), first_trial, n_trials, out.ctypes.data_as(C.c_void_p),
                                                  None if pidx is None else pidx.ctypes.data_as(C.c_void_p)),
              "frame_sweep")
        return (out, pidx) if want_packet_idx else out


@dataclass
class SweepResult:
    snr_db: np.ndarray
    counters: np.ndarray

    @property
    def ber(self) -> np.ndarray:
        c = self.counters
        return c[:, abi.C_BIT_ERR] / np.maximum(c[:, abi.C_BITS], 1)

    @property
    def evm_pre_db(self) -> np.ndarray:
        """pooled EVM before the slicer: 10 log10(sum|z-d|^2 / sum|d|^2) (OFDM.c:1104-1126)"""
        c = self.counters
        with np.errstate(divide="ignore"):
            return 10 * np.log10(c[:, abi.C_EVM_PRE_Q] / abi.EVM_Q_SCALE / np.maximum(c[:, abi.C_EVM_TERMS], 1))

    @property
    def evm_post_db(self) -> np.ndarray:
        """pooled EVM after the slicer (OFDM.c:1128-1150); -inf when no slicer error"""
        c = self.counters
        with np.errstate(divide="ignore"):
            return 10 * np.log10(2.0 * c[:, abi.C_EVM_POST_AXIS] / np.maximum(c[:, abi.C_EVM_TERMS], 1))

    @property
    def mean_frame_evm_db(self) -> np.ndarray:
        """mean over frames of the per-frame EVM_dB the reference prints per trial (OFDM.c:1126)"""
        c = self.counters
        return c[:, abi.C_EVMDB_PRE_Q] / abi.EVM_Q_SCALE / np.maximum(c[:, abi.C_FRAMES], 1)

    @property
    def mean_frame_evm_post_db(self) -> np.ndarray:
        """mean over frames of the per-frame post-slicer EVM_dB (OFDM.c:1150); -inf when any frame
        had no slicer error (that frame's own value is -inf, OFDM.c:1148-1150)"""
        c = self.counters
        m = c[:, abi.C_EVMDB_POST_Q] / abi.EVM_Q_SCALE / np.maximum(c[:, abi.C_FRAMES], 1)
        return np.where(c[:, abi.C_EVMDB_POST_FINITE] < c[:, abi.C_FRAMES], -np.inf, m)

    @property
    def mean_finite_frame_evm_post_db(self) -> np.ndarray:
        """mean of the per-frame post-slicer EVM_dB over the frames where it is finite (frames with >= 1
        slicer error); -inf only where no frame had one.  A plottable companion of mean_frame_evm_post_db
        for many trials per point (the reference's own statistic is -inf as soon as one trial is clean)."""
        c = self.counters
        fin = c[:, abi.C_EVMDB_POST_FINITE]
        m = c[:, abi.C_EVMDB_POST_Q] / abi.EVM_Q_SCALE / np.maximum(fin, 1)
        return np.where(fin > 0, m, -np.inf)

    @property
    def sync_fail_rate(self) -> np.ndarray:
        c = self.counters
        return c[:, abi.C_SYNC_FAIL] / np.maximum(c[:, abi.C_FRAMES], 1)


__all__ = ["Engine", "SweepResult", "make_cfg", "make_rx_opts"]
