"""Impaired captures for Engine.receive_captures (torch plumbing only; the receiver is the HIP kernel).

make_captures() cuts captures out of the repeated frame waveform (Transmitter(), OFDM.c:467-618) after an optional
multipath FIR, a carrier frequency offset and AWGN -- the impairments the reference's receiver spends its coarse / fine
CFO estimation (OFDM.c:773-828) and its per-subcarrier equaliser on, and that the in-kernel capture generator of
ofdm_frame_sweep (real-only AWGN over the clean waveform) cannot produce.  It runs on whatever device `wave` is on,
the CPU included.
"""
from __future__ import annotations

import numpy as np

TS_OVERSAMPLED = 25e-9        # sample period of the waveform: 2 x 20 MHz (OFDM.c:16-17, oversampling 2)
NOISE_KINDS = ("real", "complex", "none")


def _torch():
    import torch  # noqa: PLC0415
    return torch


def make_captures(wave, starts, snr_db, cfo_hz=0.0, taps=None, noise: str = "real", generator=None,
                  cap_len: int | None = None):
    """Captures [n, cap_len] (complex64, on wave's device) of the waveform `wave` (complex64 [len]).  In order:

    1. `taps` (optional): a linear FIR at the oversampled rate over the whole repeated waveform, truncated to its
       length: y[k] = sum_j taps[j] wave[k - j].
    2. the rotation exp(j 2 pi cfo_hz k 25e-9) by the absolute waveform index k.
    3. noise of variance mean|wave|^2 / 10^(snr_db / 10), measured on the unimpaired waveform as
       Transmission_Over_Air does (OFDM.c:637-647): "real" carries all of it in the real part (what OFDM.c:651
       does), "complex" splits it across both axes, "none" adds nothing.
    4. the windows [start, start + cap_len).

    starts, snr_db and cfo_hz broadcast against each other to the n captures.  cap_len None: int(0.307 len(wave))
    (OFDM.c:945).  generator: a torch.Generator on wave's device for the noise."""
    torch = _torch()
    if noise not in NOISE_KINDS:
        raise ValueError(f"noise must be one of {NOISE_KINDS}, got {noise!r}")
    wave = torch.as_tensor(wave)
    if wave.dim() != 1 or not wave.is_complex():
        raise ValueError("wave must be a one-dimensional complex tensor")
    wave = wave.to(torch.complex64)
    dev, wl = wave.device, int(wave.shape[0])
    L = int(wl * 0.307) if cap_len is None else int(cap_len)
    st, snr, cfo = torch.broadcast_tensors(
        torch.atleast_1d(torch.as_tensor(starts, device=dev)).to(torch.int64),
        torch.atleast_1d(torch.as_tensor(snr_db, device=dev)).to(torch.float64),
        torch.atleast_1d(torch.as_tensor(cfo_hz, device=dev)).to(torch.float64))
    if st.numel() and (int(st.min()) < 0 or int(st.max()) + L > wl):
        raise ValueError(f"capture windows of {L} samples must lie inside the {wl}-sample waveform")
    power = float(torch.mean(wave.real.double() ** 2 + wave.imag.double() ** 2))        # OFDM.c:637-643
    y = wave
    if taps is not None:
        h = np.asarray(taps, np.complex64).ravel()
        y = torch.zeros_like(wave)
        for j, hj in enumerate(h):
            if hj != 0 and j < wl:
                y[j:] += complex(hj) * wave[:wl - j]
    k = st[:, None] + torch.arange(L, device=dev, dtype=torch.int64)[None, :]           # absolute waveform index
    caps = y[k]
    if bool((cfo != 0).any()):
        rev = cfo[:, None] * k.double() * TS_OVERSAMPLED                                # phase in revolutions, fp64
        ang = (2.0 * np.pi) * (rev - torch.round(rev))
        caps = caps * torch.complex(torch.cos(ang), torch.sin(ang)).to(torch.complex64)
    if noise != "none":
        sigma = torch.sqrt(power / 10.0 ** (snr / 10.0))[:, None]                       # OFDM.c:645-651
        n = st.shape[0]
        if noise == "real":
            g = torch.randn((n, L), generator=generator, device=dev, dtype=torch.float32)
            nz = torch.complex(g * sigma.float(), torch.zeros_like(g))
        else:
            g = torch.randn((n, L, 2), generator=generator, device=dev, dtype=torch.float32)
            nz = torch.view_as_complex((g * (sigma.float() * (0.5 ** 0.5))[..., None]).contiguous())
        caps = caps + nz
    return caps.contiguous()


def make_stream(wave, segments, snr_db, cfo_hz=0.0, taps=None, noise: str = "real", generator=None):
    """One recording (complex64 [n], on wave's device) for Engine.receive_stream: idle gaps and slices of the repeated
    waveform `wave` (complex64 [len]) laid end to end, then make_captures' impairments 1 to 3 over the whole of it.

    segments: a sequence of ("gap", n) -- n zero samples -- and ("wave", lo, hi) -- samples [lo, hi) of the waveform
    repeated without end (index modulo its length), 0 <= lo <= hi.  The multipath FIR runs over the laid-out stream
    truncated to its length, the rotation exp(j 2 pi cfo_hz k 25e-9) goes by the stream index k, and the noise (power
    mean|wave|^2 / 10^(snr_db / 10), measured on `wave`) covers gaps and packets alike.  snr_db and cfo_hz are
    scalars.  A stream that is one whole `wave` equals make_captures(wave, 0, ..., cap_len=len(wave))[0], noise
    included when the generators start alike."""
    torch = _torch()
    if noise not in NOISE_KINDS:
        raise ValueError(f"noise must be one of {NOISE_KINDS}, got {noise!r}")
    wave = torch.as_tensor(wave)
    if wave.dim() != 1 or not wave.is_complex() or wave.shape[0] == 0:
        raise ValueError("wave must be a non-empty one-dimensional complex tensor")
    wave = wave.to(torch.complex64)
    dev, wl = wave.device, int(wave.shape[0])
    parts = []
    for seg in segments:
        kind = seg[0] if len(seg) else None
        if kind == "gap" and len(seg) == 2 and int(seg[1]) >= 0:
            parts.append(torch.zeros(int(seg[1]), dtype=torch.complex64, device=dev))
        elif kind == "wave" and len(seg) == 3 and 0 <= int(seg[1]) <= int(seg[2]):
            parts.append(wave[torch.arange(int(seg[1]), int(seg[2]), device=dev, dtype=torch.int64) % wl])
        else:
            raise ValueError(f"a segment is ('gap', n >= 0) or ('wave', lo, hi) with 0 <= lo <= hi, got {seg!r}")
    x = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.complex64, device=dev)
    power = float(torch.mean(wave.real.double() ** 2 + wave.imag.double() ** 2))        # OFDM.c:637-643
    return impair_stream(x, power, snr_db, cfo_hz, taps=taps, noise=noise, generator=generator)


def impair_stream(x, power: float, snr_db, cfo_hz=0.0, taps=None, noise: str = "real", generator=None):
    """make_stream's impairments over a recording `x` (complex64 [n]) that is already laid out -- by make_stream, or by
    Engine.transmit_packets: the multipath FIR truncated to the recording's length, the rotation
    exp(j 2 pi cfo_hz k 25e-9) by the stream index k, then noise of variance power / 10^(snr_db / 10) over gaps and
    packets alike ("real": all of it in the real part, "complex": split across both axes, "none": nothing).  x is not
    written; the result is on x's device (x itself when nothing applies)."""
    torch = _torch()
    if noise not in NOISE_KINDS:
        raise ValueError(f"noise must be one of {NOISE_KINDS}, got {noise!r}")
    if not torch.is_tensor(x) or x.dim() != 1 or x.dtype != torch.complex64:
        raise ValueError("x must be a one-dimensional complex64 tensor")
    dev, n = x.device, int(x.shape[0])
    y = x
    if taps is not None:
        h = np.asarray(taps, np.complex64).ravel()
        y = torch.zeros_like(x)
        for j, hj in enumerate(h):
            if hj != 0 and j < n:
                y[j:] += complex(hj) * x[:n - j]
    if float(cfo_hz) != 0.0:
        k = torch.arange(n, device=dev, dtype=torch.int64)
        rev = float(cfo_hz) * k.double() * TS_OVERSAMPLED
        ang = (2.0 * np.pi) * (rev - torch.round(rev))
        y = y * torch.complex(torch.cos(ang), torch.sin(ang)).to(torch.complex64)
    if noise != "none":
        sigma = torch.sqrt(torch.as_tensor(power / 10.0 ** (float(snr_db) / 10.0), dtype=torch.float64, device=dev)).float()
        if noise == "real":
            g = torch.randn((1, n), generator=generator, device=dev, dtype=torch.float32)[0]
            nz = torch.complex(g * sigma, torch.zeros_like(g))
        else:
            g = torch.randn((1, n, 2), generator=generator, device=dev, dtype=torch.float32)[0]
            nz = torch.view_as_complex((g * (sigma * (0.5 ** 0.5))).contiguous())
        y = y + nz
    return y.contiguous()


def parse_taps(text: str) -> np.ndarray:
    """'1,0,0.4+0.3j' -> complex64 taps"""
    return np.array([complex(t.strip()) for t in text.split(",") if t.strip()], np.complex64)


FADE_MAX_TAPS = 32            # OFDM_FADE_MAX_TAPS (include/ofdm_mi355x_fading.h)


def parse_pdp(text: str) -> np.ndarray:
    """'1,0.5,0.25,0.125' -> the power delay profile of Engine.draw_taps: float64 linear powers, one per 25 ns tap,
    normalised to sum 1.  At most 32 entries, each finite and not negative, not all zero."""
    try:
        p = np.array([float(t) for t in text.split(",") if t.strip()], np.float64)
    except ValueError:
        raise ValueError(f"a power delay profile is comma-separated linear powers, got {text!r}") from None
    if not 1 <= len(p) <= FADE_MAX_TAPS:
        raise ValueError(f"a power delay profile has 1 to {FADE_MAX_TAPS} taps, got {len(p)}")
    if not np.isfinite(p).all() or (p < 0).any() or p.sum() <= 0:
        raise ValueError(f"powers must be finite, not negative and not all zero, got {text!r}")
    return p / p.sum()


def fade_packets(packets, taps) -> np.ndarray:
    """Engine.transmit_faded's rule in numpy fp64 (as stream.select_packets is for detection): packets complex [n, P]
    and taps complex [n, L] -> complex128 [n, P + L - 1], row k the full convolution of packet k with its taps."""
    x = np.asarray(packets, np.complex128)
    h = np.asarray(taps, np.complex128)
    if x.ndim != 2 or h.ndim != 2 or len(x) != len(h) or h.shape[1] < 1:
        raise ValueError(f"packets [n, P] and taps [n, L >= 1] are required, got {x.shape} and {h.shape}")
    out = np.zeros((len(x), x.shape[1] + h.shape[1] - 1), np.complex128)
    for l in range(h.shape[1]):
        out[:, l:l + x.shape[1]] += h[:, l, None] * x
    return out


__all__ = ["make_captures", "make_stream", "impair_stream", "parse_taps", "parse_pdp", "fade_packets", "TS_OVERSAMPLED"]
