"""What lets the packed AWGN receivers take the truth signs from the clean spectra (demap_bin, ofdm_rxpack.hip): at
every data bin of every symbol ofdm_tx_frames builds, the receiver's spectrum FFT((-1)^n window) is a QPSK point
(+-1 +-j) / sqrt2 times the bin's constant sign cs ((-1)^k in the C convention, +1 in MATLAB's), so each component's
sign bit is far from ambiguous, and sign x cs is the bit the pair-order truth words (rows 7..9) carry."""
import numpy as np
import pytest

from test_gpu_symbol import PAIR_BINS

pytestmark = pytest.mark.gpu

N_SYM = 600


@pytest.mark.parametrize("payload", ["random", "message"])
@pytest.mark.parametrize("conv", ["c", "matlab"])
def test_clean_spectrum_signs_are_the_truth_words(engine, pkg, conv, payload):
    cfg = pkg.make_cfg(conv=conv, payload=payload)
    tx, bits = engine.tx_frames(cfg, 123456789, N_SYM // 2)
    pitch = tx.numel() // 80
    win = tx.view(80, pitch)[16:80, :N_SYM].cpu().numpy().astype(np.complex128)        # (64 samples, symbols)
    words = bits.view(10, pitch)[7:10, :N_SYM].cpu().numpy().astype(np.uint32)          # (3 words, symbols)
    X = np.fft.fft(win * ((-1.0) ** np.arange(64))[:, None], axis=0)
    seen = 0
    for p, k in enumerate(PAIR_BINS):
        for h, b in enumerate((k, 64 - k)):
            cs = -1.0 if conv == "c" and (b & 1) else 1.0
            re, im = X[b].real, X[b].imag
            assert np.all(np.abs(np.abs(re) - 0.70711) < 1e-3), (b, np.abs(re).min(), np.abs(re).max())
            assert np.all(np.abs(np.abs(im) - 0.70711) < 1e-3), (b, np.abs(im).min(), np.abs(im).max())
            pos = 31 - 4 * (p & 7) - 2 * h                       # (b0, b0 ^ b1) MSB first: im sign, then re sign
            ti = (words[p >> 3] >> pos) & 1
            tr = (words[p >> 3] >> (pos - 1)) & 1
            assert np.array_equal((im * cs < 0).astype(np.uint32), ti), b
            assert np.array_equal((re * cs < 0).astype(np.uint32), tr), b
            seen += 1
    assert seen == 48
    assert len({int(w) for w in words[0]}) > (100 if payload == "random" else 1)       # the symbols differ
