"""The folded Philox form of the LS AWGN packed receiver is Philox4x32-10 (no GPU).

rx_pack_kernel draws block index b of frame f at SNR index q as philox10(lo(f), hi(f), b, STREAM_NOISE | q; key)
(DESIGN.md §3), computed from four parts (ofdm_device.h):
  * the table words (x, y, z) of (hi(f), b, key)                 philox_words, once per launch and row;
  * the staged pair of (lo(f), b), which takes y and key word 0  philox_qword, once per item and lane;
  * the per-(f, q) pair                                          philox_head / philox_mid, once per SNR iteration;
  * rounds 4..10 on the joined state                             philox10_c2(mid, x, z, q.x, q.y).
This file restates the four parts in numpy next to a plain ten-round Philox and compares them over random seeds,
frame indices on both sides of 2^32, all 48 block indices of pack_block and SNR indices 0..63.  The plain Philox is
itself compared with the oracle's.  It pins the derivation; tests/test_gpu_pack_qwords.py and the goldens of
tests/test_gpu_pack_exact.py pin the kernel."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_NOISE = 0x5A000000
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def u(x):
    return np.asarray(x, dtype=np.uint64) & MASK


def mulhilo(m, c):
    p = m * u(c)                      # < 2^64: no wrap
    return p >> S32, p & MASK


def philox10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (u(v) for v in np.broadcast_arrays(c0, c1, c2, c3))
    for r in range(10):
        h0, l0 = mulhilo(M0, c0)
        h1, l1 = mulhilo(M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ u(k0 + r * W0), l1, h0 ^ c3 ^ u(k1 + r * W1), l0
    return c0, c1, c2, c3


def pack_block(slot):                 # ofdm_internal.h
    return 48 + slot if slot < 16 else 84 + (slot - 16) if slot < 32 else 104 + (slot - 32)


def philox_words(c1, c2, k0, k1):
    h1, l1 = mulhilo(M1, c2)
    h0, l0 = mulhilo(M0, h1 ^ u(c1) ^ u(k0))
    return l1 ^ u(k0 + W0), h0 ^ u(k1 + W1), l0 ^ u(k1 + 2 * W1)


def philox_qword(c0, wy, k0):
    _, l0 = mulhilo(M0, c0)
    h1, l1 = mulhilo(M1, l0 ^ wy)
    return h1 ^ u(k0 + 2 * W0), l1


def philox_mid(c0, c3, k1):           # philox_head, then philox_mid: (p1lo, p1hi)
    h0, _ = mulhilo(M0, c0)
    h1, l1 = mulhilo(M1, h0 ^ u(c3) ^ u(k1))
    return l1, h1


def folded(mid, wx, wz, qx, qy, k0, k1):
    p1lo, p1hi = mid
    h0, l0 = mulhilo(M0, p1hi ^ wx)
    c0, c1, c2, c3 = qx ^ p1lo, qy, h0 ^ wz, l0
    for r in range(3, 10):
        h0, l0 = mulhilo(M0, c0)
        h1, l1 = mulhilo(M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ u(k0 + r * W0), l1, h0 ^ c3 ^ u(k1 + r * W1), l0
    return c0, c1, c2, c3


def test_numpy_philox_is_the_oracles(oracle):
    rng = np.random.default_rng(3)
    for _ in range(8):
        ctr = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        key = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        got = [int(v) for v in philox10(*ctr, *key)]
        assert got == [int(v) for v in oracle.philox(ctr, key)]


def test_folded_form_is_philox():
    rng = np.random.default_rng(20)
    edge = [2 ** 32 - 65, 2 ** 32 - 64, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 63, 2 ** 33 - 1, 2 ** 33,
            0, 1, 63, 64]
    blocks = np.array([pack_block(s) for s in range(48)], dtype=np.uint64)
    assert len(set(blocks.tolist())) == 48 and blocks.min() == 48 and blocks.max() == 119
    q = np.arange(64, dtype=np.uint64)
    for _ in range(6):
        k0, k1 = (int(v) for v in rng.integers(0, 2 ** 32, 2))
        frames = np.array(edge + [int(v) for v in rng.integers(0, 2 ** 63, 12)], dtype=np.uint64)
        flo, fhi = (frames & MASK)[:, None, None], (frames >> S32)[:, None, None]
        b = blocks[None, :, None]
        c3 = (np.uint64(STREAM_NOISE) | q)[None, None, :]
        want = philox10(flo, fhi, b, c3, k0, k1)
        wx, wy, wz = philox_words(fhi, b, k0, k1)              # per (frame high word, block index)
        qx, qy = philox_qword(flo, wy, k0)                      # per (frame, block index): no SNR index in it
        assert qx.shape == (len(frames), 48, 1)
        got = folded(philox_mid(flo, c3, k1), wx, wz, qx, qy, k0, k1)
        for g, w in zip(got, want):
            assert g.shape == (len(frames), 48, 64) and np.array_equal(g, w)
