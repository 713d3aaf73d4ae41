"""The per-packet fading transmitter on the GPU (include/ofdm_mi355x_fading.h, Engine.transmit_faded and
Engine.draw_taps, csrc/ofdm_fading.hip): every faded packet against the channel kernel bit for bit, launch-shape
invariance, placement, accumulate mode, gain and carrier offset against fp64 numpy, the oracle's Transmitter() convolved
in fp64, the drawn taps against the oracle's Gaussians, the argument errors, the loopback through
Engine.receive_stream, and the link command.

The shapes: n = 67 packets (and 1) of D in {1, 2, 7, 15} data symbols -- at D = 1 the batch crosses a group boundary at
62 packets, D = 15 is the longest packet with 4 per group -- through L in {1, 2, 4, 5, 32} taps: no history, either
side of the four-sample register window, and the cap.  Payload bits are random, caller taps random complex64 x 0.25."""
import csv
import ctypes as C

import numpy as np
import pytest

import fading_ref as ref
from conftest import normwise
from fading_ref import DS, EDGE_PACKETS, LS, N, same_bits
from test_gpu_transmit import CFO_DEV_MEASURED

pytestmark = pytest.mark.gpu

TS = 25e-9
SENTINEL = np.complex64(12345.678 - 9876.5j)
GRID = [("c", d, L) for d in DS for L in LS] + [("matlab", 2, L) for L in LS]
EVERY_PACKET = {("c", 1, 4), ("c", 15, 32)}

# Test 7, measured on the MI355X: the largest normwise deviation (largest |difference| over the largest |tap| of the
# batch) of 67 packets' drawn taps from the same stream built in fp64 from the oracle's Gaussians was 9.06e-8 (four
# taps of power 1/4 at index0 11; 6.6e-8 .. 8.5e-8 for L = 3, 4 and 32 at index0 0, 2^32 - 30 and 2^40 + 7).  Asserted at
# 4 x, and it must stay below 1e-3: the share of the noise scale that the channel test's 1e-5 bound allows the same
# hardware logarithm and sine.  It is a deviation from the fp64 oracle, never from the kernel.
DRAW_DEV_MEASURED = 9.06e-8


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch(eng, pkg):
    """(conv, D, L) -> (words [67, 3 D], taps [67, L], the 67 faded packets of the dense store-mode batch), built on
    first use and left unchanged"""
    cache = {}

    def get(conv, d, L):
        if (conv, d, L) not in cache:
            words, taps = ref.rand_words(d, N, 0xFA00 + d), ref.rand_taps(N, L, 0xFB00 + 64 * d + L)
            rec = eng.transmit_faded(words, d, taps, conv=conv).cpu().numpy()
            assert rec.shape == (N * pkg.abi.faded_len(d, L),)
            cache[conv, d, L] = (words, taps, rec.reshape(N, -1))
        return cache[conv, d, L]
    return get


def through_the_channel_kernel(eng, words_k, d, taps_k, conv):
    """the packet alone from transmit_packets, L - 1 zeros appended, through impair_stream with its taps"""
    w = eng.transmit_packets(words_k[None], d, conv=conv).cpu().numpy()
    x = np.concatenate([w, np.zeros(len(taps_k) - 1, np.complex64)])
    return eng.impair_stream(x, 1.0, 10.0, taps=taps_k, noise="none").cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. the channel kernel's bits
@pytest.mark.parametrize("conv,d,L", GRID)
def test_faded_packets_are_the_channel_kernels_bit_for_bit(eng, pkg, batch, conv, d, L):
    words, taps, pk = batch(conv, d, L)
    assert pk.shape[1] == pkg.abi.packet_len(d) + L - 1
    for k in (range(N) if (conv, d, L) in EVERY_PACKET else EDGE_PACKETS):
        assert same_bits(pk[k], through_the_channel_kernel(eng, words[k], d, taps[k], conv)), k
    if L == 1:
        # one tap of exactly one leaves the transmitter's packet
        plain = eng.transmit_packets(words[:3], d, conv=conv).cpu().numpy()
        got = eng.transmit_faded(words[:3], d, np.ones((3, 1), np.complex64), conv=conv).cpu().numpy()
        assert np.array_equal(got, plain)


# ------------------------------------------------------------------------------------------- 2. launch shape
@pytest.mark.parametrize("conv,d,L", GRID)
def test_a_faded_packet_does_not_depend_on_the_launch_shape(eng, pkg, batch, conv, d, L):
    import torch
    words, taps, pk = batch(conv, d, L)
    plen = pkg.abi.faded_len(d, L)
    for k in EDGE_PACKETS:
        alone = eng.transmit_faded(words[k:k + 1], d, taps[k:k + 1], conv=conv).cpu().numpy()
        assert same_bits(alone, pk[k]), k
    acc = eng.transmit_faded(words, d, taps, accumulate=True, conv=conv).cpu().numpy()            # onto zeros
    assert same_bits(acc, pk.ravel())
    one = eng.transmit_faded(words[66:], d, taps[66:], out=torch.zeros(plen, dtype=torch.complex64, device="cuda"),
                             accumulate=True, conv=conv).cpu().numpy()
    assert same_bits(one, pk[66])


# ------------------------------------------------------------------------------------------- 3. placement
def placed(n_out, positions, packets, base):
    exp = base.copy()
    for p, w in zip(positions, packets):
        lo, hi = max(int(p), 0), min(int(p) + len(w), n_out)
        if lo < hi:
            exp[lo:hi] = w[lo - int(p):hi - int(p)]
    return exp


@pytest.mark.parametrize("d,L", [(1, 5), (2, 32), (7, 2), (15, 4), (2, 1), (15, 32)])
def test_placement_tail_and_untouched_samples(eng, pkg, batch, d, L):
    import torch
    words, taps, pk = batch("c", d, L)
    plen = pkg.abi.faded_len(d, L)
    n_out = 5 * plen + 1001
    # cut at the start, cut at the end, nothing written (twice), then descending, odd (8-byte aligned only) and even
    pos = np.array([-300, n_out - 100, -plen, n_out, 3 * plen + 701, 2 * plen + 412, plen + 101], np.int64)
    out = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    got = eng.transmit_faded(words[:len(pos)], d, taps[:len(pos)], positions=pos, out=out)
    assert got is out
    exp = placed(n_out, pos, pk, np.full(n_out, SENTINEL, np.complex64))
    res = out.cpu().numpy()
    assert same_bits(res, exp)
    assert (exp == SENTINEL).sum() == n_out - (plen - 300) - 100 - 3 * plen
    for p in pos[4:]:
        # the L - 1 tail samples are written, the sample behind them and the one in front of the packet are not
        assert (res[p + plen - L:p + plen] != SENTINEL).all() and res[p + plen] == SENTINEL and res[p - 1] == SENTINEL
    # pos0 and stride: all 67 packets, the first cut at the start, the last ones cut or outside at the end
    stride = plen + 13
    n_out = 60 * stride + 55
    out = torch.full((n_out,), complex(SENTINEL), dtype=torch.complex64, device="cuda")
    eng.transmit_faded(torch.from_numpy(words.view(np.int32)).cuda(), d, torch.from_numpy(taps).cuda(), pos0=-300,
                       stride=stride, out=out)
    exp = placed(n_out, -300 + stride * np.arange(N), pk, np.full(n_out, SENTINEL, np.complex64))
    assert same_bits(out.cpu().numpy(), exp)
    assert (exp[plen - 300:stride - 300] == SENTINEL).all() and exp[n_out - 1] != SENTINEL
    # an empty batch and an empty recording launch nothing and touch nothing
    eng.transmit_faded(words[:0], d, taps[:0], out=out)
    assert same_bits(out.cpu().numpy(), exp)
    assert eng.transmit_faded(words, d, taps, n_out=0).shape == (0,)


# ------------------------------------------------------------------------------------------- 4. accumulate
@pytest.mark.parametrize("d,L", [(1, 5), (2, 32), (7, 2), (15, 4), (2, 1), (15, 32)])
def test_accumulate_composes_two_faded_packets(eng, pkg, batch, d, L):
    words, taps, pk = batch("c", d, L)
    plen = pkg.abi.faded_len(d, L)
    pos = np.array([101, 101 + plen - 500], np.int64)            # two packets overlapping by 500 samples
    n_out = 2 * plen
    got = eng.transmit_faded(words[5:7], d, taps[5:7], positions=pos, n_out=n_out, accumulate=True).cpu().numpy()
    exp = np.zeros(n_out, np.complex64)
    for p, w in zip(pos, pk[5:7]):
        exp[p:p + plen] += w                                      # fp32, per component; two addends on a zero base
    assert np.array_equal(got, exp)
    assert np.abs(exp[pos[1]:pos[0] + plen]).min() > 0 and len(exp[pos[1]:pos[0] + plen]) == 500


# ------------------------------------------------------------------------------------------- 5. gain and carrier offset
def test_gain_and_carrier_offset_against_fp64(eng, pkg, batch):
    cfos = np.array([-60e3, 25e3, 1e6], np.float32)
    gains = np.array([0.5j, -0.8 + 0.3j, 2], np.complex64)
    rot = lambda f, n: np.exp(2j * np.pi * f * np.arange(n) * TS)
    worst = 0.0
    for d in (2, 15):
        words, taps, pk = batch("c", d, 4)
        plen = pk.shape[1]
        for accumulate in (False, True):
            got = eng.transmit_faded(words[:3], d, taps[:3], cfo_hz=cfos, accumulate=accumulate).cpu().numpy().reshape(3, -1)
            for k, f in enumerate(cfos):
                # the phase counts from the packet's first sample and runs through the L - 1 tail samples
                dev = normwise(got[k], pk[k].astype(np.complex128) * rot(float(f), plen))
                print(f"faded carrier offset D {d} f {float(f):.0f} Hz accumulate {accumulate}: normwise {dev:.3g}")
                worst = max(worst, dev)
        # gain alone: two fp32 roundings per component and their sum, as the transmitter's gain test
        got = eng.transmit_faded(words[:3], d, taps[:3], gains=gains).cpu().numpy().reshape(3, -1)
        for k, g in enumerate(gains):
            v = pk[k].astype(np.complex128)
            assert np.abs(got[k] - complex(g) * v).max() <= 4 * 2.0 ** -23 * abs(complex(g)) * np.abs(v).max(), (k, g)
        # both: the product g exp(..) is rounded to fp32 once (at most 2^-23 of |g| per component, the gain bound
        # again) on top of the phasor's own deviation
        got = eng.transmit_faded(words[:3], d, taps[:3], gains=gains, cfo_hz=cfos).cpu().numpy().reshape(3, -1)
        for k, (g, f) in enumerate(zip(gains, cfos)):
            dev = normwise(got[k], complex(g) * pk[k].astype(np.complex128) * rot(float(f), plen))
            print(f"faded gain and carrier offset D {d} packet {k}: normwise {dev:.3g}")
            assert dev <= 4 * CFO_DEV_MEASURED + 8 * 2.0 ** -23
        # an offset of zero and a gain of one change nothing; a far position does not move the phase
        zero = eng.transmit_faded(words[:2], d, taps[:2], cfo_hz=np.zeros(2, np.float32),
                                  gains=np.ones(2, np.complex64)).cpu().numpy().reshape(2, -1)
        assert same_bits(zero, pk[:2])
        near = eng.transmit_faded(words[:3], d, taps[:3], cfo_hz=cfos).cpu().numpy().reshape(3, -1)
        far = eng.transmit_faded(words[:3], d, taps[:3], cfo_hz=cfos, pos0=12345, stride=5000).cpu().numpy()
        assert same_bits(far[12345 + 2 * 5000:][:plen], near[2])
    print(f"faded carrier offset: worst normwise {worst:.3g}")
    assert worst <= 4 * CFO_DEV_MEASURED


# ------------------------------------------------------------------------------------------- 6. the oracle in fp64
@pytest.mark.parametrize("conv,d,L", GRID)
def test_faded_packets_against_the_oracle_in_fp64(eng, oracle, pkg, batch, conv, d, L):
    from ofdm_amd.channel import fade_packets
    words, taps, pk = batch(conv, d, L)
    bits = ref.bits_of(words)
    worst, worst_abs = 0.0, 0.0
    for k in EDGE_PACKETS:
        w = oracle.frame_waveform(bits[k], conv, True, 1)
        want = np.convolve(w, taps[k].astype(np.complex128))
        assert np.abs(fade_packets(w[None], taps[k:k + 1])[0] - want).max() <= 1e-12 * np.abs(want).max()
        # 2e-6: the bound the transmitter's parity test asserts on w; then the gamma-bound of a 2 L-term fma dot product
        bound = np.abs(taps[k].astype(np.complex128)).sum() * np.abs(w).max() * (2e-6 + (2 * L + 2) * 2.0 ** -24 * np.sqrt(2))
        err = max(np.abs(pk[k].real - want.real).max(), np.abs(pk[k].imag - want.imag).max())
        worst, worst_abs = max(worst, err / bound), max(worst_abs, err)
        assert err <= bound, (k, err, bound)
    print(f"faded against the oracle conv {conv} D {d} L {L}: largest component error {worst_abs:.3g}, {worst:.3g} of the bound")


# ------------------------------------------------------------------------------------------- 7. drawn taps
@pytest.mark.parametrize("L", [3, 32])
def test_drawn_taps_are_a_function_of_the_packet_index(eng, L):
    pdp = np.linspace(1.0, 0.1, L) / L
    for a in (5, 2 ** 32 - 30):                                   # the second batch crosses the counter's low word
        whole = eng.draw_taps(a % 1000 + N, pdp, seed=ref.SEED, index0=a - a % 1000).cpu().numpy()
        part = eng.draw_taps(N, pdp, seed=ref.SEED, index0=a).cpu().numpy()
        assert whole.shape == (a % 1000 + N, L) and same_bits(part, whole[a % 1000:])
    one = eng.draw_taps(1, pdp, seed=ref.SEED, index0=5 + 66).cpu().numpy()
    assert same_bits(one, eng.draw_taps(N, pdp, seed=ref.SEED, index0=5).cpu().numpy()[66:])
    other = eng.draw_taps(N, pdp, seed=ref.SEED + 1, index0=5).cpu().numpy()
    assert not same_bits(other, eng.draw_taps(N, pdp, seed=ref.SEED, index0=5).cpu().numpy())
    # a tap of zero power is exactly zero, and its neighbours are what they were
    p0 = pdp.copy()
    p0[1] = 0.0
    z = eng.draw_taps(N, p0, seed=ref.SEED, index0=5).cpu().numpy()
    full = eng.draw_taps(N, pdp, seed=ref.SEED, index0=5).cpu().numpy()
    assert not z[:, 1].any() and same_bits(np.delete(z, 1, 1), np.delete(full, 1, 1))


def test_drawn_taps_against_the_oracles_gaussians(eng, oracle):
    worst = 0.0
    for L, index0 in ((3, 0), (32, 0), (4, 2 ** 32 - 30), (32, 2 ** 40 + 7)):
        pdp = (np.exp(-np.arange(L) / 4.0) / np.exp(-np.arange(L) / 4.0).sum()).astype(np.float32)
        got = eng.draw_taps(N, pdp, seed=ref.SEED, index0=index0).cpu().numpy()
        want = ref.taps64(oracle, ref.SEED, index0, N, pdp)
        dev = normwise(got, want)
        print(f"drawn taps L {L} index0 {index0}: normwise {dev:.3g} (largest tap {np.abs(want).max():.3g})")
        worst = max(worst, dev)
    # symbol mode's channel: four taps of power 1/4, amplitude sqrt(1/8)
    got = eng.draw_taps(N, [0.25] * 4, seed=ref.SEED, index0=11).cpu().numpy()
    want = ref.taps64(oracle, ref.SEED, 11, N, [0.25] * 4)
    worst = max(worst, normwise(got, want))
    print(f"drawn taps: worst normwise {worst:.3g}")
    assert worst < 1e-3
    assert worst <= 4 * DRAW_DEV_MEASURED


def test_drawn_taps_have_the_profiles_power(eng):
    n, pdp = 65536, np.array([0.5, 0.25, 0.15, 0.1])
    h = eng.draw_taps(n, pdp, seed=ref.SEED).cpu().numpy().astype(np.complex128)
    mean = (np.abs(h) ** 2).mean(0)
    print(f"drawn taps mean power {mean.tolist()} against {pdp.tolist()}")
    # |h|^2 is exponential: its relative standard error over n packets is 1 / sqrt(n)
    assert (np.abs(mean - pdp) <= 5 / np.sqrt(n) * pdp).all()
    assert np.abs(h.mean(0)).max() <= 5 * np.sqrt(pdp.max() / n)


# ------------------------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_come_before_any_launch(eng, pkg):
    import torch
    abi, lib = pkg.abi, eng.lib
    d, n, L = 2, 3, 4
    words = torch.from_numpy(ref.rand_words(d, n, 7).view(np.int32)).cuda()
    taps = torch.from_numpy(ref.rand_taps(n, L, 8)).cuda()
    plen = abi.faded_len(d, L)
    n_out = n * plen
    out = torch.zeros(n_out + 1, dtype=torch.complex64, device="cuda")
    drawn = torch.zeros((n, L), dtype=torch.complex64, device="cuda")
    ok = abi.TxOpts(0, 1, d, 0)
    W, O, T, H = (C.c_void_p(t.data_ptr()) for t in (words, out, taps, drawn))
    pdp_ok = (C.c_float * L)(0.4, 0.3, 0.2, 0.1)

    def call(ctx=eng.ctx, opts=ok, w=W, nn=n, t=T, nt=L, o=O, no=n_out):
        return lib.ofdm_transmit_faded(ctx, None if opts is None else C.byref(opts), w, nn, None, 0, plen, None, None, t,
                                       nt, o, no)

    def draw(ctx=eng.ctx, nn=n, nt=L, pdp=pdp_ok, h=H):
        return lib.ofdm_draw_taps(ctx, ref.SEED, 0, nn, nt, pdp, h)

    eng.timing(True)
    try:
        eng.timing_reset()
        launches = lambda: (eng.timing_query(abi.K_FADE)[1], eng.timing_query(abi.K_DRAW_TAPS)[1])
        before = launches()
        bad = [dict(ctx=None), dict(opts=None), dict(w=None), dict(o=None), dict(nn=-1), dict(no=-1),
               dict(opts=abi.TxOpts(0, 1, 0, 0)), dict(opts=abi.TxOpts(0, 1, 16, 0)), dict(opts=abi.TxOpts(2, 1, d, 0)),
               dict(opts=abi.TxOpts(-1, 1, d, 0)), dict(opts=abi.TxOpts(0, 1, d, 2)), dict(opts=abi.TxOpts(0, 1, d, 3)),
               dict(o=C.c_void_p(out.data_ptr() + 4)),
               dict(t=None), dict(nt=0), dict(nt=33), dict(nt=-1), dict(t=C.c_void_p(taps.data_ptr() + 4))]
        for kw in bad:
            assert call(**kw) == -1, kw
            assert len(lib.ofdm_last_error()) > 0, kw
        bad_draw = [dict(ctx=None), dict(nn=-1), dict(nt=0), dict(nt=33), dict(pdp=None), dict(h=None),
                    dict(pdp=(C.c_float * L)(0.4, -0.1, 0.2, 0.1)), dict(pdp=(C.c_float * L)(0.4, float("nan"), 0.2, 0.1)),
                    dict(pdp=(C.c_float * L)(0.4, 0.3, float("inf"), 0.1)), dict(h=C.c_void_p(drawn.data_ptr() + 4))]
        for kw in bad_draw:
            assert draw(**kw) == -1, kw
            assert len(lib.ofdm_last_error()) > 0, kw
        assert launches() == before
        assert not out.abs().any() and not drawn.abs().any()
        # nothing to do is no error and no launch; NULL buffers are fine then
        assert call(w=None, t=None, nn=0) == 0 and call(o=None, no=0) == 0 and draw(nn=0, h=None) == 0
        assert launches() == before
        assert call() == 0 and call(opts=abi.TxOpts(1, 0, d, 1)) == 0
        assert call(o=C.c_void_p(out.data_ptr() + 8)) == 0                       # 8-byte alignment is enough
        assert draw() == 0
        assert launches() == (before[0] + 3, before[1] + 1)                      # one launch per call
    finally:
        eng.timing(False)
    # the Python layer refuses malformed inputs itself
    w_np, t_np = ref.rand_words(d, n, 7), ref.rand_taps(n, L, 8)
    for kw in (dict(taps=None), dict(taps=t_np.astype(np.complex128)), dict(taps=t_np[:2]), dict(taps=t_np.ravel()),
               dict(taps=np.zeros((n, 33), np.complex64)), dict(taps=np.zeros((n, 0), np.complex64)),
               dict(taps=torch.from_numpy(t_np)), dict(taps=taps.t().contiguous().t()),
               dict(words=w_np[:, :5]), dict(n_data=16), dict(conv="x"), dict(gains=np.ones(n, np.complex128)),
               dict(out=out, n_out=5), dict(positions=torch.zeros(n, dtype=torch.int64, device="cuda"))):
        args = dict(words=w_np, n_data=d, taps=t_np)
        args.update(kw)
        with pytest.raises(ValueError):
            eng.transmit_faded(**args)
    for kw in (dict(n=-1), dict(pdp=[]), dict(pdp=[1.0] * 33), dict(pdp=[0.5, -0.5]), dict(pdp=[float("nan")]),
               dict(seed=-1), dict(index0=1 << 64), dict(out=torch.zeros((n, 3), dtype=torch.complex64, device="cuda"))):
        args = dict(n=n, pdp=[0.4, 0.3, 0.2, 0.1])
        args.update(kw)
        with pytest.raises(ValueError):
            eng.draw_taps(**args)


# ------------------------------------------------------------------------------------------- 9. loopback
@pytest.mark.parametrize("d", [2, 15])
@pytest.mark.parametrize("channel", ["flat", "profile"])
def test_loopback_through_the_stream_receiver(eng, pkg, d, channel):
    from ofdm_amd.stream import pack_messages
    rng = np.random.default_rng(0xFADE + d)
    texts = ["".join(chr(c) for c in rng.integers(33, 127, 12 * d)) for _ in range(5)]
    assert len(set(texts)) == 5
    words, dd = pack_messages(texts)
    assert dd == d
    if channel == "flat":
        taps = eng.draw_taps(5, [1.0], seed=ref.SEED)             # flat Rayleigh, one CN(0, 1) tap per packet
    else:
        taps = (ref.LOOP_GAINS[:, None] * ref.LOOP_PROFILE[None, :]).astype(np.complex64)
    L = int(taps.shape[1])
    plen = pkg.abi.faded_len(d, L)
    pos = np.cumsum(ref.LOOP_GAPS) + plen * np.arange(5)
    n_out = int(pos[-1]) + plen + 400
    rec = eng.transmit_faded(words, d, taps, positions=pos.astype(np.int64), n_out=n_out)
    assert eng.set_long_message(texts[2]) == d                   # any text of the same D
    a = eng.receive_stream(rec)
    off = np.asarray(a["positions"]) - pos[:len(a["positions"])] if a["count"] == 5 else None
    print(f"faded loopback D {d} {channel}: found {a['found']}, offsets {None if off is None else off.tolist()}, "
          f"|h0| {np.abs(taps.cpu().numpy() if hasattr(taps, 'cpu') else taps)[:, 0].tolist()}")
    assert a["count"] == a["found"] == 5
    assert ((off >= 8) & (off <= 40 + L - 1)).all(), off          # link_sweep's grown scoring window
    assert a["messages"] == texts


# ------------------------------------------------------------------------------------------- 10. the link command
@pytest.mark.parametrize("pdp", ["1", "1,0.5,0.25,0.125"])
def test_link_command_in_process(pkg, tmp_path, pdp):
    from ofdm_amd import sweep
    from ofdm_amd.channel import parse_pdp
    from ofdm_amd.fileio import read_float_array_file
    from ofdm_amd.stream import score_packets
    out = tmp_path / "link"
    assert sweep.link_main(["--packets", "12", "--n-data", "2", "--pdp", pdp, "--snr", "25:40:15", "--noise", "complex",
                            "--out", str(out)]) == 0
    assert read_float_array_file(out / "Output_SNR.txt").tolist() == [25.0, 40.0]
    ber = read_float_array_file(out / "Output_BER.txt")
    rows = list(csv.reader(open(out / "link.csv")))
    assert tuple(rows[0]) == sweep.LINK_COLUMNS and len(rows) == 3
    for k, row in enumerate(rows[1:]):
        snr, tx, matched, missed, fa, perr, berr, bits = (float(v) for v in row)
        print(f"faded link pdp {pdp} {snr:g} dB: matched {matched:g} missed {missed:g} false alarms {fa:g} "
              f"packet_err {perr:g} bit_err {berr:g} of {bits:g}")
        assert snr == (25.0, 40.0)[k] and tx == 12 and matched + missed == 12 and fa >= 0
        assert bits == 192 * matched and perr <= matched and berr <= bits
        assert abs(ber[k] - berr / max(bits, 1)) <= 5e-3 * max(ber[k], 1e-30) + 1e-12      # the file holds '%.2e'
    # the same sweep through the library calls, scored on the host
    p = parse_pdp(pdp)
    L, gap = len(p), 500
    words = np.random.default_rng(0x80211A).integers(0, 1 << 32, (12, 6), dtype=np.uint64).astype(np.uint32)
    with pkg.Engine(0) as e:
        res = sweep.link_sweep(e, words, 2, gap, [25.0, 40.0], noise="complex", fading=dict(pdp=p, index0=0))
        stride = pkg.abi.faded_len(2, L) + gap
        h = e.draw_taps(12, p, seed=0x80211A, index0=0)
        rec = e.transmit_faded(words, 2, h, pos0=gap, stride=stride, n_out=12 * stride + gap)
        power = float((rec.abs().double() ** 2).sum()) / (12 * pkg.abi.packet_len(2))
        assert abs(res["power"] - power) <= 1e-6 * power and res["samples"] == 12 * stride + gap
        for q, s in enumerate((25.0, 40.0)):
            y = e.impair_stream(rec, res["power"], s, noise="complex", snr_index=q)
            rx = e.receive_stream(y, keep_device=True)
            host = score_packets(gap + stride * np.arange(12), words, rx["positions"],
                                 rx["d_words"][:rx["count"]].cpu().numpy().view(np.uint32), window=(8, 40 + L - 1))
            assert np.array_equal(res["totals"][q], host["totals"])
            assert [int(v) for v in rows[1 + q][1:]] == [12, host["totals"][1], 12 - host["totals"][1],
                                                         host["totals"][2] - host["totals"][1], host["totals"][5],
                                                         host["totals"][4], host["totals"][3]]


def test_link_sweep_without_fading_is_what_it_was(pkg):
    """fading=None takes the unfaded route: the transmitter's recording, stride P + gap, window (8, 40)"""
    from ofdm_amd import sweep
    words = np.random.default_rng(3).integers(0, 1 << 32, (6, 6), dtype=np.uint64).astype(np.uint32)
    with pkg.Engine(0) as e:
        e.timing(True)
        a = sweep.link_sweep(e, words, 2, 500, [30.0], noise="complex")
        assert e.timing_query(pkg.abi.K_FADE)[1] == 0 and e.timing_query(pkg.abi.K_DRAW_TAPS)[1] == 0
        assert e.timing_query(pkg.abi.K_TRANSMIT)[1] == 1
        b = sweep.link_sweep(e, words, 2, 500, [30.0], noise="complex", window=(8, 40), fading=None)
    assert a["samples"] == 6 * (980 + 500) + 500 and a["power"] == b["power"] and np.array_equal(a["totals"], b["totals"])
