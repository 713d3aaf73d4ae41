"""The link kernels past one grid sweep (transmit -> impair -> stream receive -> score): every branch that only runs when
a block loops over its grid, a scan carries across lanes, waves and trips, or a base offset is used past block 0.  The
other GPU modules stop at 21,580 samples and 67 packets, where each of these kernels runs the first trip of its loop and
the selection runs in one block.

Sizes come from the device's CU count (cap = 2 CUs blocks, the grid of the transmitters and of the decode kernel) and
from the kernels' constants, mirrored below; tests/test_scale_host.py reads the sources and fails when a mirrored value
has moved.  Every test first asserts, from these numbers, that its input reaches the branch it is there for, and prints
its sizes, the grid trips they imply and its deviations before it asserts.

Payloads: 67 random rows per D (rand_words of test_gpu_transmit.py), packet k of a large batch carrying row k % 67.  The
67-packet launch is the shape those tests pin to the oracle in fp64, so it is the bit-exact reference of every large
batch.

Two recordings, built on the device once and left unchanged (on 256 CUs):
  A  D = 15, 4 * 2 * cap + 5 = 4,101 packets behind gaps uniform in [301, 1000] and a closing gap of 700: 1.5e7 samples,
     1,026 transmit groups (three trips, the last group ragged), more than 8 * cap packets (the decode loop wraps for
     every block shape), ~200 selection blocks, ~1,900 detect tiles, more than seven sweeps of the channel's grid.
  B  D = 2, 31 * 2 * cap + 5 = 31,749 packets behind gaps uniform in [301, 2700], padded to
     301 * (256 * 1024 + 300) + 47 = 78,995,691 samples: 1,026 selection blocks, the last one ragged, so phase 1 of the
     selection makes two trips and carries.  Gaps in a seeded order move to a limit of their range until the packets
     fill the recording up to a closing gap of 1,000, so the last packets lie in slots past 256 * 1024.
each clean (transmit_packets with explicit positions into zeros) and impaired (impair_stream, real noise at 14 dB
against the packets' mean power).  Nothing of them goes to the host but bitmaps, records, payload words and short ranges.

Every comparison is bit-exact, the numpy rule the package ships (stream.select_packets, stream.score_packets,
abi.reduce_capture_records) or a tolerance an existing test carries (imported, not restated).

A record's bit_err counts against the context's message, the records' rule; the packets carry random rows, so the clean
recordings' records are held to popcount(row ^ message words) exactly and their payload words to the transmitted rows
(no bit is wrong), which is what "no bit error" means for a random payload.

The channel ranges: the whole recording's samples against the filter, rotation and the oracle's Gaussians at their
absolute indices in fp64 (channel_ref, the 1e-5 of test_device_channel_against_an_fp64_channel) and bit for bit against
the range impaired alone at its index0; with real noise alone the imaginary parts are the input's, the rule of
test_real_noise_is_transmission_over_air (ofdm_transmission_over_air itself starts at index 0 with a power of its own,
so it cannot be asked for a range of this recording).

Out of reach, and not tested: the detect grid's own wrap (more than 2^20 tiles, 8e9 samples) and positions beyond int32.

Measured on an MI355X (256 CUs).  Sizes reached: 1,026 and 1,025 transmit groups on 512 blocks (three trips); 198 (A) and
1,026 (B) selection blocks, two trips of phase 1; 4,099 to 31,749 records on 512 decode blocks (two to 63 trips); 14,872
channel tiles on 2,048 blocks (7.26 sweeps); 125 score blocks.  At 14 dB the detector finds 4,099 of A's 4,101 packets and
31,733 of B's 31,749 (31,728 within the scoring window, 44 bit errors).  Deviations: none in any bit-exact comparison;
no crossing differs from the double-precision one, at most one position of a range lies in the band; eq against
receive_captures bit-identical and both CFO estimates equal; 12 of B's 64 windows (none of A's) hold no later front and
take the second preamble; the channel against fp64 3.8e-8 (real noise) and 1.4e-7 (taps, rotation, complex noise).
Wall time (pytest --durations): the module 4.5 s, of which 1.9 s set up the context and the 67-packet launches; recordings
A and B together under 10 ms; the receive_stream fixtures 0.17 s (A clean), 0.09 s (A impaired), 0.23 s (B, either) inside
the selection tests that first use them; the first transmitter case 0.29 s, the other ten under 5 ms each; the sentinel
test 0.14 s; LAST_FRONT 0.09 s; max_packets 0.01 s; detection under 5 ms each; decode clean under 5 ms each, impaired
0.14 s (A) and 0.02 s (B); channel 0.02 and 0.04 s; scoring under 5 ms, 0.13 s and 0.08 s.  The whole `-m gpu` suite: 62 s
with this module.

Section 7, the optional kernels (ofdm_receive_stream_ex's detectors, ofdm_receive_stream_timed's kernel, scoring of
refined positions), measured on an MI355X (256 CUs, 2026-10-20).  B through the conjugate detector: Lc = n - 63 =
78,995,628 positions in 9,955 tiles and 1,026 selection blocks (two trips of phase 1); 31,681 of 31,749 packets found at
14 dB, all 31,749 at offset 16 noise-free; on the six ranges no crossing differs off the band (at most 3 positions of a
range in it), metric within 1.25e-6 of fp64 (4 x CONJ_DEV_MEASURED 1.44e-5).  Threshold 0.6 on the reference's metric:
31,731 found, no crossing differs off a band of 6e-4, a superset of the default call's crossings.  Timing on B: 31,681
records on 2,048 blocks of 4 waves, 3.87 trips of 8,192 (7,105 records in the last); 26,423 records moved, shifts -56 to
+7; all 31,643 records within a packet's first 100 samples at offset 16; 10,156 records against fp64: shift exact,
quality within 4.5e-7 (4 x TIMING_DEV_MEASURED 1.32e-6), smallest gap between the two largest L 0.041.  Timing on A
(reference detector, 4,099 records: the conjugate one finds 4,090 there, under the decode's wrap at 4,096): half a trip
of the timing grid on 256 CUs, 3,580 records moved, every record at offset 16, 200 records within 3.3e-7 of fp64.  64
moved records of each against the oracle's decode at the refined position: CFO within 0.0044 Hz.  Scoring B's refined positions: 31,643 matched with (16, 16), (8, 40) and (0, 300) alike, 0 bit errors
against 69 at the coarse positions; neighbouring records at least 603 apart.  Wall time: the four detector cases 0.09 to
0.14 s each; the timed fixture (four receive_stream runs) 0.42 s; the timing test 0.38 s, its launch shapes 0.08 s; the
others 0.02 s or less.  The whole `-m gpu` suite: 65 s with this section and tests/test_gpu_matlab_stream.py."""
import math
import time

import numpy as np
import pytest

import channel_ref as cref
import timing_ref as tr
from conftest import normwise
from fading_ref import rand_taps
from test_gpu_captures import CFO_TOL_HZ, check_against_oracle, check_against_receiver
from test_gpu_detect import BAND_REL, CONJ_DEV_MEASURED, METRIC_FLOOR
from test_gpu_stream import BAND, assert_selection_exact, metric64
from test_gpu_timing import TIMING_DEV_MEASURED
from test_gpu_transmit import bits_of, rand_words, same_bits

pytestmark = pytest.mark.gpu

# ---- the kernels' constants, mirrored (tests/test_scale_host.py holds each to its source line)
SS_THREADS = 256             # csrc/ofdm_stream.hip:43   slots per block of the selection kernel
SS_SLOT = 301                # csrc/ofdm_stream.hip:44   positions per slot
SS_SCAN_THREADS = 1024       # csrc/ofdm_stream.hip:45   blocks per trip of phase 1's scan
SDEC_MAX_WAVES = 8           # csrc/ofdm_stream.hip:48   packets per decode block at most
TXP_GROUP_SYMS = 62          # csrc/ofdm_transmit.hip:38 data symbols per group
TXP_BLOCKS_PER_CU = 2        # csrc/ofdm_transmit.hip:45
FD_GROUP_SYMS = 62           # csrc/ofdm_fading.hip:38
FD_BLOCKS_PER_CU = 2         # csrc/ofdm_fading.hip:50
CH_THREADS = 256             # csrc/ofdm_channel.hip:32
CH_QUAD = 4                  # csrc/ofdm_channel.hip:33  CH_TILE = 4 * CH_THREADS: samples per channel quad
CH_MAX_GRID = 2048           # csrc/ofdm_channel.hip:34
SC_THREADS = 256             # csrc/ofdm_channel.hip:156 transmitted packets per score block
TM_WAVES = 4                 # csrc/ofdm_stream_timing.hip:24 packets per block and sweep of the timing kernel
TM_BLOCKS_PER_CU = 8         # csrc/ofdm_stream_timing.hip:25 its grid's cap
MIRRORED = {
    "ofdm_stream.hip": dict(SS_THREADS=SS_THREADS, SS_SLOT=SS_SLOT, SS_SCAN_THREADS=SS_SCAN_THREADS,
                            SDEC_MAX_WAVES=SDEC_MAX_WAVES),
    "ofdm_transmit.hip": dict(TXP_GROUP_SYMS=TXP_GROUP_SYMS, TXP_BLOCKS_PER_CU=TXP_BLOCKS_PER_CU),
    "ofdm_fading.hip": dict(FD_GROUP_SYMS=FD_GROUP_SYMS, FD_BLOCKS_PER_CU=FD_BLOCKS_PER_CU),
    "ofdm_channel.hip": dict(CH_THREADS=CH_THREADS, CH_MAX_GRID=CH_MAX_GRID, SC_THREADS=SC_THREADS),
    "ofdm_stream_timing.hip": dict(TM_WAVES=TM_WAVES, TM_BLOCKS_PER_CU=TM_BLOCKS_PER_CU),
}
CH_TILE = CH_QUAD * CH_THREADS
DETECT_TILE = 7936           # abi.STREAM_TILE, asserted in the detection test

N = 67                       # payload rows per D
DS = (2, 15)
SNR_DB = 14.0
TRIAL, Q = 7, 3
CLOSING_GAP = 700
OFFSET = 16                  # packet_pos - position of a noise-free packet (tests/test_scale_host.py)
TEXT = {2: b"Hey! I am Vivaswan",
        15: ("fifteen data symbols per packet: the context's message the records' bit_err counts against. " * 2)[:171].encode()}
SENTINEL = complex(np.complex64(12345.678 - 9876.5j))


def words_seed(d: int) -> int:
    # seeds whose rows keep every position of the noise-free packet more than BAND from the threshold (0x7A00 + 15,
    # test_gpu_transmit's, has one 2.4e-4 from it; tests/test_scale_host.py checks all 67 rows per D)
    return 0x5CA00 + d


def rows_of(d: int) -> np.ndarray:
    return rand_words(d, N, words_seed(d))


def packet_len(d: int) -> int:
    return 2 * (320 + 80 * d) + 20


def layout(name: str, cus: int) -> dict:
    """Recording A or B for a device of `cus` CUs: d, n_tx, pos (int64 [n_tx]), n (samples) -- numpy only"""
    cap = 2 * cus
    if name == "A":
        d, n_tx = 15, 4 * 2 * cap + 5
        plen = packet_len(d)
        gaps = np.random.default_rng(0xA5CA1E).integers(301, 1001, n_tx)
        pos = (np.cumsum(gaps) + plen * np.arange(n_tx)).astype(np.int64)
        return dict(name=name, d=d, n_tx=n_tx, pos=pos, n=int(pos[-1]) + plen + CLOSING_GAP, seed=0xA5CA1E)
    d, n_tx = 2, 31 * 2 * cap + 5
    plen = packet_len(d)
    n = SS_SLOT * (SS_THREADS * SS_SCAN_THREADS + 300) + 47
    rng = np.random.default_rng(0xB5CA1E)
    gaps = rng.integers(301, 2701, n_tx)
    # the closing gap is 1000: gaps in a seeded order move to their limit until the packets and gaps fill the recording
    excess = n - 1000 - n_tx * plen - int(gaps.sum())
    for k in rng.permutation(n_tx):
        if excess == 0:
            break
        step = min(excess, 2700 - int(gaps[k])) if excess > 0 else max(excess, 301 - int(gaps[k]))
        gaps[k] += step
        excess -= step
    assert excess == 0, f"{n_tx} packets (a device of {cus} CUs) do not fill recording B with gaps in [301, 2700]"
    pos = (np.cumsum(gaps) + plen * np.arange(n_tx)).astype(np.int64)
    assert gaps.min() >= 301 and gaps.max() <= 2700 and pos[-1] + plen + 1000 == n
    return dict(name=name, d=d, n_tx=n_tx, pos=pos, n=n, seed=0xB5CA1E)


def _torch():
    import torch
    return torch


def as_bits(t):
    """a complex64 device tensor as int32 words"""
    torch = _torch()
    return torch.view_as_real(t).view(torch.int32)


def dev_same_bits(a, b) -> bool:
    return a.shape == b.shape and bool(_torch().equal(as_bits(a), as_bits(b)))


def rows_differing(a, b):
    """the rows of two [n, m] complex tensors that differ in any bit"""
    return (as_bits(a) != as_bits(b)).flatten(1).any(dim=1).nonzero().flatten().cpu().numpy()


@pytest.fixture(scope="module")
def eng(pkg):
    """A separate context, so the session engine keeps the reference message."""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev():
    cus = _torch().cuda.get_device_properties(0).multi_processor_count
    return dict(cus=cus, cap=2 * cus)


@pytest.fixture(scope="module")
def small(eng, pkg):
    """D -> the 67-packet reference: rows (uint32 [67, 3 D]), rows_dev (int32), pk (device [67, P], dense store-mode
    launch, conv c) and the packets' mean power; built once and left unchanged"""
    torch = _torch()
    out = {}
    for d in DS:
        assert pkg.abi.packet_len(d) == packet_len(d)
        rows = rows_of(d)
        pk = eng.transmit_packets(rows, d).reshape(N, -1)
        host = pk.cpu().numpy().astype(np.complex128)
        out[d] = dict(rows=rows, rows_dev=torch.from_numpy(rows.view(np.int32)).cuda(), pk=pk,
                      power=float(np.mean(host.real ** 2 + host.imag ** 2)))
    return out


def big_words(small, d, n):
    torch = _torch()
    idx = torch.arange(n, device="cuda") % N
    return idx, small[d]["rows_dev"][idx].contiguous()


@pytest.fixture(scope="module")
def recs(eng, pkg, dev, small):
    """name -> recording A / B: its layout, the packets' words and positions on the device, the clean and the impaired
    samples (device); built once and left unchanged"""
    torch = _torch()
    out = {}
    for name in "AB":
        t0 = time.perf_counter()
        r = layout(name, dev["cus"])
        d = r["d"]
        r["idx"], r["words"] = big_words(small, d, r["n_tx"])
        r["pos_dev"] = torch.from_numpy(r["pos"]).cuda()
        r["power"] = small[d]["power"]
        r["clean"] = eng.transmit_packets(r["words"], d, positions=r["pos_dev"], n_out=r["n"])
        r["noisy"] = eng.impair_stream(r["clean"], r["power"], SNR_DB, noise="real", seed=cref.SEED, trial=TRIAL, snr_index=Q)
        torch.cuda.synchronize()
        print(f"recording {name}: D {d}, {r['n_tx']} packets, {r['n']} samples ({8 * r['n'] / 1e6:.0f} MB), gaps' seed "
              f"{r['seed']:#x}, built in {time.perf_counter() - t0:.2f} s")
        out[name] = r
    return out


def receive(eng, r, x, **kw):
    """receive_stream on a device recording of r's packets, with the crossings as a boolean array and the rule on them"""
    from ofdm_amd.stream import select_packets, unpack_cross
    assert eng.set_long_message(TEXT[r["d"]]) == r["d"]
    out = eng.receive_stream(x, **kw)
    if out["cross"] is not None:
        out["bitmap"] = unpack_cross(out["cross"].cpu().numpy(), len(x) - 47)
        out["sel"] = select_packets(out["bitmap"])
    return out


@pytest.fixture(scope="module")
def rx(eng, recs):
    """(name, kind) -> the full receive_stream run of a recording with every output this module reads and a counters
    row; built on first use and left unchanged"""
    torch = _torch()
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            t0 = time.perf_counter()
            r = recs[name]
            row = eng.new_counters(1)[0]
            out = receive(eng, r, r[kind], want_bits=True, want_eq=True, want_cross=True, counters=row, keep_device=True)
            out["row"] = row.cpu().numpy().copy()
            torch.cuda.synchronize()
            print(f"receive_stream {name} {kind}: found {out['found']}, count {out['count']}, {len(out['sel']['fronts'])} "
                  f"fronts, {time.perf_counter() - t0:.2f} s")
            cache[name, kind] = out
        return cache[name, kind]
    return get


RECORDINGS = [("A", "clean"), ("A", "noisy"), ("B", "clean"), ("B", "noisy")]


# ------------------------------------------------------------------------------------------- 1. transmitters
def _reference_and_big(eng, small, d, n, case):
    """(the 67-packet launch [67, m], the n-packet launch [n, m], the samples between the packets or None)"""
    torch = _torch()
    rows_dev = small[d]["rows_dev"]
    idx, words = big_words(small, d, n)
    rng = np.random.default_rng(0x5CA1E + d)
    gains = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    cfos = rng.uniform(-110e3, 110e3, N).astype(np.float32)
    if case in ("store", "accumulate", "matlab"):
        kw = dict(accumulate=case == "accumulate", conv="matlab" if case == "matlab" else "c")
        ref = small[d]["pk"] if case == "store" else eng.transmit_packets(rows_dev, d, **kw).reshape(N, -1)
        return ref, eng.transmit_packets(words, d, **kw).reshape(n, -1), None
    if case == "impaired":
        g, f = torch.from_numpy(gains).cuda(), torch.from_numpy(cfos).cuda()
        ref = eng.transmit_packets(rows_dev, d, gains=g, cfo_hz=f).reshape(N, -1)
        return ref, eng.transmit_packets(words, d, gains=g[idx].contiguous(), cfo_hz=f[idx].contiguous()).reshape(n, -1), None
    L = {"faded4": 4, "faded32": 32}[case]
    taps = torch.from_numpy(rand_taps(N, L, 0xFB00 + 64 * d + L)).cuda()
    g, f = torch.from_numpy(gains).cuda(), torch.from_numpy(cfos).cuda()
    pl = packet_len(d) + L - 1
    stride = pl + 3                                               # odd: the tails stay apart, every other packet is 8-byte aligned only
    ref = eng.transmit_faded(rows_dev, d, taps, gains=g, cfo_hz=f).reshape(N, pl)
    big = eng.transmit_faded(words, d, taps[idx].contiguous(), gains=g[idx].contiguous(), cfo_hz=f[idx].contiguous(),
                             stride=stride, n_out=n * stride).reshape(n, stride)
    return ref, big[:, :pl], big[:, pl:]


@pytest.mark.parametrize("d,case", [(d, c) for d in (15, 2) for c in ("store", "accumulate", "impaired", "faded4", "faded32")]
                         + [(15, "matlab")])
def test_transmitters_when_blocks_loop(eng, dev, small, d, case):
    cap = dev["cap"]
    n = {15: 4, 2: 31}[d] * 2 * cap + 5
    syms, per_cu = (FD_GROUP_SYMS, FD_BLOCKS_PER_CU) if case.startswith("faded") else (TXP_GROUP_SYMS, TXP_BLOCKS_PER_CU)
    per_group = syms // d
    groups = -(-n // per_group)
    grid_cap = per_cu * dev["cus"]
    per_block = -(-groups // grid_cap)
    print(f"transmit {case} D {d}: {n} packets, {groups} groups of {per_group} (the last of {n - (groups - 1) * per_group}) "
          f"on at most {grid_cap} blocks: {per_block} trips")
    assert grid_cap == cap and groups > 2 * cap and n % per_group != 0
    ref, big, between = _reference_and_big(eng, small, d, n, case)
    idx = _torch().arange(n, device="cuda") % N
    want = ref[idx]
    bad = rows_differing(big, want)
    print(f"transmit {case} D {d}: {len(bad)} of {n} packets differ from row k % {N} of the {N}-packet launch"
          + (f", the first {bad[:8].tolist()} (groups {(bad[:8] // per_group).tolist()})" if len(bad) else ""))
    assert len(bad) == 0
    assert dev_same_bits(big, want)
    if between is not None:
        assert not as_bits(between).any()                         # nothing is written between the packets


def test_a_looped_launch_writes_the_packets_and_nothing_else(eng, small, recs):
    torch = _torch()
    for name in "AB":
        r = recs[name]
        d, plen = r["d"], packet_len(r["d"])
        at = (r["pos_dev"][:, None] + torch.arange(plen, device="cuda")[None, :]).reshape(-1)
        packets = small[d]["pk"][r["idx"]].reshape(-1)
        exp = torch.zeros(r["n"], dtype=torch.complex64, device="cuda")
        exp[at] = packets
        same = dev_same_bits(r["clean"], exp)
        print(f"recording {name} clean: {r['n_tx']} packets at explicit positions into zeros, bit-identical to the "
              f"{N}-packet launch's rows: {same}")
        assert same
        if name == "A":
            out = torch.full((r["n"],), SENTINEL, dtype=torch.complex64, device="cuda")
            assert eng.transmit_packets(r["words"], d, positions=r["pos_dev"], out=out) is out
            exp.fill_(SENTINEL)
            exp[at] = packets
            untouched = r["n"] - r["n_tx"] * plen
            kept = int((as_bits(out) == as_bits(exp[:1])).all(dim=1).sum())      # exp[0] lies in the first gap
            print(f"recording {name} into a sentinel: {kept} samples hold it after the launch, {untouched} lie outside the packets")
            assert kept == untouched
            assert dev_same_bits(out, exp)


# ------------------------------------------------------------------------------------------- 2. selection
def _selection_sizes(r):
    lc = r["n"] - 47
    nslots = -(-lc // SS_SLOT)
    return lc, nslots, -(-nslots // SS_THREADS)


@pytest.mark.parametrize("name,kind", RECORDINGS)
def test_selection_at_scale_is_exact(rx, recs, name, kind):
    r = recs[name]
    lc, nslots, nblocks = _selection_sizes(r)
    out = rx(name, kind)
    sel = out["sel"]
    front_max = int(sel["fronts"].max())
    last_conf = int(out["positions"][-1]) - 11
    print(f"selection {name} {kind}: {nslots} slots in {nblocks} blocks ({nslots - (nblocks - 1) * SS_THREADS} in the last), "
          f"phase 1 trips {-(-nblocks // SS_SCAN_THREADS)}; found {out['found']} of {r['n_tx']}, {len(sel['fronts'])} fronts, "
          f"largest front in block {front_max // (SS_SLOT * SS_THREADS)}, last packet's in block "
          f"{last_conf // (SS_SLOT * SS_THREADS)}, LAST_FRONT on {int((out['records']['flags'] & 4 != 0).sum())} records")
    assert nblocks > 64                                           # more than one wave of phase 1's scan
    assert nslots % SS_THREADS != 0
    assert front_max // (SS_SLOT * SS_THREADS) > 0                # the largest front is not in block 0
    if name == "B":
        assert nblocks > SS_SCAN_THREADS                          # the carry of phase 1's outer loop
        assert last_conf // SS_SLOT >= SS_THREADS * SS_SCAN_THREADS and front_max // SS_SLOT >= SS_THREADS * SS_SCAN_THREADS
    assert_selection_exact(out)
    assert out["found"] == out["count"]
    assert np.array_equal(out["records"]["packet_idx"], out["records"]["packet_pos"].astype(np.int32))
    assert int(out["positions"].max()) < 2 ** 31
    if kind == "clean":
        # the truth itself, not through select_packets: every packet once, at offset 16
        assert out["found"] == r["n_tx"]
        assert np.array_equal(out["positions"], r["pos"] + OFFSET)


def test_last_front_flag_past_block_0(eng, rx, recs):
    """Every packet of A and B shows a second, unconfirmed front (tests/test_scale_host.py), so no record of theirs
    carries LAST_FRONT.  Clean B cut between its last packet's confirmation and that second front ends in a confirmed
    front, in the last selection block, behind phase 1's carry."""
    r = recs["B"]
    full = rx("B", "clean")
    front = int(full["positions"][-1]) - 11
    second = int(full["sel"]["fronts"][-1])
    n_cut = front + 231 + 47 + 20                                  # Lc = front + 251: the look at front + 230 is inside
    assert second > front + 300 and n_cut - 47 <= second
    lc, nslots, nblocks = _selection_sizes(dict(n=n_cut))
    assert nblocks > SS_SCAN_THREADS and front // (SS_SLOT * SS_THREADS) >= SS_SCAN_THREADS
    out = receive(eng, r, r["clean"][:n_cut], want_bits=False, want_cross=True)
    flags = out["records"]["flags"]
    print(f"clean B cut at {n_cut}: {nblocks} blocks, found {out['found']}, the last front {front} in block "
          f"{front // (SS_SLOT * SS_THREADS)}, flags of the last records {flags[-3:].tolist()}")
    assert_selection_exact(out)
    assert out["found"] == r["n_tx"] and np.array_equal(out["positions"], r["pos"] + OFFSET)
    assert int(out["sel"]["fronts"].max()) == front
    assert flags[-1] & 4 and not (flags[:-1] & 4).any()
    assert out["records"][:-1].tobytes() == full["records"][:-1].tobytes()


def test_max_packets_cuts_at_and_around_a_blocks_prefix(eng, rx, recs):
    r = recs["B"]
    full = rx("B", "noisy")
    fronts = full["positions"] - 11
    cuts = []
    for b in (513, SS_SCAN_THREADS):                               # a block of the first trip of phase 1, the first of the second
        prefix = int((fronts < b * SS_THREADS * SS_SLOT).sum())   # blk_cnt[b] after the scan
        assert 0 < prefix < full["found"]
        cuts += [prefix - 1, prefix, prefix + 1]
    for m in cuts + [0]:
        o = receive(eng, r, r["noisy"], max_packets=m, want_bits=False)
        print(f"max_packets {m}: found {o['found']}, count {o['count']}")
        assert o["found"] == full["found"] and o["count"] == m == len(o["records"])
        assert o["records"].tobytes() == full["records"][:m].tobytes()


# ------------------------------------------------------------------------------------------- 3. detection
@pytest.mark.parametrize("kind", ["noisy", "clean"])
def test_detection_at_scale(pkg, rx, recs, kind):
    T = pkg.abi.STREAM_TILE
    assert T == DETECT_TILE
    r = recs["B"]
    lc = r["n"] - 47
    tiles = -(-lc // T)
    got_all = rx("B", kind)["bitmap"]
    rng = np.random.default_rng(0xDE7EC7)
    starts = [0, (tiles - 2) * T] + [int(t) * T for t in rng.integers(1, tiles - 3, 2)] \
        + [int(s) for s in rng.integers(T, lc - 3 * T, 2)]
    assert lc % T != 0 and all(s % T == 0 for s in starts[:4]) and all(s % T for s in starts[4:])
    for s in starts:
        e = min(s + 2 * T, lc)
        x = r[kind][s:e + 47].cpu().numpy()
        ref = metric64(x)
        got = got_all[s:e]
        with np.errstate(invalid="ignore"):
            want = ref > 0.75
            band = np.abs(ref - 0.75) <= BAND
        diff = int((got != want)[~band].sum())
        print(f"detect B {kind}: positions [{s}, {e}) (tiles {s // T} .. {(e - 1) // T} of {tiles}): {int(got.sum())} crossings, "
              f"{diff} differ off the band, {int(band.sum())} positions ({100 * band.mean():.2f} %) in it, "
              f"{int((got != want)[band].sum())} differ there")
        assert len(ref) == e - s and got.any()
        assert diff == 0
        assert band.mean() <= 0.01
        assert not got[~np.isfinite(ref)].any()
        if kind == "clean":
            assert not band.any() and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- 4. decode
def _decode_sizes(r, out, dev):
    cap = dev["cap"]
    print(f"decode {r['name']}: {out['count']} records on at most {cap} blocks of W <= {SDEC_MAX_WAVES} waves: "
          f"{-(-out['count'] // (SDEC_MAX_WAVES * cap))} trips at W = {SDEC_MAX_WAVES}, {-(-out['count'] // cap)} at W = 1")
    assert out["count"] > SDEC_MAX_WAVES * cap


def _counters_and_records_only(eng, pkg, r, x, out):
    want = pkg.abi.reduce_capture_records(out["records"], r["d"])
    print(f"decode {r['name']}: counters row {out['row'].tolist()}")
    assert np.array_equal(out["row"], want)
    only = receive(eng, r, x, want_bits=False)
    assert only["bits"] is None and only["records"].tobytes() == out["records"].tobytes()


@pytest.mark.parametrize("name", ["A", "B"])
def test_decode_when_the_loop_wraps_clean(eng, pkg, dev, rx, recs, small, name):
    from ofdm_amd.stream import pack_messages
    r = recs[name]
    d = r["d"]
    out = rx(name, "clean")
    _decode_sizes(r, out, dev)
    assert out["count"] == r["n_tx"]
    words = out["d_words"][:out["count"]]
    wrong = (words != r["words"]).any(dim=1).nonzero().flatten().cpu().numpy()
    print(f"decode {name} clean: {len(wrong)} records with payload words other than the transmitted row"
          + (f", the first {wrong[:8].tolist()}" if len(wrong) else ""))
    assert len(wrong) == 0
    # bit_err counts against the context's message: exactly the row's distance from it
    msg = pack_messages([TEXT[d]], d)[0][0]
    dist = np.unpackbits((small[d]["rows"] ^ msg).view(np.uint8), axis=1).sum(axis=1)
    rec = out["records"]
    assert np.array_equal(rec["bit_err"], dist[np.arange(r["n_tx"]) % N])
    assert np.array_equal(rec["ber"], (rec["bit_err"].astype(np.float32) / np.float32(96 * d)))
    flags = rec["flags"]
    print(f"decode {name} clean: flags of the last record {int(flags[-1])}, the rule's {int(out['sel']['flags'][-1])}")
    assert not flags[:-1].any() and flags[-1] == out["sel"]["flags"][-1] and flags[-1] in (0, 4)
    _counters_and_records_only(eng, pkg, r, r["clean"], out)


@pytest.mark.parametrize("name", ["A", "B"])
def test_decode_when_the_loop_wraps_impaired(eng, pkg, dev, rx, recs, name):
    torch = _torch()
    r = recs[name]
    d, cap = r["d"], dev["cap"]
    out = rx(name, "noisy")
    _decode_sizes(r, out, dev)
    count = out["count"]
    cap_len = pkg.abi.capture_len(d)
    picks = [0, count - 1] + [w * cap + o for w in (1, 4, 5, 8) for o in (-1, 0, 1)]
    assert max(picks) < count, (max(picks), count)
    rng = np.random.default_rng(0xDEC0DE + d)
    fill = [int(k) for k in rng.permutation(count) if int(k) not in picks]
    picks = np.array(picks + fill[:64 - len(picks)])
    assert len(set(picks.tolist())) == 64
    p = out["positions"][picks]
    starts = torch.from_numpy(p - 411).cuda()
    at = starts[:, None] + torch.arange(cap_len, device="cuda")[None, :]
    inside = (at >= 0) & (at < r["n"])
    x = r["noisy"]
    windows = torch.where(inside, x[at.clamp(0, r["n"] - 1)], torch.zeros((), dtype=x.dtype, device="cuda")).contiguous()
    assert eng.set_long_message(TEXT[d]) == d
    capt = eng.receive_captures(windows, want_bits=True, want_eq=True)
    crec = {k: v.cpu().numpy() for k, v in capt["records"].items()}
    # Receiver()'s own Packet_Selection refuses a capture's last front (OFDM.c:745-760).  A window whose next packet
    # lies beyond it (B: gaps up to 2,700 against a capture of 3,008) and whose packet shows no second front under the
    # noise ends in a sync failure by that rule, not by the decode under test.  Such a window must show, in the
    # stream's own crossings, no front behind the record's; it then takes a copy of its samples [100, 1100) -- 295 idle
    # samples and the packet's first 705, the preamble -- at 525 samples behind the packet's end.  The samples the
    # decode reads, [p - 20, p + 2 nfr - 2], stay the recording's, and the window must then reproduce the record.
    from ofdm_amd.stream import select_packets
    refused = np.nonzero(crec["packet_idx"] != 411)[0]
    dst = 411 - OFFSET + packet_len(d) + 525
    assert dst + 1000 <= cap_len
    for k in refused:
        s = int(p[k]) - 411
        fronts = select_packets(out["bitmap"][max(s, 0):s + cap_len - 47])["fronts"] + max(s, 0) - s
        assert crec["flags"][k] & 1 and crec["packet_idx"][k] == 0 and fronts.max() == 400, (picks[k], fronts)
    if len(refused):
        windows[torch.from_numpy(refused).cuda(), dst:dst + 1000] = windows[torch.from_numpy(refused).cuda(), 100:1100]
        capt = eng.receive_captures(windows, want_bits=True, want_eq=True)
        crec = {k: v.cpu().numpy() for k, v in capt["records"].items()}
    print(f"decode {name} impaired: {len(refused)} of 64 windows hold no front behind the record's (records "
          f"{picks[refused].tolist()}) and take a second preamble")
    rec = out["records"][picks].copy()
    picks_dev = torch.from_numpy(picks).cuda()
    bits, eq = out["bits"][picks_dev].cpu().numpy(), out["eq"][picks_dev].cpu().numpy()
    wh = windows.cpu().numpy()
    dev_eq = normwise(eq, capt["eq"].cpu().numpy())
    cfo_dev = max(np.abs(rec["cfo_coarse_hz"].astype(np.float64) - crec["cfo_coarse_hz"]).max(),
                  np.abs(rec["cfo_fine_hz"].astype(np.float64) - crec["cfo_fine_hz"]).max())
    print(f"decode {name} impaired: records {picks[:14].tolist()} and 50 seeded ones against receive_captures on "
          f"[p - 411, p - 411 + {cap_len}): eq normwise {dev_eq:.3g}, CFO estimates within {cfo_dev:.4g} Hz, "
          f"bit_err {int(rec['bit_err'].min())} .. {int(rec['bit_err'].max())}, "
          f"{int(((at < 0) | (at >= r['n'])).any(dim=1).sum())} windows reach past the recording")
    assert np.array_equal(crec["packet_idx"], np.full(64, 411))
    assert np.array_equal(crec["flags"], rec["flags"] & 3)
    assert np.array_equal(capt["bits"].cpu().numpy(), bits)
    assert np.array_equal(crec["bit_err"], rec["bit_err"])
    assert dev_eq < 1e-6
    assert cfo_dev <= CFO_TOL_HZ
    # the single-capture receiver on the same windows, by test_gpu_captures' rule
    rec_w = rec.copy()
    rec_w["packet_idx"] = 411
    rec_w["flags"] &= 3
    for k in range(64):
        o = check_against_receiver(eng, wh[k], rec_w[k], eq[k])
        assert np.array_equal(o["bits"], bits[k]), picks[k]
        assert int(rec["bit_err"][k]) == int(crec["bit_err"][k])
    _counters_and_records_only(eng, pkg, r, r["noisy"], out)


# ------------------------------------------------------------------------------------------- 5. channel
CHANNEL_SETTINGS = {"real noise alone": (None, 0.0, "real", SNR_DB),
                    "three taps, 40 kHz, complex noise": (np.array([1, 0, 0.4 + 0.3j], np.complex64), 40e3, "complex", 25.0)}


@pytest.mark.parametrize("setting", list(CHANNEL_SETTINGS))
def test_channel_when_the_tile_loop_wraps(eng, oracle, recs, setting):
    torch = _torch()
    taps, cfo, noise, snr = CHANNEL_SETTINGS[setting]
    r = recs["A"]
    x, n, power = r["clean"], r["n"], r["power"]
    sweep = CH_MAX_GRID * CH_TILE
    tiles = -(-n // CH_TILE)
    print(f"channel ({setting}): {n} samples, {tiles} tiles on {CH_MAX_GRID} blocks: {n / sweep:.2f} sweeps")
    assert n > 7 * sweep
    kw = dict(cfo_hz=cfo, taps=taps, noise=noise, seed=cref.SEED, trial=TRIAL, snr_index=Q)
    whole = eng.impair_stream(x, power, snr, **kw)
    if taps is None:
        assert dev_same_bits(whole, r["noisy"])                  # the fixture's own launch
    parts = torch.empty_like(whole)
    sizes, lo, k = (2 ** 20 + 3, 2 ** 21 - 1, 777_777), 0, 0
    while lo < n:
        hi = min(lo + sizes[k % 3], n)
        assert hi - lo <= sweep
        lead = min(31, lo)                                        # as test_chunks_equal_the_whole
        got = eng.impair_stream(x[lo - lead:hi], power, snr, index0=lo, lead=lead, out=parts[lo:hi], **kw)
        assert got.shape == (hi - lo,)
        lo, k = hi, k + 1
    diff = int((as_bits(parts) != as_bits(whole)).any(dim=1).sum())
    print(f"channel ({setting}): {k} chunks, {diff} samples differ from the whole recording's")
    assert k >= 10 and diff == 0
    assert not dev_same_bits(whole, x)
    H = 0 if taps is None else len(taps) - 1
    for s in (0, sweep - 2048 - 3, n - 4096):
        e = s + 4096
        assert 0 <= s and e <= n
        lead = min(H, s)
        xin = x[s - lead:e].cpu().numpy()
        got = whole[s:e].cpu().numpy()
        alone = eng.impair_stream(x[s - lead:e], power, snr, index0=s, lead=lead, **kw).cpu().numpy()
        y = cref.fir64(xin, taps)[lead:]
        if cfo:
            y = y * cref.rotation64(cfo, s, e - s)
        want = y + cref.noise64(oracle, e - s, power / 10.0 ** (snr / 10.0), noise, TRIAL, Q, cref.SEED, index0=s)
        dv = normwise(got, want)
        print(f"channel ({setting}): samples [{s}, {e}) (tiles {s // CH_TILE} .. {(e - 1) // CH_TILE}) against fp64: normwise {dv:.3g}")
        assert same_bits(got, alone)
        assert np.abs(xin).max() > 0 and dv < 1e-5
        if noise == "real" and taps is None and not cfo:
            assert np.array_equal(got.imag.view(np.int32), xin.imag.view(np.int32)) and not same_bits(got, xin)


# ------------------------------------------------------------------------------------------- 6. scoring
def _score_both(eng, pkg, r, o):
    """Engine.score_packets and stream.score_packets on the same records"""
    from ofdm_amd.stream import score_packets
    dev_out = eng.score_packets(r["words"], r["d"], o, positions=r["pos_dev"])
    scores, totals = dev_out["scores"].cpu().numpy(), dev_out["totals"].cpu().numpy()
    rw = o["d_words"][:o["count"]].cpu().numpy().view(np.uint32)
    host = score_packets(r["pos"], r["words"].cpu().numpy().view(np.uint32), o["positions"], rw)
    abi = pkg.abi
    print(f"score: {r['n_tx']} packets in {-(-r['n_tx'] // SC_THREADS)} blocks against {o['count']} records: totals {totals.tolist()}")
    assert scores.shape == (r["n_tx"], 2) and scores.dtype == np.int32 and totals.dtype == np.int64
    assert np.array_equal(scores[:, 0], host["rx_index"]) and np.array_equal(scores[:, 1], host["bit_err"])
    assert np.array_equal(totals, host["totals"])
    assert totals[abi.S_TRANSMITTED] == r["n_tx"] and totals[abi.S_RECEIVED] == o["count"]
    assert totals[abi.S_MATCHED] + int((scores[:, 0] < 0).sum()) == r["n_tx"]
    return scores, totals


def test_scoring_at_scale(eng, pkg, rx, recs):
    r = recs["B"]
    assert r["n_tx"] > 100 * SC_THREADS and r["n_tx"] % SC_THREADS != 0
    scores, totals = _score_both(eng, pkg, r, rx("B", "noisy"))
    print(f"score B: matched {totals[pkg.abi.S_MATCHED]} of {r['n_tx']}, bit errors {totals[pkg.abi.S_BIT_ERR]}")
    assert totals[pkg.abi.S_BITS] == 96 * r["d"] * totals[pkg.abi.S_MATCHED]


def test_scoring_with_every_seventh_packet_missing(eng, pkg, recs):
    torch = _torch()
    r = recs["B"]
    gains = torch.ones(r["n_tx"], dtype=torch.complex64, device="cuda")
    gains[::7] = 0
    missing = math.ceil(r["n_tx"] / 7)
    # noise-free, where every transmitted packet is found (tests/test_scale_host.py): at 14 dB the detector itself
    # misses a few packets in 10,000, and the count below could not be exact
    clean = eng.transmit_packets(r["words"], r["d"], positions=r["pos_dev"], gains=gains, n_out=r["n"])
    o = receive(eng, r, clean, want_bits=True, keep_device=True)
    scores, totals = _score_both(eng, pkg, r, o)
    lost = np.nonzero(scores[:, 0] < 0)[0]
    print(f"score B, every seventh packet at gain 0: found {o['found']}, matched {totals[pkg.abi.S_MATCHED]} of {r['n_tx']}, "
          f"{len(lost)} unmatched ({int((lost % 7 != 0).sum())} of them transmitted)")
    assert totals[pkg.abi.S_MATCHED] == r["n_tx"] - missing
    assert np.array_equal(lost, np.arange(0, r["n_tx"], 7))


def test_scoring_with_records_cut_inside_a_score_block(eng, pkg, rx, recs):
    r = recs["B"]
    full = rx("B", "noisy")
    m = 61 * SC_THREADS + 100
    assert m < full["found"]
    o = receive(eng, r, r["noisy"], max_packets=m, want_bits=True, keep_device=True)
    assert o["count"] == m and o["found"] == full["found"]
    scores, totals = _score_both(eng, pkg, r, o)
    last = int(np.nonzero(scores[:, 0] >= 0)[0].max())
    print(f"score B with {m} records: the last matched packet is {last} (block {last // SC_THREADS}, thread {last % SC_THREADS})")
    assert last % SC_THREADS not in (0, SC_THREADS - 1) and (scores[last + 1:, 0] == -1).all()
    assert np.array_equal(scores[:last + 1], _score_both(eng, pkg, r, full)[0][:last + 1])


# ------------------------------------------------------------------------------------------- 7. the optional kernels
# ofdm_receive_stream_ex's detectors and ofdm_receive_stream_timed's kernel on the same recordings: tiles far from the
# start, the selection and the decode with the conjugate detector's Lc = n - 63 where their loops carry, the timing
# kernel's own packet loop (i += gridDim.x * TM_WAVES, the grid capped at TM_BLOCKS_PER_CU blocks per CU) past its
# first trip, and ofdm_score_packets on refined positions.
OPTIONAL_DETECTORS = [("conjugate", 0.75), ("reference", 0.6)]      # stream_detect_conj_kernel, stream_detect_thr_kernel


def receive_opt(eng, r, x, detector="conjugate", threshold=0.75, timing="none", **kw):
    """receive() with ofdm_receive_stream_ex's and ofdm_receive_stream_timed's options: the bitmap has the detector's
    own Lc positions"""
    from ofdm_amd.stream import positions, select_packets, unpack_cross
    assert eng.set_long_message(TEXT[r["d"]]) == r["d"]
    out = eng.receive_stream(x, detector=detector, threshold=threshold, timing=timing, **kw)
    if out["cross"] is not None:
        out["bitmap"] = unpack_cross(out["cross"].cpu().numpy(), positions(len(x), detector))
        out["sel"] = select_packets(out["bitmap"])
    return out


@pytest.mark.parametrize("kind", ["noisy", "clean"])
@pytest.mark.parametrize("detector,threshold", OPTIONAL_DETECTORS)
def test_optional_detectors_at_scale(eng, pkg, rx, recs, detector, threshold, kind):
    from ofdm_amd.stream import detection_metric, positions
    T = pkg.abi.STREAM_TILE
    r = recs["B"]
    halo = r["n"] - positions(r["n"], detector)
    lc = r["n"] - halo
    tiles = -(-lc // T)
    nslots = -(-lc // SS_SLOT)
    nblocks = -(-nslots // SS_THREADS)
    conj = detector == "conjugate"
    t0 = time.perf_counter()
    out = receive_opt(eng, r, r[kind], detector, threshold, want_bits=False, want_cross=True, want_metric=conj)
    _torch().cuda.synchronize()
    print(f"optional detector {detector} {threshold} B {kind}: Lc {lc} (halo {halo}), {tiles} tiles, {nslots} slots in {nblocks} "
          f"selection blocks, phase 1 trips {-(-nblocks // SS_SCAN_THREADS)}; found {out['found']} of {r['n_tx']}, "
          f"{time.perf_counter() - t0:.2f} s")
    assert halo == (63 if conj else 47) and nblocks > SS_SCAN_THREADS and tiles > 9000
    got_all = out["bitmap"]
    rng = np.random.default_rng(0xDE7EC7)
    starts = [0, (tiles - 2) * T] + [int(t) * T for t in rng.integers(1, tiles - 3, 2)] \
        + [int(s) for s in rng.integers(T, lc - 3 * T, 2)]
    assert lc % T != 0 and all(s % T == 0 for s in starts[:4]) and all(s % T for s in starts[4:])
    worst = 0.0
    for s in starts:
        e = min(s + 2 * T, lc)
        x = r[kind][s:e + halo].cpu().numpy()
        ref = detection_metric(x, detector)
        got = got_all[s:e]
        ok = np.isfinite(ref)
        with np.errstate(invalid="ignore"):
            want = ref > threshold
            band = np.abs(ref - threshold) <= BAND_REL * threshold
        diff = int((got != want)[~band].sum())
        text = ""
        if conj:
            g = out["metric"][s:e].cpu().numpy().astype(np.float64)
            dev = float((np.abs(g[ok] - ref[ok]) / np.maximum(ref[ok], METRIC_FLOOR)).max())
            worst = max(worst, dev)
            text = f", metric deviation {dev:.3g} (4 x CONJ_DEV_MEASURED {4 * CONJ_DEV_MEASURED:.3g})"
            assert np.isfinite(g[ok]).all()
        print(f"detect {detector} {threshold} B {kind}: positions [{s}, {e}) (tiles {s // T} .. {(e - 1) // T} of {tiles}): "
              f"{int(got.sum())} crossings, {diff} differ off the band, {int(band.sum())} positions ({100 * band.mean():.2f} %) in it, "
              f"{int((got != want)[band].sum())} differ there{text}")
        assert len(ref) == e - s and got.any()
        assert diff == 0
        assert band.mean() <= 0.01
        assert not got[~ok].any()
    if conj:
        assert BAND_REL * 0.75 == BAND and 4 * CONJ_DEV_MEASURED < 1e-3 and worst <= 4 * CONJ_DEV_MEASURED
    else:
        # the two kernels' sums are bit-identical, so the default call's 0.75-crossings nest in the 0.6-crossings
        base = rx("B", kind)["bitmap"]
        assert len(base) == len(got_all) and not (base & ~got_all).any() and got_all.sum() > base.sum()
    # the selection on the whole bitmap, with the detector's own Lc
    assert len(got_all) == lc
    assert_selection_exact(out)
    assert out["found"] == out["count"] and int(out["positions"].max()) < 2 ** 31
    last_conf = int(out["positions"][-1]) - 11
    assert last_conf // SS_SLOT >= SS_THREADS * SS_SCAN_THREADS      # behind the carry of phase 1's outer loop
    if kind == "clean" and conj:
        # tests/test_scale_host.py: every payload row alone is found once at offset 16 by this detector too
        assert out["found"] == r["n_tx"] and np.array_equal(out["positions"], r["pos"] + OFFSET)


def test_max_packets_cuts_at_a_blocks_prefix_under_the_conjugate_detector(eng, timed, recs):
    r = recs["B"]
    full = timed["B"]["none"]
    fronts = full["positions"] - 11
    prefix = int((fronts < SS_SCAN_THREADS * SS_THREADS * SS_SLOT).sum())     # the first block of phase 1's second trip
    assert 0 < prefix < full["found"]
    o = receive_opt(eng, r, r["noisy"], max_packets=prefix, want_bits=False)
    print(f"conjugate detector, max_packets {prefix}: found {o['found']}, count {o['count']}")
    assert o["found"] == full["found"] and o["count"] == prefix == len(o["records"])
    assert o["records"].tobytes() == full["records"][:prefix].tobytes()


# ---- timing
TIMED_DETECTOR = {"B": "conjugate", "A": "reference"}


@pytest.fixture(scope="module")
def tmpl(pkg, oracle):
    return tr.template(oracle)


@pytest.fixture(scope="module")
def timed(eng, recs):
    """name -> the noisy recording without timing and with "ltf", each with bits, eq, a counters row and the device
    tensors; built once and left unchanged.  B through the conjugate detector.  A through the reference's: at 14 dB it
    finds 4,099 of A's packets and the conjugate one 4,090, and A is here for the decode loop's wrap past
    SDEC_MAX_WAVES * cap = 4,096 records."""
    torch = _torch()
    out = {}
    for name in "BA":
        r = recs[name]
        out[name] = {}
        for timing in ("none", "ltf"):
            t0 = time.perf_counter()
            row = eng.new_counters(1)[0]
            o = receive_opt(eng, r, r["noisy"], TIMED_DETECTOR[name], timing=timing, want_bits=True, want_eq=True, counters=row,
                            keep_device=True)
            o["row"] = row.cpu().numpy().copy()
            torch.cuda.synchronize()
            print(f"receive_stream {name} noisy, {TIMED_DETECTOR[name]} detector, timing {timing}: found {o['found']}, count {o['count']}, "
                  f"{time.perf_counter() - t0:.2f} s")
            out[name][timing] = o
    return out


def _timing_trip(dev) -> int:
    return TM_BLOCKS_PER_CU * dev["cus"] * TM_WAVES


def _whole_run_assertions(r, none, ltf):
    """what holds for every record of a timed run, whatever the recording"""
    n, count = r["n"], ltf["count"]
    assert count == ltf["found"] == none["count"] == none["found"]
    assert np.array_equal(ltf["coarse_pos"], none["positions"])                       # byte-identical: both int64
    assert ltf["coarse_pos"].tobytes() == none["positions"].tobytes()
    assert np.array_equal(ltf["positions"], ltf["coarse_pos"] + ltf["shift"])
    assert (np.diff(ltf["positions"]) > 0).all()                                      # "the records stay ascending"
    assert ((ltf["shift"] >= -56) & (ltf["shift"] <= 7)).all()
    inside = ltf["coarse_pos"] + tr.SPAN < n
    q = ltf["quality"]
    assert np.isfinite(q).all() and ((q[inside] > 0) & (q[inside] <= 1)).all()
    assert not q[~inside].any() and not ltf["shift"][~inside].any()
    rec = ltf["records"]
    assert np.array_equal(rec["packet_pos"], ltf["positions"])
    assert np.array_equal(rec["packet_idx"], rec["packet_pos"].astype(np.int32)) and not rec["reserved8"].any()
    # a record that did not move is the untimed record, eq included
    keep = np.nonzero(ltf["shift"] == 0)[0]
    assert rec[keep].tobytes() == none["records"][keep].tobytes()
    keep_dev = _torch().from_numpy(keep).cuda()
    assert dev_same_bits(ltf["eq"][keep_dev], none["eq"][keep_dev])
    return inside, keep


def _subset_against_fp64(r, ltf, picks, tmpl):
    """the records `picks`: their 641 samples [p, p + 641) from the device in one gather, stream.refine_timing on them
    with the oracle's template; shift exactly and quality under test_gpu_timing's bound.  Returns the largest quality
    deviation and the smallest relative gap between the two largest fp64 L."""
    from ofdm_amd.stream import refine_timing
    torch = _torch()
    picks = np.asarray(picks)
    coarse = ltf["coarse_pos"][picks]
    assert (coarse >= 0).all() and (coarse + tr.SPAN < r["n"]).all()
    at = torch.from_numpy(coarse).cuda()[:, None] + torch.arange(tr.SPAN + 1, device="cuda")[None, :]
    y = r["noisy"][at].cpu().numpy().reshape(-1)
    want = refine_timing(y, (tr.SPAN + 1) * np.arange(len(picks)), tmpl)
    gap = float(tr.top_gap(want["metric"]).min())
    dev = float(np.abs(ltf["quality"][picks].astype(np.float64) - want["quality"]).max())
    print(f"timing {r['name']}: {len(picks)} records against fp64: smallest gap between the two largest L {gap:.3g}, shifts "
          f"{int(want['shift'].min())}..{int(want['shift'].max())}, quality {want['quality'].min():.3f}..{want['quality'].max():.3f}, "
          f"largest quality deviation {dev:.3g} (4 x TIMING_DEV_MEASURED {4 * TIMING_DEV_MEASURED:.3g})")
    assert gap > 1.2e-4                                               # before equality is demanded
    assert np.array_equal(ltf["shift"][picks], want["shift"])
    assert 4 * TIMING_DEV_MEASURED < 6e-5 and dev <= 4 * TIMING_DEV_MEASURED
    return dev, gap


def test_timing_when_the_packet_loop_wraps(eng, pkg, dev, timed, recs, tmpl):
    r = recs["B"]
    none, ltf = timed["B"]["none"], timed["B"]["ltf"]
    count, trip = ltf["count"], _timing_trip(dev)
    full, ragged = count // trip, count % trip
    print(f"timing B: {count} records on {TM_BLOCKS_PER_CU * dev['cus']} blocks of {TM_WAVES} waves: {count / trip:.2f} trips of "
          f"{trip} ({full} full, {ragged} records in the last)")
    assert count > trip and ragged != 0                              # more than one trip, the last one ragged
    inside, keep = _whole_run_assertions(r, none, ltf)
    assert inside.all()                                               # B ends in a closing gap of 1,000
    print(f"timing B: shifts {int(ltf['shift'].min())}..{int(ltf['shift'].max())}, {count - len(keep)} records moved, quality "
          f"{ltf['quality'].min():.3f}..{ltf['quality'].max():.3f}")
    # every record that belongs to a transmitted packet sits at its first sample + 16
    off, _ = tr.offsets(ltf["positions"], r["pos"])
    real = (off >= 0) & (off < 100)
    coff, _ = tr.offsets(none["positions"], r["pos"])
    print(f"timing B: {int(real.sum())} records within a packet's first 100 samples, coarse offsets "
          f"{int(coff[real].min())}..{int(coff[real].max())}, refined {sorted(set(off[real].tolist()))}")
    assert real.sum() > 0.99 * count and (off[real] == OFFSET).all()
    # the fp64 rule on the first records, the ragged trip and 1,000 seeded records of each full trip
    rng = np.random.default_rng(0x71317)
    picks = list(range(64)) + list(range(count - ragged, count))
    for t in range(full):
        picks += (t * trip + rng.choice(trip, 1000, replace=False)).tolist()
    picks = np.unique(picks)
    assert len(picks) >= 64 + ragged + 1000 * full - 64 and (picks // trip).max() == full
    _subset_against_fp64(r, ltf, picks, tmpl)
    # the counters row is the reduction of the records
    assert np.array_equal(ltf["row"], pkg.abi.reduce_capture_records(ltf["records"], r["d"]))


def test_timing_launch_shapes_at_the_wrap(eng, dev, timed, recs):
    r = recs["B"]
    full = timed["B"]["ltf"]
    trip = _timing_trip(dev)
    assert full["count"] > trip + 1
    for m in (trip, trip + 1):                                        # one exact trip with no wrap; one record into the second
        o = receive_opt(eng, r, r["noisy"], timing="ltf", max_packets=m, want_bits=True, want_eq=True, keep_device=True)
        blocks = min(-(-m // TM_WAVES), TM_BLOCKS_PER_CU * dev["cus"])
        print(f"timing B, max_packets {m}: {blocks} blocks, {-(-m // (blocks * TM_WAVES))} trips; found {o['found']}, count {o['count']}")
        assert o["found"] == full["found"] and o["count"] == m
        assert o["records"].tobytes() == full["records"][:m].tobytes()
        assert o["d_timing"][:m].cpu().numpy().tobytes() == full["d_timing"][:m].cpu().numpy().tobytes()
        assert bool(_torch().equal(o["d_words"][:m], full["d_words"][:m])) and dev_same_bits(o["eq"], full["eq"][:m])


def test_timed_decode_at_the_moved_positions(eng, oracle, timed, recs):
    """64 seeded records whose position the timing kernel moved, against the oracle's decode_at at the refined position
    on the recording's own samples.  (Receiver()'s own Packet_Selection on a window cut at the refined position finds
    its own coarse position, not the refined one, so receive_captures cannot stand in here as it does for the untimed
    records of test_decode_when_the_loop_wraps_impaired; records that did not move are byte-identical to those.)"""
    from ofdm_amd.stream import pack_messages
    torch = _torch()
    for name in "BA":
        r = recs[name]
        d = r["d"]
        ltf = timed[name]["ltf"]
        moved = np.nonzero(ltf["shift"])[0]
        nfr = 320 + 80 * d
        L = 2 * nfr + 100
        ok = moved[(ltf["positions"][moved] - 40 >= 0) & (ltf["positions"][moved] - 40 + L <= r["n"])]
        picks = np.sort(np.random.default_rng(0x5EED + d).choice(ok, 64, replace=False))
        at = torch.from_numpy(ltf["positions"][picks] - 40).cuda()[:, None] + torch.arange(L, device="cuda")[None, :]
        caps = r["noisy"][at].cpu().numpy().astype(np.complex128)
        truth = bits_of(pack_messages([TEXT[d]], d)[0])[0]
        ora = [oracle.decode_at(c, truth, 40, dumps=True, cap_len=L) for c in caps]
        rec = ltf["records"][picks].copy()
        rec["packet_idx"] = 40
        rec["flags"] &= 3
        picks_dev = torch.from_numpy(picks).cuda()
        bits, eq = ltf["bits"][picks_dev].cpu().numpy(), ltf["eq"][picks_dev].cpu().numpy()
        same = check_against_oracle(rec, bits, eq, ora, list(caps), truth, 0)
        cfo_dev = max(max(abs(float(rec["cfo_coarse_hz"][k]) - float(ora[k]["cfo"][0])),
                          abs(float(rec["cfo_fine_hz"][k]) - float(ora[k]["cfo"][1]))) for k in same)
        print(f"timed decode {name}: {len(moved)} records moved (shifts {sorted(set(ltf['shift'][picks].tolist()))} among the 64 picked), "
              f"CFO estimates within {cfo_dev:.4g} Hz of the oracle's")
        assert len(same) == 64 and cfo_dev <= CFO_TOL_HZ


def test_timing_on_fifteen_symbol_packets_at_the_decode_wrap(eng, pkg, dev, timed, recs, tmpl):
    r = recs["A"]
    none, ltf = timed["A"]["none"], timed["A"]["ltf"]
    count, trip = ltf["count"], _timing_trip(dev)
    print(f"timing A: {count} records, {count / trip:.2f} trips of the timing grid ({trip}): "
          f"{'wraps' if count > trip else 'does not wrap on this device'}; the decode loop wraps past {SDEC_MAX_WAVES * dev['cap']}")
    assert count > SDEC_MAX_WAVES * dev["cap"]
    inside, keep = _whole_run_assertions(r, none, ltf)
    off, _ = tr.offsets(ltf["positions"], r["pos"])
    real = (off >= 0) & (off < 100)
    print(f"timing A: {count - len(keep)} records moved, refined offsets {sorted(set(off[real].tolist()))}, quality "
          f"{ltf['quality'][inside].min():.3f}..{ltf['quality'].max():.3f}")
    assert real.sum() > 0.99 * count and (off[real] == OFFSET).all()
    picks = np.sort(np.random.default_rng(0xA71).choice(np.nonzero(inside)[0], 200, replace=False))
    _subset_against_fp64(r, ltf, picks, tmpl)
    assert np.array_equal(ltf["row"], pkg.abi.reduce_capture_records(ltf["records"], r["d"]))


# ---- scoring refined positions
def _score_window(eng, r, o, window):
    """Engine.score_packets and stream.score_packets on the same records with a window: the device totals"""
    from ofdm_amd.stream import score_packets
    dev_out = eng.score_packets(r["words"], r["d"], o, positions=r["pos_dev"], window=window)
    scores, totals = dev_out["scores"].cpu().numpy(), dev_out["totals"].cpu().numpy()
    rw = o["d_words"][:o["count"]].cpu().numpy().view(np.uint32)
    host = score_packets(r["pos"], r["words"].cpu().numpy().view(np.uint32), o["positions"], rw, window=window)
    assert np.array_equal(scores[:, 0], host["rx_index"]) and np.array_equal(scores[:, 1], host["bit_err"])
    assert np.array_equal(totals, host["totals"])
    return totals


def test_scoring_refined_positions(eng, pkg, timed, recs):
    from ofdm_amd.stream import SCORE_MAX_WINDOW
    abi = pkg.abi
    r = recs["B"]
    none, ltf = timed["B"]["none"], timed["B"]["ltf"]
    nearest = int(np.diff(ltf["positions"]).min())
    exact, default = _score_window(eng, r, ltf, (16, 16)), _score_window(eng, r, ltf, (8, 40))
    widest = _score_window(eng, r, ltf, (0, SCORE_MAX_WINDOW))
    coarse = _score_window(eng, r, none, (8, 40))
    print(f"score B refined: neighbouring records at least {nearest} apart (coarse {int(np.diff(none['positions']).min())}); matched "
          f"{exact[abi.S_MATCHED]} with (16, 16), {default[abi.S_MATCHED]} with (8, 40), {widest[abi.S_MATCHED]} with (0, 300), "
          f"{coarse[abi.S_MATCHED]} without timing; bit errors {default[abi.S_BIT_ERR]} against {coarse[abi.S_BIT_ERR]}")
    assert nearest >= 301 - 56 - 7 == 238
    assert SCORE_MAX_WINDOW == 300
    assert exact[abi.S_MATCHED] == default[abi.S_MATCHED] and np.array_equal(exact, default)
    assert default[abi.S_MATCHED] >= coarse[abi.S_MATCHED]
    assert widest[abi.S_MATCHED] >= default[abi.S_MATCHED]
