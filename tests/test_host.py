"""Host-side checks that need no GPU: the C-ABI library loads and exports every symbol its header
declares, the ctypes structs match the header, the file writer keeps the reference format."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle.orc import REF_SRC


def header_functions():
    h = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(ofdm_\w+)\(", h, re.M)))


def test_header_matches_binding(pkg):
    assert header_functions() == sorted(pkg.abi.EXPORTS)


def test_library_loads_and_exports(pkg):
    lib = pkg.load_library()      # raises if the HIP library is missing: no fallback
    for name in header_functions():
        assert hasattr(lib, name), name
    assert lib.ofdm_abi_version() == pkg.abi.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", str(pkg.abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in header_functions():
        assert re.search(rf"\bT {name}\b", out), name


def test_library_has_gfx950_code_object(pkg):
    # the embedded HIP fat binary names its only target
    blob = pkg.abi.LIB_PATH.read_bytes()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob


def test_product_kernels_do_not_spill(pkg):
    # build_lib writes hipcc's resource-usage remarks next to the objects and refuses a spilling build;
    # this re-reads that report so a stale library built before the check cannot slip through
    from ofdm_amd import build_lib
    if not build_lib.RESOURCE_REPORT.exists():
        pytest.skip("library not built in this tree (no resource report)")
    rows = json.loads(build_lib.RESOURCE_REPORT.read_text())
    names = {x["name"] for x in rows}
    for k in ("ofdm::rx_pack_kernel<0, 0, 0, false>", "ofdm::rx_pack_kernel<2, 0, 0, false>",
              "ofdm::rx_pack_kernel<2, 0, 1, false>", "ofdm::frame_sync_kernel<2, 3008, 12>", "ofdm::frame_sync_kernel<0, 0, 4>",
              "ofdm::frame_sync_kernel<0, 0, 1>", "ofdm::frame_sym_kernel<false, 2>",
              "ofdm::frame_sym_kernel<false, 0>",
              "ofdm::rx_ls_kernel<1, 1, false>", "ofdm::tx_symbols_kernel<0>"):
        assert k in names, k
    assert build_lib.spilling_kernels(rows) == []


def test_struct_layout(pkg):
    import ctypes as C
    assert C.sizeof(pkg.abi.Cfg) == 48
    assert C.sizeof(pkg.abi.RxOpts) == 32


def test_errors_without_context(pkg):
    lib = pkg.load_library()
    # a NULL context must be rejected with an error code and a message, never exit()
    rc = lib.ofdm_fft64(None, None, None, 0, 0, 0)
    assert rc == -1 and b"bad" in lib.ofdm_last_error()
    rc = lib.ofdm_tx_bytes(-1, None, None)
    assert rc == -1


def test_every_entry_point_rejects_a_null_context(pkg):
    """Each entry point that takes an ofdm_ctx returns OFDM_E_ARG with a message for a NULL context (all
    other arguments zero / NULL), before any HIP call: an error code, never a crash or exit()."""
    import ctypes as C
    from ofdm_amd import abi
    lib = pkg.load_library()
    checked = 0
    for name, (_, argtypes) in abi._SIGS.items():
        if not argtypes or argtypes[0] is not abi._V or name == "ofdm_ctx_destroy":   # destroy(NULL) is a no-op
            continue
        args = [None if t in (abi._V, C.c_char_p) or t.__name__.startswith("LP_") else 0 for t in argtypes]
        rc = getattr(lib, name)(*args)
        assert rc == -1, (name, rc)
        assert lib.ofdm_last_error(), name
        checked += 1
    assert checked == len([n for n, (_, t) in abi._SIGS.items() if t and t[0] is abi._V]) - 1, checked
    assert lib.ofdm_ctx_destroy(None) == 0


def test_tx_bytes(pkg):
    import ctypes as C
    lib = pkg.load_library()
    tb, bb = C.c_int64(), C.c_int64()
    assert lib.ofdm_tx_bytes(17, C.byref(tb), C.byref(bb)) == 0
    # 17 frames = 34 symbols -> pitch = 64 (whole wave) + 64 (guard wave); rows of 80 samples x 8 B
    assert tb.value == 80 * 128 * 8 and bb.value == 10 * 128 * 4    # 3 payload + 4 demap + 3 pair-order words
    assert lib.ofdm_tx_bytes(1 << 23, C.byref(tb), C.byref(bb)) == 0
    assert lib.ofdm_tx_bytes((1 << 23) + 1, C.byref(tb), C.byref(bb)) == -1     # int32 element offsets


def test_write_float_array_format(pkg, tmp_path):
    p = tmp_path / "x.txt"
    pkg.write_float_array_to_file([6, -10.84, float("-inf"), 0.0, 3.5e-5], p)
    assert p.read_text() == "6.00e+00\t-1.08e+01\t-inf\t0.00e+00\t3.50e-05\n"
    assert np.allclose(pkg.read_float_array_file(p)[[0, 1, 3, 4]], [6, -10.8, 0, 3.5e-5])


def test_reference_files_parse(pkg, tmp_path):
    files = json.loads((GOLDEN / "reference_data.json").read_text())
    for name, text in files.items():
        (tmp_path / name).write_text(text)
        v = pkg.read_float_array_file(tmp_path / name)
        assert len(v) == 35
    snr = pkg.read_float_array_file(tmp_path / "Output_SNR.txt")
    assert np.array_equal(snr, np.arange(6, 41))


def test_write_reference_outputs_refuses_missing_dir(pkg, tmp_path):
    with pytest.raises(FileNotFoundError):
        pkg.write_reference_outputs(tmp_path / "nope", [1], [1], [1], [1])


# The reference tree (its scripts/ and data/), where it is present: next to the source the oracle's `ref`
# recipe compiles (OFDM_REF_SRC).  os.path.exists: a tree this user may not enter counts as absent.  The tests
# below check the project's files on their own and, where the tree is here, also run its scripts unchanged.
REF_TREE = REF_SRC.parent.parent
REF_SCRIPTS = REF_TREE / "scripts"
HAVE_REF_SCRIPTS = os.path.exists(REF_SCRIPTS / "compare_double.py") and os.path.exists(REF_SCRIPTS / "OFDM_Plotting.py")
GPU_KAT_FILE = GOLDEN / "gpu_kat_Code_Output.txt"
MATLAB_FILE = GOLDEN / "Matlab_Output.txt"         # the reference's data/Matlab_Output.txt, byte for byte


def _script_numbers(text):
    """A result file as the reference's scripts read it (compare_double.py / OFDM_Plotting.py read_double_file):
    newlines to blanks, split on white space, every word a float; the plotting script maps INF / inf words by sign
    and NaN / #J / #IND words to -40."""
    out = []
    for w in text.replace("\n", " ").split():
        if "INF" in w or "inf" in w:
            out.append(float("-inf") if "-" in w else float("inf"))
        elif "NaN" in w or "#J" in w or "#IND" in w:
            out.append(-40.0)
        else:
            out.append(float(w))
    return out


def test_reference_plotting_script_reads_our_files(pkg, tmp_path):
    """scripts/OFDM_Plotting.py must drop in unchanged.  The four files write_reference_outputs leaves in data/ parse
    by the script's own reading rule into the 35 values written, in the layout of the reference's own result files
    (tests/golden/reference_data.json: tab-separated words, one line).  Where the reference tree is present
    the script itself is run as well: it resolves data/ and results/ relative to its own location, so it runs from a
    scratch copy of its directory layout."""
    base = tmp_path / "ref"
    (base / "scripts").mkdir(parents=True)
    (base / "data").mkdir()
    snr = np.arange(6, 41)
    evm, evm_agc, ber = -snr - 1.3, np.full(35, -np.inf), np.where(snr < 10, 1e-2, 0)
    pkg.write_reference_outputs(base / "data", snr, evm, evm_agc, ber)
    theirs = json.loads((GOLDEN / "reference_data.json").read_text())
    assert sorted(p.name for p in (base / "data").iterdir()) == sorted(theirs)
    for name, want in (("Output_SNR.txt", snr), ("Output_EVM_AGC.txt", evm), ("Output_EVM_AGC_DB.txt", evm_agc),
                       ("Output_BER.txt", ber)):
        text = (base / "data" / name).read_text()
        got = _script_numbers(text)
        assert len(got) == 35 == len(_script_numbers(theirs[name])), name
        # %.2e as the reference writes it: three significant digits
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.allclose(got, want, rtol=5.1e-3, atol=0), name
        assert text.count("\n") == theirs[name].count("\n") and text.count("\t") == theirs[name].count("\t"), name
    import importlib.util
    if not HAVE_REF_SCRIPTS or importlib.util.find_spec("matplotlib") is None:      # the script plots with it
        return
    import shutil
    shutil.copy(REF_SCRIPTS / "OFDM_Plotting.py", base / "scripts")
    r = subprocess.run([sys.executable, str(base / "scripts" / "OFDM_Plotting.py")], capture_output=True, text=True,
                       env={"MPLBACKEND": "Agg", "PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stderr
    assert "Extracted 35 valid numbers" in r.stdout
    assert (base / "results" / "ber_vs_snr.png").exists()


def _kat_mismatches(code_output_text):
    """compare_double.py's verdict, restated: both files hold 96 numbers and the indices whose absolute difference
    exceeds its tolerance 1e-6 (compare_double.py:41-42) are returned."""
    ours, theirs = _script_numbers(code_output_text), _script_numbers(MATLAB_FILE.read_text())
    assert len(ours) == len(theirs) == 96
    return [i for i, (a, b) in enumerate(zip(ours, theirs)) if abs(a - b) > 1e-6]


def _run_compare_double(cwd, code_output_text):
    """scripts/compare_double.py unchanged, as its __main__ runs it: Code_Output.txt against
    Matlab_Output.txt in the current directory with tolerance 1e-6 (compare_double.py:41-42)."""
    import shutil
    cwd.mkdir(parents=True, exist_ok=True)
    shutil.copy(REF_SCRIPTS / "compare_double.py", cwd)
    assert (REF_TREE / "data" / "Matlab_Output.txt").read_bytes() == MATLAB_FILE.read_bytes()
    shutil.copy(MATLAB_FILE, cwd)
    (cwd / "Code_Output.txt").write_text(code_output_text)
    r = subprocess.run([sys.executable, "compare_double.py"], cwd=cwd, capture_output=True, text=True,
                       env={"PATH": "/usr/bin:/bin"})
    assert r.returncode == 0, r.stderr
    return r.stdout


def _assert_compare_double_clean(out):
    assert out.count("Extracted 96 numbers.") == 2, out          # equal lengths: no early return
    assert "Files have different lengths" not in out
    assert "Max Error: 0.000000e+00" in out, out
    assert "Average Error: 0.000000e+00" in out, out
    assert "Mismatch" not in out, out


def test_reference_compare_double_reads_our_code_output(pkg, oracle, tmp_path):
    """north_star: scripts/compare_*.py drop in unchanged.  The KAT receiver's bits (frame mode, MATLAB
    convention, Tester payload, noiseless capture [0, 3000): D6) written by fileio.write_bits_file are
    diffed against data/Matlab_Output.txt (tests/golden/Matlab_Output.txt) by compare_double.py's rule: zero
    mismatches.  Where the reference tree is present, the unmodified compare_double.py does the same diff.
    (a) bits of the oracle's KAT receiver (equal to the GPU's: tests/test_gpu_frame.py::test_matlab_known_answer);
    (b) the Code_Output.txt the GPU KAT test wrote on an MI355X (tests/golden/gpu_kat_Code_Output.txt)."""
    from ofdm_amd import fileio
    tb = oracle.tester_bits()
    w = oracle.frame_waveform(tb, "matlab", False, 10)
    o = oracle.receiver_frame(w[:3000], tb, "matlab")
    p = tmp_path / "bits.txt"
    fileio.write_bits_file(o["bits"][:96], p)
    assert GPU_KAT_FILE.exists(), "the GPU KAT record is committed with the tests"
    # the check is not vacuous: one flipped bit is reported as a mismatch
    bad = p.read_text().split("\t")
    bad[5] = str(1 - int(bad[5]))
    assert _kat_mismatches(p.read_text()) == []
    assert _kat_mismatches(GPU_KAT_FILE.read_text()) == []
    assert _kat_mismatches("\t".join(bad)) == [5]
    if not HAVE_REF_SCRIPTS:
        return
    _assert_compare_double_clean(_run_compare_double(tmp_path / "a", p.read_text()))
    _assert_compare_double_clean(_run_compare_double(tmp_path / "b", GPU_KAT_FILE.read_text()))
    out = _run_compare_double(tmp_path / "c", "\t".join(bad))
    assert "Mismatch at index 5" in out and "Max Error: 1.000000e+00" in out


def test_shard_ranges(pkg):
    from ofdm_amd import dist
    for n in (0, 1, 7, 1000, 10 ** 7 + 3):
        for w in (1, 2, 3, 8):
            rs = [dist.shard_range(n, r, w) for r in range(w)]
            assert rs[0][0] == 0 and rs[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(rs, rs[1:]))


def test_allreduce_refuses_world_without_group(pkg, monkeypatch):
    """a sharded sweep must never be written from one rank's share: with WORLD_SIZE > 1
    and no process group the reduction raises instead of silently returning."""
    import torch
    from ofdm_amd import dist as odist
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(odist.DistError):
        odist.allreduce_counters(torch.zeros((2, 16), dtype=torch.int64))
    with pytest.raises(odist.DistError):
        odist.allreduce_counters_np(np.zeros((2, 16), np.int64))
    monkeypatch.setenv("WORLD_SIZE", "1")
    c = np.arange(32, dtype=np.int64).reshape(2, 16)
    assert odist.allreduce_counters_np(c) is c


def test_mean_trial_evm_semantics(pkg):
    """Output_EVM_AGC*.txt values for trials > 1: mean of the per-trial EVM_dB; the post-slicer mean
    is -inf once any trial had no slicer error (that trial's own value is -inf, OFDM.c:1148-1150)."""
    from ofdm_amd import abi
    c = np.zeros((2, 16), np.int64)
    c[:, abi.C_FRAMES] = 4
    c[:, abi.C_EVMDB_PRE_Q] = [-40 << 20, 8 << 20]
    c[:, abi.C_EVMDB_POST_Q] = [0, 6 << 20]
    c[:, abi.C_EVMDB_POST_FINITE] = [0, 4]
    r = pkg.SweepResult(np.array([30.0, 0.0]), c)
    assert list(r.mean_frame_evm_db) == [-10.0, 2.0]
    assert np.isneginf(r.mean_frame_evm_post_db[0]) and r.mean_frame_evm_post_db[1] == 1.5
    # --evm finite: the post-slicer mean over the finite trials only (-inf only with none finite)
    c[0, abi.C_EVMDB_POST_Q], c[0, abi.C_EVMDB_POST_FINITE] = -30 << 20, 2
    r = pkg.SweepResult(np.array([30.0, 0.0]), c)
    assert np.isneginf(r.mean_frame_evm_post_db[0])
    assert list(r.mean_finite_frame_evm_post_db) == [-15.0, 1.5]
    c[0, abi.C_EVMDB_POST_FINITE] = 0
    assert np.isneginf(pkg.SweepResult(np.array([30.0, 0.0]), c).mean_finite_frame_evm_post_db[0])


def test_reference_symbol_chain_baseline_is_the_genie_workload(reflib):
    """bench.py's cpu_baseline for c2-c5 runs the reference's own stage functions as the genie symbol
    chain (ref_harness.c ref_time_symbol_chain): its BER at 0 / 4 dB is the genie fixture's."""
    rows = {r["snr_db"]: r for r in json.loads((GOLDEN / "ref_genie_ls_curve.json").read_text())["rows"]}
    for snr, n in ((0.0, 3000), (4.0, 6000)):
        t, acc = reflib.time_symbol_chain([snr], n)
        ber, ref = acc[0] / acc[1], rows[snr]["bit_err"] / rows[snr]["bits"]
        sd = np.sqrt(ref / acc[1] + ref / rows[snr]["bits"]) * 3      # ~3 bit errors per error event
        assert abs(ber - ref) < 5 * sd, (snr, ber, ref)
        assert t > 0
