"""The batched receiver for caller-supplied captures (include/ofdm_mi355x_captures.h), the checks that need no GPU:
the extension header against the library and the binding, the record's layout as a C compiler sees it, the argument
checks that come before any device work, the kernel's resource report, and channel.make_captures on the CPU against a
numpy restatement and its noise statistics."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, normwise

MSG = b"Hey! I am Vivaswan"


def captures_header_functions():
    h = (ROOT / "include" / "ofdm_mi355x_captures.h").read_text()
    return sorted(set(re.findall(r"^\s*int\s+(ofdm_\w+)\(", h, re.M)))


def test_captures_header_is_exported_and_bound(pkg):
    abi = pkg.abi
    names = captures_header_functions()
    assert names == sorted(abi.CAPTURES_EXPORTS) == ["ofdm_receive_captures"]
    assert not set(names) & set(abi.EXPORTS) and not set(names) & set(abi.LONG_EXPORTS)
    assert abi.CAPTURES_HEADER.read_text().count('#include "ofdm_mi355x.h"') == 1
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    for name in names:
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), name
    assert lib.ofdm_abi_version() == 1 and abi.ABI_VERSION == 1
    # the base header is untouched by the extension
    base = (ROOT / "include" / "ofdm_mi355x.h").read_text()
    assert "ofdm_receive_captures" not in base and re.search(r"#define OFDM_ABI_VERSION 1\b", base)


def test_capture_result_layout_matches_the_header(pkg, tmp_path):
    abi = pkg.abi
    st = abi.CaptureResult
    assert C.sizeof(st) == 48
    fields = [n for n, _ in st._fields_]
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ofdm_mi355x_captures.h"\n'
                   "int main(void) { printf(\"%zu\", sizeof(ofdm_capture_result)); "
                   + " ".join(f'printf(" %zu", offsetof(ofdm_capture_result, {f}));' for f in fields)
                   + ' printf(" %d %d\\n", OFDM_CAPTURE_MAX_LEN, OFDM_NCOUNTERS); return 0; }\n')
    exe = tmp_path / "offsets"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got[0] == 48
    assert got[1:1 + len(fields)] == [getattr(st, f).offset for f in fields]
    assert got[-2:] == [abi.CAPTURE_MAX_LEN, abi.NCOUNTERS]
    dt = abi.capture_result_dtype()
    assert dt.itemsize == 48 and list(dt.names) == fields
    assert [dt.fields[f][1] for f in fields] == [getattr(st, f).offset for f in fields]


def test_argument_errors_come_before_any_device_work(pkg):
    lib = pkg.load_library()
    opts = pkg.abi.make_rx_opts("c")
    assert lib.ofdm_receive_captures(None, None, 1, 3008, C.byref(opts), 1, None, None, None, None) == -1
    assert lib.ofdm_last_error()


def test_capture_kernel_is_built_spill_free(pkg):
    from ofdm_amd import build_lib
    assert "ofdm_captures.hip" in build_lib.SOURCES
    rows = [x for x in json.loads(build_lib.RESOURCE_REPORT.read_text()) if x["source"] == "ofdm_captures.hip"]
    names = {x["name"] for x in rows}
    assert names == {"ofdm::capture_rx_kernel<true>", "ofdm::capture_rx_kernel<false>"}
    for x in rows:
        assert not x["dump_variant"]                                   # no spill allowance
        assert not x.get("VGPRs Spill", 0) and not x.get("ScratchSize [bytes/lane]", 0), x["name"]
        assert x["VGPRs"] <= 256                                       # eight-wave blocks: two waves per SIMD
    # the rows the shared chain (ofdm_rxchain.h) builds to
    assert {x["name"]: (x["VGPRs"], x["LDS Size [bytes/block]"]) for x in rows} == {
        "ofdm::capture_rx_kernel<true>": (235, 0), "ofdm::capture_rx_kernel<false>": (194, 0)}


def test_reduce_capture_records_rule(pkg):
    abi = pkg.abi
    rec = np.zeros(3, abi.capture_result_dtype())
    rec["flags"] = [0, 1, 3]
    rec["bit_err"] = [0, 7, 96]
    rec["post_axis_err"] = [0, 5, 90]
    rec["evm_pre_sum"] = np.float32([0.125, 3.5, 190.0])
    rec["evm_db_pre"] = np.float32([-28.5, -14.25, 3.0])
    rec["evm_db_post"] = np.float32([-np.inf, -12.5, -0.25])
    c = abi.reduce_capture_records(rec, 2)
    assert list(c[:7]) == [3, 6, 576, 103, 2, 2, 288]
    assert c[abi.C_EVM_PRE_Q] == (0.125 + 3.5 + 190.0) * 2 ** 20 and c[abi.C_EVM_POST_AXIS] == 95
    assert c[abi.C_EVMDB_PRE_Q] == (-28.5 - 14.25 + 3.0) * 2 ** 20
    assert c[abi.C_EVMDB_POST_Q] == (-12.75) * 2 ** 20 and c[abi.C_EVMDB_POST_FINITE] == 2
    assert c[abi.C_OOB] == 1 and not c[abi.C_WL_MIN_Q:].any()


def test_reduce_capture_records_leaves_non_finite_terms_out(pkg):
    """A capture that ends before its long training symbols has S = 0 and Z = 0 / 0: evm_pre_sum and evm_db_pre are
    NaN, and both are left out of the row, as a -inf evm_db_post is; everything else of the record counts."""
    abi = pkg.abi
    rec = np.zeros(3, abi.capture_result_dtype())
    rec["flags"] = [0, 2, 2]
    rec["bit_err"] = [0, 100, 96]
    rec["post_axis_err"] = [0, 101, 90]
    rec["evm_pre_sum"] = np.float32([0.125, np.nan, np.inf])
    rec["evm_db_pre"] = np.float32([-28.5, np.nan, np.inf])
    rec["evm_db_post"] = np.float32([-np.inf, 0.25, -0.25])
    c = abi.reduce_capture_records(rec, 2)
    assert list(c[:3]) == [3, 6, 576] and c[abi.C_EVM_TERMS] == 288
    assert c[abi.C_BIT_ERR] == 196 and c[abi.C_EVM_POST_AXIS] == 191
    assert c[abi.C_EVM_PRE_Q] == 0.125 * 2 ** 20 and c[abi.C_EVMDB_PRE_Q] == -28.5 * 2 ** 20
    assert c[abi.C_EVMDB_POST_Q] == 0 and c[abi.C_EVMDB_POST_FINITE] == 2 and c[abi.C_OOB] == 2


# ---------------------------------------------------------------- channel.make_captures on the CPU
@pytest.fixture(scope="module")
def wave(oracle):
    return oracle.frame_waveform(oracle.message_bits(MSG))             # 9800 samples, complex128


def test_make_captures_against_numpy(pkg, wave):
    import torch
    from ofdm_amd.channel import make_captures
    starts = np.array([0, 1234, 6791])
    cfos = np.array([0.0, 40e3, -90e3])
    taps = np.array([1, 0, 0.4 + 0.3j])
    got = make_captures(torch.from_numpy(wave.astype(np.complex64)), starts, 10.0, cfos, taps=taps, noise="none")
    assert got.dtype == torch.complex64 and tuple(got.shape) == (3, 3008) and got.device.type == "cpu"
    # the restatement: FIR over the whole waveform truncated to its length, rotation by absolute index, windows
    y = np.convolve(wave, taps)[:len(wave)]
    k = np.arange(len(wave))
    for i in range(3):
        ref = (y * np.exp(2j * np.pi * cfos[i] * k * 25e-9))[starts[i]:starts[i] + 3008]
        assert normwise(got[i].numpy(), ref) < 2e-6, i
    # no taps, no offset: the windows themselves; cap_len and broadcasting of a scalar start
    plain = make_captures(torch.from_numpy(wave.astype(np.complex64)), 17, [1.0, 2.0], noise="none", cap_len=500)
    assert tuple(plain.shape) == (2, 500)
    assert np.array_equal(plain[1].numpy(), wave[17:517].astype(np.complex64))
    with pytest.raises(ValueError):
        make_captures(torch.from_numpy(wave.astype(np.complex64)), 9800 - 3007, 10.0, noise="none")
    with pytest.raises(ValueError):
        make_captures(torch.from_numpy(wave.astype(np.complex64)), 0, 10.0, noise="pink")


@pytest.mark.parametrize("noise", ["real", "complex"])
def test_make_captures_noise_statistics(pkg, wave, noise):
    import torch
    from ofdm_amd.channel import make_captures
    w = torch.from_numpy(wave.astype(np.complex64))
    gen = torch.Generator()
    gen.manual_seed(7)
    starts = np.arange(64) * 100
    clean = make_captures(w, starts, 10.0, noise="none").numpy()
    got = make_captures(w, starts, 10.0, noise=noise, generator=gen).numpy()
    nz = got - clean
    P = np.mean(np.abs(wave) ** 2)
    var = np.mean(np.abs(nz.astype(np.complex128)) ** 2)
    assert abs(var / (P / 10.0) - 1.0) < 0.05
    if noise == "real":
        assert not nz.imag.any()
    else:
        assert abs(np.mean(nz.real.astype(np.float64) ** 2) / (P / 20.0) - 1.0) < 0.05
        assert abs(np.mean(nz.imag.astype(np.float64) ** 2) / (P / 20.0) - 1.0) < 0.05
