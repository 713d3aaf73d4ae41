#!/usr/bin/env python3
"""Record the outputs of the packet, fading and frame transmitters of the loaded library into an .npz
(tests/transmit_exact_cases.py's runs).

tests/golden/transmit_chain_parent.npz is this script's output with the library of the commit before
csrc/ofdm_txchain.h existed (OFDM_MI355X_LIB pointing at that build):
    OFDM_MI355X_LIB=variants/libofdm_parent.so python3 tools/record_transmit_exact.py tests/golden/transmit_chain_parent.npz
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ofdm_pkg  # noqa: E402
import transmit_exact_cases as tc  # noqa: E402


def main():
    out = Path(sys.argv[1])
    pkg = ofdm_pkg.load()
    rec = {}
    with pkg.Engine(0) as eng:
        for kernel in tc.PACKETS:
            for name in tc.PACKETS[kernel]:
                rec.update(tc.run_packets(eng, kernel, name))
        for conv in tc.CONVS:
            for nd in tc.WAVE_SYMBOLS:
                rec.update(tc.run_wave(eng, conv, nd))
            rec.update(tc.run_sweep(eng, pkg, conv))
    assert sorted(rec) == sorted(tc.all_keys())
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} arrays -> {out} ({out.stat().st_size} bytes), library {pkg.abi.library_file()}")


if __name__ == "__main__":
    main()
