#!/usr/bin/env python3
"""Record the packed receivers' counters of the loaded library into an .npz (tests/pack_exact_cases.py's runs).

tests/golden/pack_counters_parent.npz is this script's output with the library of the commit before the truth signs
moved from the pair-order words to the clean spectra (OFDM_MI355X_LIB pointing at that build):
    OFDM_MI355X_LIB=variants/libofdm_parent.so python3 tools/record_pack_counters.py tests/golden/pack_counters_parent.npz
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ofdm_pkg  # noqa: E402
import pack_exact_cases as pc  # noqa: E402


def set_cap(cap):
    if cap is None:
        os.environ.pop("OFDM_RX_GRID_CAP", None)
    else:
        os.environ["OFDM_RX_GRID_CAP"] = str(cap)


def main():
    out = Path(sys.argv[1])
    pkg = ofdm_pkg.load()
    rec = {}
    with pkg.Engine(0) as eng:
        for kw in pc.PACKED:
            for case in pc.CASES:
                for path, cnt in pc.run_case(eng, pkg, kw, case, set_cap).items():
                    rec[pc.key(kw, case, path)] = np.asarray(cnt, np.int64)
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} arrays -> {out} ({out.stat().st_size} bytes), library {pkg.abi.library_file()}")


if __name__ == "__main__":
    main()
