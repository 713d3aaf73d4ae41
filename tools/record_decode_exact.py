#!/usr/bin/env python3
"""Record the raw outputs of the capture, stream and tracking receivers of the loaded library into an .npz
(tests/decode_exact_cases.py's runs).

tests/golden/decode_chain_parent.npz is this script's output with the library of the commit before the three kernels'
copies of the post-selection chain became csrc/ofdm_rxchain.h (OFDM_MI355X_LIB pointing at that build):
    OFDM_MI355X_LIB=variants/libofdm_parent.so python3 tools/record_decode_exact.py tests/golden/decode_chain_parent.npz
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ofdm_pkg  # noqa: E402
import decode_exact_cases as dc  # noqa: E402


def main():
    out = Path(sys.argv[1])
    pkg = ofdm_pkg.load()
    rec = {}
    with pkg.Engine(0) as eng:
        for name in dc.STREAMS:
            rec.update(dc.run_stream(eng, pkg, name))
        for name in dc.CAPTURES:
            rec.update(dc.run_captures(eng, pkg, name))
    assert sorted(rec) == sorted(dc.all_keys())
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **rec)
    print(f"{len(rec)} arrays -> {out} ({out.stat().st_size} bytes), library {pkg.abi.library_file()}")


if __name__ == "__main__":
    main()
