"""gcc build of tests/c_caller/stream_caller.c against include/ofdm_mi355x.h, include/ofdm_mi355x_stream.h and
libofdm_mi355x.so.  The program allocates its device buffers with three HIP runtime calls it declares itself, so it
links libamdhip64 from the ROCm tree the library was built with.  Test infrastructure; __graft_entry__.build() builds
the binary in-tree so it travels with the library.
"""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
SRC = HERE / "stream_caller.c"
OUT = HERE / "_build"


def build(lib: Path, hipcc: str, out_dir: Path = OUT) -> Path:
    """Compile + link the caller (rpath to the library's directory and to ROCm's).  Raises RuntimeError with gcc's
    output on failure."""
    out_dir.mkdir(parents=True, exist_ok=True)
    exe = out_dir / "stream_caller"
    lib = Path(lib).resolve()
    rocm_lib = Path(hipcc).resolve().parent.parent / "lib"
    rpath = "$ORIGIN/" + os.path.relpath(lib.parent, out_dir.resolve())
    cmd = ["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(SRC), "-o", str(exe),
           f"-L{lib.parent}", "-l:" + lib.name, f"-L{rocm_lib}", "-lamdhip64", f"-Wl,-rpath,{rpath}", f"-Wl,-rpath,{rocm_lib}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"gcc failed:\n{r.stderr[-4000:]}")
    return exe
