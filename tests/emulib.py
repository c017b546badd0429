"""The CPU lane emulators of tests/emu, compiled on demand: the one builder every ``*_cases.py`` module loads its emulator through.

``library("emu_fit")`` is tests/emu/libemu_fit.so, compiled first when it is missing or older than tests/emu/emu_fit.cpp, any header next
to it, or ANY header of regularizepsf_amd/csrc - no list of headers to keep by hand.  Without a compiler that is an error, not a skip.
"""

from __future__ import annotations

import ctypes
import os
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
EMU = ROOT / "tests" / "emu"


def compiler() -> str:
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not pathlib.Path(clang).exists():
        clang = shutil.which("clang++") or shutil.which("hipcc")
    assert clang is not None, "no clang++ to build the emulators of tests/emu"
    return clang


def is_stale(out: pathlib.Path, src: pathlib.Path) -> bool:
    headers = [*(ROOT / "regularizepsf_amd" / "csrc").glob("*.hpp"), *EMU.glob("*.hpp")]
    return not out.exists() or out.stat().st_mtime < max(p.stat().st_mtime for p in [src, *headers])


def library(stem: str) -> ctypes.CDLL:
    src, out = EMU / f"{stem}.cpp", EMU / f"lib{stem}.so"
    if is_stale(out, src):
        fresh = out.with_name(f"lib{stem}.{os.getpid()}.so")  # written aside and moved into place: test processes may run side by side
        subprocess.run([compiler(), "-std=c++20", "-O1", "-shared", "-fPIC", "-o", str(fresh), str(src)], check=True)
        os.replace(fresh, out)
    return ctypes.CDLL(str(out))
