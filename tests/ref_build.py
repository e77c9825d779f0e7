"""The one place where a scalar CPU restatement (tests/*_ref.c) becomes a loaded library.

TEST INFRASTRUCTURE ONLY: nothing under feature_tracker_amd/ may import it, and it imports nothing from there.  Bit identity of device
results to the restatements is the project's main correctness claim, so the flags that make a restatement mean what it says stand here:
``STRICT`` keeps gcc from contracting a * b + c into an fma the source did not write and from any fast-math rewrite.  A restatement
whose flags differ passes its own list and says why in a comment at the call.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

STRICT = ["-O3", "-std=c99", "-ffp-contract=off", "-fno-fast-math"]


def _cpu_has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


# for the restatements that call fmaf: one instruction instead of a libm call, the same correctly rounded operation either way
FMA = ["-mfma"] if _cpu_has_fma() else []

_tmpdir = None  # one directory for every restatement, removed when the process ends; nothing is written into the tree
_libs = {}


def compile_ref(stem, sources, flags=STRICT, libs=("-lm",)) -> ctypes.CDLL:
    """``gcc flags -shared -fPIC -o <tmp>/lib<stem>.so sources libs``, loaded; compiled once per ``stem`` per process.  A compile
    error raises CalledProcessError with gcc's text in ``stderr``."""
    global _tmpdir
    if stem not in _libs:
        if _tmpdir is None:
            _tmpdir = tempfile.TemporaryDirectory(prefix="ftk_ref_")
        path = os.path.join(_tmpdir.name, f"lib{stem}.so")
        subprocess.run(["gcc"] + list(flags) + ["-shared", "-fPIC", "-o", path] + list(sources) + list(libs), check=True, capture_output=True)
        _libs[stem] = ctypes.CDLL(path)
    return _libs[stem]
