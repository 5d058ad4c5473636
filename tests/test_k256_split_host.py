"""The K = 256 GEMM work split (csrc/k256_split.h) as host code: contiguous chunk ranges, equal to within
one chunk, no empty block (csrc/selftest_k256_split.cpp, built with ASan+UBSan, run directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_k256_split_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_k256_selftest()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_k256_split ok" in r.stdout
