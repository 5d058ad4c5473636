"""The DTW direction-plane index arithmetic (csrc/dtw_index.h) as host code: a scalar DTW through the header's
indexing against a plain 2-D-array DTW, every plane byte stored exactly once, 64-bit plane sizes
(csrc/selftest_dtw_index.cpp, built with ASan+UBSan, run directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_dtw_index_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_dtw_selftest()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_dtw_index ok" in r.stdout
