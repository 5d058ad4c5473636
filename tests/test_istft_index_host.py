"""The iSTFTNet head's index arithmetic (csrc/istft_index.h) as host code: tile -> frames -> rows -> samples and
the window envelope against a brute-force overlap-add, every T in 2..200 at tile heights 32 / 64 / 128
(csrc/selftest_istft_index.cpp, built with ASan+UBSan, run directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_istft_index_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_istft_selftest()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_istft_index ok" in r.stdout
