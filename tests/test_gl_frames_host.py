"""The Griffin-Lim index arithmetic (csrc/gl_frames.h) as host code: covering-frame ranges against a brute-force
scan, reflected indices in range, every sample read (csrc/selftest_gl_frames.cpp, built with ASan+UBSan, run
directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_gl_frames_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_gl_selftest()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_gl_frames ok" in r.stdout
