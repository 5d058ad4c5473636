"""The GEMM dispatch (csrc/gemm_route.h) as host code: every route of a sweep over shapes, epilogue forms and
switches names an instantiation that exists with a grid and offsets its kernel can take, and routes derived by
hand from the rules stay pinned (csrc/selftest_gemm_route.cpp, built with ASan+UBSan, run directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_gemm_route_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_selftest("gemm_route", build.SELFTESTS["gemm_route"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_gemm_route ok" in r.stdout
