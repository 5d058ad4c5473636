"""The attention block map (csrc/attn_blockmap.h) as host code: a bijection that keeps a sequence's
blocks on one XCD residue (csrc/selftest_attn_blockmap.cpp, built with ASan+UBSan, run directly)."""
import os
import shutil
import subprocess
import sys

import pytest


def test_attn_blockmap_selftest():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "csrc"))
    import build

    exe = build.build_blockmap_selftest()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_attn_blockmap ok" in r.stdout
