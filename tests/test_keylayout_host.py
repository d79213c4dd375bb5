# Host half of include/bk_keylayout.h: tests/keylayout_roundtrip.cpp is a
# stand-alone program (its own main, only bk_common.h and the shared header)
# built here with the plain host compiler and run once. No GPU.
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keylayout_round_trip_and_finalize(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the host check of bk_keylayout.h needs it")
    exe = str(tmp_path / "keylayout_roundtrip")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "keylayout_roundtrip.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keylayout ok" in r.stdout
