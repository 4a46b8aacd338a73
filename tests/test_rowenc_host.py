"""nbg_rows_encode's host-side tables (nebula_amd/csrc/rowenc.h: the per-chunk OVER positions, the
string constants outside the dictionary) under AddressSanitizer and UBSan: a stand-alone program
(tests/host/rowenc_host.cpp) built for the CPU and run as its own process.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_tables_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "rowenc_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nebula_amd", "csrc"), os.path.join(ROOT, "tests", "host", "rowenc_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0, out.stdout.decode()
    assert b"rowenc host tables OK" in out.stdout
