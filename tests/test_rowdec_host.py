"""nbg_rows_decode's host side (nebula_amd/csrc/rowdec.h: the walk of the length prefixes, and the
cell reader the kernel shares) under AddressSanitizer and UBSan: a stand-alone program
(tests/host/rowdec_host.cpp) built for the CPU and run as its own process.  It decodes well-formed
rowsets against compiled-in values and every malformed case of nbg_rows_decode's statuses 5 and 6,
each input in a heap block of exactly its length.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_and_cells_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "rowdec_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nebula_amd", "csrc"), os.path.join(ROOT, "tests", "host", "rowdec_host.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0, out.stdout.decode()
    assert b"rowdec host walk and cells OK" in out.stdout
