"""The sort pass's register network (csrc/fs_pair_search.h: fs_pair_sort16, shared by the kernel and the host) on the CPU:
scripts/sanitize/pair_sort_check.cpp -- a stand-alone program, built here with AddressSanitizer and UBSan -- proves the
network on all 2^16 zero-one inputs and sorts random columns of every length from 0 to 96 the way fs_pair_sort_column does,
neighbours of the column untouched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_sort_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "pair_sort_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-D__host__=", "-D__device__=",
                           os.path.join(ROOT, "scripts", "sanitize", "pair_sort_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pair sort ok" in out.stdout, out.stdout + out.stderr
