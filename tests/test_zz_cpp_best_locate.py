"""cs::FMIndex::locate_best_mismatch through the drop-in header (include/cs/fm_index.hpp) linked
to libcs_fmindex.so: tests/cpp/best_locate_tests.cpp compiled with g++ and run on the GPU against
values hard-coded from the oracle's enumeration.  (That it compiles and links without a GPU is in
tests/test_best_locate_abi_cpu.py.  Named to collect after the suites that were here before
it.)"""
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "best_locate_tests.cpp")


@pytest.mark.gpu
def test_best_locate_program_runs(tmp_path):
    exe = str(tmp_path / "best_locate_tests")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + PKG_DIR, "-lcs_fmindex", "-Wl,-rpath," + PKG_DIR], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "PASSED" in r.stdout
