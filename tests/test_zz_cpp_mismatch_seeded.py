"""cs::FMIndex::locate_mismatches_seeded through the drop-in header (include/cs/fm_index.hpp) and
the seeded locate's C ABI, linked to libcs_fmindex.so: tests/cpp/seeded_tests.cpp compiled with
g++ (CPU; tests/test_seeded_abi_cpu.py holds that it compiles and links) and run on the GPU
against distances the program computes itself by a plain loop.  (Named to collect after the
suites that were here before it.)"""
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "seeded_tests.cpp")


@pytest.mark.gpu
def test_seeded_program_runs(tmp_path):
    exe = str(tmp_path / "seeded_tests")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L" + PKG_DIR, "-lcs_fmindex", "-Wl,-rpath," + PKG_DIR], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "PASSED" in r.stdout
