"""cs::FMIndex::locate_mismatches through the drop-in header (include/cs/fm_index.hpp) linked to
libcs_fmindex.so: tests/cpp/mismatch_locate_tests.cpp compiled with g++ (CPU, here) and run on
the GPU box against values hard-coded from the oracle.  (Named to collect after the suites
that were here before it.)"""
import os
import subprocess

import pytest

from conftest import PKG_DIR, ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "mismatch_locate_tests.cpp")


def _compile(out):
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-o", out,
                    "-L" + PKG_DIR, "-lcs_fmindex", "-Wl,-rpath," + PKG_DIR], check=True)


def test_mismatch_locate_program_compiles_and_links(tmp_path):
    _compile(str(tmp_path / "mismatch_locate_tests"))


@pytest.mark.gpu
def test_mismatch_locate_program_runs(tmp_path):
    exe = str(tmp_path / "mismatch_locate_tests")
    _compile(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "PASSED" in r.stdout
