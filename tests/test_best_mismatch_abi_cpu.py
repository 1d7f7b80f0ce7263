"""CPU-side checks of the best-stratum interface (include/cs_fmindex_approx_best.h): the header
declares its three entry points and CS_MM_NONE, the library exports them, the Python mirror
carries their signatures, the define and the methods, the facade declares best_mismatch, a null
handle is refused, and the C++ program compiles and links.  No GPU, no compute call.  (That
cs_fmindex.h and cs_fmindex_approx.h stay as they were is held by tests/test_mismatch_abi_cpu.py
and tests/test_mismatch_locate_abi_cpu.py.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import PKG_DIR, ROOT, load_pkg

ENTRY_POINTS = ["cs_fm_best_mismatch_device", "cs_fm_best_mismatch_batch", "cs_fm_best_mismatch"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_define():
    src = _read("include", "cs_fmindex_approx_best.h")
    assert re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", src, re.M) == ENTRY_POINTS
    assert re.findall(r"^#define (CS_\w+) (\w+)$", src, re.M) == [("CS_MM_NONE", "0xFFu")]


def test_library_exports_them():
    pkg = load_pkg()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (cs_[A-Za-z0-9_]+)$", out, flags=re.M))
    src = _read("include", "cs_fmindex_approx_best.h")
    for s in ENTRY_POINTS:
        assert s in exported and s in pkg.SIGNATURES and hasattr(L, s), s
        # argument count of the mirror against the header's parameter list
        params = re.search(r"^cs_status %s\((.*?)\);" % s, src, re.M | re.S).group(1)
        assert len(params.split(",")) == len(pkg.SIGNATURES[s][1]), s


def test_python_mirror():
    pkg = load_pkg()
    assert pkg.CS_MM_NONE == 0xFF
    for name in ("best_mismatch", "best_mismatches_batch", "best_mismatch_device"):
        assert callable(getattr(pkg.FMIndex, name)), name


def test_facade_header_declares_best_mismatch():
    src = _read("include", "cs", "fm_index.hpp")
    assert re.search(r"std::pair<int, uint64_t> best_mismatch\(std::string_view \w+,\s*unsigned k\) const;", src)


def test_null_handle_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    d = (C.c_uint8 * 1)(7)
    c = (C.c_uint64 * 1)(7)
    assert L.cs_fm_best_mismatch(None, b"a", 1, 1, d, c) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    offs = (C.c_uint64 * 2)(0, 1)
    buf = (C.c_uint8 * 1)(65)
    assert L.cs_fm_best_mismatch_batch(None, buf, offs, 1, 1, d, c, None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert L.cs_fm_best_mismatch_device(None, None, None, 0, 0, 1, None, None, 0, None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert d[0] == 7 and c[0] == 7  # nothing written


def test_cpp_program_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "best_mismatch_tests.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-o",
                    str(tmp_path / "best_mismatch_tests"), "-L" + PKG_DIR, "-lcs_fmindex",
                    "-Wl,-rpath," + PKG_DIR], check=True)
