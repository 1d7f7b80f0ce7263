"""CPU-side checks of the best-stratum locate interface
(include/cs_fmindex_approx_best_locate.h): the header declares exactly its three entry points,
the library exports them, the Python mirror carries their signatures and the methods, the facade
declares locate_best_mismatch, a null handle is refused with nothing written, and the C++ program
compiles and links.  No GPU, no compute call.  (That the earlier headers stay as they were is
held by the ABI tests that came with them.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import PKG_DIR, ROOT, load_pkg

HEADER = ("include", "cs_fmindex_approx_best_locate.h")
ENTRY_POINTS = ["cs_fm_locate_best_mismatch_device", "cs_fm_locate_best_mismatch_batch",
                "cs_fm_locate_best_mismatch"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_exactly_the_entry_points():
    src = _read(*HEADER)
    assert re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", src, re.M) == ENTRY_POINTS
    assert not re.findall(r"^#define (CS_\w+) ", src, re.M)  # CS_MM_NONE stays where it is
    nocomment = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(cs_[A-Za-z0-9_]+)\s*\(", nocomment))) == sorted(ENTRY_POINTS)


def test_library_exports_them():
    pkg = load_pkg()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (cs_[A-Za-z0-9_]+)$", out, flags=re.M))
    src = _read(*HEADER)
    for s in ENTRY_POINTS:
        assert s in exported and s in pkg.SIGNATURES and hasattr(L, s), s
        # argument count of the mirror against the header's parameter list
        params = re.search(r"^cs_status %s\((.*?)\);" % s, src, re.M | re.S).group(1)
        assert len(params.split(",")) == len(pkg.SIGNATURES[s][1]), s
    assert [len(pkg.SIGNATURES[s][1]) for s in ENTRY_POINTS] == [13, 11, 8]


def test_python_mirror():
    pkg = load_pkg()
    for name in ("locate_best_mismatches", "locate_best_mismatches_batch", "locate_best_mismatch_device"):
        assert callable(getattr(pkg.FMIndex, name)), name


def test_facade_header_declares_locate_best_mismatch():
    src = _read("include", "cs", "fm_index.hpp")
    assert re.search(r"std::pair<int, std::vector<uint64_t>> locate_best_mismatch\(std::string_view \w+,"
                     r"\s*unsigned k\) const;", src)


def test_null_handle_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    d = (C.c_uint8 * 1)(7)
    oo = (C.c_uint64 * 2)(7, 7)
    pos = (C.c_uint64 * 4)(7, 7, 7, 7)
    tot = C.c_uint64(7)
    assert L.cs_fm_locate_best_mismatch(None, b"a", 1, 1, d, pos, 4, C.byref(tot)) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    offs = (C.c_uint64 * 2)(0, 1)
    buf = (C.c_uint8 * 1)(65)
    assert L.cs_fm_locate_best_mismatch_batch(None, buf, offs, 1, 1, d, oo, pos, 4, C.byref(tot),
                                              None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert L.cs_fm_locate_best_mismatch_device(None, None, None, 0, 0, 1, None, None, None, 0, C.byref(tot), 0,
                                               None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert d[0] == 7 and list(oo) == [7, 7] and list(pos) == [7] * 4 and tot.value == 7  # nothing written


def test_cpp_program_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "best_locate_tests.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-o",
                    str(tmp_path / "best_locate_tests"), "-L" + PKG_DIR, "-lcs_fmindex",
                    "-Wl,-rpath," + PKG_DIR], check=True)
