"""CPU-side checks of the seeded locate's interface (include/cs_fmindex_approx_seeded.h): the
header declares exactly its three entry points and its one define, the library exports them, the
Python mirror carries their signatures and the methods, the facade declares
locate_mismatches_seeded, a null handle is refused with nothing written, and the C++ program
compiles and links.  No GPU, no compute call.  (That the earlier headers stay as they were is
held by the ABI tests that came with them.)"""
import ctypes as C
import os
import re
import subprocess

from conftest import PKG_DIR, ROOT, load_pkg

HEADER = ("include", "cs_fmindex_approx_seeded.h")
ENTRY_POINTS = ["cs_fm_locate_mismatch_seeded_device", "cs_fm_locate_mismatch_seeded_batch",
                "cs_fm_locate_mismatch_seeded"]
TWIN = "cs_fm_locate_mismatch_seeded_phases_device"  # include/cs_fmindex_diag.h


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_exactly_the_entry_points():
    src = _read(*HEADER)
    assert re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", src, re.M) == ENTRY_POINTS
    assert re.findall(r"^#define (CS_\w+) (\w+)$", src, re.M) == [("CS_SEED_MAX_K", "15u")]
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
    assert [len(pkg.SIGNATURES[s][1]) for s in ENTRY_POINTS] == [14, 12, 8]
    assert pkg.SEED_MAX_K == 15
    # the measurement twin: the device form's arguments and the phase times
    diag = _read("include", "cs_fmindex_diag.h")
    params = re.search(r"^cs_status %s\((.*?)\);" % TWIN, diag, re.M | re.S).group(1)
    assert TWIN in exported and len(params.split(",")) == len(pkg.SIGNATURES[TWIN][1]) == 15


def test_python_mirror():
    pkg = load_pkg()
    for name in ("locate_mismatches_seeded", "locate_mismatches_seeded_batch", "locate_mismatch_seeded_device"):
        assert callable(getattr(pkg.FMIndex, name)), name


def test_facade_header_declares_locate_mismatches_seeded():
    src = _read("include", "cs", "fm_index.hpp")
    assert re.search(r"std::vector<std::pair<uint64_t, uint8_t>> locate_mismatches_seeded\(std::string_view \w+,"
                     r"\s*unsigned k\) const;", src)


def test_null_handle_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    d = (C.c_uint8 * 4)(7, 7, 7, 7)
    oo = (C.c_uint64 * 2)(7, 7)
    pos = (C.c_uint64 * 4)(7, 7, 7, 7)
    tot, cand = C.c_uint64(7), C.c_uint64(7)
    assert L.cs_fm_locate_mismatch_seeded(None, b"ab", 2, 1, pos, d, 4, C.byref(tot)) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    offs = (C.c_uint64 * 2)(0, 2)
    buf = (C.c_uint8 * 2)(65, 66)
    assert L.cs_fm_locate_mismatch_seeded_batch(None, buf, offs, 1, 1, oo, pos, d, 4, C.byref(tot), C.byref(cand),
                                                None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert L.cs_fm_locate_mismatch_seeded_device(None, None, None, 0, 0, 1, None, None, None, 0, C.byref(tot),
                                                 C.byref(cand), 0, None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    ms = (C.c_float * 5)(7, 7, 7, 7, 7)
    assert L.cs_fm_locate_mismatch_seeded_phases_device(None, None, None, 0, 0, 1, None, None, None, 0,
                                                        C.byref(tot), C.byref(cand), 0, ms,
                                                        None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    assert list(d) == [7] * 4 and list(oo) == [7, 7] and list(pos) == [7] * 4  # nothing written
    assert tot.value == 7 and cand.value == 7 and list(ms) == [7.0] * 5


def test_cpp_program_compiles_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "seeded_tests.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-o",
                    str(tmp_path / "seeded_tests"), "-L" + PKG_DIR, "-lcs_fmindex",
                    "-Wl,-rpath," + PKG_DIR], check=True)
