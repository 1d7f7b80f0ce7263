"""CPU-side checks of the approximate-count interface (include/cs_fmindex_approx.h): the header
declares its three entry points, the library exports them, the Python mirror carries the bound
and the methods, and the drop-in header stays as it was.  No GPU, no compute call."""
import os
import re
import subprocess

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "cs_fmindex_approx.h")
ENTRY_POINTS = ["cs_fm_count_mismatch_device", "cs_fm_count_mismatch_batch", "cs_fm_count_mismatch"]


def _header():
    return open(HEADER).read()


def test_header_declares_the_entry_points():
    decls = re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", _header(), re.M)
    assert decls == ENTRY_POINTS


def test_library_exports_them():
    pkg = load_pkg()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (cs_[A-Za-z0-9_]+)$", out, flags=re.M))
    for s in ENTRY_POINTS:
        assert s in exported and s in pkg.SIGNATURES and hasattr(L, s), s


def test_bound_mirrors_header():
    pkg = load_pkg()
    (v,) = re.findall(r"^#define CS_MM_MAX (\d+)u$", _header(), re.M)
    assert pkg.CS_MM_MAX == int(v) == 3


def test_python_methods():
    pkg = load_pkg()
    for name in ("count_mismatches", "count_mismatches_batch", "count_mismatch_device"):
        assert callable(getattr(pkg.FMIndex, name)), name


def test_dropin_header_does_not_mention_them():
    src = open(os.path.join(ROOT, "include", "cs_fmindex.h")).read()
    assert "mismatch" not in src and "CS_MM_MAX" not in src


def test_null_handle_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    assert L.cs_fm_count_mismatch(None, b"a", 1, 1, None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
