"""CPU-side checks of the approximate-locate interface (include/cs_fmindex_approx_locate.h): the
header declares its three entry points, the library exports them, the Python mirror carries
their signatures and the methods, and the two headers the existing ABI tests pin keep
satisfying those tests.  No GPU, no compute call."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT, load_pkg

HEADER = os.path.join(ROOT, "include", "cs_fmindex_approx_locate.h")
ENTRY_POINTS = ["cs_fm_locate_mismatch_device", "cs_fm_locate_mismatch_batch", "cs_fm_locate_mismatch"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_entry_points():
    decls = re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", _read("include", "cs_fmindex_approx_locate.h"), re.M)
    assert decls == ENTRY_POINTS


def test_header_documents_the_order():
    src = _read("include", "cs_fmindex_approx_locate.h")
    assert "Order inside a pattern" in src and "row order" in src and "cs_fm_locate_device" in src


def test_library_exports_them():
    pkg = load_pkg()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (cs_[A-Za-z0-9_]+)$", out, flags=re.M))
    for s in ENTRY_POINTS:
        assert s in exported and s in pkg.SIGNATURES and hasattr(L, s), s
    # argument counts of the mirror against the header's parameter lists
    src = _read("include", "cs_fmindex_approx_locate.h")
    for s in ENTRY_POINTS:
        params = re.search(r"^cs_status %s\((.*?)\);" % s, src, re.M | re.S).group(1)
        assert len(params.split(",")) == len(pkg.SIGNATURES[s][1]), s


def test_python_methods():
    pkg = load_pkg()
    for name in ("locate_mismatches", "locate_mismatches_batch", "locate_mismatch_device"):
        assert callable(getattr(pkg.FMIndex, name)), name


def test_pinned_headers_keep_their_contracts():
    """cs_fmindex_approx.h still declares exactly the count's three entry points and
    cs_fmindex.h still does not mention mismatches (tests/test_mismatch_abi_cpu.py), with its
    30 entry points at most (tests/test_capi_cpu.py)."""
    approx = _read("include", "cs_fmindex_approx.h")
    assert re.findall(r"^cs_status (cs_[a-z0-9_]+)\(", approx, re.M) == [
        "cs_fm_count_mismatch_device", "cs_fm_count_mismatch_batch", "cs_fm_count_mismatch"]
    assert "locate_mismatch" not in approx
    dropin = _read("include", "cs_fmindex.h")
    assert "mismatch" not in dropin and "CS_MM_MAX" not in dropin
    decls = re.findall(r"^(?:cs_status|uint64_t|void|const char\*) (cs_[a-z0-9_]+)\(", dropin, re.M)
    assert len(decls) <= 30, decls


def test_facade_header_declares_locate_mismatches():
    src = _read("include", "cs", "fm_index.hpp")
    assert re.search(r"std::vector<std::pair<uint64_t, uint8_t>> locate_mismatches\(std::string_view \w+,\s*"
                     r"unsigned k\) const;", src)


def test_null_handle_is_invalid():
    pkg = load_pkg()
    L = pkg.lib()
    n = C.c_uint64(7)
    assert L.cs_fm_locate_mismatch(None, b"a", 1, 1, None, None, 0, C.byref(n)) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
    oo = (C.c_uint64 * 2)()
    offs = (C.c_uint64 * 2)(0, 1)
    buf = (C.c_uint8 * 1)(65)
    assert L.cs_fm_locate_mismatch_batch(None, buf, offs, 1, 1, oo, None, None, 0, C.byref(n),
                                         None) == pkg.CS_ERR_INVALID
    assert L.cs_fm_locate_mismatch_device(None, None, None, 0, 0, 1, None, None, None, 0, C.byref(n), 0,
                                          None) == pkg.CS_ERR_INVALID
    assert b"null index handle" in L.cs_fm_last_error()
