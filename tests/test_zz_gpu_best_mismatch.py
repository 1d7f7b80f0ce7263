"""Best stratum (include/cs_fmindex_approx_best.h): the smallest distance d <= k at which a
pattern occurs and the count there, against best_from_hist of a histogram the library never
computed — the enumeration on the small texts, the cyclic Hamming scan on the family texts and
the mixed batch (tests/helpers/best_ref.py; the batches' conditions are held without a GPU in
tests/test_best_mismatch_ref_cpu.py).  That best_count equals the library histogram's column is
an extra consistency check, never the expectation.

The rounds of launch_best_mm are what is new here: the pending lists between them (831, 660,
484 entries on the mixed batch: several blocks, no multiple of a wave), blocks past a list's end,
empty and full lists, and temporaries that are stream-ordered.  Named to collect after the
suites that were here before it.
"""
import numpy as np
import pytest
import torch

from conftest import load_pkg
from helpers.best_ref import (NONE, TEXTS, VARIANTS, best_family_case, best_from_hist, device_best,
                              device_best_async, mixed_case, read_best, same_best, small_case)
from helpers.mismatch_ref import KMAX, _dev, device_hist, scan_hamming

pytestmark = pytest.mark.gpu


def _build(text, vname):
    pkg = load_pkg()
    with pkg.build_options(VARIANTS[vname]):
        return pkg.FMIndex.build_from_text(text)


def _check_all_k(g, pats, table, what, host=True, hist_column=True):
    """The device call (and the host batch) at k = 0..3 against best_from_hist of `table`; the
    count also against the library histogram's own column."""
    lib3 = device_hist(g, pats, KMAX) if hist_column else None
    for k in range(KMAX + 1):
        want = best_from_hist(table, k)
        got = device_best(g, pats, k)
        same_best(got, want, what + (k, "device"))
        if host:
            hd, hc = g.best_mismatches_batch(pats, k)
            assert hd.dtype == np.uint8 and hc.dtype == np.uint64
            same_best((hd, hc), want, what + (k, "host"))
        if hist_column:
            hit = np.flatnonzero(got[0] != NONE)
            assert got[1][hit].tolist() == lib3[hit, got[0][hit]].tolist(), what + (k, "histogram column")


# ---- 1. small texts x the eight engine variants ------------------------------------------------
@pytest.mark.parametrize("vname", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_engines_small_texts(name, vname):
    text, pats, table = small_case(name)
    g = _build(text, vname)
    _check_all_k(g, pats, table, (name, vname))
    for k in range(KMAX + 1):  # the single-pattern call
        wd, wc = best_from_hist(table, k)
        for q in range(0, len(pats), 3):
            d, c = g.best_mismatch(pats[q], k)
            assert (NONE if d is None else d, c) == (int(wd[q]), int(wc[q])), (name, vname, k, q)


# ---- 2. family texts ---------------------------------------------------------------------------
DNA_VARIANTS = ("auto", "noprefix", "learned", "qwm", "wavelet", "wide_bucketed")
FAMILY_CASES = ([(n, v) for n in ("fam_dna", "fam_dna_N") for v in DNA_VARIANTS] +
                [(n, v) for n in ("fam_alpha12", "fam_bytes") for v in ("auto", "wavelet")])


@pytest.mark.parametrize("name,vname", FAMILY_CASES, ids=["%s-%s" % c for c in FAMILY_CASES])
def test_family_texts(name, vname):
    pkg = load_pkg()
    text, pats, table = best_family_case(name)
    g = _build(text, vname)
    _check_all_k(g, pats, table, (name, vname))
    sel = [q for q, p in enumerate(pats) if len(p) == 33]  # fixed_m with d_offs = NULL
    assert len(sel) >= 13
    sub = [pats[q] for q in sel]
    for k in range(KMAX + 1):
        same_best(device_best(g, sub, k, fixed_m=33), best_from_hist(table[sel], k), (name, vname, k, "fixed_m"))
    if vname == "auto":
        for f in (pkg.Q_NO_PREFIX, pkg.Q_NO_CONTEXTS, pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS):
            for k in range(KMAX + 1):
                same_best(device_best(g, pats, k, flags=f), best_from_hist(table, k), (name, k, "flags", f))


# ---- 3. the mixed batch ------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["auto", "qwm", "wavelet"])
def test_mixed_batch(vname):
    text, pats, table = mixed_case()
    g = _build(text, vname)
    _check_all_k(g, pats, table, ("mixed", vname), host=vname == "auto")
    rev = pats[::-1]  # per pattern, whatever its place in the batch and in the lists
    for k in range(KMAX + 1):
        wd, wc = best_from_hist(table, k)
        same_best(device_best(g, rev, k), (wd[::-1], wc[::-1]), ("mixed reversed", vname, k))


# ---- 4. list edges -----------------------------------------------------------------------------
def test_list_edges_prefixes():
    text, pats, table = mixed_case()
    g = _build(text, "auto")
    for npat in (1, 63, 64, 65, 257):
        for k in range(KMAX + 1):
            same_best(device_best(g, pats[:npat], k), best_from_hist(table[:npat], k), ("prefix", npat, k))


def test_list_edges_all_exact_and_none():
    text, _, _ = mixed_case()
    g = _build(text, "auto")
    n = len(text)
    rng = np.random.default_rng(31)
    # every pattern occurs exactly: the later rounds get empty lists and write nothing
    starts = rng.integers(0, n - 1 - 30, 700)
    exact = [text[int(i):int(i) + 30] for i in starts]
    want = scan_hamming(text, exact, 0)[0][:, 0]
    assert (want > 0).all() and want.max() > 1  # (windows of the planted copies occur more than once)
    for k in range(KMAX + 1):
        d, c = device_best(g, exact, k)  # (read_best: every entry written, canaries kept)
        assert (d == 0).all() and c.tolist() == want.tolist(), k
    # no pattern resolves within 3: every list stays full
    absent = [b"#####"] * 300
    assert b"#" not in text
    for k in range(KMAX + 1):
        d, c = device_best(g, absent, k)
        assert (d == NONE).all() and (c == 0).all(), k
    d, c = g.best_mismatches_batch(absent, KMAX)
    assert (d == NONE).all() and (c == 0).all()
    assert g.best_mismatch(b"#####", KMAX) == (None, 0)


def test_npat_zero_and_errors():
    pkg = load_pkg()
    text, pats, table = mixed_case()
    g = _build(text, "auto")
    st = torch.cuda.current_stream().cuda_stream
    d_d = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    d_c = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    g.best_mismatch_device(None, None, 0, 3, d_d.data_ptr(), d_c.data_ptr(), stream=st)
    g.best_mismatch_device(None, None, 0, 3, None, None, stream=st)  # nothing touched, nothing needed
    torch.cuda.synchronize()
    assert (d_d.cpu().numpy() == 0xEE).all() and (d_c.cpu().numpy() == -1).all()
    d, c = g.best_mismatches_batch([], 2)
    assert len(d) == 0 and len(c) == 0
    d_p = _dev(np.frombuffer(b"ACGTACGT", np.uint8), torch.uint8)
    for args in ((d_p.data_ptr(), None, 2, 1, None, d_c.data_ptr()),   # null outputs with npat > 0
                 (d_p.data_ptr(), None, 2, 1, d_d.data_ptr(), None),
                 (d_p.data_ptr(), None, 2, 4, d_d.data_ptr(), d_c.data_ptr())):  # k > CS_MM_MAX
        with pytest.raises(pkg.FMIndexError) as ei:
            g.best_mismatch_device(*args, fixed_m=4, stream=st)
        assert ei.value.status == pkg.CS_ERR_INVALID
    with pytest.raises(pkg.FMIndexError) as ei:
        g.best_mismatches_batch(pats[:3], 4)
    assert ei.value.status == pkg.CS_ERR_INVALID and "CS_MM_MAX" in str(ei.value)
    with pytest.raises(pkg.FMIndexError) as ei:
        g.best_mismatches_batch(buf=np.frombuffer(b"ACGT", np.uint8), offs=np.array([0, 3, 2], np.uint64), k=1)
    assert ei.value.status == pkg.CS_ERR_INVALID
    # a batch of empty patterns may pass d_pats = NULL: every entry is (0, n)
    d_o = _dev(np.array([7, 7, 7, 7], np.int64), torch.int64)
    g.best_mismatch_device(None, d_o.data_ptr(), 3, 2, d_d.data_ptr(), d_c.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert d_d.cpu().tolist() == [0, 0, 0, 0xEE] and d_c.cpu().tolist() == [len(text)] * 3 + [-1]


def test_two_calls_queued_on_one_stream():
    """Two calls back to back with no synchronisation between them: the second call's lists
    and lengths must not be the first call's while it still runs."""
    text, pats, table = mixed_case()
    g = _build(text, "auto")
    a = device_best_async(g, pats, KMAX)
    b = device_best_async(g, pats[::-1][:777], 2)
    same_best(read_best(a), best_from_hist(table, KMAX), ("queued", "first"))
    wd, wc = best_from_hist(table[::-1][:777], 2)
    same_best(read_best(b), (wd, wc), ("queued", "second"))
