"""Count and locate within k mismatches on long patterns, against the cyclic Hamming scan.

The first two mismatch suites stop at 8 characters (one 20-mer test apart) because their
reference enumerates every neighbour.  Here the reference is the scan of
tests/helpers/mismatch_ref.py (checked against the oracle without a GPU in
tests/test_mismatch_scan_cpu.py), so the patterns are windows of 9 to 290 characters, windows
through the terminator and a pattern longer than the text, on texts whose planted copies keep
the search alive at d = 1, 2, 3 with a hundred characters still to go.  That is where the
mismatch search differs from the exact one: frame K of mm_frame finishing a neighbour either by
count_rest from a range reached mid-pattern (left contexts, verification against the text) or
by count_pattern<SubPat<K>> from the prefix table, for K = 1, 2, 3, on every engine and on the
index layouts production-size indexes get (context records, escaped and wide table entries,
no contexts, no full suffix array); and mm_rest / launch_locate_walk on long leaves.

A count and a locate test per text x variant, 0.1 to 2.5 s each on occurrence lines and the
quaternary matrix, 2 to 4 s on the binary matrix (DESIGN §10.2 has the figures and what sets
them: the pattern longer than the text, whose frame 0 alone has n + 5 nodes, in every call);
the expected tables are computed once per text (family_case) and shared.  Named to collect
after the suites that were here before it.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the device calls of the helpers run on its stream)

from conftest import load_pkg
from helpers.mismatch_ref import (KMAX, PREFIX_KS, _check, _cut, device_hist, device_pairs, family_case,
                                  host_pairs)

pytestmark = pytest.mark.gpu

# the 8 variants of the first mismatch suites (one per instantiation of with_engine) ...
VARIANTS = {
    "auto": {},
    "noprefix": {"CS_FM_PREFIX_K": "0"},
    "learned": {"CS_FM_ENGINE": "learned"},
    "qwm": {"CS_FM_ENGINE": "qwm"},
    "wavelet": {"CS_FM_ENGINE": "wavelet"},
    "wavelet_line64": {"CS_FM_ENGINE": "wavelet", "CS_FM_LINE_BYTES": "64", "CS_FM_DEVICE_TEXT": "0"},
    "wide_bucketed": {"CS_FM_WIDE": "1", "CS_FM_SA_BUILDER": "bucketed", "CS_FM_DEVICE_TEXT": "0"},
    "wide_wavelet": {"CS_FM_WIDE": "1", "CS_FM_ENGINE": "wavelet"},
    # ... and the index layouts of ENGINE_VARIANTS (tests/test_gpu_parity.py) they leave out
    "auto_nolctx": {"CS_FM_LCTX": "0"},
    "auto_rec": {"CS_FM_CTX_RECORDS": "1"},
    "auto_rec16": {"CS_FM_CTX_RECORDS": "16", "CS_FM_COUNT_U": "1", "CS_FM_LOCATE_U": "1"},
    "auto_nosa": {"CS_FM_FULL_SA": "0"},
    "wide_rec16_esc": {"CS_FM_WIDE": "1", "CS_FM_CTX_RECORDS": "16", "CS_FM_PTAB_WMAX": "3"},
    "wide_ptab_esc": {"CS_FM_WIDE": "1", "CS_FM_PTAB_WMAX": "3"},
    "learned_sb4": {"CS_FM_ENGINE": "learned", "CS_FM_LEARNED_SHIFT": "2"},
    # the table's depth forced to 8, so that the restart zone (fewer than prefix_k characters
    # consumed) is wide at n = 4,121
    "auto_prefix8": {"CS_FM_PREFIX_K": "8"},
}
# (A table of depth 8 has sigma^8 entries: only the DNA texts, 5^8 and 6^8 entries, are built
# with it; 13^8 entries would be 6.5 GB.)
# The two larger alphabets run no occurrence lines whatever the variant asks for (info().engine:
# auto, qwm, learned, learned_sb4 and wide_bucketed all build the quaternary matrix there), and
# a search costs them one E::step per listed symbol at every node, so they keep the variants
# whose engine or layout differs on them: fam_alpha12 the default with and without the table,
# without contexts, with narrow and wide 16-B records, and the binary matrix; fam_bytes the
# default (17 symbols coded densely: three quaternary levels) and the binary matrix (eight).  Line64, Line32W and the
# rest run on the two DNA texts.
ALPHA12_VARIANTS = ("auto", "noprefix", "wavelet", "auto_nolctx", "auto_rec16", "wide_rec16_esc")
BYTES_VARIANTS = ("auto", "wavelet")
TEXTS = ("fam_dna", "fam_dna_N", "fam_alpha12", "fam_bytes")
FLAG_VARIANTS = ("auto", "auto_rec16", "qwm")


def _variants_of(name):
    if name == "fam_bytes":
        return BYTES_VARIANTS
    if name == "fam_alpha12":
        return ALPHA12_VARIANTS
    if name == "fam_dna_N":  # N is an ordinary sixth symbol to the binary matrix: one variant of it
        return [v for v in VARIANTS if v not in ("wavelet_line64", "wide_wavelet")]
    return list(VARIANTS)


CASES = [(name, v) for name in TEXTS for v in _variants_of(name)]


def _build(name, vname):
    pkg = load_pkg()
    with pkg.build_options(VARIANTS[vname]):
        return pkg.FMIndex.build_from_text(family_case(name)[0])


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def built(request):
    """(text name, variant name, index): one build for the count and the locate test."""
    name, vname = request.param
    g = _build(name, vname)
    pk = g.info().prefix_k
    # the patterns carry their planted pair around m - prefix_k for exactly these depths
    assert pk in (0,) + PREFIX_KS[name], pk
    if vname == "auto_prefix8":
        assert pk == 8
    if vname == "noprefix":
        assert pk == 0
    if vname == "auto" and PREFIX_KS[name]:
        assert pk == PREFIX_KS[name][0]
    yield name, vname, g


def _same_hist(got, want, pats, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, [(int(q), len(pats[q]), got[q].tolist(), want[q].tolist()) for q in bad[:8]])


def _of_length(pats, m):
    sel = [q for q, p in enumerate(pats) if len(p) == m]
    assert len(sel) >= 7
    return sel


# ---- 1. count: texts x variants x k --------------------------------------------------------
def test_count(built):
    name, vname, g = built
    text, pats, _, hist, _ = family_case(name)
    exact = g.count_batch(pats)
    assert exact.tolist() == hist[:, 0].tolist()
    for k in range(KMAX + 1):
        got_d = device_hist(g, pats, k)
        _same_hist(got_d, hist[:, :k + 1], pats, (name, vname, k, "device"))
        _same_hist(g.count_mismatches_batch(pats, k), hist[:, :k + 1], pats, (name, vname, k, "host"))
        assert got_d[:, 0].tolist() == exact.tolist()
    for m in (33, 130):  # fixed_m with d_offs = NULL
        sel = _of_length(pats, m)
        sub = [pats[q] for q in sel]
        _same_hist(device_hist(g, sub, KMAX, fixed_m=m), hist[sel], sub, (name, vname, "fixed_m", m))


# ---- 2. count under the query flags ----------------------------------------------------------
@pytest.mark.parametrize("name,vname", [(n, v) for n in TEXTS for v in FLAG_VARIANTS if v in _variants_of(n)])
def test_count_flags(name, vname):
    pkg = load_pkg()
    text, pats, _, hist, _ = family_case(name)
    g = _build(name, vname)
    exact = g.count_batch(pats).tolist()
    for f in (pkg.Q_NO_PREFIX, pkg.Q_NO_CONTEXTS, pkg.Q_NO_VERIFY, pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS):
        for k in range(KMAX + 1):
            got = device_hist(g, pats, k, flags=f)
            _same_hist(got, hist[:, :k + 1], pats, (name, vname, k, "flags", f))
            assert got[:, 0].tolist() == exact


# ---- 3. locate: texts x variants x k -------------------------------------------------------
def test_locate(built):
    name, vname, g = built
    text, pats, _, hist, pairs = family_case(name)
    rows3 = g.count_mismatches_batch(pats, KMAX)  # (test_count: bound k is its first k + 1 columns)
    for k in range(KMAX + 1):
        want = _cut(pairs, k)
        oo, got = device_pairs(g, pats, k)
        _check(oo, got, want, (name, vname, k, "device"))
        oo, got = host_pairs(g, pats, k)
        _check(oo, got, want, (name, vname, k, "host"))
        for q, p in enumerate(pats):
            if p:
                assert int(rows3[q, :k + 1].sum()) == len(want[q]), (name, vname, k, q)
            else:
                assert len(want[q]) == 0 and rows3[q, 0] == len(text)
    for m in (33, 130):  # fixed_m with d_offs = NULL
        sel = _of_length(pats, m)
        oo, got = device_pairs(g, [pats[q] for q in sel], KMAX, fixed_m=m)
        _check(oo, got, [pairs[q] for q in sel], (name, vname, "fixed_m", m))


# ---- 4. position phases ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fam_dna", "fam_dna_N"])
def test_position_phases(name):
    pkg = load_pkg()
    text, pats, _, _, pairs = family_case(name)
    builds = {"full_sa": {}, "walk_lines": {"CS_FM_FULL_SA": "0"},
              "engine_lf": {"CS_FM_FULL_SA": "0", "CS_FM_WALK": "0"}}
    for label, opts in builds.items():
        with pkg.build_options(opts):
            g = pkg.FMIndex.build_from_text(text)
        oo, got = device_pairs(g, pats, KMAX)
        _check(oo, got, pairs, (name, label))
        if label == "full_sa":
            for f in (pkg.Q_NO_FULL_SA, pkg.Q_NO_FULL_SA | pkg.Q_NO_WALK_LINES):
                oo, got = device_pairs(g, pats, KMAX, flags=f)
                _check(oo, got, pairs, (name, label, f))
