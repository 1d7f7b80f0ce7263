"""Locate within k mismatches (include/cs_fmindex_approx_locate.h) against the oracle.

The pairs (pos, d) of a pattern are the union, over every string S at Hamming distance d <= k
from it over the symbols present in the text, of the oracle's exact locate of S (limit >= n)
labelled d: the expected table enumerates those neighbours (itertools), counts them all in one
oracle batch and locates the ones that occur.  The table of a bound k is the k = 3 table cut at
d <= k, so a text's table is computed once and shared.  Compared per pattern as sorted pairs;
the offsets must be the scan of the expected sizes, the sizes the row sums of the count's
histogram (m > 0), and the entries after the last one must come back untouched.

abab_noterm and all_same are not among the texts: the oracle's exact locate raises "LF walk
exceeded text length" on both (no unique terminator), so abab_noterm is the overrun case.
The file's 48 tests take 13 s on one MI355X, 0.3-0.6 s per case (the C++ program's wrapper 0.7 s
more).  The file is named to collect after every suite that was here before it.
"""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg
from helpers.mismatch_ref import (KMAX, _absent_byte, _check, _cut, _dev, _present, device_pairs, expected_pairs,
                                  host_pairs)

pytestmark = pytest.mark.gpu

VARIANTS = {
    "auto": {},
    "noprefix": {"CS_FM_PREFIX_K": "0"},
    "learned": {"CS_FM_ENGINE": "learned"},
    "qwm": {"CS_FM_ENGINE": "qwm"},
    "wavelet": {"CS_FM_ENGINE": "wavelet"},
    "wavelet_line64": {"CS_FM_ENGINE": "wavelet", "CS_FM_LINE_BYTES": "64", "CS_FM_DEVICE_TEXT": "0"},
    "wide_bucketed": {"CS_FM_WIDE": "1", "CS_FM_SA_BUILDER": "bucketed", "CS_FM_DEVICE_TEXT": "0"},
    "wide_wavelet": {"CS_FM_WIDE": "1", "CS_FM_ENGINE": "wavelet"},
}


def _dna_with_n(seed, length, count):
    t = O.gen_dna(seed, length).copy()
    rng = np.random.default_rng(seed)
    t[rng.choice(length, count, replace=False)] = ord("N")
    return t.tobytes()


def _alpha12(seed, length):
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"abcdefghijkl", np.uint8)[rng.integers(0, 12, length)])


TEXTS = {
    "banana": lambda: b"banana$",
    "straddle_649": lambda: O.gen_dna(649, 649).tobytes(),  # a range straddling a line edge
    "dna_5k": lambda: O.gen_dna(7, 5000).tobytes(),
    "rare_N_40": lambda: _dna_with_n(11, 5000, 40),  # the rare-row list
    "alpha_12": lambda: _alpha12(12, 2000),
}


def _patterns(name, text):
    """Substrings of length 1, 2, 3, 8 at random positions; the same with one and two
    characters replaced by other present symbols; a byte absent from the text at the first, a
    middle and the last position; the empty pattern; a pattern shorter than k."""
    rng = np.random.default_rng(len(text))
    syms = _present(text)
    pats = []
    for m in (1, 2, 3, 8):
        m = min(m, len(text))
        i = int(rng.integers(0, len(text) - m + 1))
        p = bytearray(text[i:i + m])
        pats.append(bytes(p))
        for nrep in (1, 2):
            r = bytearray(p)
            for j in rng.choice(m, min(nrep, m), replace=False):
                other = [s for s in syms if s != r[j]]
                if other:
                    r[j] = other[int(rng.integers(0, len(other)))]
            pats.append(bytes(r))
    i = int(rng.integers(0, max(len(text) - 5, 1)))
    base = (text[i:i + 5] + text[:5])[:5]
    for at in (0, 2, 4):
        r = bytearray(base)
        r[at] = _absent_byte(text)
        pats.append(bytes(r))
    pats.append(b"")
    pats.append(text[:1])  # m = 1 < k = 3
    if name == "banana":
        pats.append(b"banana$ba")  # longer than the text (m = 9 > n = 7; cyclic)
    return pats


_CASES = {}


def _case(name):
    """(text, patterns, expected k = 3 pairs, widest leaf, oracle), computed once per text."""
    if name not in _CASES:
        text = TEXTS[name]()
        ref = O.Index(text)
        pats = _patterns(name, text)
        want, widest = expected_pairs(ref, text, pats, KMAX)
        _CASES[name] = (text, pats, want, widest, ref)
    return _CASES[name]


# ---- 1. engines x small texts -------------------------------------------------
@pytest.fixture(params=sorted(VARIANTS))
def variant(request):
    m = load_pkg()
    with m.build_options(VARIANTS[request.param]):
        yield m


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_engines_small_texts(variant, name):
    text, pats, want3, widest, _ = _case(name)
    g = variant.FMIndex.build_from_text(text)
    if name == "dna_5k":  # its m = 1 and m = 2 patterns: leaves of more than kLocSmall = 32 rows
        assert widest > 32
    for k in range(KMAX + 1):
        want = _cut(want3, k)
        oo, got = device_pairs(g, pats, k)
        _check(oo, got, want, (name, k, "device"))
        oo, got = host_pairs(g, pats, k)
        _check(oo, got, want, (name, k, "host"))
        hist = g.count_mismatches_batch(pats, k)
        for q, p in enumerate(pats):
            if p:
                assert int(hist[q].sum()) == len(want[q]), (name, k, q)
            else:
                assert len(want[q]) == 0 and hist[q, 0] == len(text)
        if text.endswith(b"$"):  # a unique terminator: a position occurs at most once per pattern
            for w in want:      # (without one the reference's own walk can report a position twice)
                assert len(np.unique(w[:, 0])) == len(w)


# ---- 2. position phases -------------------------------------------------------
@pytest.mark.parametrize("name", ["dna_5k", "rare_N_40"])
def test_position_phases(name):
    pkg = load_pkg()
    text, pats, want3, _, _ = _case(name)
    want = _cut(want3, 2)
    builds = {"full_sa": {}, "walk_lines": {"CS_FM_FULL_SA": "0"},
              "engine_lf": {"CS_FM_FULL_SA": "0", "CS_FM_WALK": "0"}}
    for label, opts in builds.items():
        with pkg.build_options(opts):
            g = pkg.FMIndex.build_from_text(text)
        oo, got = device_pairs(g, pats, 2)
        _check(oo, got, want, (name, label))
        if label == "full_sa":
            for f in (pkg.Q_NO_FULL_SA | pkg.Q_NO_WALK_LINES, pkg.Q_NO_FULL_SA,
                      pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS):
                oo, got = device_pairs(g, pats, 2, flags=f)
                _check(oo, got, want, (name, label, f))


# ---- 3. k = 0 is the exact locate ----------------------------------------------
def test_k0_equals_exact_locate():
    pkg = load_pkg()
    text, pats, _, _, _ = _case("dna_5k")
    g = pkg.FMIndex.build_from_text(text)
    n = len(text)
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    tot, ok = g.locate_device(d_p.data_ptr(), d_o.data_ptr(), npat, n, d_oo.data_ptr(), None, 0)
    d_pos = torch.zeros(max(tot, 1), dtype=torch.int64, device="cuda")
    tot, ok = g.locate_device(d_p.data_ptr(), d_o.data_ptr(), npat, n, d_oo.data_ptr(), d_pos.data_ptr(), tot)
    assert ok and tot > 32
    oo, pos, dist = device_pairs(g, pats, 0, raw=True)
    assert oo.tolist() == d_oo.cpu().tolist()
    assert pos.tolist() == d_pos[:tot].cpu().tolist()  # element for element, unsorted
    assert not dist.any()


# ---- 4. the workload's shape ----------------------------------------------------
def test_workload_shape():
    pkg = load_pkg()
    text = O.gen_dna(3, 100_000).tobytes()
    ref = O.Index(text)
    P = O.gen_patterns_text(np.frombuffer(text, np.uint8), 20, 300, seed=9).copy()
    rng = np.random.default_rng(9)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for q in range(len(P)):
        for j in rng.choice(20, q % 3, replace=False):
            P[q, j] = rng.choice(acgt[acgt != P[q, j]])
    pats = [bytes(p) for p in P]
    want, _ = expected_pairs(ref, text, pats, 2)
    g = pkg.FMIndex.build_from_text(text)
    oo, got = device_pairs(g, pats, 2, fixed_m=20)
    _check(oo, got, want, "workload")
    assert min(len(w) for w in want) > 0
    hist = g.count_mismatches_batch(pats, 2)
    assert hist.sum(axis=1).tolist() == [len(w) for w in want]


# ---- 5. grid edges ----------------------------------------------------------------
def test_grid_edges():
    pkg = load_pkg()
    text, _, _, _, ref = _case("dna_5k")
    base = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(text, np.uint8), 6, 64, seed=2)]
    base[5] = b"AC##AC"   # two absent bytes, k = 1: no hit, equal consecutive offsets
    base[6] = b"#CGTA#"
    base[40] = b"##ACGT"
    want = expected_pairs(ref, text, base, 1)[0]
    assert not len(want[5]) and not len(want[6]) and not len(want[40]) and len(want[7])
    g = pkg.FMIndex.build_from_text(text)
    for npat in (1, 255, 257, 3000):
        pats = [base[q % 64] for q in range(npat)]
        oo, got = device_pairs(g, pats, 1)
        _check(oo, got, [want[q % 64] for q in range(npat)], npat)


# ---- 6. capacity and errors ---------------------------------------------------------
def test_capacity_and_errors():
    pkg = load_pkg()
    text, pats, want3, _, _ = _case("dna_5k")
    want = _cut(want3, 2)
    g = pkg.FMIndex.build_from_text(text)
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    total = sum(len(w) for w in want)
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    d_dist = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    # one short: the total, the offsets, nothing else
    tot = pkg.C.c_uint64()
    s = pkg.lib().cs_fm_locate_mismatch_device(g._h, d_p.data_ptr(), d_o.data_ptr(), 0, npat, 2, d_oo.data_ptr(),
                                               d_pos.data_ptr(), d_dist.data_ptr(), total - 1, pkg.C.byref(tot),
                                               0, st)
    torch.cuda.synchronize()
    assert s == pkg.CS_ERR_CAPACITY and tot.value == total
    assert d_oo.cpu().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert (d_pos == -1).all().item() and (d_dist == 0xFF).all().item()
    # the sizing call
    tot2, written = g.locate_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), npat, 2, d_oo.data_ptr(), None, None,
                                             0, stream=st)
    assert tot2 == total and not written
    # the host batch with a capacity one short: CS_ERR_CAPACITY, the total and the offsets
    out_offs = np.zeros(npat + 1, np.uint64)
    hp, hd = np.full(total, 7, np.uint64), np.full(total, 9, np.uint8)
    s = pkg.lib().cs_fm_locate_mismatch_batch(g._h, pkg._u8(buf), pkg._u64(offs), npat, 2, pkg._u64(out_offs),
                                              pkg._u64(hp), pkg._u8(hd), total - 1, pkg.C.byref(tot), None)
    assert s == pkg.CS_ERR_CAPACITY and tot.value == total and out_offs[-1] == total
    assert (hp == 7).all() and (hd == 9).all()
    # k = 4 from all three forms
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatches_batch(pats, 4)
    assert ei.value.status == pkg.CS_ERR_INVALID and "CS_MM_MAX" in str(ei.value) and "3" in str(ei.value)
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), npat, 4, d_oo.data_ptr(), None, None, 0, stream=st)
    assert ei.value.status == pkg.CS_ERR_INVALID and "CS_MM_MAX" in str(ei.value)
    n1 = pkg.C.c_uint64()
    assert pkg.lib().cs_fm_locate_mismatch(g._h, b"ACG", 3, 4, None, None, 0, pkg.C.byref(n1)) == pkg.CS_ERR_INVALID
    assert b"CS_MM_MAX" in pkg.lib().cs_fm_last_error()
    # decreasing host offsets
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatches_batch(buf=np.frombuffer(b"ACGT", np.uint8), offs=np.array([0, 3, 2], np.uint64), k=1)
    assert ei.value.status == pkg.CS_ERR_INVALID
    # a batch of empty patterns may pass d_pats = NULL: no positions
    d_e = _dev(np.array([7, 7, 7, 7], np.int64), torch.int64)
    d_oo3 = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    tot3, written = g.locate_mismatch_device(0, d_e.data_ptr(), 3, 2, d_oo3.data_ptr(), None, None, 0, stream=st)
    assert tot3 == 0 and written and d_oo3.cpu().tolist() == [0, 0, 0, 0]
    assert g.count_batch(pats).tolist() == [int((w[:, 1] == 0).sum()) if p else len(text)
                                            for p, w in zip(pats, want)]


# ---- 7. single pattern ----------------------------------------------------------------
def test_single_pattern():
    pkg = load_pkg()
    text = b"banana$"
    want = expected_pairs(O.Index(text), text, [b"ana"], 3)[0][0]
    g = pkg.FMIndex.build_from_text(text)
    pos, dist = g.locate_mismatches(b"ana", 3)
    assert pos.dtype == np.uint64 and dist.dtype == np.uint8
    assert sorted(zip(pos.tolist(), dist.tolist())) == [tuple(r) for r in want.tolist()]
    assert sorted(g.locate_mismatches(b"ana", 0)[0].tolist()) == [1, 3]
    assert len(g.locate_mismatches(b"", 2)[0]) == 0


# ---- 8. LF overrun ----------------------------------------------------------------------
def test_overrun_is_reported_and_the_handle_stays_usable():
    """A text without a unique terminator: the oracle's exact locate raises, and so does the
    position phase here — the error return of a bounded walk (every walk stops after n
    steps).  The handle answers an exact count afterwards."""
    pkg = load_pkg()
    text = b"abababab"
    ref = O.Index(text)
    with pytest.raises(RuntimeError, match="LF walk exceeded text length"):
        ref.locate(b"ab", limit=100)
    g = pkg.FMIndex.build_from_text(text)
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns([b"ab", b"ba"])
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_pos = torch.zeros(64, dtype=torch.int64, device="cuda")
    d_dist = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), 2, 1, d_oo.data_ptr(), d_pos.data_ptr(),
                                 d_dist.data_ptr(), 64, flags=pkg.Q_NO_FULL_SA | pkg.Q_NO_WALK_LINES, stream=st)
    assert ei.value.status == pkg.CS_ERR_LF_OVERRUN
    assert str(ei.value) == "locate: LF walk exceeded text length"
    pats = [b"ab", b"ba", b"aa", b"abab"]
    assert g.count_batch(pats).tolist() == [ref.count(p) for p in pats]
