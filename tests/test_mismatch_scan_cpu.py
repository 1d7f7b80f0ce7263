"""The cyclic Hamming scan (tests/helpers/mismatch_ref.py) against the oracle, without a GPU.

tests/test_zz_gpu_mismatch_families.py compares the mismatch kernels with the scan's histograms
and pairs on the family texts.  Everything that comparison rests on is checked here: on every
family text the scan equals the oracle's exact count and locate at d = 0 for every pattern
(long, wrapped through the terminator and longer than the text included), and equals the
enumeration reference of the first mismatch suites at k <= 2 for the patterns short enough to
enumerate.  The conditions on the generated inputs (the hits the GPU tests exist for) are
asserted from the scan alone, so a change of the generator cannot quietly empty them.
"""
import numpy as np
import pytest

import oracle as O
from helpers.mismatch_ref import (FAMILIES, KMAX, LENGTHS, PREFIX_KS, _cut, check_scannable, expected_hist,
                                  expected_pairs, family_case, mismatch_positions, scan_hamming, widest_leaf)

_REFS = {}


def _ref(name):
    if name not in _REFS:
        _REFS[name] = O.Index(family_case(name)[0])
    return _REFS[name]


def test_scan_small_known():
    hist, pairs = scan_hamming(b"banana$", [b"ana", b"", b"banana$ba", b"nab"], 3)
    # worked by hand: "ana" against ban, ana, nan, ana, na$, a$b, $ba; "nab" against the same
    assert hist.tolist() == [[2, 0, 2, 3], [7, 0, 0, 0], [1, 0, 0, 0], [0, 2, 2, 3]]
    assert pairs[0].tolist() == [[0, 3], [1, 0], [2, 3], [3, 0], [4, 3], [5, 2], [6, 2]]
    assert pairs[3].tolist() == [[0, 2], [1, 3], [2, 1], [3, 3], [4, 1], [5, 2], [6, 3]]
    assert pairs[1].tolist() == [] and pairs[2].tolist() == [[0, 0]]
    for text in (b"abababab", b"a" * 100, b"ba$na$", b"$banana"):  # not the rotations' order
        with pytest.raises(AssertionError):
            check_scannable(text)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_scan_d0_equals_exact_count_and_locate(name):
    text, pats, _, hist, pairs = family_case(name)
    ref = _ref(name)
    assert len(pats) < 100 and len(text) in (1741, 4121)
    assert hist[:, 0].tolist() == ref.count_batch(pats, nthreads=8).tolist()
    for q, p in enumerate(pats):
        exact = pairs[q][pairs[q][:, 1] == 0][:, 0].tolist()
        assert exact == sorted(ref.locate(p, limit=len(text) + 1)), q
        assert len(exact) == (hist[q, 0] if p else 0)
    assert sorted({len(p) for p in pats}) == sorted({0, 1, 3, 27, len(text) + 5} | set(LENGTHS))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_scan_equals_enumeration_short(name):
    """k <= 2, the patterns of at most 10 characters (over bytes, 16 substitutes a position:
    the 1- and 3-mers and one 9-mer with a planted substitution)."""
    text, pats, _, hist, pairs = family_case(name)
    sel = [q for q, p in enumerate(pats) if len(p) <= 10]
    if name == "fam_bytes":
        sel = [q for q in sel if len(pats[q]) <= 3] + [next(q for q in sel if len(pats[q]) == 9) + 1]
    assert len(sel) >= 4
    short = [pats[q] for q in sel]
    assert expected_hist(_ref(name), text, short, 2).tolist() == hist[sel, :3].tolist()
    want, _ = expected_pairs(_ref(name), text, short, 2)
    got = _cut([pairs[q] for q in sel], 2)
    for q, (a, b) in enumerate(zip(got, want)):
        assert a.tolist() == b.tolist(), sel[q]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_inputs_hold_the_hits_the_gpu_tests_need(name):
    text, pats, planted, hist, pairs = family_case(name)
    # every long length has hits at each of d = 0, 1, 2, 3
    for m in LENGTHS:
        if m >= 21:
            tot = hist[[q for q, p in enumerate(pats) if len(p) == m]].sum(axis=0)
            assert (tot > 0).all(), (m, tot.tolist())
    # a hit at d >= 1 whose mismatches all lie inside the prefix table's depth (frame K then
    # restarts from the table), for each depth the text is built with; one with a mismatch at
    # position 0 (consumed last); both on patterns long enough to be verified against the text
    for pk in PREFIX_KS[name]:
        assert any(len(p) >= pk + 10 and min(mismatch_positions(text, p, pos)) >= len(p) - pk + 1
                   for p, pr in zip(pats, pairs) for pos, d in pr.tolist() if d >= 1), pk
    assert any(len(p) >= 21 and 0 in mismatch_positions(text, p, pos)
               for p, pr in zip(pats, pairs) for pos, d in pr.tolist() if d >= 1)
    # a hit at d = 3 with a hundred characters still to consume after its last mismatch
    assert any(d == 3 and min(mismatch_positions(text, p, pos)) >= 100
               for p, pr in zip(pats, pairs) for pos, d in pr.tolist())
    # the planted pairs straddle the restart boundary: m - prefix_k + 1 is the first substituted
    # position whose leaf restarts from the table, m - prefix_k the last whose leaf does not;
    # and at every verifiable length the pair yields a hit whose lowest mismatch (the one the
    # leaf frame spends) is m - prefix_k, with the one above it inside the restart zone
    for pk in PREFIX_KS[name]:
        for m in LENGTHS:
            assert (m - pk, m - pk + 1) in [w for p, w in zip(pats, planted) if len(p) == m]
            assert (m - pk + 1,) in [w for p, w in zip(pats, planted) if len(p) == m]
            if m >= pk + 10:
                for where in ([m - pk, m - pk + 1], [m - pk + 1]):
                    assert any(len(p) == m and mismatch_positions(text, p, pos).tolist() == where
                               for p, pr in zip(pats, pairs) for pos, d in pr.tolist() if d >= 1), (pk, m, where)
    # the wrapped window whose terminator is overwritten: one hit, at d = 1, on the terminator
    n = len(text)
    q = next(q for q, p in enumerate(pats) if len(p) == 27) + 1
    assert len(pats[q]) == 27 and pairs[q].tolist() == [[n - 12, 1]]
    assert mismatch_positions(text, pats[q], n - 12).tolist() == [11]
    assert pairs[q - 1].tolist() == [[n - 12, 0]]
    # a leaf of more than kLocSmall = 32 rows (the wide path of the distance expansion)
    assert max(widest_leaf(text, p, pr) for p, pr in zip(pats, pairs) if 0 < len(p) <= 3) > 32
    # the absent byte really is absent, the patterns fall on every byte alignment
    assert sum(1 for p in pats if p and not set(p) <= set(text)) == 3
    starts = np.cumsum([0] + [len(p) for p in pats[:-1]])
    assert set((starts % 8).tolist()) == set(range(8))
    assert KMAX == 3
