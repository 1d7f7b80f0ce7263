"""The seeded locate's restatement (tests/helpers/seeded_ref.py) against the cyclic Hamming scan,
without a GPU: on the four family texts with their committed patterns (those with m = 0 or
m > k) and k in {0, 1, 3, 4, 8}, pigeonhole seeds plus the ownership rule give exactly the scan's
pairs, each once, and no accepted start lacks a clean piece.  And the inputs hold what the GPU
tests exist for: hits at every distance up to 8 on long patterns, candidates the ownership rule
rejects, windows through the end of the text and a pattern longer than the text.
"""
import numpy as np
import pytest

from helpers.mismatch_ref import FAMILIES
from helpers.seeded_ref import (SEED_KMAX, SEED_KS, kept, piece_starts, restated_case, restated_pairs, scan_pairs,
                                seeded_case)

TEXTS = tuple(FAMILIES)


def test_piece_split():
    for m in (1, 2, 9, 10, 21, 33, 64, 97, 130, 290, 4126):
        for k in range(0, 16):
            a = piece_starts(m, k)
            assert a[0] == 0 and a[-1] == m and len(a) == k + 2
            assert all(x <= y for x, y in zip(a, a[1:]))
            if m > k:  # no piece is empty, and the lengths differ by at most one
                lens = [y - x for x, y in zip(a, a[1:])]
                assert min(lens) >= 1 and max(lens) - min(lens) <= 1
    assert piece_starts(10, 2) == [0, 3, 6, 10] and piece_starts(9, 8) == list(range(10))


@pytest.mark.parametrize("name", TEXTS)
@pytest.mark.parametrize("k", SEED_KS)
def test_restatement_equals_scan(name, k):
    text, pats, dist = seeded_case(name)
    sel = kept(pats, k)
    assert len(sel) >= len(pats) - 2 and any(not pats[q] for q in sel)
    rs, C = restated_case(name, k)
    want = scan_pairs(dist, sel, k)
    n_pairs = 0
    for q, r, w in zip(sel, rs, want):
        if r is None:
            assert len(w) == 0
            continue
        got = restated_pairs(r)
        assert len(np.unique(got[:, 0])) == len(got), (name, k, q)  # each start once
        assert got[np.argsort(got[:, 0], kind="stable")].tolist() == w.tolist(), (name, k, q)
        # pigeonhole: every start within k has a clean piece, so some candidate proposed it
        assert set(w[:, 0].tolist()) <= set(r["s"].tolist()), (name, k, q)
        n_pairs += len(got)
    assert C >= n_pairs > 0


@pytest.mark.parametrize("name,top", [("fam_dna", 7), ("fam_dna_N", 8)])
def test_long_patterns_hit_every_distance(name, top):
    """The patterns of m >= 21 have hits at every distance from 0 to `top`."""
    text, pats, dist = seeded_case(name)
    tot = np.zeros(SEED_KMAX + 1, np.int64)
    for p, d in zip(pats, dist):
        if len(p) >= 21:
            tot += np.bincount(d[d <= SEED_KMAX], minlength=SEED_KMAX + 1)
    assert (tot[:top + 1] > 0).all(), tot.tolist()
    if name == "fam_dna_N":
        d8 = sum(int((d == 8).sum()) for p, d in zip(pats, dist) if len(p) == 290)
        assert d8 > 0


@pytest.mark.parametrize("name", TEXTS)
def test_inputs_exercise_ownership_and_wrapping(name):
    text, pats, dist = seeded_case(name)
    n = len(text)
    assert any(len(p) == n + 5 for p in pats)
    for k in (3, 8):
        rs, C = restated_case(name, k)
        sel = kept(pats, k)
        # a candidate within k that an earlier clean piece owns: an alignment with two clean pieces
        owned = sum(int((r["clean_before"] & (r["d"] <= k)).sum()) for r in rs if r is not None)
        assert owned > 0, (name, k)
        # candidates verified and rejected by the distance
        assert sum(int((r["d"] > k).sum()) for r in rs if r is not None) > 0, (name, k)
        # an accepted window through the end of the text, on a pattern shorter than the text
        wrapped = 0
        for q, r in zip(sel, rs):
            if r is not None and len(pats[q]) <= n:
                wrapped += int((r["keep"] & (r["s"] + len(pats[q]) > n)).sum())
        assert wrapped > 0, (name, k)
        # the pattern longer than the text is found
        for q, r in zip(sel, rs):
            if len(pats[q]) == n + 5:
                assert r["keep"].sum() >= 1


def test_candidate_counts_grow_with_k():
    cs = [restated_case("fam_dna", k)[1] for k in SEED_KS]
    assert all(a < b for a, b in zip(cs, cs[1:])), cs
    assert cs[-1] <= 210000  # what one GPU call of the suite verifies at most
