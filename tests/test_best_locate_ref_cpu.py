"""The best-stratum locate reference and the inputs of tests/test_zz_gpu_best_locate.py, without a
GPU: best_pairs (tests/helpers/best_locate_ref.py) on hand-made tables and on the enumeration,
and the conditions the GPU tests' batches must meet, from the references alone — positions at
every distance 0..3, strata of more than one leaf, leaves wider than kLocSmall = 32 rows, and a
best stratum that is a small share of the pairs within 3 on the family texts (what the call is
for).  The figures in the comments are the cyclic scan's; they are asserted as inequalities and
shares.  The library computes nothing here."""
import numpy as np
import pytest

import oracle as O
from helpers.best_locate_ref import (best_pairs, family_locate_case, leaves_of, mixed_locate_case,
                                     multi_leaf_strata, small_locate_case, stratum_sizes)
from helpers.best_ref import NONE, best_from_hist
from helpers.mismatch_ref import KMAX, expected_hist, expected_pairs, family_case, scan_hamming

FAMILY = ("fam_dna", "fam_dna_N", "fam_alpha12", "fam_bytes")


def test_best_pairs_by_hand():
    hist = np.array([[2, 0, 1, 0], [0, 0, 2, 1], [0, 0, 0, 0], [9, 0, 0, 0]], np.uint64)
    pairs = [np.array([[5, 0], [1, 0], [3, 2]], np.int64), np.array([[4, 3], [8, 2], [2, 2]], np.int64),
             np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64)]  # (the last: an empty pattern, hist[0] = n)
    for k, dist, pos in [(0, [0, NONE, NONE, 0], [[1, 5], [], [], []]),
                         (1, [0, NONE, NONE, 0], [[1, 5], [], [], []]),
                         (2, [0, 2, NONE, 0], [[1, 5], [2, 8], [], []]),
                         (3, [0, 2, NONE, 0], [[1, 5], [2, 8], [], []])]:
        d, p = best_pairs(hist, pairs, k)
        assert d.dtype == np.uint8 and d.tolist() == dist, k
        assert [x.tolist() for x in p] == pos and all(x.dtype == np.int64 for x in p), k
    assert stratum_sizes(hist, pairs) == [2, 0, 2, 0]


def test_semantics_on_banana():
    """The consequences the header lists, from the enumeration: m = 0 gives distance 0 and no
    positions; an absent symbol never counts; d > m never resolves; k = 0 is the exact locate;
    for m > 0 a pattern's size is best_count."""
    text = b"banana$"
    ref = O.Index(text)
    pats = [b"", b"ana", b"bnn", b"x", b"xx", b"a", b"banana$ba", b"xxxx"]
    hist = expected_hist(ref, text, pats, KMAX)
    pairs, _ = expected_pairs(ref, text, pats, KMAX)
    d, p = best_pairs(hist, pairs, KMAX)
    assert d.tolist() == [0, 0, 1, 1, 2, 0, 0, NONE]
    assert [x.tolist() for x in p] == [[], [1, 3], [0], list(range(7)), list(range(7)), [1, 3, 5], [0], []]
    d0, p0 = best_pairs(hist, pairs, 0)
    assert d0.tolist() == [0, 0, NONE, NONE, NONE, 0, 0, NONE]
    assert [x.tolist() for x in p0] == [sorted(ref.locate(q, limit=100)) for q in pats]
    for k in range(KMAX + 1):
        dk, pk = best_pairs(hist, pairs, k)
        _, ck = best_from_hist(hist, k)
        assert [len(x) for x in pk[1:]] == ck[1:].tolist(), k


@pytest.mark.parametrize("name", ["banana", "dna_5k"])
def test_small_cases_reach_beyond_exact(name):
    text, pats, hist, pairs = small_locate_case(name)
    assert len(hist) == len(pairs) == len(pats)
    sizes = stratum_sizes(hist, pairs)
    assert sizes[0] > 0 and sizes[1] > 0 and sum(sizes[2:]) > 0, sizes
    if name == "dna_5k":  # its 1-mer: one leaf of more than kLocSmall = 32 rows at d = 0
        d, p = best_pairs(hist, pairs, KMAX)
        q = next(q for q, x in enumerate(pats) if len(x) == 1)
        assert d[q] == 0 and max(leaves_of(text, pats[q], p[q]).values()) > 32


@pytest.mark.parametrize("name", FAMILY)
def test_family_texts(name):
    text, pats, hist, pairs = family_locate_case(name)
    assert len(pats) == len(hist) == len(pairs)
    # the scan's pairs and its table agree (the added patterns were scanned twice)
    for q in range(len(pats)):
        if pats[q]:
            assert np.bincount(pairs[q][:, 1], minlength=KMAX + 1).tolist() == hist[q].tolist(), q
    sizes = stratum_sizes(hist, pairs)
    assert all(v > 0 for v in sizes), sizes
    # strata of more than one leaf at d >= 1 (fam_dna 8, fam_dna_N 15, fam_alpha12 2, fam_bytes 4)
    assert multi_leaf_strata(text, pats, hist, pairs) >= 2
    # best-stratum positions against all pairs within 3: 1,983 of 9,845 (fam_dna), 1,919 of
    # 9,522 (fam_dna_N), 356 of 3,757 (fam_alpha12), 358 of 3,764 (fam_bytes)
    within3 = sum(len(p) for p in pairs)
    assert 0 < sum(sizes) * 4 < within3, (sum(sizes), within3)
    # a stratum of more than kLocSmall = 32 rows in one leaf at d = 0: the 1-mer
    d, p = best_pairs(hist, pairs, KMAX)
    q = next(q for q, x in enumerate(pats) if len(x) == 1)
    assert d[q] == 0 and len(leaves_of(text, pats[q], p[q])) == 1 and len(p[q]) > 32


def test_mixed_batch_conditions():
    text, pats, hist, pairs = mixed_locate_case()
    sizes = stratum_sizes(hist, pairs)  # 1,467 / 1,512 / 1,417 / 1,556
    assert all(v >= 1000 for v in sizes), sizes
    within3 = sum(len(p) for p in pairs)  # 5,952 of 7,177
    assert sum(sizes) < within3 and sum(sizes) * 4 > within3 * 3, (sum(sizes), within3)
    assert multi_leaf_strata(text, pats, hist, pairs) >= 20  # 56
    # per-round resolved lists: several blocks' worth is not needed, but no list is empty and
    # none is a multiple of a wave
    d, _ = best_pairs(hist, pairs, KMAX)
    per_round = [int((d == r).sum()) for r in range(KMAX + 1)]
    assert all(v > 64 and v % 64 for v in per_round), per_round


def test_absent_byte_patterns_resolve_with_wide_leaves():
    """'#', '##', '###' on fam_dna: every window is at distance m, so they resolve at d = 1, 2,
    3 with n positions each, the terminator's window included; their leaves (one per string
    over the present symbols that occurs) are wider than 32 rows and are reached from frames
    below the top."""
    text = family_case("fam_dna")[0]
    n = len(text)
    assert b"#" not in text
    pats = [b"#", b"##", b"###"]
    hist, pairs = scan_hamming(text, pats, KMAX)
    d, p = best_pairs(hist, pairs, KMAX)
    assert d.tolist() == [1, 2, 3]
    for q in range(3):
        assert p[q].tolist() == list(range(n))
        leaves = leaves_of(text, pats[q], p[q])
        assert len(leaves) > 1 and max(leaves.values()) > 32, (q, len(leaves))
    for k in range(KMAX):
        assert best_pairs(hist, pairs, k)[0].tolist() == [1, 2, 3][:k] + [NONE] * (3 - k)
