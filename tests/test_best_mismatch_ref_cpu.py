"""The best-stratum reference and the inputs of tests/test_zz_gpu_best_mismatch.py, without a
GPU: best_from_hist (tests/helpers/best_ref.py) on hand-made tables, on the enumeration and on
the scan, and the conditions the GPU tests' batches must meet — every outcome 0, 1, 2, 3 and
"none" on each family text, and on the mixed batch every outcome at 10 % or more with
pending-list lengths that span several blocks and are no multiple of a wave.  Only
expected_hist and scan_hamming are used; the library computes nothing here."""
import numpy as np
import pytest

import oracle as O
from helpers.best_ref import (MIXED_N, NONE, best_family_case, best_from_hist, mixed_case, outcomes,
                              pending_lengths)
from helpers.mismatch_ref import KMAX, expected_hist, scan_hamming


def test_best_from_hist_by_hand():
    hist = np.array([[2, 0, 5, 1], [0, 0, 5, 1], [0, 0, 0, 9], [0, 0, 0, 0], [0, 3, 0, 0]], np.uint64)
    for k, dist, cnt in [(0, [0, NONE, NONE, NONE, NONE], [2, 0, 0, 0, 0]),
                         (1, [0, NONE, NONE, NONE, 1], [2, 0, 0, 0, 3]),
                         (2, [0, 2, NONE, NONE, 1], [2, 5, 0, 0, 3]),
                         (3, [0, 2, 3, NONE, 1], [2, 5, 9, 0, 3])]:
        d, c = best_from_hist(hist, k)
        assert d.dtype == np.uint8 and c.dtype == np.uint64
        assert d.tolist() == dist and c.tolist() == cnt, k
    d, c = best_from_hist(np.zeros((0, 4), np.uint64), 3)
    assert len(d) == 0 and len(c) == 0


def test_semantics_on_banana():
    """The consequences the header lists, from the enumeration: m = 0 gives (0, n); an absent
    symbol never counts; d > m never resolves; k = 0 is the exact count."""
    text = b"banana$"
    ref = O.Index(text)
    pats = [b"", b"ana", b"bnn", b"x", b"xx", b"a", b"banana$ba"]
    hist = expected_hist(ref, text, pats, KMAX)
    d, c = best_from_hist(hist, KMAX)
    assert d.tolist() == [0, 0, 1, 1, 2, 0, 0] and c.tolist() == [7, 2, 1, 7, 7, 3, 1]
    d0, c0 = best_from_hist(hist, 0)
    assert d0.tolist() == [0, 0, NONE, NONE, NONE, 0, 0]
    assert c0.tolist() == [ref.count(p) for p in pats]
    d1, _ = best_from_hist(hist, 1)
    assert d1.tolist() == [0, 0, 1, 1, NONE, 0, 0]  # "xx": two absent symbols need d = 2
    # best_count is column best_dist of the histogram at any bound >= best_dist
    for k in range(KMAX + 1):
        dk, ck = best_from_hist(hist, k)
        for q in np.flatnonzero(dk != NONE):
            assert ck[q] == hist[q, dk[q]] and dk[q] == d[q]


def test_enumeration_and_scan_agree_on_best():
    text = O.gen_dna(5, 300).tobytes()[:-1] + b"$"
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pats = [bytes(acgt[rng.integers(0, 4, m)]) for m in (3, 5, 6, 7) for _ in range(5)] + [b""]
    a = best_from_hist(expected_hist(O.Index(text), text, pats, KMAX), KMAX)
    b = best_from_hist(scan_hamming(text, pats, KMAX)[0], KMAX)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


@pytest.mark.parametrize("name", ["fam_dna", "fam_dna_N", "fam_alpha12", "fam_bytes"])
def test_family_texts_hold_every_outcome(name):
    text, pats, hist = best_family_case(name)
    out = outcomes(hist)
    assert len(hist) == len(pats) and sum(out) == len(pats)
    assert all(v >= 5 for v in out), out
    if name == "fam_dna":
        assert out[:4] == [14, 35, 19, 21]
    # the "none" outcome comes from the added random 21- and 33-mers (and the absent-byte
    # patterns need d = 1 at least)
    dist, cnt = best_from_hist(hist, KMAX)
    assert (dist[-12:] == NONE).all() and (cnt[-12:] == 0).all()
    assert sorted({len(p) for p in pats[-12:]}) == [21, 33]


def test_mixed_batch_conditions():
    text, pats, hist = mixed_case()
    assert len(pats) == MIXED_N == 1000 and all(12 <= len(p) <= 16 for p in pats)
    out = outcomes(hist)
    assert sum(out) == MIXED_N and all(v >= MIXED_N // 10 for v in out), out
    lens = pending_lengths(hist)
    assert all(v > 256 and v % 64 for v in lens), lens
    assert lens == [MIXED_N - sum(out[:d + 1]) for d in range(KMAX)]
    # the prefixes the list-edge test takes hold more than one outcome from 63 patterns on
    dist, _ = best_from_hist(hist, KMAX)
    assert len(set(dist[:63].tolist())) == 5
