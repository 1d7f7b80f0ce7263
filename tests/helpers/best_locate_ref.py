"""What the best-stratum locate suites share (tests/test_best_locate_ref_cpu.py,
tests/test_zz_gpu_best_locate.py; include/cs_fmindex_approx_best_locate.h).

The reference is best_pairs: best_from_hist over a histogram, then the reference pairs with
d == best_dist.  Neither ever comes from the library: the enumeration (expected_hist,
expected_pairs) on the small texts, the cyclic Hamming scan (scan_hamming) on the family texts
and the mixed batch, all of tests/helpers/mismatch_ref.py.
"""
import numpy as np

import oracle as O
from helpers.best_ref import NONE, best_family_case, best_from_hist, mixed_case, small_case
from helpers.mismatch_ref import CANARY, KMAX, _dev, expected_pairs, family_case, scan_hamming

SMALL_TEXTS = ("banana", "straddle_649", "dna_5k", "rare_N_40", "alpha_12")  # (the oracle locates on these)


def best_pairs(hist, pairs, k):
    """(best_dist uint8 [npat], per pattern the sorted int64 positions at that distance) of a
    histogram table [npat, >= k + 1] and the reference pairs (int64 [count, 2] per pattern)."""
    dist, _ = best_from_hist(hist, k)
    pos = [np.sort(p[p[:, 1] == int(dist[q]), 0]).astype(np.int64) if dist[q] != NONE
           else np.zeros(0, np.int64) for q, p in enumerate(pairs)]
    return dist, pos


def stratum_sizes(hist, pairs, k=KMAX):
    """Best-stratum positions per distance 0..k, summed over the patterns."""
    dist, pos = best_pairs(hist, pairs, k)
    return [int(sum(len(pos[q]) for q in np.flatnonzero(dist == d))) for d in range(k + 1)]


def leaves_of(text, pat, positions):
    """The leaves a stratum's positions fall into: window string -> its number of rows."""
    t = np.frombuffer(text, np.uint8)
    groups = {}
    for p in positions:
        w = t[(int(p) + np.arange(len(pat))) % len(t)].tobytes()
        groups[w] = groups.get(w, 0) + 1
    return groups


def multi_leaf_strata(text, pats, hist, pairs, k=KMAX):
    """How many patterns have a best stratum at d >= 1 that holds more than one leaf."""
    dist, pos = best_pairs(hist, pairs, k)
    return sum(1 for q, p in enumerate(pats)
               if dist[q] != NONE and dist[q] >= 1 and len(leaves_of(text, p, pos[q])) > 1)


# ---- the reference cases, each computed once and left unchanged ------------------------------
_SMALL, _FAMILY, _MIXED = {}, {}, {}


def small_locate_case(name):
    """(text, patterns, the enumeration's k = 3 table, the enumeration's k = 3 pairs)."""
    if name not in _SMALL:
        text, pats, table = small_case(name)
        pairs, _ = expected_pairs(O.Index(text), text, pats, KMAX)
        _SMALL[name] = (text, pats, table, pairs)
    return _SMALL[name]


def family_locate_case(name):
    """(text, best_family_case's patterns, the scan's k = 3 table, the scan's k = 3 pairs)."""
    if name not in _FAMILY:
        text, pats, table = best_family_case(name)
        fam = family_case(name)
        nfam = len(fam[1])
        assert pats[:nfam] == list(fam[1])
        _, extra = scan_hamming(text, pats[nfam:], KMAX)
        _FAMILY[name] = (text, pats, table, list(fam[4]) + extra)
    return _FAMILY[name]


def mixed_locate_case():
    """(text, patterns, the scan's k = 3 table, the scan's k = 3 pairs) of the mixed batch:
    mixed_case() keeps only the histogram, so the pairs are scanned again here."""
    if "m" not in _MIXED:
        text, pats, table = mixed_case()
        hist, pairs = scan_hamming(text, pats, KMAX)
        assert np.array_equal(hist, table)
        _MIXED["m"] = (text, pats, table, pairs)
    return _MIXED["m"]


# ---- the device call -------------------------------------------------------------------------
def device_best_locate(g, pats, k, flags=0, fixed_m=None, raw=False):
    """locate_best_mismatch_device: a sizing call (cap = 0, null positions), then the call, over
    CSR offsets or fixed_m with d_offs = NULL -> (dist, offsets, per-pattern sorted positions;
    raw: the positions as written).  best_dist is prefilled with 0xEE plus canaries, positions
    with all-ones plus canaries; every entry must be written, every canary kept, and the sizing
    call must already give the distances and offsets."""
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p = _dev(buf if len(buf) else np.zeros(1, np.uint8), torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    kw = dict(flags=flags, stream=st)
    if fixed_m is not None:
        kw["fixed_m"] = fixed_m
    d_offs_arg = d_o.data_ptr() if fixed_m is None else None
    d_d = torch.full((npat + CANARY,), 0xEE, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((npat + 1 + CANARY,), -1, dtype=torch.int64, device="cuda")
    total, written = g.locate_best_mismatch_device(d_p.data_ptr(), d_offs_arg, npat, k, d_d.data_ptr(),
                                                   d_oo.data_ptr(), None, 0, **kw)
    torch.cuda.synchronize()
    assert written == (total == 0)
    sized_oo, sized_d = d_oo.cpu().numpy().copy(), d_d.cpu().numpy().copy()
    d_pos = torch.full((total + CANARY,), -1, dtype=torch.int64, device="cuda")
    d_oo.fill_(-1)
    d_d.fill_(0xEE)
    tot2, written = g.locate_best_mismatch_device(d_p.data_ptr(), d_offs_arg, npat, k, d_d.data_ptr(),
                                                  d_oo.data_ptr(), d_pos.data_ptr(), total, **kw)
    torch.cuda.synchronize()
    assert written and tot2 == total
    oo, dist, pos = d_oo.cpu().numpy(), d_d.cpu().numpy(), d_pos.cpu().numpy()
    assert oo.tolist() == sized_oo.tolist() and dist.tolist() == sized_d.tolist(), "the sizing call differs"
    assert (oo[npat + 1:] == -1).all() and (dist[npat:] == 0xEE).all() and (pos[total:] == -1).all(), \
        "canary overwritten"
    assert (dist[:npat] != 0xEE).all() and (oo[:npat + 1] != -1).all() and (pos[:total] != -1).all(), \
        "entry not written"
    assert oo[npat] == total
    oo, dist, pos = oo[:npat + 1], dist[:npat], pos[:total]
    return dist, oo, (pos if raw else split_positions(oo, pos))


def split_positions(oo, pos):
    return [np.sort(np.asarray(pos[int(oo[q]):int(oo[q + 1])]).astype(np.int64)) for q in range(len(oo) - 1)]


def host_best_locate(g, pats, k):
    dist, oo, pos = g.locate_best_mismatches_batch(pats, k)
    assert dist.dtype == np.uint8 and oo.dtype == np.uint64 and pos.dtype == np.uint64
    assert len(dist) == len(pats) and len(oo) == len(pats) + 1 and len(pos) == oo[-1]
    return dist, oo, split_positions(oo, pos)


def same_best_locate(got, want, what):
    """got: (dist, offsets, per-pattern sorted positions); want: best_pairs' (dist, positions)."""
    gd, goo, gp = got
    wd, wp = want
    bad = np.flatnonzero(np.asarray(gd) != wd)
    assert not len(bad), (what, "dist", [(int(q), int(gd[q]), int(wd[q])) for q in bad[:8]])
    sizes = [len(w) for w in wp]
    assert np.asarray(goo).astype(np.int64).tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist(), \
        (what, "offsets")
    for q, (a, b) in enumerate(zip(gp, wp)):
        assert a.tolist() == b.tolist(), (what, "positions of pattern", q)
