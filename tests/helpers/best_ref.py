"""What the best-stratum suites share (tests/test_best_mismatch_ref_cpu.py,
tests/test_zz_gpu_best_mismatch.py; include/cs_fmindex_approx_best.h).

The reference is best_from_hist over a histogram that never comes from the library: the
enumeration (expected_hist) on the small texts, the cyclic Hamming scan (scan_hamming) on the
family texts, both of tests/helpers/mismatch_ref.py.

The small TEXTS / VARIANTS tables and the pattern construction are those of the first mismatch
suite (tests/test_zz_gpu_mismatch.py), copied: a test module is not imported from here.
"""
import numpy as np

import oracle as O
from helpers.mismatch_ref import (CANARY, KMAX, _absent_byte, _dev, _present, expected_hist, family_case,
                                  scan_hamming)

NONE = 0xFF  # CS_MM_NONE


def best_from_hist(hist, k):
    """(best_dist uint8 [npat], best_count uint64 [npat]) of a histogram table [npat, >= k + 1]
    at bound k: the first non-zero column among 0..k and its value, (NONE, 0) without one."""
    h = np.atleast_2d(np.asarray(hist, np.uint64))[:, :k + 1]
    hit = h > 0
    any_ = hit.any(axis=1)
    first = hit.argmax(axis=1)
    dist = np.where(any_, first, NONE).astype(np.uint8)
    count = np.where(any_, h[np.arange(len(h)), first], 0).astype(np.uint64)
    return dist, count


def outcomes(hist, k=KMAX):
    """How many patterns resolve at 0, 1, .., k and how many at none: k + 2 figures."""
    dist, _ = best_from_hist(hist, k)
    return [int((dist == d).sum()) for d in range(k + 1)] + [int((dist == NONE).sum())]


def pending_lengths(hist, k=KMAX):
    """The pending-list lengths after rounds 0..k-1: the patterns with no hit at or below d."""
    dist, _ = best_from_hist(hist, k)
    return [int((dist > d).sum()) for d in range(k)]  # NONE = 255 is above every d


# ---- the small texts of the first mismatch suite --------------------------------------------
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
    "abab_noterm": lambda: b"abababab",           # no terminator: cyclic
    "all_same": lambda: b"a" * 100,
    "straddle_649": lambda: O.gen_dna(649, 649).tobytes(),  # a range straddling a line edge
    "dna_5k": lambda: O.gen_dna(7, 5000).tobytes(),
    "rare_N_40": lambda: _dna_with_n(11, 5000, 40),  # the rare-row list
    "alpha_12": lambda: _alpha12(12, 2000),
}


def small_patterns(name, text):
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
        pats.append(b"banana$ba")  # longer than the text (m = 9 > n = 7; cyclic count 1)
    return pats


_SMALL = {}


def small_case(name):
    """(text, patterns, the enumeration's k = 3 table), computed once per text and shared."""
    if name not in _SMALL:
        text = TEXTS[name]()
        pats = small_patterns(name, text)
        want = expected_hist(O.Index(text), text, pats, KMAX)
        want.setflags(write=False)
        _SMALL[name] = (text, pats, want)
    return _SMALL[name]


# ---- the family texts, with patterns that resolve nowhere ------------------------------------
_BEST_FAMILY = {}


def best_family_case(name):
    """(text, patterns, the scan's k = 3 table): family_case's patterns and table, then six
    uniform random 21- and 33-mers over the text's symbols scanned here (the "none" outcome:
    a random 21-mer has no window within 3 on these texts), computed once per text."""
    if name not in _BEST_FAMILY:
        text, pats, _, hist, _ = family_case(name)
        syms = np.array([s for s in _present(text) if s != text[-1]], np.uint8)
        rng = np.random.default_rng(7000 + len(text))
        extra = [bytes(syms[rng.integers(0, len(syms), m)]) for m in (21, 33) for _ in range(6)]
        ehist, _ = scan_hamming(text, extra, KMAX)
        table = np.concatenate([hist, ehist])
        table.setflags(write=False)
        _BEST_FAMILY[name] = (text, list(pats) + extra, table)
    return _BEST_FAMILY[name]


# ---- the mixed batch -------------------------------------------------------------------------
MIXED_N, MIXED_SEED = 1000, 2026
_MIXED = {}


def mixed_patterns(text):
    """MIXED_N patterns of length 12..16 on a DNA text with a terminator: pattern q is a text
    window with q mod 6 substitutions by other ACGT symbols at distinct places; q mod 6 = 5 is
    a uniform random ACGT string instead."""
    rng = np.random.default_rng(MIXED_SEED)
    t = np.frombuffer(text, np.uint8)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pats = []
    for q in range(MIXED_N):
        m = int(rng.integers(12, 17))
        if q % 6 == 5:
            pats.append(bytes(acgt[rng.integers(0, 4, m)]))
            continue
        i = int(rng.integers(0, len(t) - 1 - m))  # the window stays clear of the terminator
        p = t[i:i + m].copy()
        for j in rng.choice(m, q % 6, replace=False):
            o = acgt[acgt != p[j]]
            p[j] = o[int(rng.integers(0, len(o)))]
        pats.append(bytes(p))
    return pats


def mixed_case():
    """(text, patterns, the scan's k = 3 table) of the mixed batch on fam_dna, computed once."""
    if "m" not in _MIXED:
        text = family_case("fam_dna")[0]
        pats = mixed_patterns(text)
        hist, _ = scan_hamming(text, pats, KMAX)
        hist.setflags(write=False)
        _MIXED["m"] = (text, pats, hist)
    return _MIXED["m"]


# ---- the device call -------------------------------------------------------------------------
def device_best_async(g, pats, k, flags=0, fixed_m=None, stream=None):
    """Queues best_mismatch_device over CSR offsets (or fixed_m with d_offs = NULL) on the
    current stream without synchronising; the outputs carry CANARY prefilled entries after the
    last one.  -> the tensors to keep alive and read with read_best."""
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p = _dev(buf if len(buf) else np.zeros(1, np.uint8), torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    d_d = torch.full((npat + CANARY,), 0xEE, dtype=torch.uint8, device="cuda")
    d_c = torch.full((npat + CANARY,), -1, dtype=torch.int64, device="cuda")
    if fixed_m is None:
        g.best_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), npat, k, d_d.data_ptr(), d_c.data_ptr(),
                               flags=flags, stream=st)
    else:
        g.best_mismatch_device(d_p.data_ptr(), None, npat, k, d_d.data_ptr(), d_c.data_ptr(), fixed_m=fixed_m,
                               flags=flags, stream=st)
    return d_p, d_o, d_d, d_c, npat


def read_best(queued):
    """(dist, count) of a queued call after a synchronisation; every entry written (no 0xEE
    distance, no all-ones count left) and the canary entries untouched."""
    import torch
    _, _, d_d, d_c, npat = queued
    torch.cuda.synchronize()
    dist = d_d.cpu().numpy()
    cnt = d_c.cpu().numpy().view(np.uint64)
    assert (dist[npat:] == 0xEE).all() and (cnt[npat:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "canary overwritten"
    assert (dist[:npat] != 0xEE).all() and (cnt[:npat] != np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "entry not written"
    return dist[:npat], cnt[:npat]


def device_best(g, pats, k, flags=0, fixed_m=None):
    return read_best(device_best_async(g, pats, k, flags=flags, fixed_m=fixed_m))


def same_best(got, want, what):
    gd, gc = got
    wd, wc = want
    bad = np.flatnonzero((np.asarray(gd) != wd) | (np.asarray(gc) != wc))
    assert not len(bad), (what, [(int(q), int(gd[q]), int(gc[q]), int(wd[q]), int(wc[q])) for q in bad[:8]])
