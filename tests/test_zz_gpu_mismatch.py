"""Count within k mismatches, per distance (include/cs_fmindex_approx.h) against the oracle.

hist[d] of a pattern is the sum of the oracle's exact count over every string at Hamming
distance d from it, over the symbols present in the text: the expected table enumerates those
neighbours (itertools) and counts them all in one oracle batch.  The histogram of a bound k is
the first k + 1 columns of the k = 3 table, so a text's table is computed once and shared.
The file's 62 tests take 4.3 s on one MI355X (the C++ program's wrapper 0.7 s more).
The file is named to collect after every suite that was here before it, so those keep the
positions they had in a run.
"""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg
from helpers.mismatch_ref import KMAX, _absent_byte, _dev, _present, device_hist, expected_hist

pytestmark = pytest.mark.gpu

# one variant per instantiation of with_engine (fm_search.hpp): occurrence lines with and
# without the prefix table, learned lines, the quaternary matrix, the binary wavelet matrix in
# Line32 / Line64 / Line32W lines, and wide occurrence lines
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
        pats.append(b"banana$ba")  # longer than the text (m = 9 > n = 7; cyclic count 1)
    return pats


_CASES = {}


def _case(name):
    """(text, patterns, expected k = 3 table, oracle), computed once per text."""
    if name not in _CASES:
        text = TEXTS[name]()
        ref = O.Index(text)
        pats = _patterns(name, text)
        _CASES[name] = (text, pats, expected_hist(ref, text, pats, KMAX), ref)
    return _CASES[name]


# ---- 1. engines x small texts -------------------------------------------------
@pytest.fixture(params=sorted(VARIANTS))
def variant(request):
    m = load_pkg()
    with m.build_options(VARIANTS[request.param]):
        yield m


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_engines_small_texts(variant, name):
    text, pats, want, _ = _case(name)
    g = variant.FMIndex.build_from_text(text)
    exact = g.count_batch(pats)
    for k in range(KMAX + 1):
        got_d = device_hist(g, pats, k)
        got_h = g.count_mismatches_batch(pats, k)
        assert got_d.tolist() == want[:, :k + 1].tolist(), (name, k, "device")
        assert got_h.tolist() == want[:, :k + 1].tolist(), (name, k, "host")
        assert got_d[:, 0].tolist() == exact.tolist()


# ---- 2. full byte alphabet ------------------------------------------------------
@pytest.mark.parametrize("engine", ["qwm", "wavelet"])
def test_full_byte_alphabet(engine):
    pkg = load_pkg()
    if "bytes" not in _CASES:
        text = O.gen_bytes(21, 2000).tobytes()
        ref = O.Index(text)
        pats = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(text, np.uint8), 4, 50, seed=5)]
        _CASES["bytes"] = (text, pats, expected_hist(ref, text, pats, 1), ref)
    text, pats, want, _ = _CASES["bytes"]
    with pkg.build_options({"CS_FM_ENGINE": engine}):
        g = pkg.FMIndex.build_from_text(text)
    assert device_hist(g, pats, 1).tolist() == want.tolist()
    assert g.count_mismatches_batch(pats, 1).tolist() == want.tolist()


# ---- 3. the workload's shape ----------------------------------------------------
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
    want = expected_hist(ref, text, pats, 2)
    g = pkg.FMIndex.build_from_text(text)
    got = device_hist(g, pats, 2, fixed_m=20)
    assert got.tolist() == want.tolist()
    assert (want.sum(axis=1) > 0).all()


# ---- 4. grid edges ----------------------------------------------------------------
def test_grid_edges():
    pkg = load_pkg()
    text, _, _, ref = _case("dna_5k")
    base = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(text, np.uint8), 6, 64, seed=2)]
    want = expected_hist(ref, text, base, 1)
    g = pkg.FMIndex.build_from_text(text)
    for npat in (1, 255, 257, 3000):
        pats = [base[q % 64] for q in range(npat)]
        got = device_hist(g, pats, 1)
        assert got.tolist() == want[np.arange(npat) % 64].tolist(), npat


# ---- 5. flags and errors ------------------------------------------------------------
def test_flags_and_errors():
    pkg = load_pkg()
    text, pats, want, _ = _case("dna_5k")
    g = pkg.FMIndex.build_from_text(text)
    plain = device_hist(g, pats, 2)
    assert plain.tolist() == want[:, :3].tolist()
    assert device_hist(g, pats, 2, flags=pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS).tolist() == plain.tolist()
    with pytest.raises(pkg.FMIndexError) as ei:
        g.count_mismatches_batch(pats, 4)
    assert ei.value.status == pkg.CS_ERR_INVALID and "CS_MM_MAX" in str(ei.value) and "3" in str(ei.value)
    with pytest.raises(pkg.FMIndexError) as ei:
        device_hist(g, pats, 4)
    assert ei.value.status == pkg.CS_ERR_INVALID
    with pytest.raises(pkg.FMIndexError) as ei:
        g.count_mismatches(b"ACG", 4)
    assert ei.value.status == pkg.CS_ERR_INVALID
    with pytest.raises(pkg.FMIndexError) as ei:
        g.count_mismatches_batch(buf=np.frombuffer(b"ACGT", np.uint8), offs=np.array([0, 3, 2], np.uint64), k=1)
    assert ei.value.status == pkg.CS_ERR_INVALID
    # a batch of empty patterns may pass d_pats = NULL: every row is [n, 0, ...]
    st = torch.cuda.current_stream().cuda_stream
    d_o = _dev(np.array([7, 7, 7, 7], np.int64), torch.int64)
    d_h = torch.full((3 * 3,), -1, dtype=torch.int64, device="cuda")
    g.count_mismatch_device(0, d_o.data_ptr(), 3, 2, d_h.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert d_h.cpu().tolist() == [len(text), 0, 0] * 3


# ---- 6. single pattern ----------------------------------------------------------------
def test_single_pattern():
    pkg = load_pkg()
    text = b"banana$"
    want = expected_hist(O.Index(text), text, [b"ana"], 1)[0]
    g = pkg.FMIndex.build_from_text(text)
    got = g.count_mismatches(b"ana", 1)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist()
    assert want[0] == 2
