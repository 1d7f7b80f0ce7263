"""Best-stratum locate (include/cs_fmindex_approx_best_locate.h): per pattern the smallest distance
d <= k with a hit and the positions at that distance only, against best_pairs of a histogram and
pairs the library never computed — the enumeration on the small texts, the cyclic Hamming scan
on the family texts and the mixed batch (tests/helpers/best_locate_ref.py; the batches'
conditions are held without a GPU in tests/test_best_locate_ref_cpu.py).  That the sizes equal
best_mismatches_batch's counts and that the raw output equals locate_mismatch_device's filtered
to d == best, in order, are consistency checks, never the expectation.

What is new here are the rounds of launch_best_locate_mm_size / _emit: the pending lists and the
resolved slices between them, emit launches over slices that are empty, one entry or several
blocks long, and the leaves of all rounds in one walk.  Family cases: every variant of
tests/test_zz_gpu_best_mismatch.py runs at every k and every length.  Named to collect after the
suites that were here before it.
"""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg
from helpers.best_locate_ref import (SMALL_TEXTS, best_pairs, device_best_locate, family_locate_case,
                                     host_best_locate, mixed_locate_case, same_best_locate, small_locate_case,
                                     split_positions)
from helpers.best_ref import NONE, VARIANTS
from helpers.mismatch_ref import KMAX, _dev, device_pairs, scan_hamming

pytestmark = pytest.mark.gpu


def _build(text, vname="auto", opts=None):
    pkg = load_pkg()
    with pkg.build_options(VARIANTS[vname] if opts is None else opts):
        return pkg.FMIndex.build_from_text(text)


def _check_all_k(g, pats, table, pairs, what, host=True):
    for k in range(KMAX + 1):
        want = best_pairs(table, pairs, k)
        same_best_locate(device_best_locate(g, pats, k), want, what + (k, "device"))
        if host:
            same_best_locate(host_best_locate(g, pats, k), want, what + (k, "host"))


def _filtered_locate(g, pats, k, dist):
    """locate_mismatch_device's raw output at bound k, the pairs with d == the pattern's best
    distance kept, in the order written."""
    oo, pos, dd = device_pairs(g, pats, k, raw=True)
    own = np.repeat(np.arange(len(pats)), np.diff(oo))
    keep = dd == np.asarray(dist)[own]
    return pos[keep]


# ---- 1. small texts x the eight engine variants ------------------------------------------------
@pytest.mark.parametrize("vname", sorted(VARIANTS))
@pytest.mark.parametrize("name", SMALL_TEXTS)
def test_engines_small_texts(name, vname):
    text, pats, table, pairs = small_locate_case(name)
    g = _build(text, vname)
    _check_all_k(g, pats, table, pairs, (name, vname))
    for k in range(KMAX + 1):
        wd, wp = best_pairs(table, pairs, k)
        for q in range(0, len(pats), 3):  # the single-pattern call
            d, pos = g.locate_best_mismatches(pats[q], k)
            assert pos.dtype == np.uint64
            assert (NONE if d is None else d, sorted(pos.tolist())) == (int(wd[q]), wp[q].tolist()), \
                (name, vname, k, q)
        # consistency only: the best-stratum call's counts, and the mismatch locate's order
        dist, oo, raw = device_best_locate(g, pats, k, raw=True)
        bd, bc = g.best_mismatches_batch(pats, k)
        assert bd.tolist() == dist.tolist()
        assert [int(c) for c, p in zip(bc, pats) if p] == [int(s) for s, p in zip(np.diff(oo), pats) if p]
        assert raw.tolist() == _filtered_locate(g, pats, k, dist).tolist(), (name, vname, k, "order")


# ---- 2. family texts ---------------------------------------------------------------------------
DNA_VARIANTS = ("auto", "noprefix", "learned", "qwm", "wavelet", "wide_bucketed")
FAMILY_CASES = ([(n, v) for n in ("fam_dna", "fam_dna_N") for v in DNA_VARIANTS] +
                [(n, v) for n in ("fam_alpha12", "fam_bytes") for v in ("auto", "wavelet")])


@pytest.mark.parametrize("name,vname", FAMILY_CASES, ids=["%s-%s" % c for c in FAMILY_CASES])
def test_family_texts(name, vname):
    pkg = load_pkg()
    text, pats, table, pairs = family_locate_case(name)
    g = _build(text, vname)
    _check_all_k(g, pats, table, pairs, (name, vname), host=vname == "auto")
    sel = [q for q, p in enumerate(pats) if len(p) == 33]  # fixed_m with d_offs = NULL
    assert len(sel) >= 13
    sub = [pats[q] for q in sel]
    for k in range(KMAX + 1):
        same_best_locate(device_best_locate(g, sub, k, fixed_m=33),
                         best_pairs(table[sel], [pairs[q] for q in sel], k), (name, vname, k, "fixed_m"))
    if vname == "auto":
        for f in (pkg.Q_NO_PREFIX, pkg.Q_NO_CONTEXTS, pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS):
            for k in range(KMAX + 1):
                same_best_locate(device_best_locate(g, pats, k, flags=f), best_pairs(table, pairs, k),
                                 (name, k, "flags", f))


# ---- 3. the mixed batch ------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["auto", "qwm", "wavelet"])
def test_mixed_batch(vname):
    text, pats, table, pairs = mixed_locate_case()
    g = _build(text, vname)
    _check_all_k(g, pats, table, pairs, ("mixed", vname), host=vname == "auto")
    rev = pats[::-1]  # per pattern, whatever its place in the batch and in the lists
    for k in range(KMAX + 1):
        wd, wp = best_pairs(table, pairs, k)
        same_best_locate(device_best_locate(g, rev, k), (wd[::-1], wp[::-1]), ("mixed reversed", vname, k))
    if vname == "auto":  # consistency only: the order of the mismatch locate, 56 multi-leaf strata
        dist, _, raw = device_best_locate(g, pats, KMAX, raw=True)
        assert raw.tolist() == _filtered_locate(g, pats, KMAX, dist).tolist()


# ---- 4. list edges -----------------------------------------------------------------------------
def test_list_edges_prefixes():
    text, pats, table, pairs = mixed_locate_case()
    g = _build(text)
    for npat in (1, 63, 64, 65, 257):
        for k in range(KMAX + 1):
            same_best_locate(device_best_locate(g, pats[:npat], k), best_pairs(table[:npat], pairs[:npat], k),
                             ("prefix", npat, k))


def test_list_edges_all_exact_none_and_absent():
    text, _, _, _ = mixed_locate_case()
    g = _build(text)
    n = len(text)
    rng = np.random.default_rng(31)
    # every pattern occurs exactly: the later resolved lists are empty, their emit launches skipped
    starts = rng.integers(0, n - 1 - 30, 700)
    exact = [text[int(i):int(i) + 30] for i in starts]
    hist, pairs = scan_hamming(text, exact, 0)
    assert (hist[:, 0] > 0).all() and hist[:, 0].max() > 1
    for k in range(KMAX + 1):
        got = device_best_locate(g, exact, k)
        assert (got[0] == 0).all()
        same_best_locate(got, best_pairs(hist, pairs, 0), ("all exact", k))
    # no pattern resolves within 3: every pending list stays full, nothing is emitted
    absent = [b"#####"] * 300
    assert b"#" not in text
    for k in range(KMAX + 1):
        dist, oo, pos = device_best_locate(g, absent, k)
        assert (dist == NONE).all() and not oo.any() and all(len(p) == 0 for p in pos), k
    dist, oo, pos = g.locate_best_mismatches_batch(absent, KMAX)
    assert (dist == NONE).all() and not oo.any() and len(pos) == 0
    d, pos = g.locate_best_mismatches(b"#####", KMAX)
    assert d is None and len(pos) == 0
    # '#', '##', '###' (d = 1, 2, 3 with n positions each, leaves wider than 32 rows from frames
    # below the top) between exact patterns
    mix = []
    for i in range(40):
        mix += [exact[i], [b"#", b"##", b"###"][i % 3]]
    hist, pairs = scan_hamming(text, mix, KMAX)
    for k in range(KMAX + 1):
        want = best_pairs(hist, pairs, k)
        same_best_locate(device_best_locate(g, mix, k), want, ("absent mixed", k))
    assert best_pairs(hist, pairs, KMAX)[0][1:6:2].tolist() == [1, 2, 3]
    assert [len(p) for p in best_pairs(hist, pairs, KMAX)[1][1:6:2]] == [n, n, n]


# ---- 5. position phases ------------------------------------------------------------------------
def test_position_phases():
    pkg = load_pkg()
    text, pats, table, pairs = small_locate_case("dna_5k")
    want = best_pairs(table, pairs, 2)
    builds = {"full_sa": {}, "walk_lines": {"CS_FM_FULL_SA": "0"},
              "engine_lf": {"CS_FM_FULL_SA": "0", "CS_FM_WALK": "0"}}
    for label, opts in builds.items():
        g = _build(text, opts=opts)
        same_best_locate(device_best_locate(g, pats, 2), want, (label,))
        if label == "full_sa":
            for f in (pkg.Q_NO_FULL_SA | pkg.Q_NO_WALK_LINES, pkg.Q_NO_FULL_SA,
                      pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS):
                same_best_locate(device_best_locate(g, pats, 2, flags=f), want, (label, f))


# ---- 6. k = 0 is the exact locate --------------------------------------------------------------
def test_k0_equals_exact_locate():
    pkg = load_pkg()
    text, pats, _, _ = small_locate_case("dna_5k")
    g = _build(text)
    n = len(text)
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    tot, ok = g.locate_device(d_p.data_ptr(), d_o.data_ptr(), npat, n, d_oo.data_ptr(), None, 0)
    d_pos = torch.zeros(max(tot, 1), dtype=torch.int64, device="cuda")
    tot, ok = g.locate_device(d_p.data_ptr(), d_o.data_ptr(), npat, n, d_oo.data_ptr(), d_pos.data_ptr(), tot)
    assert ok and tot > 32
    dist, oo, pos = device_best_locate(g, pats, 0, raw=True)
    assert oo.tolist() == d_oo.cpu().tolist()
    assert pos.tolist() == d_pos[:tot].cpu().tolist()  # element for element, unsorted
    sizes = np.diff(oo)
    assert [int(d) for d in dist] == [0 if (s or not p) else NONE for s, p in zip(sizes, pats)]


# ---- 7. capacity -------------------------------------------------------------------------------
def test_capacity():
    pkg = load_pkg()
    text, pats, table, pairs = small_locate_case("dna_5k")
    wd, wp = best_pairs(table, pairs, 2)
    want_oo = np.concatenate([[0], np.cumsum([len(p) for p in wp])]).tolist()
    total = want_oo[-1]
    g = _build(text)
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_d = torch.full((npat,), 0xEE, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    # one short: the total, the offsets and the distances, nothing else
    tot = pkg.C.c_uint64()
    s = pkg.lib().cs_fm_locate_best_mismatch_device(g._h, d_p.data_ptr(), d_o.data_ptr(), 0, npat, 2,
                                                    d_d.data_ptr(), d_oo.data_ptr(), d_pos.data_ptr(), total - 1,
                                                    pkg.C.byref(tot), 0, st)
    torch.cuda.synchronize()
    assert s == pkg.CS_ERR_CAPACITY and tot.value == total
    assert d_oo.cpu().tolist() == want_oo and d_d.cpu().tolist() == wd.tolist()
    assert (d_pos == -1).all().item()
    # the sizing call: cap = 0 with null positions — also a best-stratum call
    d_d.fill_(0xEE)
    d_oo.fill_(-1)
    tot2, written = g.locate_best_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), npat, 2, d_d.data_ptr(),
                                                  d_oo.data_ptr(), None, 0, stream=st)
    torch.cuda.synchronize()
    assert tot2 == total and not written
    assert d_oo.cpu().tolist() == want_oo and d_d.cpu().tolist() == wd.tolist()
    # the host batch with a capacity one short: the early return after the sizing step
    out_offs = np.zeros(npat + 1, np.uint64)
    out_dist = np.full(npat, 0xEE, np.uint8)
    hp = np.full(total, 7, np.uint64)
    s = pkg.lib().cs_fm_locate_best_mismatch_batch(g._h, pkg._u8(buf), pkg._u64(offs), npat, 2, pkg._u8(out_dist),
                                                   pkg._u64(out_offs), pkg._u64(hp), total - 1, pkg.C.byref(tot),
                                                   None)
    assert s == pkg.CS_ERR_CAPACITY and tot.value == total
    assert out_offs.tolist() == want_oo and out_dist.tolist() == wd.tolist() and (hp == 7).all()
    # the single-pattern call: a capacity one short, then enough
    q = next(q for q, p in enumerate(wp) if len(p) > 1)
    one_d = (pkg.C.c_uint8 * 1)(0xEE)
    one_p = np.full(len(wp[q]), 7, np.uint64)
    nout = pkg.C.c_uint64()
    s = pkg.lib().cs_fm_locate_best_mismatch(g._h, pats[q], len(pats[q]), 2, one_d, pkg._u64(one_p), len(wp[q]) - 1,
                                             pkg.C.byref(nout))
    assert s == pkg.CS_ERR_CAPACITY and nout.value == len(wp[q]) and one_d[0] == wd[q] and (one_p == 7).all()
    s = pkg.lib().cs_fm_locate_best_mismatch(g._h, pats[q], len(pats[q]), 2, one_d, pkg._u64(one_p), len(wp[q]),
                                             pkg.C.byref(nout))
    assert s == pkg.CS_OK and nout.value == len(wp[q]) and sorted(one_p.tolist()) == wp[q].tolist()


# ---- 8. npat = 0 and errors --------------------------------------------------------------------
def test_npat_zero_and_errors():
    pkg = load_pkg()
    text, pats, _, _ = small_locate_case("dna_5k")
    g = _build(text)
    st = torch.cuda.current_stream().cuda_stream
    d_d = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    # npat = 0: d_out_offs[0] = 0, total = 0, nothing else touched (and nothing else needed)
    tot, written = g.locate_best_mismatch_device(None, None, 0, 3, d_d.data_ptr(), d_oo.data_ptr(),
                                                 d_pos.data_ptr(), 4, stream=st)
    torch.cuda.synchronize()
    assert (tot, written) == (0, True)
    assert d_oo.cpu().tolist() == [0, -1, -1, -1] and (d_d == 0xEE).all().item() and (d_pos == -1).all().item()
    d_oo.fill_(-1)
    assert g.locate_best_mismatch_device(None, None, 0, 3, None, d_oo.data_ptr(), None, 0, stream=st) == (0, True)
    torch.cuda.synchronize()
    assert d_oo.cpu().tolist() == [0, -1, -1, -1]
    dist, oo, pos = g.locate_best_mismatches_batch([], 2)
    assert len(dist) == 0 and oo.tolist() == [0] and len(pos) == 0
    # null outputs, k > CS_MM_MAX
    d_p = _dev(np.frombuffer(b"ACGTACGT", np.uint8), torch.uint8)
    P, D, OO, POS = d_p.data_ptr(), d_d.data_ptr(), d_oo.data_ptr(), d_pos.data_ptr()
    for args in ((P, None, 2, 1, None, OO, POS, 4),   # null distances with npat > 0
                 (P, None, 2, 1, D, None, POS, 4),    # null offsets
                 (P, None, 2, 1, D, OO, None, 4),     # null positions with cap > 0
                 (P, None, 2, 4, D, OO, POS, 4)):     # k > CS_MM_MAX
        with pytest.raises(pkg.FMIndexError) as ei:
            g.locate_best_mismatch_device(*args, fixed_m=4, stream=st)
        assert ei.value.status == pkg.CS_ERR_INVALID
    tot = pkg.C.c_uint64()
    assert pkg.lib().cs_fm_locate_best_mismatch_device(g._h, P, None, 4, 2, 1, D, OO, POS, 4, None, 0,
                                                       st) == pkg.CS_ERR_INVALID  # null total
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_best_mismatches_batch(pats[:3], 4)
    assert ei.value.status == pkg.CS_ERR_INVALID and "CS_MM_MAX" in str(ei.value)
    n1 = pkg.C.c_uint64()
    one_d = (pkg.C.c_uint8 * 1)(0xEE)
    assert pkg.lib().cs_fm_locate_best_mismatch(g._h, b"ACG", 3, 4, one_d, None, 0,
                                                pkg.C.byref(n1)) == pkg.CS_ERR_INVALID
    assert b"CS_MM_MAX" in pkg.lib().cs_fm_last_error()
    assert pkg.lib().cs_fm_locate_best_mismatch(g._h, b"ACG", 3, 1, None, None, 0,
                                                pkg.C.byref(n1)) == pkg.CS_ERR_INVALID  # null out_dist
    # non-monotone host offsets
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_best_mismatches_batch(buf=np.frombuffer(b"ACGT", np.uint8), offs=np.array([0, 3, 2], np.uint64),
                                       k=1)
    assert ei.value.status == pkg.CS_ERR_INVALID
    torch.cuda.synchronize()
    assert (d_d == 0xEE).all().item() and (d_pos == -1).all().item()  # the refused calls wrote nothing
    # a batch of empty patterns may pass d_pats = NULL: distance 0, no positions
    d_e = _dev(np.array([7, 7, 7, 7], np.int64), torch.int64)
    d_oo.fill_(-1)
    tot3, written = g.locate_best_mismatch_device(0, d_e.data_ptr(), 3, 2, d_d.data_ptr(), d_oo.data_ptr(), None, 0,
                                                  stream=st)
    torch.cuda.synchronize()
    assert tot3 == 0 and written and d_oo.cpu().tolist() == [0, 0, 0, 0] and d_d.cpu().tolist() == [0, 0, 0, 0xEE]


# ---- 9. LF overrun -----------------------------------------------------------------------------
def test_overrun_is_reported_and_the_handle_stays_usable():
    """A text without a unique terminator: the oracle's exact locate raises, and so does the
    position phase here (every walk stops after n steps).  The next call on the handle — a
    sizing call, which walks nothing — succeeds, as does an exact count."""
    pkg = load_pkg()
    text = b"abababab"
    ref = O.Index(text)
    with pytest.raises(RuntimeError, match="LF walk exceeded text length"):
        ref.locate(b"ab", limit=100)
    g = pkg.FMIndex.build_from_text(text)
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns([b"ab", b"bb"])
    d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
    d_d = torch.full((2,), 0xEE, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_pos = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_best_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), 2, 1, d_d.data_ptr(), d_oo.data_ptr(),
                                      d_pos.data_ptr(), 64, flags=pkg.Q_NO_FULL_SA | pkg.Q_NO_WALK_LINES, stream=st)
    assert ei.value.status == pkg.CS_ERR_LF_OVERRUN
    assert str(ei.value) == "locate: LF walk exceeded text length"
    tot, written = g.locate_best_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), 2, 1, d_d.data_ptr(),
                                                 d_oo.data_ptr(), None, 0, stream=st)
    torch.cuda.synchronize()
    # "ab" occurs at 4 rows; "bb" does not occur, its neighbours "ab" and "ba" hold 4 rows each
    assert (tot, written) == (12, False) and d_d.cpu().tolist() == [0, 1] and d_oo.cpu().tolist() == [0, 4, 12]
    pats = [b"ab", b"ba", b"aa", b"abab"]
    assert g.count_batch(pats).tolist() == [ref.count(p) for p in pats]


# ---- 10. two calls on one stream ---------------------------------------------------------------
def test_two_calls_queued_on_one_stream():
    """Two calls back to back on one stream with no synchronisation of the caller's between
    them, then a third over other patterns: a call's lists and plan are its own."""
    pkg = load_pkg()
    text, pats, table, pairs = mixed_locate_case()
    g = _build(text)
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for sub, k in ((pats, KMAX), (pats[::-1][:777], 2)):
        buf, offs = pkg.pack_patterns(sub)
        d_p, d_o = _dev(buf, torch.uint8), _dev(offs.astype(np.int64), torch.int64)
        cap = sum(len(p) for p in pairs)  # every pair within 3: more than any best stratum
        d_d = torch.full((len(sub),), 0xEE, dtype=torch.uint8, device="cuda")
        d_oo = torch.full((len(sub) + 1,), -1, dtype=torch.int64, device="cuda")
        d_pos = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
        tot, written = g.locate_best_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), len(sub), k, d_d.data_ptr(),
                                                     d_oo.data_ptr(), d_pos.data_ptr(), cap, stream=st)
        assert written
        outs.append((d_p, d_o, d_d, d_oo, d_pos, tot))
    torch.cuda.synchronize()
    for (_, _, d_d, d_oo, d_pos, tot), (tb, pr, k) in zip(
            outs, ((table, pairs, KMAX), (table[::-1][:777], pairs[::-1][:777], 2))):
        oo = d_oo.cpu().numpy()
        pos = d_pos.cpu().numpy()
        assert oo[-1] == tot and (pos[tot:] == -1).all()
        same_best_locate((d_d.cpu().numpy(), oo, split_positions(oo, pos[:tot])), best_pairs(tb, pr, k),
                         ("queued", k))
