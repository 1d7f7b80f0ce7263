"""The seeded locate (include/cs_fmindex_approx_seeded.h) against the cyclic Hamming scan.

On the family texts of tests/helpers/mismatch_ref.py with their committed patterns (those a call
at bound k accepts: m = 0 or m > k), for k in {0, 1, 3, 4, 8}: the offsets and the per-pattern
sorted pairs equal the scan's, the candidate count equals the restatement's
(tests/helpers/seeded_ref.py, checked against the scan without a GPU in
tests/test_seeded_ref_cpu.py), the host batch gives the same, and at k <= 3 so does the
backtracking locate on the same handle.  The variants are index layouts the piece search and the
position phase differ on (the names and options are those of
tests/test_zz_gpu_mismatch_families.py); the verification reads only the byte text.

The verification kernel has one form (a lane per candidate: the form with eight lanes per
candidate lost at every length measured and was deleted), so no selector is needed
to reach it; every case also runs once through the measurement twin
(cs_fm_locate_mismatch_seeded_phases_device, include/cs_fmindex_diag.h).

n = 4,121 and 1,741; at most 2.1e5 candidates per call.  Named to collect after the suites that
were here before it.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library: the device calls of the helpers run on its stream)

from conftest import load_pkg
from helpers.mismatch_ref import CANARY, _check, _dev, device_pairs
from helpers.seeded_ref import (SEED_KS, kept, piece_mismatches, piece_starts, restated_case, scan_pairs,
                                seeded_case, seeded_device, seeded_host)

pytestmark = pytest.mark.gpu

VARIANTS = {
    "auto": {},
    "noprefix": {"CS_FM_PREFIX_K": "0"},
    "learned": {"CS_FM_ENGINE": "learned"},
    "qwm": {"CS_FM_ENGINE": "qwm"},
    "wavelet": {"CS_FM_ENGINE": "wavelet"},
    "wavelet_line64": {"CS_FM_ENGINE": "wavelet", "CS_FM_LINE_BYTES": "64", "CS_FM_DEVICE_TEXT": "0"},
    "auto_nosa": {"CS_FM_FULL_SA": "0"},
    "wide_ptab_esc": {"CS_FM_WIDE": "1", "CS_FM_PTAB_WMAX": "3"},
}
CASES = ([("fam_dna", v) for v in ("auto", "noprefix", "qwm", "wavelet", "learned", "auto_nosa", "wide_ptab_esc")] +
         [(t, "auto") for t in ("fam_dna_N", "fam_alpha12", "fam_bytes")] + [("fam_bytes", "wavelet")])


def _build(name, vname):
    pkg = load_pkg()
    with pkg.build_options(VARIANTS[vname]):
        return pkg.FMIndex.build_from_text(seeded_case(name)[0])


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def built(request):
    name, vname = request.param
    g = _build(name, vname)
    assert g.info().text_in_hbm == 1
    yield name, vname, g


@pytest.fixture(scope="module")
def auto_dna():
    return _build("fam_dna", "auto")


def _sub(pats, sel):
    return [pats[q] for q in sel]


# ---- 1. texts x variants x k ---------------------------------------------------------------
@pytest.mark.parametrize("k", SEED_KS)
def test_pairs(built, k):
    name, vname, g = built
    text, pats, dist = seeded_case(name)
    sel = kept(pats, k)
    sub = _sub(pats, sel)
    want = scan_pairs(dist, sel, k)
    C = restated_case(name, k)[1]
    for phases in (False, True):
        oo, got, cand = seeded_device(g, sub, k, phases=phases)
        _check(oo, got, want, (name, vname, k, "device", phases))
        assert cand == C, (name, vname, k, phases)
    oo, got = seeded_host(g, sub, k)
    _check(oo, got, want, (name, vname, k, "host"))
    if k <= 3:  # the backtracking locate on the same handle
        oo2, got2 = device_pairs(g, sub, k)
        _check(oo2, got2, want, (name, vname, k, "backtracking"))
        assert oo2.tolist() == np.asarray(oo).astype(np.int64).tolist()


# ---- 2. handles the call does not serve ------------------------------------------------------
def _refused(g, pats, k):
    pkg = load_pkg()
    buf, offs = pkg.pack_patterns(pats)
    d_p = _dev(buf, torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.full((len(pats) + 1,), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((CANARY,), -1, dtype=torch.int64, device="cuda")
    d_dist = torch.full((CANARY,), 0xFF, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatch_seeded_device(d_p.data_ptr(), d_o.data_ptr(), len(pats), k, d_oo.data_ptr(),
                                        d_pos.data_ptr(), d_dist.data_ptr(), CANARY,
                                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_oo.cpu().numpy() == -1).all() and (d_pos.cpu().numpy() == -1).all()
    assert (d_dist.cpu().numpy() == 0xFF).all(), "canary overwritten"
    return ei.value


def test_unsupported_without_device_text():
    pkg = load_pkg()
    g = _build("fam_dna", "wavelet_line64")
    assert g.info().text_in_hbm == 0
    text, pats, _ = seeded_case("fam_dna")
    e = _refused(g, _sub(pats, kept(pats, 3)), 3)
    assert e.status == pkg.CS_ERR_UNSUPPORTED and "text in HBM" in str(e)
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatches_seeded_batch([pats[10]], 1)
    assert ei.value.status == pkg.CS_ERR_UNSUPPORTED


def test_unsupported_without_unique_smallest_last_byte():
    pkg = load_pkg()
    g = pkg.FMIndex.build_from_text(b"abab")
    e = _refused(g, [b"ab", b"ba"], 1)
    assert e.status == pkg.CS_ERR_UNSUPPORTED and "smallest last symbol" in str(e)


# ---- 3. raw order ----------------------------------------------------------------------------
def test_raw_order_k0_is_the_exact_locate(auto_dna):
    g = auto_dna
    text, pats, _ = seeded_case("fam_dna")
    sub = _sub(pats, kept(pats, 0))
    oo, pos, dist, _ = seeded_device(g, sub, 0, raw=True)
    loffs, lpos = g.locate_batch(sub, limit=len(text) + 1)
    assert oo.tolist() == loffs.astype(np.int64).tolist() and len(lpos) > 0
    assert pos.tolist() == lpos.astype(np.int64).tolist() and not dist.any()


def test_raw_order_k3_follows_the_pieces(auto_dna):
    """Pieces ascending, each piece's exact-locate order kept, owned alignments only: the
    sequence built from the exact locate of the pieces."""
    g = auto_dna
    k = 3
    text, pats, _ = seeded_case("fam_dna")
    n = len(text)
    sub = _sub(pats, kept(pats, k))
    pieces, owner = [], []
    for q, p in enumerate(sub):
        a = piece_starts(len(p), k)
        for pp in range(k + 1):
            pieces.append(p[a[pp]:a[pp + 1]])
            owner.append((q, pp, a[pp]))
    loffs, lpos = g.locate_batch(pieces, limit=n + 1)
    lpos = lpos.astype(np.int64)
    want_pos, want_dist, want_offs = [], [], [0]
    for q, p in enumerate(sub):
        for pp in range(k + 1):
            j = q * (k + 1) + pp
            x = lpos[int(loffs[j]):int(loffs[j + 1])]
            if len(p) and len(x):
                s = (x - owner[j][2]) % n
                mm = piece_mismatches(text, p, k, s)
                keep = ~(mm[:, :pp] == 0).any(axis=1) & (mm.sum(axis=1) <= k)
                want_pos += s[keep].tolist()
                want_dist += mm.sum(axis=1)[keep].tolist()
        want_offs.append(len(want_pos))
    oo, pos, dist, cand = seeded_device(g, sub, k, raw=True)
    assert cand == int(loffs[-1]) and len(want_pos) > 100
    assert oo.tolist() == want_offs
    assert pos.tolist() == want_pos and dist.tolist() == want_dist
    # the order is not the sorted one: the check above holds more than the pair sets
    assert any(pos[int(oo[q]):int(oo[q + 1])].tolist() != sorted(pos[int(oo[q]):int(oo[q + 1])].tolist())
               for q in range(len(sub)))


# ---- 4. fixed_m, misaligned buffers, flags ---------------------------------------------------
@pytest.mark.parametrize("m", [33, 130])
def test_fixed_m(auto_dna, m):
    g = auto_dna
    text, pats, dist = seeded_case("fam_dna")
    sel = [q for q, p in enumerate(pats) if len(p) == m]
    assert len(sel) >= 7
    for k in (4, 8):
        oo, got, _ = seeded_device(g, _sub(pats, sel), k, fixed_m=m)
        _check(oo, got, scan_pairs(dist, sel, k), ("fixed_m", m, k))


@pytest.mark.parametrize("pad", [1, 3, 7, 13])
def test_misaligned_pattern_buffer(auto_dna, pad):
    g = auto_dna
    k = 4
    text, pats, dist = seeded_case("fam_dna")
    sel = kept(pats, k)
    want = scan_pairs(dist, sel, k)
    oo, got, cand = seeded_device(g, _sub(pats, sel), k, pad=pad)
    _check(oo, got, want, ("pad", pad))
    assert cand == restated_case("fam_dna", k)[1]


def test_flags(auto_dna):
    pkg = load_pkg()
    g = auto_dna
    k = 4
    text, pats, dist = seeded_case("fam_dna")
    sel = kept(pats, k)
    want = scan_pairs(dist, sel, k)
    for f in (pkg.Q_NO_PREFIX | pkg.Q_NO_CONTEXTS, pkg.Q_NO_FULL_SA):
        oo, got, cand = seeded_device(g, _sub(pats, sel), k, flags=f)
        _check(oo, got, want, ("flags", f))
        assert cand == restated_case("fam_dna", k)[1]


# ---- 5. errors -------------------------------------------------------------------------------
def test_short_patterns_are_invalid(auto_dna):
    pkg = load_pkg()
    g = auto_dna
    text, pats, _ = seeded_case("fam_dna")
    assert len(pats[0]) == 1 and len(pats[1]) == 3
    e = _refused(g, pats, 3)  # the full list holds a 1-mer and a 3-mer
    assert e.status == pkg.CS_ERR_INVALID and "pattern 0 " in str(e)
    e = _refused(g, pats[1:], 3)
    assert e.status == pkg.CS_ERR_INVALID and "pattern 0 " in str(e)
    e = _refused(g, pats[2:4] + pats[1:2] + pats[4:], 3)
    assert e.status == pkg.CS_ERR_INVALID and "pattern 2 " in str(e)
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatches_seeded_batch(pats, 3)
    assert ei.value.status == pkg.CS_ERR_INVALID and "pattern 0 " in str(ei.value)


def test_fixed_m_not_longer_than_k_and_k_past_the_bound(auto_dna):
    pkg = load_pkg()
    g = auto_dna
    d_p = _dev(np.frombuffer(b"ACGACG" + b"A" * 40, np.uint8), torch.uint8)
    d_oo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    for k, fixed_m in ((3, 3), (16, 20)):
        with pytest.raises(pkg.FMIndexError) as ei:
            g.locate_mismatch_seeded_device(d_p.data_ptr(), None, 2, k, d_oo.data_ptr(), None, None, 0,
                                            fixed_m=fixed_m)
        assert ei.value.status == pkg.CS_ERR_INVALID
        assert (d_oo.cpu().numpy() == -1).all()
    with pytest.raises(pkg.FMIndexError) as ei:
        g.locate_mismatches_seeded(b"A" * 40, 16)
    assert ei.value.status == pkg.CS_ERR_INVALID


def test_capacity_one_short(auto_dna):
    pkg = load_pkg()
    g = auto_dna
    k = 4
    text, pats, dist = seeded_case("fam_dna")
    sel = kept(pats, k)
    want = scan_pairs(dist, sel, k)
    total = sum(len(w) for w in want)
    buf, offs = pkg.pack_patterns(_sub(pats, sel))
    d_p = _dev(buf, torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    d_oo = torch.full((len(sel) + 1,), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    d_dist = torch.full((total,), 0xFF, dtype=torch.uint8, device="cuda")
    tot, cand, written = g.locate_mismatch_seeded_device(d_p.data_ptr(), d_o.data_ptr(), len(sel), k,
                                                         d_oo.data_ptr(), d_pos.data_ptr(), d_dist.data_ptr(),
                                                         total - 1)
    torch.cuda.synchronize()
    assert not written and tot == total and cand == restated_case("fam_dna", k)[1]
    assert d_oo.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert (d_pos.cpu().numpy() == -1).all() and (d_dist.cpu().numpy() == 0xFF).all()


def test_empty_batches(auto_dna):
    g = auto_dna
    oo, pos, dist = g.locate_mismatches_seeded_batch([], 2)
    assert oo.tolist() == [0] and len(pos) == 0
    oo, got, cand = seeded_device(g, [b"", b""], 5)
    assert oo.tolist() == [0, 0, 0] and cand == 0
    oo, got, cand = seeded_device(g, [b"#" * 30], 5)  # a byte absent from the text: no candidate
    assert oo.tolist() == [0, 0] and cand == 0
