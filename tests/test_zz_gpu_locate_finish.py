"""The finish of the one-call locate (fm_locate.hip: tile scan, emit, listed walks, wide ranges)
over more than one tile, against the two phases (locate_ranges_device + locate_walk_device):
totals equal, offsets equal, positions equal element by element.

A tile is a search block's 512 patterns (kLocTile); a pattern with at most 32 reported rows
(kLocSmall) is emitted by its lane (full suffix array) or listed for k_locate_walks (walk
lines: 512 slots per tile, the emit walks what does not fit), one with more goes to
k_locate_emit_wide, and a pattern's only position is stashed by the search kernel.  The text
is 4,095 DNA characters and '$' with a 12-mer motif planted 100 times, so a pattern inside the
motif has about 100 rows.  The batches mix the classes: a text 12-mer (nearly always one
occurrence), a 4-mer of the text (several), a piece of the motif (about 100), an absent
14-mer, the empty pattern (locate reports nothing for it) — in that order, so a batch of one
pattern is the text 12-mer alone.  The class counts each case relies on are asserted from the returned offsets.
Every batch runs again with room for total - 1 positions: the same total and offsets, and no
positions promised.
The file is named to collect after every suite that was here before it.
"""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg

pytestmark = pytest.mark.gpu

# kPos 0 (full suffix array), 1 (WalkLine), 2 (WalkLineW)
BUILDS = {
    "full_sa": {},
    "nosa": {"CS_FM_FULL_SA": "0"},
    "wide_nosa": {"CS_FM_WIDE": "1", "CS_FM_FULL_SA": "0"},
}
MOTIF = b"GATTACAGGCTA"
K_SMALL, TILE = 32, 512


def make_text():
    t = O.gen_dna(77, 4095).copy()  # 4,095 bases, then '$'
    at = np.random.default_rng(78).choice(np.arange(0, 4095 - len(MOTIF), len(MOTIF)), 100, replace=False)
    for a in at:
        t[a:a + len(MOTIF)] = np.frombuffer(MOTIF, np.uint8)
    return t.tobytes()


def make_classes(text):
    """(once, few, motif, absent) pattern lists: text 12-mers, text 4-mers, pieces of the
    motif, 14-mers that do not occur."""
    t = np.frombuffer(text, np.uint8)
    once = [bytes(p) for p in O.gen_patterns_text(t[:-1], 12, 400, seed=79)]
    few = [bytes(p) for p in O.gen_patterns_text(t[:-1], 4, 400, seed=80)]
    motif = [MOTIF[a:b] for a in range(4) for b in range(a + 6, len(MOTIF) + 1)]
    absent = [bytes(p) for p in O.gen_patterns_unif("dna", 14, 600, seed=81) if text.find(bytes(p)) < 0]
    return once, few, motif, absent


def mixed_batch(classes, npat):
    once, few, motif, absent = classes
    cyc = (once, few, motif, absent, [b""])
    return [cyc[q % 5][(q // 5) % len(cyc[q % 5])] for q in range(npat)]


_STATE = {}


def _setup(build):
    """(index, classes) per build; the text and the classes are made once."""
    if "text" not in _STATE:
        _STATE["text"] = make_text()
        _STATE["classes"] = make_classes(_STATE["text"])
    if build not in _STATE:
        pkg = load_pkg()
        with pkg.build_options(BUILDS[build]):
            _STATE[build] = pkg.FMIndex.build_from_text(_STATE["text"])
    return _STATE[build], _STATE["classes"]


def _takes_one_call(g, build):
    """launch_locate_onepass's route decision, from what the index reports."""
    inf = g.info()
    wide = "CS_FM_WIDE" in BUILDS[build]
    by_sa = inf.full_sa_bytes > 0 and not wide
    by_walk = inf.full_sa_bytes == 0 and inf.walk_bytes > 0 and inf.walk_marks == 2
    occ_fast = inf.engine == 1 and inf.prefix_k > 0 and inf.context_q > 0 and (by_sa or by_walk)
    return occ_fast or by_sa


def _compare(g, pats, limit):
    """One call == two phases; then the one call with room for total - 1 positions.
    Returns the per-pattern numbers of reported positions."""
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = O.pack_patterns(pats)
    npat = len(pats)
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros(8, np.uint8)])).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    sp = torch.empty(npat, dtype=torch.int64, device="cuda")
    oo2 = torch.empty(npat + 1, dtype=torch.int64, device="cuda")
    tot2 = g.locate_ranges_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, limit, sp.data_ptr(),
                                  oo2.data_ptr(), st)
    pos2 = torch.empty(max(tot2, 1), dtype=torch.int64, device="cuda")
    g.locate_walk_device(sp.data_ptr(), oo2.data_ptr(), npat, tot2, pos2.data_ptr(), st)
    guard = 64  # words after the capacity, which no kernel may write
    oo1 = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
    pos1 = torch.full((tot2 + guard,), -1, dtype=torch.int64, device="cuda")
    tot1, ok = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, limit, oo1.data_ptr(),
                               pos1.data_ptr(), tot2, st)
    torch.cuda.synchronize()
    assert tot1 == tot2 and ok  # (ok False: a total over the capacity, that is over tot2)
    assert torch.equal(oo1, oo2)
    assert torch.equal(pos1[:tot1], pos2[:tot2])
    assert bool((pos1[tot1:] == -1).all())
    if tot2:  # room for one position less: the total and the offsets, and no positions promised
        oo3 = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
        pos3 = torch.full((tot2 - 1 + guard,), -1, dtype=torch.int64, device="cuda")
        tot3, ok3 = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, limit, oo3.data_ptr(),
                                    pos3.data_ptr(), tot2 - 1, st)
        torch.cuda.synchronize()
        assert not ok3 and tot3 == tot2
        assert torch.equal(oo3, oo2)
        assert bool((pos3[tot2 - 1:] == -1).all())
    return np.diff(oo2.cpu().numpy())


def _finish_ran(g, classes):
    """Whether cs_fm_locate_device runs the one call on this index, seen from outside: the one
    call puts its records, counts and tiles into the caller's workspace, the two phases leave
    the workspace alone.  (info() does not report lf_exact or the sample arrays, so
    _takes_one_call alone could say yes where the library takes the two phases, and every
    comparison here would then be the two phases against themselves.)"""
    pats = mixed_batch(classes, 5)
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros(8, np.uint8)])).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    nb = g.workspace_bytes(len(pats))
    work = torch.zeros((nb + 7) // 8, dtype=torch.int64, device="cuda")  # (zero-filled, as the ABI asks)
    oo = torch.empty(len(pats) + 1, dtype=torch.int64, device="cuda")
    pos = torch.empty(8192, dtype=torch.int64, device="cuda")
    g.locate_device_ws(d_buf.data_ptr(), d_offs.data_ptr(), len(pats), 3, oo.data_ptr(), pos.data_ptr(),
                       pos.numel(), work.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bool((work != 0).any())  # (a found pattern's record is never 0)


def _index(build):
    g, classes = _setup(build)
    if not _takes_one_call(g, build):
        pytest.skip("a %s build of this text does not take the one call" % build)
    ran = _STATE.setdefault("ran", {})
    if build not in ran:
        ran[build] = _finish_ran(g, classes)
    assert ran[build], "the index should take the one call, and its workspace was not written"
    return g, classes


@pytest.mark.parametrize("limit", [0, 1, 2, 32, 33, 10**5])
@pytest.mark.parametrize("npat", [1, 511, 512, 513, 1537])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_finish_mixed(build, npat, limit):
    """Tile edges (511, 512, 513) and three tiles plus one pattern, each side of kLocSmall."""
    g, classes = _index(build)
    pats = mixed_batch(classes, npat)
    cnt = _compare(g, pats, limit)
    assert (cnt <= limit).all()
    if limit == 0 or npat == 1:
        assert cnt.sum() == min(limit, 1) * npat  # the text 12-mer alone occurs
        return
    k = np.arange(npat) % 5
    assert (cnt[k == 3] == 0).all() and (k == 3).any()          # absent
    assert (cnt[k == 4] == 0).all()                              # the empty pattern
    assert (cnt[k == 0] == 1).sum() >= 50                        # one position: the stash
    if limit >= 2:
        assert ((cnt[k == 1] >= 2) & (cnt[k == 1] <= K_SMALL)).sum() >= 50  # rows by the lane / listed
    if limit > K_SMALL:
        assert (cnt[k == 2] > K_SMALL).sum() >= 20               # the motif: k_locate_emit_wide
    else:
        assert (cnt[k == 2] == limit).sum() >= 20


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_finish_tile_overflow(build):
    """512 patterns that occur at least 3 times each, at limit 3: the first tile reports 1,536
    rows, more than its 512 walk slots, so on walk lines the emit walks the overflow itself;
    then an absent pattern, a text 12-mer and the empty pattern in the second tile."""
    g, (once, few, motif, absent) = _index(build)
    text = _STATE["text"]
    often = [p for p in dict.fromkeys(few + motif) if text.count(p) >= 3]
    assert len(often) >= 128
    pats = [often[q % len(often)] for q in range(TILE)] + [absent[0], once[0], b""]
    cnt = _compare(g, pats, 3)
    assert (cnt[:TILE] == 3).all() and cnt[:TILE].sum() > TILE
    assert cnt[TILE] == 0 and 1 <= cnt[TILE + 1] <= 3 and cnt[TILE + 2] == 0


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_finish_wide_ranges(build):
    """Pieces of the motif among the classes, unlimited: about 100 rows each, more than
    kLocSmall, so they are appended to the wide list and emitted a block per range."""
    g, classes = _index(build)
    motif = classes[2]
    base = mixed_batch(classes, 2 * TILE + 7)
    pats = [motif[q % len(motif)] if q % 3 == 0 else base[q] for q in range(len(base))]
    cnt = _compare(g, pats, 10**5)
    wide = cnt[::3]
    assert (wide > K_SMALL).all() and (wide >= 100).sum() >= len(wide) // 2
    assert (cnt == 0).any() and (cnt == 1).any()
