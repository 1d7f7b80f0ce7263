"""GPU parity: the HIP engine (through the C ABI) against the genuine reference's
golden vectors and the CPU restatement (oracle/), bit for bit.

Layers checked separately, bottom-up:
  suffix array      (device prefix doubling)    vs src/core/sais.hpp:8-16 order
  level rank1       (32/64-B rank lines)           vs BitVector::rank1, every position
  wavelet rank      (node-table descent, or one occurrence-line read)
                                                 vs WaveletTree::rank, every (c, i)
  access / LF       (fused descent)              vs BWT / FMIndex::LF, every row
  count / locate    (batched kernels)            vs golden vectors and the oracle
"""
import os

import numpy as np
import pytest
import torch  # before the engine's library loads: one HIP runtime in the process

import oracle as O
from conftest import fm_golden_cases, golden_text, load_golden, load_pkg

pytestmark = pytest.mark.gpu


ENGINE_VARIANTS = {
    # name: environment of the builder (test hooks in csrc/fm_build.hip / fm_query.hip)
    # default: occurrence lines when <= 4 symbols hold all but 128 BWT rows, else
    # the wavelet matrix in 32-B lines (Line32)
    "auto": {},
    "auto_noprefix": {"CS_FM_PREFIX_K": "0"},       # prefix table off
    "auto_rowmarks": {"CS_FM_WALK_MARKS": "row", "CS_FM_FULL_SA": "0"},  # walks over row-marked walk lines
    # locate walks the occurrence lines; extract by LF inversion (no text in HBM)
    "auto_nowalk": {"CS_FM_WALK": "0", "CS_FM_FULL_SA": "0", "CS_FM_DEVICE_TEXT": "0"},
    "auto_nolctx": {"CS_FM_LCTX": "0"},             # count steps to the end (no left contexts)
    "auto_rec": {"CS_FM_CTX_RECORDS": "1"},         # context records at any table depth
    # compact 16-B context records at any table depth; one pattern per lane in the
    # staged count and locate kernels
    "auto_rec16": {"CS_FM_CTX_RECORDS": "16", "CS_FM_COUNT_U": "1", "CS_FM_LOCATE_U": "1"},
    "auto_nosa": {"CS_FM_FULL_SA": "0"},            # locate walks (no full suffix array kept)
    # (round 6: auto_nosa_rows, auto_bar and auto_pstride_ssa — CS_QT_WALK_ROWS, CS_QT_BARRIER
    # and PSTRIDE=32, no default path — are in test_selectors_without_a_variant)
    "qwm": {"CS_FM_ENGINE": "qwm"},                 # quaternary wavelet matrix for every text
    "qwm_unstaged": {"CS_FM_ENGINE": "qwm", "CS_FM_QCTX_STAGED": "0"},  # its count one pattern per lane
    "learned": {"CS_FM_ENGINE": "learned"},         # learned occurrence lines where occurrence lines apply
    "learned_sb4": {"CS_FM_ENGINE": "learned", "CS_FM_LEARNED_SHIFT": "2"},  # 4-line superblocks
    "wavelet": {"CS_FM_ENGINE": "wavelet"},         # binary wavelet matrix for every text
    "wavelet_line64": {"CS_FM_ENGINE": "wavelet", "CS_FM_LINE_BYTES": "64",  # 64-B rank lines,
                       "CS_FM_DEVICE_TEXT": "0"},                             # LF-inversion extract
    # the n >= 2^32 engines at small n: u64 samples/table, bucketed sorter, and
    # occurrence lines or 32-B wide rank lines (Line32W)
    "wide_bucketed": {"CS_FM_WIDE": "1", "CS_FM_SA_BUILDER": "bucketed", "CS_FM_DEVICE_TEXT": "0"},
    "wide_wavelet": {"CS_FM_WIDE": "1", "CS_FM_ENGINE": "wavelet"},
    # packed wide prefix-table entries with every range of 3+ rows escaped (C[] start)
    "wide_ptab_esc": {"CS_FM_WIDE": "1", "CS_FM_PTAB_WMAX": "3"},
    # compact context records of a wide index (sp bits 32-41 in the record; C5), and with
    # escaped table ranges
    "wide_rec16": {"CS_FM_WIDE": "1", "CS_FM_CTX_RECORDS": "16"},
    "wide_rec16_esc": {"CS_FM_WIDE": "1", "CS_FM_CTX_RECORDS": "16", "CS_FM_PTAB_WMAX": "3"},
}

# Test-hook layouts and selector variants that no default path builds (round 6, VERDICT r05
# item 6: the suite's time): they run the whole matrix on HOOK_TEXTS — the terminator and
# cyclic cases, a run-heavy and an all-one-symbol text, DNA with rare rows, bytes, a line
# edge, a 64-symbol alphabet and a skewed histogram — instead of all 31 texts.
HOOK_VARIANTS = {"learned_sb4", "wide_ptab_esc", "wide_rec16_esc", "wavelet_line64", "qwm_unstaged"}
HOOK_TEXTS = {"banana", "abab_noterm", "all_same", "dna_5k", "bytes_5k", "runs", "rare_N_41",
              "rare_runs", "line_edge_448", "straddle_649", "alpha_64", "skewed_55"}


@pytest.fixture(autouse=True)
def _hook_subset(request):
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    if params.get("pkg") in HOOK_VARIANTS and params.get("name") in TEXTS and params["name"] not in HOOK_TEXTS:
        pytest.skip("test-hook variant: HOOK_TEXTS only")


@pytest.fixture(scope="module", params=sorted(ENGINE_VARIANTS))
def pkg(request):
    """Every test runs on each engine variant (see ENGINE_VARIANTS): the variant's build
    options for every handle the module constructs (cs_fm_set_build_options, round 6 — no
    test reads or writes the environment to choose an engine)."""
    m = load_pkg()
    with m.build_options(ENGINE_VARIANTS[request.param]):
        yield m


def _bar_count(g, buf, offs):
    """The staged count kernel's general search behind the block barrier (CS_QT_BARRIER, a
    per-call tuning selector; the default reads the node table through the caches, no
    barrier, since round 4).  The learned variants re-count under it (the learned lines'
    instantiation); test_selectors_without_a_variant covers the rest."""
    return _count_bo(g, buf, offs, flags=load_pkg().QT_BARRIER)


def _opt(name, default=None):
    """The current build options' value of a CS_FM_* name (ENGINE_VARIANTS, _env)."""
    cur = load_pkg().current_build_options() or {}
    v = cur.get(name)
    return default if v is None else str(v)


class _env:
    """Build options (cs_fmindex_tuning.h, the CS_FM_* names) for the handles constructed
    inside, over the variant's: a thread scope (cs_fm_set_build_options), not the process
    environment.  Per-call kernel choices are the CS_QT_* flags bits (pkg.QT_*)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        m = load_pkg()
        self.scope = m.build_options(dict(m.current_build_options() or {}, **self.kw))
        self.scope.__enter__()

    def __exit__(self, *a):
        self.scope.__exit__(*a)


def _learned():
    return _opt("CS_FM_ENGINE") == "learned"


def _wide():
    return _opt("CS_FM_WIDE") == "1"


def _texts():
    rng = np.random.default_rng(11)
    out = {
        "banana": b"banana$",
        "single": b"x",
        "two_same": b"aa",
        "abab_noterm": b"abab",
        "all_same": b"z" * 3000,
        "dna_5k": O.gen_dna(42, 4999).tobytes(),
        "bytes_5k": O.gen_bytes(42, 4999).tobytes(),
        "raw_bytes_3k": rng.integers(0, 256, 3000).astype(np.uint8).tobytes(),
        "binary_ab": bytes(rng.choice(list(b"ab"), 4000).astype(np.uint8)) + b"$",
        "runs": (b"ab" * 700) + (b"a" * 500) + b"$",
        "line_edge_448": bytes(rng.choice(list(b"ACGT"), 447).astype(np.uint8)) + b"$",
        "line_edge_896": bytes(rng.choice(list(b"ACGT"), 896).astype(np.uint8)),
        "line_edge_224": bytes(rng.choice(list(b"ACGT"), 223).astype(np.uint8)) + b"$",
        "line_edge_672": bytes(rng.choice(list(b"ACG"), 672).astype(np.uint8)),
        # 32-B lines hold 224 bits = 3.5 ballot groups: n in the last half group
        "straddle_201": bytes(rng.choice(list(b"ab"), 200).astype(np.uint8)) + b"$",
        "straddle_649": bytes(rng.choice(list(b"ACGT"), 648).astype(np.uint8)) + b"$",
        # occurrence lines hold 64 rows: n around line edges
        "occ_edge_63": bytes(rng.choice(list(b"ACGT"), 62).astype(np.uint8)) + b"$",
        "occ_edge_64": bytes(rng.choice(list(b"ACGT"), 63).astype(np.uint8)) + b"$",
        "occ_edge_65": bytes(rng.choice(list(b"ACGT"), 64).astype(np.uint8)) + b"$",
        "occ_edge_128": bytes(rng.choice(list(b"ACGT"), 128).astype(np.uint8)),
        # rare symbols (stored as code 0 and listed in the node table)
        "rare_N_41": _sprinkle(rng, 3000, b"N" * 40) + b"$",
        "rare_128": _sprinkle(rng, 5000, b"N" * 127) + b"$",        # the table's capacity
        "rare_129": _sprinkle(rng, 5000, b"N" * 128) + b"$",        # one more: wavelet matrix
        "rare_both_ends": _sprinkle(rng, 2000, b"!!~~~\x00\xff") + b"$",  # below and above ACGT
        "rare_runs": b"ACGT" * 200 + b"N" * 60 + b"TTGCA" * 100 + b"$",
    }
    # quaternary-matrix level boundaries (k symbols + the terminator): 6 / 16 symbols ->
    # 2 levels, 17 / 64 -> 3, 65 / 201 -> 4
    for k in (5, 15, 16, 63, 64, 200):
        alpha = np.arange(40, 40 + k, dtype=np.uint8)
        out["alpha_%d" % k] = bytes(rng.choice(alpha, 3000).astype(np.uint8)) + b"\x01"
    # skewed histogram: one dominant symbol, many rare ones (pure nodes at every level)
    sk = np.where(rng.random(4000) < 0.97, 65, rng.integers(66, 120, 4000)).astype(np.uint8)
    out["skewed_55"] = bytes(sk) + b"$"
    return out


def _sprinkle(rng, n, rare):
    """n random ACGT bytes with the `rare` bytes written at distinct random places."""
    t = rng.choice(list(b"ACGT"), n).astype(np.uint8)
    at = rng.choice(n, len(rare), replace=False)
    t[at] = np.frombuffer(rare, np.uint8)
    return t.tobytes()


TEXTS = _texts()


@pytest.fixture(scope="module")
def built(pkg):
    cache = {}

    def get(name, stride=32):
        key = (name, stride)
        if key not in cache:
            t = TEXTS[name]
            cache[key] = (pkg.FMIndex.build_from_text(t, pkg.BuildParams(ssa_stride=stride)),
                          O.Index(t, ssa_stride=stride))
        return cache[key]
    return get


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_suffix_array(pkg, name):
    t = TEXTS[name]
    ref = O.sa_naive(t) if len(t) <= 4096 else O.sa_doubling(t)
    assert pkg.sa_build(t).astype(np.uint64).tolist() == ref.tolist()


def test_suffix_array_random_sweep(pkg):
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 1500))
        alpha = [b"ab", b"ACGT$", bytes(range(256)), b"a", b"\x00\x01"][trial % 5]
        t = bytes(rng.choice(list(alpha), size=n).astype(np.uint8))
        assert pkg.sa_build(t).astype(np.uint64).tolist() == O.sa_naive(t).tolist(), t[:50]


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_level_rank1_every_position(built, pkg, name):
    g, o = built(name)
    n = len(TEXTS[name])
    if g.info().engine != 0:  # occurrence lines / quaternary matrix: no binary levels
        with pytest.raises(pkg.FMIndexError):
            g.level_rank1(0, np.arange(4, dtype=np.uint64))
        return
    pos = np.arange(n + 3, dtype=np.uint64)  # includes i >= size (count_ones path)
    for l in range(8):
        lv = o.level(l)
        want = np.array([lv.rank1(int(i)) for i in pos], np.uint64)
        assert g.level_rank1(l, pos).tolist() == want.tolist(), (name, l)


def test_engine_choice(built):
    """Occurrence lines iff <= 4 symbols hold all but at most 128 BWT rows, else the
    quaternary matrix (unless an engine is forced); rare rows are listed in the node
    table; both get walk lines for locate."""
    forced = _opt("CS_FM_ENGINE")
    # (engine, rare rows, LF one cycle: the text ends in a unique smallest symbol, so the
    # walk lines mark sampled text positions (2) instead of the reference's rows (1))
    want = {"dna_5k": (1, 1, True), "banana": (1, 0, True), "single": (1, 0, True),
            "rare_N_41": (1, 41, True), "rare_128": (1, 128, True), "rare_129": (2, 0, True),
            "bytes_5k": (2, 0, True), "rare_both_ends": (1, 8, False),
            "abab_noterm": (1, 0, False)}
    levels = {"rare_129": 2, "bytes_5k": 4, "dna_5k": 2, "banana": 1, "single": 1,
              "rare_N_41": 2, "rare_128": 2, "rare_both_ends": 2, "abab_noterm": 1}
    for name, (engine, rare, cyc) in want.items():
        info = built(name)[0].info()
        if forced == "wavelet":
            engine, rare = 0, 0
        elif forced == "qwm":
            engine, rare = 2, 0
        elif forced == "learned" and engine == 1:
            engine = 3
        marks = 0 if engine == 0 else (2 if cyc else 1)
        full_sa = (cyc and _opt("CS_FM_FULL_SA") != "0"
                   and _opt("CS_FM_SA_BUILDER") != "bucketed")
        if _opt("CS_FM_WALK") == "0":
            marks = 0
        elif _opt("CS_FM_WALK_MARKS") == "row" and marks:
            marks = 1
        elif full_sa:  # locate reads the full suffix array: no walk lines
            marks = 0
        assert (info.engine, info.rare_rows, info.walk_marks) == (engine, rare, marks), name
        want_levels = {0: 8, 1: 1, 2: levels[name], 3: 1}[engine]
        assert info.levels == want_levels and info.line_bytes in (32, 64), name
        # left contexts: occurrence lines 7 x 2-bit codes in u16 (16 rows per 32-B
        # sector), quaternary matrix 32 / (2 x levels) dense codes in u32 (8 rows)
        ctx, R = {1: (7, 16), 3: (7, 16), 2: (min(16, 32 // (2 * info.levels)), 8)}.get(engine, (0, 1))
        if _opt("CS_FM_LCTX") == "0":
            ctx = 0
        assert info.context_q == ctx, name
        wide = _opt("CS_FM_WIDE") == "1"
        assert info.full_sa_bytes == (4 * info.n if full_sa else 0), name
        assert info.position_stride == (int(_opt("CS_FM_PSTRIDE", "0")) or 4), name
        assert info.context_bytes == (((info.n + R - 1) // R + 1) * 32 if ctx else 0), name
        # context records: narrow occurrence-line indexes with contexts and a table of
        # 14+ characters (none of these texts) or forced; 16 B when forced compact
        rec = {"1": 32, "16": 16}.get(_opt("CS_FM_CTX_RECORDS", ""), 0)
        if wide and rec:  # wide indexes: compact records only
            rec = 16
        if not (ctx and engine in (1, 3) and info.prefix_k):
            rec = 0
        # quaternary matrix: 16-B records (u32 contexts of 2 rows) when the table's
        # ranges average at most 2 rows
        if (engine == 2 and ctx and not wide and info.prefix_k and _opt("CS_FM_CTX_RECORDS") != "0"
                and info.n <= 2 * info.prefix_sigma ** info.prefix_k):
            rec = 16
        assert info.record_bytes == rec, name
        assert info.text_in_hbm == (_opt("CS_FM_DEVICE_TEXT") != "0"), name
        # the 2-bit text of long-pattern verification: occurrence lines (not learned), narrow,
        # LF one n-cycle, with the full suffix array and the text in HBM — or (round 6) without
        # the full SA, over walk lines with text-position marks (C5's layout: its long
        # patterns are verified at their walks' positions), from the build's text
        ptext = engine == 1 and ((full_sa and info.text_in_hbm and not wide) or (not full_sa and marks == 2))
        assert info.packed_text_bytes == ((info.n + 31) // 32 * 8 if ptext else 0), name
        assert info.prefix_bytes == (max(rec, 8) * info.prefix_sigma ** info.prefix_k if info.prefix_k else 0), name


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_wavelet_rank_access_lf(built, name):
    g, o = built(name)
    t = TEXTS[name]
    n = len(t)
    syms = sorted(set(t)) + [0, 255, ord("q")]
    pos = np.arange(0, n + 2, max(1, n // 300), dtype=np.uint64)
    for c in syms:
        want = [o.wt_rank(c, int(i)) for i in pos]
        got = g.wt_rank(np.full(len(pos), c, np.uint8), pos)
        assert got.tolist() == want, (name, c)
    rows = np.arange(n, dtype=np.uint64)
    assert g.wt_access(rows).tobytes() == o.bwt().tobytes()
    assert g.lf(rows).tolist() == [o.lf(int(i)) for i in rows]
    assert g.C().tolist() == o.C().tolist()
    assert g.ssa().tolist() == o.ssa().tolist()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_count_every_text_vs_oracle(built, name):
    """count() of substrings and one-symbol mutants of every test text: ranges of
    every width around the left contexts' 32-B sectors (one or two, or too wide),
    chains through rare rows (escaped contexts), patterns the text lacks."""
    g, o = built(name)
    t = TEXTS[name]
    n = len(t)
    rng = np.random.default_rng(n)
    pats = []
    for m in (1, 2, 3, 5, 6, 7, 8, 9, 12, 20):
        for i in rng.integers(0, max(1, n - m + 1), 40):
            p = bytearray(t[i:i + m])
            pats.append(bytes(p))
            if p:
                p[rng.integers(0, len(p))] = t[rng.integers(0, n)]
                pats.append(bytes(p))
    want = [o.count(p) for p in pats]
    assert g.count_batch(pats).tolist() == want, name
    # every general search listed for the list kernel (a wave lists them from 2 by default)
    assert _count_ex(g, pats, flags=load_pkg().QT_GENERAL_LIST_ALL)[0].tolist() == want, name
    if _learned():
        assert _bar_count(g, *O.pack_patterns(pats)).tolist() == want, name
    for p in pats[::37]:  # single-pattern path (kernel arguments)
        assert g.count(p) == o.count(p), (name, p)
    # locate of the same patterns: ranges finished over the contexts hand windows of
    # matching rows to the walk (lf_exact texts), limits cutting inside a window
    for lim in (3, 1000):
        for p in pats[::3]:
            try:
                want = o.locate(p, limit=lim)
            except RuntimeError as e:
                with pytest.raises(RuntimeError, match=str(e)):
                    g.locate(p, limit=lim)
                continue
            assert g.locate(p, limit=lim) == want, (name, p, lim)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_count_fixed_length(built, name):
    """cs_fm_count_device with d_offs = NULL — patterns of one length m back to back, no offsets
    array — equals the oracle's count for substrings and mutants, and n for m = 0."""
    g, o = built(name)
    t = TEXTS[name]
    n = len(t)
    rng = np.random.default_rng(n + 1)
    for m in (1, 3, 7, 13, 20, 33):
        if m > n:
            continue
        pats = []
        for i in rng.integers(0, n - m + 1, 50):
            p = bytearray(t[i:i + m])
            pats.append(bytes(p))
            p[rng.integers(0, m)] = t[rng.integers(0, n)]
            pats.append(bytes(p))
        buf = torch.tensor(list(b"".join(pats)), dtype=torch.uint8, device="cuda")
        out = torch.empty(len(pats), dtype=torch.int64, device="cuda")
        g.count_fixed_device(buf.data_ptr(), m, len(pats), out.data_ptr())
        torch.cuda.synchronize()
        assert out.tolist() == [o.count(p) for p in pats], (name, m)
    out = torch.empty(3, dtype=torch.int64, device="cuda")
    g.count_fixed_device(out.data_ptr(), 0, 3, out.data_ptr())  # fm_index.cpp:80
    torch.cuda.synchronize()
    assert out.tolist() == [n] * 3


def test_locate_context_windows(pkg):
    """Locate over context windows (phase-1 records): patterns with up to 40 hits in
    one window (repeats: the window's match span exceeds the record's 22 bits and the
    search steps on), and hits separated by non-matching rows."""
    rng = np.random.default_rng(8)
    rnd = lambda k: bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
    core = rnd(14)
    parts = []
    for i in range(40):  # 40 copies of core, each after a different 6-mer
        parts += [rnd(30), rnd(6), core]
    t = b"".join(parts) + rnd(200) + b"$"
    g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    pats = [core, core[1:], core[:10], core[3:]] + [t[i:i + 20] for i in range(0, len(t) - 20, 13)]
    pats += [t[i:i + 17] for i in range(0, len(t) - 17, 29)]
    for lim in (1, 5, 21, 22, 23, 100000):
        offs, pos = g.locate_batch(pats, limit=lim)
        for q, p in enumerate(pats):
            assert pos[offs[q]:offs[q + 1]].tolist() == o.locate(p, limit=lim), (p, lim)


def _check_fm_case(pkg, case):
    text = golden_text(case["text"])
    g = pkg.FMIndex.build_from_text(text, pkg.BuildParams(ssa_stride=case["ssa_stride"]))
    pats = [bytes.fromhex(h) for h in case["patterns_hex"]]
    assert g.count_batch(pats).tolist() == case["count"], case["name"]
    # single-pattern facade = batch of 1
    for k in range(0, len(pats), max(1, len(pats) // 7)):
        assert g.count(pats[k]) == case["count"][k]
    ok = [q for q, loc in enumerate(case["locate"]) if "pos" in loc]
    bad = [q for q, loc in enumerate(case["locate"]) if "error" in loc]
    if ok:
        offs, pos = g.locate_batch([pats[q] for q in ok], limit=case["limit"])
        for i, q in enumerate(ok):
            assert pos[offs[i]:offs[i + 1]].tolist() == case["locate"][q]["pos"], (case["name"], pats[q])
    for q in bad:
        with pytest.raises(RuntimeError) as ei:
            g.locate(pats[q], limit=case["limit"])
        if case["locate"][q]["error"] != "exception":
            assert str(ei.value) == case["locate"][q]["error"]
    for ex in case.get("extract", []):
        assert g.extract(ex["pos"], ex["len"]).hex() == ex["hex"]


@pytest.mark.parametrize("case", fm_golden_cases("fm_kat.json", "fm_100k.json", "fm_1m.json"))
def test_fm_golden(pkg, case):
    _check_fm_case(pkg, case)


def test_bad_offsets_rejected(pkg):
    g = pkg.FMIndex.build_from_text(b"banana$")
    buf = np.frombuffer(b"anaban", np.uint8)
    with pytest.raises(pkg.FMIndexError, match="non-decreasing"):
        g.count_batch(buf=buf, offs=np.array([0, 3, 1, 6], np.uint64))
    with pytest.raises(pkg.FMIndexError, match="non-decreasing"):
        g.locate_batch(buf=buf, offs=np.array([0, 4, 2], np.uint64))


def test_batch_edge_cases(pkg):
    t = O.gen_dna(7, 20000).tobytes()
    g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    rng = np.random.default_rng(1)
    pats = [b"", b"A", b"$", b"N", b"AN", b"ACGTN" * 3, t[100:1100], t[-30:], t[:40],
            b"\x00", b"\xff" * 5]
    pats += [t[i:i + m] for i, m in zip(rng.integers(0, 19000, 200), rng.integers(1, 40, 200))]
    assert g.count_batch(pats).tolist() == [o.count(p) for p in pats]
    offs, pos = g.locate_batch(pats, limit=50)
    for q, p in enumerate(pats):
        assert pos[offs[q]:offs[q + 1]].tolist() == o.locate(p, limit=50), p[:20]
    # batch of zero patterns, empty pattern alone
    assert g.count_batch([]).tolist() == []
    assert g.count(b"") == len(t)
    assert g.locate(b"") == []
    # each host path: single pattern in the kernel arguments (<= 128 B), through the
    # pinned arena (longer, or small batches), and staged through HBM (> 1 MiB)
    for p in (t[5:133], t[5:134], t[100:1100]):
        assert g.count(p) == o.count(p)
    big = [t[i:i + 30] for i in rng.integers(0, 19900, 40000)]  # 1.2 MB of patterns
    assert g.count_batch(big).tolist() == [o.count(p) for p in big]


_LARGE = {}  # (gen, m) -> the text, its batch and the oracle's answers (the same for every variant)


def _large_case(gen, m):
    if (gen, m) not in _LARGE:
        n = 2_000_000
        t = (O.gen_dna(42, n) if gen == "dna" else O.gen_bytes(42, n))
        o = O.Index(t.tobytes())
        q_text = O.gen_patterns_text(t, m, 20000, seed=4242)
        alpha = b"ACGT" if gen == "dna" else bytes(range(1, 256))
        q_unif = O.gen_patterns_uniform(alpha, m, 5000, seed=4243)
        short = O.gen_patterns_text(t, 3, 300, seed=1)
        pats = [bytes(p) for p in q_text] + [bytes(p) for p in q_unif] + [bytes(p) for p in short]
        buf, offs = O.pack_patterns(pats)
        want = o.count_batch(buf=buf, offs=offs, nthreads=8)
        woffs, wpos = o.locate_batch(buf=buf, offs=offs, limit=1000, nthreads=8)
        _LARGE[(gen, m)] = (t.tobytes(), buf, offs, want, woffs, wpos)
    return _LARGE[(gen, m)]


@pytest.mark.parametrize("gen,m", [("dna", 20), ("bytes", 8)])
def test_random_large_vs_oracle(pkg, gen, m):
    t, buf, offs, want, woffs, wpos = _large_case(gen, m)
    g = pkg.FMIndex.build_from_text(t)
    got = g.count_batch(buf=buf, offs=offs)
    assert np.array_equal(got, want)
    assert (got[:20000] >= 1).all()
    if _learned():
        assert np.array_equal(_bar_count(g, buf, offs), want)
    goffs, gpos = g.locate_batch(buf=buf, offs=offs, limit=1000)
    assert np.array_equal(goffs, woffs)
    assert np.array_equal(gpos, wpos)


def test_count_long_kernel_large(pkg):
    """The long-pattern kernel (k_count_long, CS_Q_LONG) at scale: a 2 M DNA text with rare
    symbols (N runs, so windows and contexts meet rare rows), 12 k Q_text patterns of 33-200
    characters plus one-symbol mutants and patterns holding an N — counts equal the
    oracle's through the packed text (default), the byte text (CS_QT_LONG_BYTE_TEXT) and
    round 2's kernel (0), and every pattern of a random length batch agrees."""
    rng = np.random.default_rng(21)
    t = O.gen_dna(7, 2_000_000)
    for at in rng.integers(0, len(t) - 40, 30):  # 30 runs of 1-3 N (<= 128 rare rows)
        t[at:at + int(rng.integers(1, 4))] = ord("N")
    t = t.tobytes()
    g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    pats = []
    for m in rng.integers(33, 201, 6000):
        i = int(rng.integers(0, len(t) - m))
        p = bytearray(t[i:i + m])
        pats.append(bytes(p))
        p[int(rng.integers(0, m))] = b"ACGTN"[int(rng.integers(0, 5))]
        pats.append(bytes(p))
    buf, offs = O.pack_patterns(pats)
    want = o.count_batch(buf=buf, offs=offs, nthreads=8)
    assert (want[::2] >= 1).all()
    # k_count_long on the packed text (default), the byte text, round 2's kernel; 8-B
    # pattern / window loads instead of the 16-B vectors
    for f in (0, pkg.QT_LONG_BYTE_TEXT, pkg.QT_LONG_ROUND2, pkg.QT_LONG_LOADS8):
        got, _, _ = _count_ex(g, pats, flags=32 | f)
        assert np.array_equal(got, want), f
    for _ in range(2):  # the default path: long-pattern routing inside the call
        got, _, _ = _count_ex(g, pats)
        assert np.array_equal(got, want)
    # locate in one call: k_locate_long (CS_Q_LONG), then the default path's routing (indexes
    # with the 2-bit text)
    if g.info().packed_text_bytes:
        woffs, wpos = o.locate_batch(buf=buf, offs=offs, limit=100, nthreads=8)
        want_l = [wpos[woffs[q]:woffs[q + 1]].tolist() for q in range(len(pats))]
        for f in (32, 0, 0):
            assert _locate_one(g, pats, 100, f) == want_l, f


@pytest.mark.parametrize("stride", [1, 3, 8, 33, 64])
def test_ssa_strides_vs_oracle(pkg, stride):
    t = O.gen_dna(3, 50000).tobytes()
    g = pkg.FMIndex.build_from_text(t, pkg.BuildParams(ssa_stride=stride))
    o = O.Index(t, ssa_stride=stride)
    pats = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(t, np.uint8), 6, 400, seed=stride)]
    offs, pos = g.locate_batch(pats, limit=100)
    for q, p in enumerate(pats):
        assert pos[offs[q]:offs[q + 1]].tolist() == o.locate(p, limit=100)


def test_prefix_table_sweep(pkg):
    """Prefix tables of every depth give the same counts (k forced 2..8)."""
    t = O.gen_dna(9, 30000).tobytes()
    o = O.Index(t)
    rng = np.random.default_rng(2)
    pats = [t[i:i + m] for i, m in zip(rng.integers(0, 29000, 400), rng.integers(1, 25, 400))]
    pats += [bytes(rng.choice(list(b"ACGT$"), int(m)).astype(np.uint8)) for m in rng.integers(1, 12, 100)]
    want = [o.count(p) for p in pats]
    for k in range(2, 9):
        with _env(CS_FM_PREFIX_K=str(k)):
            g = pkg.FMIndex.build_from_text(t)
        assert g.info().prefix_k == k
        assert g.count_batch(pats).tolist() == want, k


def test_lf_overrun_message(pkg):
    """Cyclic-BWT quirk without a terminator: the walk never meets a sampled row
    (fm_index.cpp:136-138) — same exception text as the reference."""
    case = [c for c in load_golden("fm_kat.json")["cases"] if c["name"] == "no_terminator_abab"][0]
    g = pkg.FMIndex.build_from_text(b"abab")
    for h, loc in zip(case["patterns_hex"], case["locate"]):
        with pytest.raises(RuntimeError) as ei:
            g.locate(bytes.fromhex(h))
        assert str(ei.value) == loc["error"]
    # the engine stays usable after the error
    assert g.count(b"ab") == 2


def test_save_open_directory_roundtrip(pkg, tmp_path):
    """On-disk format (the reference's open_directory TODO): the reopened index
    answers identically; an index without its text extracts on the device."""
    t = O.gen_dna(21, 40000).tobytes()
    g = pkg.FMIndex.build_from_text(t)
    d = str(tmp_path / "idx")
    g.save_directory(d)
    h = pkg.FMIndex.open_directory(d)
    assert h.n == len(t)
    assert (h.info().context_q, h.info().context_bytes) == (g.info().context_q, g.info().context_bytes)
    rng = np.random.default_rng(4)
    pats = [t[i:i + m] for i, m in zip(rng.integers(0, 39000, 300), rng.integers(1, 30, 300))]
    assert h.count_batch(pats).tolist() == g.count_batch(pats).tolist()
    a = g.locate_batch(pats, limit=20)
    b = h.locate_batch(pats, limit=20)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert h.extract(100, 50) == t[100:150]
    assert h.extract_batch([100, len(t) - 5], [50, 10]) == [t[100:150], t[-5:]]
    if g.info().text_in_hbm:
        # the text travels as the device part dtext.bin (no host text.bin beside it)
        assert h.info().text_in_hbm == 1 and not os.path.exists(os.path.join(d, "text.bin"))
        part, key = "dtext.bin", "has_dtext"
    else:  # CS_FM_DEVICE_TEXT=0: the host text_ copy is saved as text.bin
        assert h.info().text_in_hbm == 0 and os.path.exists(os.path.join(d, "text.bin"))
        part, key = "text.bin", "has_text"
    os.remove(os.path.join(d, part))
    meta = open(os.path.join(d, "cs_fmindex.meta")).read().replace(key + " 1", key + " 0")
    open(os.path.join(d, "cs_fmindex.meta"), "w").write(meta)
    k = pkg.FMIndex.open_directory(d)
    assert k.info().text_in_hbm == 0
    assert k.extract(100, 50) == t[100:150]  # device LF inversion
    assert k.extract(len(t) - 5, 10) == t[-5:]


@pytest.mark.parametrize("dtext", ["1", "0"])
def test_device_extract(pkg, dtext):
    """Batched extract == text slices (fm_index.cpp:163-167 clamping), for every start
    position of a small text: copied from the text in HBM, or (CS_FM_DEVICE_TEXT=0) by
    LF inversion from inverse-SA samples."""
    for stride in (1, 5, 32):
        t = O.gen_dna(stride, 3000).tobytes()
        with _env(CS_FM_DEVICE_TEXT=dtext):
            g = pkg.FMIndex.build_from_text(t, pkg.BuildParams(ssa_stride=stride))
        assert g.info().text_in_hbm == int(dtext)
        pos = list(range(0, len(t) + 3))
        lens = [(p * 7) % 45 for p in pos]
        got = g.extract_batch(pos, lens)
        assert got == [t[p:p + l] for p, l in zip(pos, lens)]
    g = pkg.FMIndex.build_from_text(b"abab")  # no unique smallest terminator:
    assert g.extract_batch([0, 3], [2, 5]) == [b"ab", b"b"]  # the host text copy, as text_
    assert g.extract(0, 2) == b"ab"


def test_bucketed_multi_pass(pkg):
    """The bucketed sorter split into many passes (small pass budget) emits the same
    BWT / SSA / counts / positions as the oracle."""
    base = O.gen_dna(32, 30000).tobytes()[:-1]
    seg = base[1000:1500]  # 500-char repeat copied 6 times: ~24 refinement rounds
    rep = b"".join(base[i * 5000:(i + 1) * 5000] + seg for i in range(6)) + b"$"
    for t, budget in ((O.gen_dna(31, 60000).tobytes(), 4000),
                      (O.gen_bytes(31, 50000).tobytes(), 4000),
                      (rep, 4000)):
        with _env(CS_FM_SA_BUILDER="bucketed", CS_FM_PASS_MAX=str(budget)):
            g = pkg.FMIndex.build_from_text(t)
        o = O.Index(t)
        rows = np.arange(len(t), dtype=np.uint64)
        assert g.wt_access(rows).tobytes() == o.bwt().tobytes()
        assert g.ssa().tolist() == o.ssa().tolist()
        pats = [t[i:i + 12] for i in range(0, len(t) - 12, 997)]
        assert g.count_batch(pats).tolist() == [o.count(p) for p in pats]
        offs, pos = g.locate_batch(pats, limit=50)
        for q, p in enumerate(pats):
            assert pos[offs[q]:offs[q + 1]].tolist() == o.locate(p, limit=50)


def test_bucketed_long_repeats(pkg):
    """Exact repeats far longer than one key chunk (20 000-char copies, a 12 000-char
    run of one symbol, a period-3 stretch): the bucketed sorter refines only the
    still-tied suffixes, round after round, and emits the oracle's BWT / SSA."""
    base = O.gen_dna(33, 60000).tobytes()[:-1]
    seg = base[:20000]
    texts = [
        base[20000:25000] + seg + base[25000:30000] + seg + base[30000:31000] + seg + b"$",
        base[:3000] + b"A" * 12000 + base[3000:6000] + b"$",
        base[:2000] + b"ACG" * 5000 + base[2000:4000] + b"ACG" * 4000 + b"$",
    ]
    for t in texts:
        with _env(CS_FM_SA_BUILDER="bucketed"):
            g = pkg.FMIndex.build_from_text(t)
        o = O.Index(t)
        rows = np.arange(len(t), dtype=np.uint64)
        assert g.wt_access(rows).tobytes() == o.bwt().tobytes()
        assert g.ssa().tolist() == o.ssa().tolist()
        pats = [t[i:i + 30] for i in range(0, len(t) - 30, 1999)]
        assert g.count_batch(pats).tolist() == [o.count(p) for p in pats]


@pytest.mark.parametrize("name", ["banana", "dna_5k", "bytes_5k", "abab_noterm", "rare_N_41",
                                  "alpha_16", "runs"])
def test_create_from_arrays(pkg, name):
    """cs_fm_create: the index from the reference's own members (bwt_, ssa_), no suffix
    sort on the device; same counts / positions as the oracle, extract from the text
    when given, CS_ERR_UNSUPPORTED without it."""
    t = TEXTS[name]
    o = O.Index(t, ssa_stride=16)
    g = pkg.FMIndex.create(o.bwt().tobytes(), o.ssa(), 16)
    gt = pkg.FMIndex.create(o.bwt().tobytes(), o.ssa(), 16, text=t)
    rng = np.random.default_rng(len(t))
    pats = [t[i:i + k] for i, k in zip(rng.integers(0, max(1, len(t) - 8), 300),
                                       rng.integers(1, 9, 300))]
    pats += [b"", b"\xfe\xfd", t[:3]]
    want = [o.count(p) for p in pats]
    assert g.count_batch(pats).tolist() == want
    assert [g.count(p) for p in pats[:20]] == want[:20]
    for p in pats[:60]:
        try:
            w = o.locate(p, limit=50)
        except RuntimeError as e:
            with pytest.raises(RuntimeError) as ei:
                g.locate(p, limit=50)
            assert str(ei.value) == str(e)
            continue
        assert g.locate(p, limit=50) == w
    assert gt.extract(1, 7) == t[1:8]
    assert gt.info().text_in_hbm == (_opt("CS_FM_DEVICE_TEXT") != "0")
    assert g.info().text_in_hbm == 0
    assert gt.extract_batch([1, 0, len(t) - 2], [7, 3, 9]) == [t[1:8], t[0:3], t[-2:]]
    with pytest.raises(RuntimeError):
        g.extract(1, 7)


# ---- query forms: flags (CS_Q_*), count widths, packed DNA ----------------------

FLAG_SETS = {"none": 0, "no_prefix": 1, "no_contexts": 2, "loop": 3, "no_verify": 16}


def _substrings_and_mutants(t, lengths, per, seed):
    rng = np.random.default_rng(seed)
    n = len(t)
    pats = []
    for m in lengths:
        for i in rng.integers(0, max(1, n - m + 1), per):
            p = bytearray(t[i:i + m])
            pats.append(bytes(p))
            if p:
                p[rng.integers(0, len(p))] = t[rng.integers(0, n)]
                pats.append(bytes(p))
    return pats


def _count_bo(g, buf, offs, flags=0):
    """count of a packed batch (buf, offs) through cs_fm_count_device under flags."""
    d_buf = torch.from_numpy(np.ascontiguousarray(buf).copy()).cuda()
    d_offs = torch.from_numpy(np.asarray(offs).astype(np.int64)).cuda()
    npat = len(offs) - 1
    out = torch.zeros(max(npat, 1), dtype=torch.int64, device="cuda")
    g.count_device_ex(d_buf.data_ptr(), d_offs.data_ptr(), npat, out.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    return out[:npat].cpu().numpy().astype(np.uint64)


def _count_ex(g, pats, width=8, flags=0, exc_cap=1 << 16):
    """count through cs_fm_count_device under `flags` -> (counts as uint64, exception pairs)."""
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    npat = len(pats)
    dt = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[width]
    out = torch.zeros(max(npat, 1), dtype=dt, device="cuda")
    exc = torch.zeros(2 * max(exc_cap, 1), dtype=torch.int64, device="cuda")
    exc_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    g.count_device_ex(d_buf.data_ptr(), d_offs.data_ptr(), npat, out.data_ptr(), width=width,
                      flags=flags, d_exc=exc.data_ptr(), exc_cap=exc_cap, d_exc_n=exc_n.data_ptr())
    torch.cuda.synchronize()
    got = out[:npat].cpu().numpy().astype(np.uint64)
    pairs = exc[: 2 * min(int(exc_n.item()), exc_cap)].view(-1, 2).cpu().numpy()
    return got, pairs, int(exc_n.item())


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_query_flags_count(built, pkg, name):
    """The same counts with the prefix table, the left contexts / context records, or
    both left out (CS_Q_NO_PREFIX / CS_Q_NO_CONTEXTS): the plain backward-search loop of
    fm_index.cpp:84-98 on the same index, and its algorithmic bytes only grow."""
    g, o = built(name)
    t = TEXTS[name]
    pats = _substrings_and_mutants(t, (1, 2, 5, 7, 9, 14, 20, 33), 25, len(t) + 7)
    want = [o.count(p) for p in pats]
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    nb = {}
    for fname, f in FLAG_SETS.items():
        got, _, _ = _count_ex(g, pats, flags=f)
        assert got.tolist() == want, (name, fname)
        qb = torch.zeros(len(pats), dtype=torch.int64, device="cuda")
        g.count_bytes_device(d_buf.data_ptr(), d_offs.data_ptr(), len(pats), qb.data_ptr(), flags=f)
        torch.cuda.synchronize()
        nb[fname] = int(qb.sum().item())
    # the table replaces rank steps; it can cost at most its entry per pattern more, when
    # the steps it replaces were served from the node table (rare symbols) or were cheaper
    # than a 16-B record (skewed texts with compact records)
    eb = max(g.info().record_bytes, 8)
    assert nb["loop"] + eb * len(pats) >= nb["no_contexts"] or g.info().prefix_k == 0, nb
    if g.info().context_q == 0:  # no contexts: CS_Q_NO_CONTEXTS leaves out only the verification
        assert nb["no_contexts"] == nb["no_verify"], nb


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_count_verify_long(built, pkg, name):
    """Long patterns, with and without the verification of narrow ranges against the
    text (CS_Q_NO_VERIFY; fm_query.hip verify_count): substrings and mutants up to 500
    characters, cyclic substrings across the end of the text (through the terminator) and
    periodic patterns longer than the text — the oracle's counts (fm_index.cpp:84-100)."""
    g, o = built(name)
    t = TEXTS[name]
    n = len(t)
    rng = np.random.default_rng(n + 17)
    pats = _substrings_and_mutants(t, (12, 18, 24, 40, 64, 130, 500), 6, n + 11)
    tt = t * 3
    for _ in range(12):  # rotations' prefixes that wrap: the tail, then the head
        a = int(rng.integers(1, min(n, 40) + 1))
        b = int(rng.integers(0, min(n, 40) + 1))
        pats.append(t[n - a:] + t[:b])
    for m in (n - 1, n, n + 1, 2 * n + 3):
        if m > 0:
            i = int(rng.integers(0, n))
            pats.append(tt[i:i + m])
    pats = [p for p in pats if p]
    want = [o.count(p) for p in pats]
    for f in (0, 16, 32, 48):  # 32: CS_Q_LONG (k_count_long: one pattern per lane)
        got, _, _ = _count_ex(g, pats, flags=f)
        assert got.tolist() == want, (name, f)
    # CS_Q_LONG through round 2's kernel, on the byte text, with 8-B pattern and window loads
    for f in (pkg.QT_LONG_ROUND2, pkg.QT_LONG_BYTE_TEXT, pkg.QT_LONG_LOADS8):
        got, _, _ = _count_ex(g, pats, flags=32 | f)
        assert got.tolist() == want, (name, f)
    # long-pattern routing of the default path (inside the call since round 4): the staged
    # kernel counts the short patterns and lists the rest for k_count_long; short-only and
    # mixed batches alternate
    short = [p for p in pats if len(p) <= 32]
    for _ in range(2):
        got, _, _ = _count_ex(g, pats)
        assert got.tolist() == want, name
        got, _, _ = _count_ex(g, short)
        assert got.tolist() == [w for p, w in zip(pats, want) if len(p) <= 32], name
    # round 5: every batch routes (no size threshold); unrouted (CS_QT_NO_ROUTE: the staged
    # kernel's general search takes the long patterns), routed with the general searches kept
    # in the lane (CS_QT_GENERAL_INLANE), and the host batch
    for f in (pkg.QT_NO_ROUTE, pkg.QT_GENERAL_INLANE, pkg.QT_GENERAL_LIST_ALL):
        got, _, _ = _count_ex(g, pats, flags=f)
        assert got.tolist() == want, (name, f)
    assert g.count_batch(pats).tolist() == want, (name, "host batch")
    # CS_Q_LONG at the narrow widths: uint32, and uint8 with the exception pairs
    got4, _, _ = _count_ex(g, pats, width=4, flags=32)
    assert got4.tolist() == want, name
    got1, pairs, ne = _count_ex(g, pats, width=1, flags=32)
    assert ne == sum(1 for c in want if c >= 255), name
    got1[pairs[:, 0].astype(np.int64)] = pairs[:, 1].astype(np.uint64)
    assert got1.tolist() == want, name
    # host batches (cs_fm_count_batch): all longer than 96 characters -> the long-pattern
    # kernel unasked; with one short pattern among them -> the staged kernel
    lp = [i for i, p in enumerate(pats) if len(p) > 96]
    if lp:
        assert g.count_batch([pats[i] for i in lp]).tolist() == [want[i] for i in lp], name
        assert g.count_batch([pats[i] for i in lp] + [b"A"]).tolist()[:-1] == [want[i] for i in lp], name
    # fixed-length batches (cs_fm_count_device with fixed_m, no offsets array): 33 and 64 through
    # the staged kernel's general search, 130 through the long-pattern kernel (m > 96)
    for m in (33, 64, 130):
        if n < m:
            continue
        fx = _substrings_and_mutants(t, (m,), 20, n + m)
        fx = [p for p in fx if len(p) == m]
        d = torch.from_numpy(np.frombuffer(b"".join(fx), np.uint8).copy()).cuda()
        out = torch.zeros(len(fx), dtype=torch.int64, device="cuda")
        g.count_fixed_device(d.data_ptr(), m, len(fx), out.data_ptr())
        torch.cuda.synchronize()
        assert out.cpu().numpy().astype(np.uint64).tolist() == [o.count(p) for p in fx], (name, m)
    # single patterns (k_count_one: the pattern in the kernel arguments, up to 128 bytes)
    one = [i for i, p in enumerate(pats) if len(p) <= 128][::3]
    assert [g.count(pats[i]) for i in one] == [want[i] for i in one], name


def _locate_two_phase(g, pats, lim, flags):
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    npat = len(pats)
    d_sp = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    tot = g.locate_ranges_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim, d_sp.data_ptr(),
                                 d_oo.data_ptr(), flags=flags)
    d_pos = torch.zeros(max(tot, 1), dtype=torch.int64, device="cuda")
    g.locate_walk_device(d_sp.data_ptr(), d_oo.data_ptr(), npat, tot, d_pos.data_ptr(), flags=flags)
    oo = d_oo.cpu().numpy()
    pos = d_pos[:tot].cpu().numpy()
    return [pos[oo[q]:oo[q + 1]].tolist() for q in range(npat)]


def _locate_one(g, pats, lim, flags=0):
    """cs_fm_locate_device under `flags`: per pattern its positions (a first call for the total)."""
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    npat = len(pats)
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    tot, ok = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim, d_oo.data_ptr(), 0, 0,
                              flags=flags)
    d_pos = torch.zeros(max(tot, 1), dtype=torch.int64, device="cuda")
    if tot:
        tot2, ok = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim, d_oo.data_ptr(),
                                   d_pos.data_ptr(), tot, flags=flags)
        assert ok and tot2 == tot
    oo = d_oo.cpu().numpy()
    assert oo[-1] == tot
    pos = d_pos[:tot].cpu().numpy()
    return [pos[oo[q]:oo[q + 1]].tolist() for q in range(npat)]


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_locate_verify_long(built, pkg, name):
    """locate of long patterns: with the full suffix array and the text in HBM a narrow
    range finishes by verification (fm_query.hip locate_search: a verified-window record,
    positions SA[r] - k), without it (CS_Q_NO_VERIFY, CS_Q_NO_FULL_SA) by rank steps — in
    one call and in two phases, at limits that cut the windows: the oracle's positions in
    row order (fm_index.cpp:107-157), or its overrun error."""
    g, o = built(name)
    t = TEXTS[name]
    n = len(t)
    rng = np.random.default_rng(n + 29)
    pats = _substrings_and_mutants(t, (10, 16, 24, 40, 64, 130, 300), 5, n + 13)
    tt = t * 3
    for _ in range(8):  # windows through the end of the text
        a = int(rng.integers(1, min(n, 40) + 1))
        b = int(rng.integers(0, min(n, 40) + 1))
        pats.append(t[n - a:] + t[:b])
    for m in (n - 1, n + 1):
        if m > 0:
            i = int(rng.integers(0, n))
            pats.append(tt[i:i + m])
    pats = [p for p in pats if p]
    for lim in (1, 2, 100000):
        try:
            want = [o.locate(p, limit=lim) for p in pats]
        except RuntimeError:
            want = None  # the reference's overrun (no unique terminator)
        for f in (0, 16, 4):
            try:
                got = _locate_two_phase(g, pats, lim, f)
            except RuntimeError as e:
                assert want is None and str(e) == "locate: LF walk exceeded text length", (name, lim, f)
                continue
            assert want is not None, (name, lim, f)
            for q, p in enumerate(pats):
                assert got[q] == want[q], (name, lim, f, p)
        if want is None:
            continue
        offs, pos = g.locate_batch(pats, limit=lim)
        for q, p in enumerate(pats):
            assert pos[offs[q]:offs[q + 1]].tolist() == want[q], (name, lim, p)
        # the one call: CS_Q_LONG (k_locate_long for every pattern, then k_locate_list), the
        # default path twice (the staged kernel lists the long patterns for k_locate_long in
        # the same call), 8-B loads (CS_QT_LONG_LOADS8) — on the indexes that take
        # the long-pattern kernels (the 2-bit text; the others' one call is checked above)
        if not g.info().packed_text_bytes:
            if lim == 100000:  # CS_Q_LONG where the long-pattern kernels do not apply: the usual call
                assert _locate_one(g, pats, lim, 32) == want, (name, lim, "Q_LONG")
            continue
        for f in (32, 0, 0):
            assert _locate_one(g, pats, lim, f) == want, (name, lim, f)
        assert _locate_one(g, pats, lim, 32 | pkg.QT_LONG_LOADS8) == want, (name, lim, "loads8")
        short = [i for i, p in enumerate(pats) if len(p) < 32]  # nothing to list
        assert _locate_one(g, [pats[i] for i in short], lim) == [want[i] for i in short], (name, lim)
        lp = [i for i, p in enumerate(pats) if len(p) > 31]  # host batch: CS_Q_LONG unasked
        if lp:
            offs, pos = g.locate_batch([pats[i] for i in lp], limit=lim)
            for j, i in enumerate(lp):
                assert pos[offs[j]:offs[j + 1]].tolist() == want[i], (name, lim, pats[i])


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_query_flags_locate(built, pkg, name):
    """locate with phase 2 forced onto the LF walk (CS_Q_NO_FULL_SA) and onto the
    reference's row-sampled SSA walk over the rank structure (CS_Q_NO_WALK_LINES,
    fm_index.cpp:125-153), with and without the prefix table / contexts in phase 1: the
    oracle's positions in row order, or its overrun error."""
    g, o = built(name)
    t = TEXTS[name]
    pats = _substrings_and_mutants(t, (1, 3, 6, 9, 20), 12, len(t) + 3)
    lim = 40
    for f in (4, 4 | 8, 1 | 2 | 4 | 8, 2 | 8):
        buf, offs = O.pack_patterns(pats)
        d_buf = torch.from_numpy(buf.copy()).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        npat = len(pats)
        d_sp = torch.zeros(npat, dtype=torch.int64, device="cuda")
        d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
        tot = g.locate_ranges_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim, d_sp.data_ptr(),
                                     d_oo.data_ptr(), flags=f)
        d_pos = torch.zeros(max(tot, 1), dtype=torch.int64, device="cuda")
        try:
            g.locate_walk_device(d_sp.data_ptr(), d_oo.data_ptr(), npat, tot, d_pos.data_ptr(),
                                 flags=f)
        except RuntimeError as e:
            assert str(e) == "locate: LF walk exceeded text length"
            with pytest.raises(RuntimeError, match="LF walk exceeded"):
                for p in pats:
                    o.locate(p, limit=lim)
            continue
        oo = d_oo.cpu().numpy()
        pos = d_pos[:tot].cpu().numpy()
        for q, p in enumerate(pats):
            assert pos[oo[q]:oo[q + 1]].tolist() == o.locate(p, limit=lim), (name, f, p)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_locate_one_call(built, pkg, name):
    """cs_fm_locate_device (one launch over full-SA indexes: search, look-back scan,
    positions; the two phases otherwise): the oracle's positions in row order for every
    pattern, at limits that cut context windows and wide ranges; with a capacity one short
    of the total it reports the total and leaves the offsets right."""
    g, o = built(name)
    t = TEXTS[name]
    pats = _substrings_and_mutants(t, (1, 2, 4, 7, 12, 20), 20, len(t) + 5) + [b""]
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    npat = len(pats)
    for lim in (1, 3, 40, 100000):
        want = []
        try:
            want = [o.locate(p, limit=lim) for p in pats]
        except RuntimeError:
            want = None  # the reference's overrun (no unique terminator)
        d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
        tot_w = sum(len(w) for w in want) if want is not None else npat * min(lim, len(t))
        d_pos = torch.zeros(max(tot_w, 1), dtype=torch.int64, device="cuda")
        try:
            tot, ok = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim, d_oo.data_ptr(),
                                      d_pos.data_ptr(), d_pos.numel())
        except RuntimeError as e:
            assert want is None and str(e) == "locate: LF walk exceeded text length", (name, lim, e)
            continue
        assert want is not None and ok, (name, lim)
        oo = d_oo.cpu().numpy()
        assert tot == oo[-1] == tot_w, (name, lim)
        pos = d_pos[:tot].cpu().numpy()
        for q, p in enumerate(pats):
            assert pos[oo[q]:oo[q + 1]].tolist() == want[q], (name, lim, p)
        if lim == 40:  # cs_fm_locate_device under CS_Q_NO_PREFIX | CS_Q_NO_CONTEXTS: the two phases
            assert _locate_one(g, pats, lim, 3) == want, (name, lim)
        if tot:
            d_oo2 = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
            tot2, ok2 = g.locate_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, lim,
                                        d_oo2.data_ptr(), d_pos.data_ptr(), tot - 1)
            assert tot2 == tot and not ok2 and torch.equal(d_oo2, d_oo), (name, lim)


def test_locate_records(pkg):
    """The one-call locate through the locate records (fm_device.hpp kLocRec*: the SA values
    of each k-mer's (64 B) or (k+1)-mer's (16 B) rows beside their contexts, round 4) against
    the oracle's positions in
    row order and against the same call without them (CS_Q_NO_LOC_RECORDS): a DNA text with
    40-base pieces copied 2-7 times (so (k+1)-mers have 0..7+ rows) and a few N, every pattern
    length from k-1 to k+7 (text substrings, one-character mutants, uniform), limits 1, 2 and
    100000; also with the records' misses deferred to k_locate_list (CS_FM_LOC_DEFER=1), routed
    and not.  Built with 16-B and with 32-B context records (CS_FM_CTX_RECORDS=16 / 1, their
    precondition); the variants without the records' other preconditions skip."""
    rng = np.random.default_rng(5)
    t = bytearray(O.gen_dna(77, 199_999)[:-1].tobytes())
    for c in range(400):
        a = int(rng.integers(0, len(t) - 40))
        piece = bytes(t[a:a + 40])
        for _ in range(1 + c % 7):
            b = int(rng.integers(0, len(t) - 40))
            t[b:b + 40] = piece
    for i in rng.integers(0, len(t), 12):
        t[int(i)] = ord("N")
    t = bytes(t) + b"$"
    o = O.Index(t)
    built_any = False
    # compact 16-B context records (C4), 32-B ones (C2); 64-B k-mer locate records read by
    # four lanes (the default) and the 16-B (k+1)-mer ones (CS_FM_LOC_REC64=0)
    for rec, w64 in (("16", "1"), ("1", "1"), ("16", "0"), ("1", "0")):
        with _env(CS_FM_CTX_RECORDS=rec, CS_FM_LOC_REC64=w64):
            g = pkg.FMIndex.build_from_text(t, pkg.BuildParams())
        info = g.info()
        if not info.locate_record_bytes:
            continue
        built_any = True
        assert info.record_bytes == (16 if rec == "16" else 32)
        assert info.locate_record_bytes == 16 * 4 ** (info.prefix_k + 1)  # 64 * 4^k as well
        assert info.locate_record_width == (64 if w64 == "1" else 16)
        K = info.prefix_k
        pats = []
        for m in range(max(1, K - 1), K + 8):
            pats += _substrings_and_mutants(t, (m,), 150, m)
            pats += [bytes(p) for p in O.gen_patterns_uniform(b"ACGT", m, 20, seed=m)]
        for lim in (1, 2, 100000):
            want = [o.locate(p, limit=lim) for p in pats]
            assert _locate_one(g, pats, lim) == want, (rec, lim)
            assert _locate_one(g, pats, lim, pkg.Q_NO_LOC_RECORDS) == want, (rec, lim)
            # the misses deferred to the list kernel (CS_QT_LOC_DEFER), with and without routing
            assert _locate_one(g, pats, lim, pkg.QT_LOC_DEFER) == want, (rec, lim, "defer")
            assert _locate_one(g, pats, lim, pkg.QT_LOC_DEFER | pkg.QT_NO_ROUTE) == want, \
                (rec, lim, "defer, unrouted")
        del g
    if not built_any:
        pytest.skip("this variant builds no locate records")


@pytest.mark.parametrize("name", ["dna_5k", "bytes_5k", "all_same", "runs", "rare_N_41", "banana"])
def test_count_widths(built, pkg, name):
    """uint32 counts equal the uint64 ones; uint8 counts saturate at 255 with every
    larger count listed exactly once as (pattern, count); pairs past the capacity are
    counted but not stored."""
    g, o = built(name)
    t = TEXTS[name]
    pats = _substrings_and_mutants(t, (1, 2, 3, 8, 20), 30, 9) + [b""]
    want = np.array([o.count(p) for p in pats], np.uint64)
    for f in (0, 3):
        got4, _, _ = _count_ex(g, pats, width=4, flags=f)
        assert np.array_equal(got4, want), (name, f)
        got1, pairs, nexc = _count_ex(g, pats, width=1, flags=f)
        big = np.nonzero(want >= 255)[0]
        assert nexc == len(big)
        assert np.array_equal(got1, np.minimum(want, 255))
        assert sorted(pairs[:, 0].tolist()) == big.tolist()
        assert all(want[q] == c for q, c in pairs.tolist())
        if len(big) > 2:
            _, pairs2, nexc2 = _count_ex(g, pats, width=1, flags=f, exc_cap=2)
            assert nexc2 == len(big) and len(pairs2) == 2
            assert all(want[q] == c for q, c in pairs2.tolist())


@pytest.mark.parametrize("name", ["dna_5k", "banana", "rare_N_41", "rare_both_ends", "line_edge_896",
                                  "occ_edge_65", "bytes_5k", "abab_noterm"])
def test_count_packed(built, pkg, name):
    """2-bit packed DNA patterns (cs_fm_count_packed_device) count as the byte strings
    they spell, at every length 0..32, under every flag set and width."""
    g, o = built(name)
    t = TEXTS[name]
    rng = np.random.default_rng(3)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for m in (0, 1, 4, 7, 12, 15, 16, 19, 20, 21, 27, 32):
        pats = []
        # substrings of the text mapped onto ACGT (exact hits on DNA texts) and random ones
        for i in (rng.integers(0, len(t) - m + 1, 30) if len(t) >= m else []):
            s = np.frombuffer(t[i:i + m], np.uint8)
            pats.append(acgt[s % 4].tobytes() if not set(s.tolist()) <= set(b"ACGT") else s.tobytes())
        pats += [acgt[rng.integers(0, 4, m)].tobytes() for _ in range(20)]
        want = np.array([o.count(p) for p in pats], np.uint64)
        packed = torch.from_numpy(pkg.pack_dna(pats).view(np.int64)).cuda()
        for f in (0, 1, 2, 3):
            for width in (8, 4):
                dt = torch.int64 if width == 8 else torch.int32
                out = torch.zeros(len(pats), dtype=dt, device="cuda")
                g.count_packed_device(packed.data_ptr(), m, len(pats), out.data_ptr(), width=width,
                                      flags=f)
                torch.cuda.synchronize()
                assert out.cpu().numpy().astype(np.uint64).tolist() == want.tolist(), (name, m, f, width)


def test_repetitive_text_vs_oracle(pkg):
    """Heavy-tailed ranges (genomic repeats): 500 copies of a 4000-base seed with ~1 %
    substitutions — 20-mers occur hundreds of times, so searches leave the context
    records and the left contexts and step through wide ranges, and locate walks many
    rows per pattern; counts and positions (limit 50 and 5000) equal the oracle's."""
    rng = np.random.default_rng(12)
    seed = rng.choice(list(b"ACGT"), 4000).astype(np.uint8)
    t = np.tile(seed, 500)
    mut = rng.random(len(t)) < 0.01
    t[mut] = rng.choice(list(b"ACGT"), int(mut.sum())).astype(np.uint8)
    t = t.tobytes() + b"$"
    g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    P = O.gen_patterns_text(np.frombuffer(t, np.uint8), 20, 3000, seed=4)
    pats = [bytes(p) for p in P] + [bytes(p) for p in O.gen_patterns_text(np.frombuffer(t, np.uint8), 9, 500, seed=5)]
    buf, offs = O.pack_patterns(pats)
    want = o.count_batch(buf=buf, offs=offs, nthreads=8)
    assert np.median(want[:3000]) > 100
    assert np.array_equal(g.count_batch(buf=buf, offs=offs), want)
    if _learned():  # most searches here take the general path the hook changes
        assert np.array_equal(_bar_count(g, buf, offs), want)
    # the routed default lists the general searches for the list kernel; in the lane
    # (CS_QT_GENERAL_INLANE) and unrouted (CS_QT_NO_ROUTE) the same counts
    for f in (pkg.QT_GENERAL_INLANE, pkg.QT_GENERAL_LIST_ALL, pkg.QT_NO_ROUTE):
        assert np.array_equal(_count_bo(g, buf, offs, flags=f), want), f
    for lim in (50, 5000):
        sub = pats[::7]
        b2, o2 = O.pack_patterns(sub)
        woffs, wpos = o.locate_batch(buf=b2, offs=o2, limit=lim, nthreads=8)
        goffs, gpos = g.locate_batch(buf=b2, offs=o2, limit=lim)
        assert np.array_equal(goffs, woffs) and np.array_equal(gpos, wpos), lim


def test_selectors_without_a_variant(pkg):
    """The tuning selectors that no engine variant turns on give the oracle's answers:
    CS_QT_COUNT_U1 / CS_QT_COUNT_U4 (one / four patterns per lane in the staged count) and
    CS_QT_BARRIER (its general search behind a block barrier) on a uniform and a repetitive text;
    CS_QT_WALK_PERSISTENT (phase 2's persistent walk kernel), CS_QT_WALK_ROWS (walks from an
    expanded rows buffer) and CS_QT_LOCATE_U1 (phase 1 with one pattern per lane), the two phases
    forced with CS_QT_NO_ONEPASS, on an index without the full suffix array, at limits that cut
    ranges and at ones that do not; CS_QT_ONEPASS_SA (the one-call locate over the full suffix
    array only) on that index, where the call falls back to the two phases, and on a default
    build, where it runs from the suffix array; and position samples at the SSA's stride (build
    option PSTRIDE=32: locate walks and extract by LF inversion)."""
    rng = np.random.default_rng(31)
    seed = rng.choice(list(b"ACGT"), 2000).astype(np.uint8)
    rep = np.tile(seed, 100)
    mut = rng.random(len(rep)) < 0.01
    rep[mut] = rng.choice(list(b"ACGT"), int(mut.sum())).astype(np.uint8)
    texts = {"dna": O.gen_dna(77, 150_000).tobytes(), "repeats": rep.tobytes() + b"$"}
    for name, t in texts.items():
        with _env(CS_FM_FULL_SA="0"):
            g = pkg.FMIndex.build_from_text(t)
        o = O.Index(t)
        u8 = np.frombuffer(t, np.uint8)
        pats = [bytes(p) for p in O.gen_patterns_text(u8, 20, 1000, seed=6)]
        pats += [bytes(p) for p in O.gen_patterns_text(u8, 7, 200, seed=7)]
        pats += [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in rng.integers(1, 40, 200)]
        pats += [b"", b"N" * 5, t[:25], t[-26:-1]]
        buf, offs = O.pack_patterns(pats)
        want = o.count_batch(buf=buf, offs=offs, nthreads=8)
        assert np.array_equal(_count_bo(g, buf, offs, flags=pkg.QT_COUNT_U1), want), name
        assert np.array_equal(_count_bo(g, buf, offs, flags=pkg.QT_COUNT_U4), want), name
        assert np.array_equal(_count_bo(g, buf, offs, flags=pkg.QT_BARRIER), want), name
        sub = pats[::5]
        b2, o2 = O.pack_patterns(sub)
        for lim in (3, 100_000):
            woffs, wpos = o.locate_batch(buf=b2, offs=o2, limit=lim, nthreads=8)
            sels = [pkg.QT_NO_ONEPASS | s for s in (pkg.QT_WALK_PERSISTENT, pkg.QT_WALK_ROWS, pkg.QT_LOCATE_U1)]
            runs = [(g, f) for f in sels]
            if name == "dna" and lim == 3:  # without the full SA (the two phases) and with it
                runs += [(g, pkg.QT_ONEPASS_SA), (pkg.FMIndex.build_from_text(t), pkg.QT_ONEPASS_SA)]
            for gi, f in runs:
                got = _locate_one(gi, sub, lim, flags=f)
                assert np.array_equal(np.cumsum([0] + [len(q) for q in got]), woffs.astype(np.int64)), (name, lim, f)
                flat = [x for q in got for x in q]
                assert np.array_equal(np.asarray(flat, np.int64), wpos.astype(np.int64)), (name, lim, f)
    t = texts["dna"]
    with _env(CS_FM_PSTRIDE="32", CS_FM_FULL_SA="0", CS_FM_DEVICE_TEXT="0"):
        g = pkg.FMIndex.build_from_text(t)
    assert g.info().position_stride == 32
    o = O.Index(t)
    pats = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(t, np.uint8), 12, 300, seed=8)]
    b2, o2 = O.pack_patterns(pats)
    woffs, wpos = o.locate_batch(buf=b2, offs=o2, limit=50, nthreads=8)
    got = _locate_one(g, pats, 50)
    assert [x for q in got for x in q] == wpos.astype(np.int64).tolist()
    pos = list(range(0, len(t), 997))
    assert g.extract_batch(pos, [40] * len(pos)) == [t[p:p + 40] for p in pos]


def test_dna_character_map(pkg):
    """The staged count maps a standard-DNA index's characters four per dword in registers
    (fm_query.hip, DevIndex::dna_std, round 6) and every other index's through the LDS table;
    CS_QT_MAP_LDS forces the table.  Patterns of text substrings with one byte replaced by each
    of the 256 byte values (lowercase acgt, 'N', 0xC1 = 'A' | 0x80, 'E' whose bits read as 'G',
    NUL) at every position of a 20-mer and a 9-mer, plus uniform patterns, give the oracle's
    counts both ways."""
    t = O.gen_dna(91, 120_000).tobytes()
    g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    u8 = np.frombuffer(t, np.uint8)
    rng = np.random.default_rng(41)
    pats = []
    for m, seed in ((20, 3), (9, 4), (31, 5)):
        base = [bytes(p) for p in O.gen_patterns_text(u8, m, 256, seed=seed)]
        for b, p in enumerate(base):
            q = bytearray(p)
            q[int(rng.integers(0, m))] = b
            pats += [p, bytes(q)]
    pats += [bytes(rng.choice(list(b"ACGT"), int(m)).astype(np.uint8)) for m in rng.integers(1, 33, 300)]
    buf, offs = O.pack_patterns(pats)
    want = o.count_batch(buf=buf, offs=offs, nthreads=8)
    assert np.array_equal(_count_bo(g, buf, offs), want)
    assert np.array_equal(_count_bo(g, buf, offs, flags=pkg.QT_MAP_LDS), want)


def test_majority_records_vs_oracle(pkg):
    """Wide compact records keep their two most frequent contexts with exact counts
    (fm_device.hpp kRec16Maj, round 4): on a repetitive text (copies of a seed with ~1 %
    substitutions) a pattern of k + 5 characters whose k-mer range is hundreds of rows wide
    is counted from the record alone.  Counts of k+3 .. k+7-mers — text substrings (the
    dominant context), mutants of their first characters (minority and absent contexts) and
    uniform patterns — equal the oracle's through the staged device batch, the host batch, the
    fixed-length form and the reference's plain steps (CS_Q_NO_CONTEXTS); most (k+5)-mer
    substrings then take one 16-B read (the measurement twin's bytes)."""
    rng = np.random.default_rng(21)
    seed = rng.choice(list(b"ACGT"), 5000).astype(np.uint8)
    t = np.tile(seed, 300)
    mut = rng.random(len(t)) < 0.01
    t[mut] = rng.choice(list(b"ACGT"), int(mut.sum())).astype(np.uint8)
    t = t.tobytes() + b"$"
    with _env(CS_FM_CTX_RECORDS="16"):
        g = pkg.FMIndex.build_from_text(t)
    o = O.Index(t)
    info = g.info()
    K = max(info.prefix_k, 1)
    pats = []
    for m in range(K + 3, K + 8):
        P = O.gen_patterns_text(np.frombuffer(t, np.uint8), m, 400, seed=m)
        for p in P:
            pats.append(bytes(p))
            q = bytearray(p)
            q[int(rng.integers(0, min(5, m)))] = b"ACGT"[int(rng.integers(0, 4))]
            pats.append(bytes(q))
        pats += [bytes(p) for p in O.gen_patterns_uniform(b"ACGT", m, 50, seed=m + 100)]
    buf, offs = O.pack_patterns(pats)
    want = o.count_batch(buf=buf, offs=offs, nthreads=8)
    got, _, _ = _count_ex(g, pats)
    assert np.array_equal(got, want)
    assert np.array_equal(g.count_batch(buf=buf, offs=offs), want)
    got, _, _ = _count_ex(g, pats, flags=2)  # CS_Q_NO_CONTEXTS: the reference's steps
    assert np.array_equal(got, want)
    m5 = [p for p in pats if len(p) == K + 5]
    d5 = torch.from_numpy(np.frombuffer(b"".join(m5), np.uint8).copy()).cuda()
    f5 = torch.empty(len(m5), dtype=torch.int64, device="cuda")
    g.count_fixed_device(d5.data_ptr(), K + 5, len(m5), f5.data_ptr())
    torch.cuda.synchronize()
    assert f5.cpu().numpy().astype(np.uint64).tolist() == [int(w) for p, w in zip(pats, want) if len(p) == K + 5]
    if info.record_bytes == 16 and info.engine in (1, 3) and not _wide():
        sub = [bytes(p) for p in O.gen_patterns_text(np.frombuffer(t, np.uint8), K + 5, 400, seed=K + 5)]
        b2, o2 = O.pack_patterns(sub)
        d_b, d_o = torch.from_numpy(b2.copy()).cuda(), torch.from_numpy(o2.astype(np.int64)).cuda()
        qb = torch.empty(len(sub), dtype=torch.int64, device="cuda")
        g.count_bytes_device(d_b.data_ptr(), d_o.data_ptr(), len(sub), qb.data_ptr())
        cnt = o.count_batch(buf=b2, offs=o2)
        torch.cuda.synchronize()
        wide = cnt > 9
        assert wide.mean() > 0.5 and (qb.cpu().numpy()[wide] == 16).mean() > 0.8


def test_open_reference_style_directory(pkg, tmp_path):
    """open_directory on a directory shaped like the reference's shipped sample.csidx/
    (only its text.txt; tests/golden/sample_csidx is that file): built as
    tools/build_index.cpp builds it ('$' appended, stride 32), answers as the oracle."""
    import shutil
    d = tmp_path / "sample.csidx"
    shutil.copytree(os.path.join(os.path.dirname(__file__), "golden", "sample_csidx"), d)
    t = open(d / "text.txt", "rb").read()
    g = pkg.FMIndex.open_directory(str(d))
    o = O.Index(t + b"$")
    assert g.n == len(t) + 1
    for p in (b"banana", b"ana", b"band", b"a", b"$", b"nan", b"x"):
        assert g.count(p) == o.count(p), p
        try:  # '$' is not the text's smallest symbol: the reference's cyclic-BWT walks
            want = o.locate(p)  # may overrun (fm_index.cpp:136-138), and so must these
        except RuntimeError as e:
            with pytest.raises(RuntimeError, match=str(e)):
                g.locate(p)
            continue
        assert g.locate(p) == want, p
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(RuntimeError, match="cannot open"):
        pkg.FMIndex.open_directory(str(empty))
