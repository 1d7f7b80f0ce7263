"""What the mismatch suites share (tests/test_zz_gpu_mismatch*.py, tests/test_mismatch_scan_cpu.py).

Two references of "count / locate within k mismatches" (include/cs_fmindex_approx.h):

* the enumeration (expected_hist, expected_pairs): every Hamming neighbour of the pattern over
  the text's present symbols, counted and located by the oracle.  It follows the definition on
  any text, cyclic ones included, but its cost is C(m, k) * sigma^k strings per pattern, so it
  serves short patterns only;
* the cyclic Hamming scan (scan_hamming): for a text whose last byte is unique and smaller than
  every other byte, the BWT rows are the rotations of the text, so hist[d] is the number of
  starts i in [0, n) with Hamming(P, t[(i + j) mod n], j < m) = d, and the pairs are (i, d(i))
  with d(i) <= k.  No index, no enumeration, n * m bytes per pattern whatever k is.
  tests/test_mismatch_scan_cpu.py holds the agreement of the two (and of the scan with the
  oracle's exact count and locate at d = 0) without a GPU.

The "family" texts plant the neighbours a long pattern has only by accident on random text:
copies of one random segment, copy c carrying c mod 5 substitutions, between random spacers.
A pattern's search tree then stays alive along each copy, so leaves at d = 1, 2, 3 are reached
with a hundred characters still to verify.

The device-call wrappers (device_hist, device_pairs, _split, _check) were written for the two
first mismatch files and moved here unchanged.
"""
import itertools

import numpy as np

KMAX = 3
CANARY = 16  # entries after the last one, prefilled with all-ones bytes


# ---- the enumeration reference -------------------------------------------------------------
def _present(text):
    return sorted(set(text))


def _absent_byte(text):
    have = set(text)
    return next(b for b in b"#%&0123456789" if b not in have)


def _neighbours(p, syms, d):
    """Every string at Hamming distance d from p over syms, as a uint8 [count, len(p)] array."""
    a = np.frombuffer(p, np.uint8)
    m = len(a)
    out = [np.zeros((0, m), np.uint8)]
    if d <= m:
        for pos in itertools.combinations(range(m), d):
            subs = [[s for s in syms if s != a[i]] for i in pos]
            tuples = list(itertools.product(*subs))
            prod = np.array(tuples, np.uint8).reshape(len(tuples), d)
            blk = np.tile(a, (len(prod), 1))
            blk[:, list(pos)] = prod
            out.append(blk)
    return np.concatenate(out)


def expected_hist(ref, text, pats, k):
    """uint64 [len(pats), k + 1]: the oracle sum of the definition."""
    syms = _present(text)
    chunks, lens, gid = [], [], []
    for q, p in enumerate(pats):
        for d in range(k + 1):
            nb = _neighbours(p, syms, d)
            chunks.append(nb.reshape(-1))
            lens.append(np.full(len(nb), len(p), np.uint64))
            gid.append(np.full(len(nb), q * (k + 1) + d, np.int64))
    lens = np.concatenate(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    buf = np.concatenate(chunks + [np.zeros(1, np.uint8)])
    cnt = ref.count_batch(buf=buf, offs=offs, nthreads=8)
    tot = np.bincount(np.concatenate(gid), weights=cnt.astype(np.float64), minlength=len(pats) * (k + 1))
    assert tot.max(initial=0) < 2.0 ** 53
    return tot.astype(np.uint64).reshape(len(pats), k + 1)


def expected_pairs(ref, text, pats, k, syms=None):
    """Per pattern the sorted (pos, d) pairs of the definition, as an int64 [count, 2] array,
    and the largest number of rows one neighbour (one leaf of the search) holds."""
    syms = _present(text) if syms is None else syms
    n = len(text)
    chunks, lens, owner, dist = [], [], [], []
    for q, p in enumerate(pats):
        if not p:
            continue  # fm_index.cpp:109: an empty pattern has no positions
        for d in range(k + 1):
            nb = _neighbours(p, syms, d)
            chunks.append(nb.reshape(-1))
            lens.append(np.full(len(nb), len(p), np.uint64))
            owner.append(np.full(len(nb), q, np.int64))
            dist.append(np.full(len(nb), d, np.int64))
    lens, owner, dist = np.concatenate(lens), np.concatenate(owner), np.concatenate(dist)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    buf = np.concatenate(chunks + [np.zeros(1, np.uint8)])
    cnt = ref.count_batch(buf=buf, offs=offs, nthreads=8)
    hit = np.flatnonzero(cnt)
    hbuf = np.concatenate([buf[int(offs[i]):int(offs[i + 1])] for i in hit] + [np.zeros(1, np.uint8)])
    hoffs = np.concatenate([[0], np.cumsum(lens[hit])]).astype(np.uint64)
    loffs, lpos = ref.locate_batch(buf=hbuf, offs=hoffs, limit=n + 1, nthreads=8)
    per = np.diff(loffs.astype(np.int64))
    assert per.tolist() == cnt[hit].astype(np.int64).tolist()
    own, dd = np.repeat(owner[hit], per), np.repeat(dist[hit], per)
    out = []
    for q in range(len(pats)):
        sel = own == q
        pairs = np.stack([lpos[sel].astype(np.int64), dd[sel]], axis=1).reshape(-1, 2)
        out.append(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])
    return out, int(per.max(initial=0))


# ---- the device calls ----------------------------------------------------------------------
def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def device_hist(g, pats, k, flags=0, fixed_m=None, canary_rows=1):
    """count_mismatch_device over CSR offsets (or fixed_m with d_offs = NULL) -> [npat, k + 1];
    the rows after the last histogram row must come back untouched."""
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    d_p = _dev(buf, torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    d_h = torch.full(((npat + canary_rows) * (k + 1),), -1, dtype=torch.int64, device="cuda")
    if fixed_m is None:
        g.count_mismatch_device(d_p.data_ptr(), d_o.data_ptr(), npat, k, d_h.data_ptr(), flags=flags, stream=st)
    else:
        g.count_mismatch_device(d_p.data_ptr(), None, npat, k, d_h.data_ptr(), fixed_m=fixed_m, flags=flags,
                                stream=st)
    torch.cuda.synchronize()
    h = d_h.cpu().numpy().view(np.uint64).reshape(npat + canary_rows, k + 1)
    assert (h[npat:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "canary row overwritten"
    return h[:npat]


def device_pairs(g, pats, k, flags=0, fixed_m=None, raw=False):
    """locate_mismatch_device (a sizing call with cap = 0 and null outputs, then the call) over
    CSR offsets, or fixed_m with d_offs = NULL -> (offsets, per-pattern sorted pairs); the
    entries after the last position and distance must come back untouched.  raw: the
    positions and distances as written."""
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
    d_oo = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
    total, written = g.locate_mismatch_device(d_p.data_ptr(), d_offs_arg, npat, k, d_oo.data_ptr(), None, None, 0,
                                              **kw)
    assert written == (total == 0)
    sized = d_oo.cpu().numpy().copy()
    d_pos = torch.full((total + CANARY,), -1, dtype=torch.int64, device="cuda")
    d_dist = torch.full((total + CANARY,), 0xFF, dtype=torch.uint8, device="cuda")
    d_oo.fill_(-1)
    tot2, written = g.locate_mismatch_device(d_p.data_ptr(), d_offs_arg, npat, k, d_oo.data_ptr(),
                                             d_pos.data_ptr(), d_dist.data_ptr(), total, **kw)
    torch.cuda.synchronize()
    assert written and tot2 == total
    oo = d_oo.cpu().numpy()
    assert oo.tolist() == sized.tolist() and oo[-1] == total
    pos, dist = d_pos.cpu().numpy(), d_dist.cpu().numpy()
    assert (pos[total:] == -1).all() and (dist[total:] == 0xFF).all(), "canary overwritten"
    if raw:
        return oo, pos[:total], dist[:total]
    return oo, _split(oo, pos[:total], dist[:total])


def _split(oo, pos, dist):
    out = []
    for q in range(len(oo) - 1):
        a, b = int(oo[q]), int(oo[q + 1])
        pairs = np.stack([pos[a:b].astype(np.int64), dist[a:b].astype(np.int64)], axis=1).reshape(-1, 2)
        out.append(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])
    return out


def _check(got_offs, got, want, what):
    sizes = [len(w) for w in want]
    assert np.asarray(got_offs).astype(np.int64).tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist(), what
    for q, (a, b) in enumerate(zip(got, want)):
        assert a.tolist() == b.tolist(), (what, q)


def host_pairs(g, pats, k):
    oo, pos, dist = g.locate_mismatches_batch(pats, k)
    assert pos.dtype == np.uint64 and dist.dtype == np.uint8 and len(pos) == len(dist) == oo[-1]
    return oo, _split(oo, pos, dist)


def _cut(want, k):
    return [w[w[:, 1] <= k] for w in want]


# ---- the cyclic Hamming scan ---------------------------------------------------------------
def check_scannable(text):
    """The scan is the definition only where the BWT rows are the text's rotations: a last byte
    that occurs once and is smaller than every other byte."""
    t = np.frombuffer(text, np.uint8)
    assert len(t) >= 2 and (t[:-1] > t[-1]).all(), "the scan needs a unique smallest last byte"


def scan_distances(text, pat):
    """d(i) = Hamming(pat, t[(i + j) mod n] for j < m) for every start i in [0, n); m >= 1."""
    t = np.frombuffer(text, np.uint8)
    p = np.frombuffer(pat, np.uint8)
    n, m = len(t), len(p)
    cyc = np.tile(t, (n + m - 2) // n + 1)[:n + m - 1]
    win = np.lib.stride_tricks.sliding_window_view(cyc, m)  # [n, m]: row i is the window at i
    return (win != p).sum(axis=1)


def scan_hamming(text, pats, k):
    """(hist, pairs): hist a uint64 [len(pats), k + 1] table, pairs per pattern the (pos, d) with
    d <= k as an int64 [count, 2] array sorted by position.  m = 0: [n, 0, ...] and no pairs."""
    check_scannable(text)
    n = len(text)
    hist = np.zeros((len(pats), k + 1), np.uint64)
    pairs = []
    for q, p in enumerate(pats):
        if not p:
            hist[q, 0] = n
            pairs.append(np.zeros((0, 2), np.int64))
            continue
        d = scan_distances(text, p)
        pos = np.flatnonzero(d <= k)
        hist[q] = np.bincount(d[pos], minlength=k + 1)
        pairs.append(np.stack([pos.astype(np.int64), d[pos].astype(np.int64)], axis=1).reshape(-1, 2))
    return hist, pairs


def mismatch_positions(text, pat, pos):
    """The pattern indices at which the cyclic window at pos differs from pat."""
    t = np.frombuffer(text, np.uint8)
    p = np.frombuffer(pat, np.uint8)
    return np.flatnonzero(t[(pos + np.arange(len(p))) % len(t)] != p)


def widest_leaf(text, pat, pairs):
    """The most rows one neighbour (one leaf of the search) of pat holds: the largest group of
    hits whose windows spell the same string."""
    t = np.frombuffer(text, np.uint8)
    groups = {}
    for pos in pairs[:, 0]:
        w = t[(int(pos) + np.arange(len(pat))) % len(t)].tobytes()
        groups[w] = groups.get(w, 0) + 1
    return max(groups.values(), default=0)


# ---- texts with planted neighbours ---------------------------------------------------------
SEG, SPACER = 300, 40
LENGTHS = (9, 10, 21, 33, 64, 97, 130, 290)  # 9 | 10: the verification threshold; 33 = kFastM + 1

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_A12 = np.frombuffer(b"abcdefghijkl", np.uint8)
# 16 byte values drawn from 1..254 (255 stays out of the text: the absent-byte patterns use it).
# The wavelet engines take one E::step per listed symbol at every node of the search, and the
# pattern longer than the text has n + 5 nodes in frame 0 alone: with all of 1..254 present and
# n = 4,121 that one lane took 2.1 s per traversal on an MI355X (a locate call at k = 3 17 s;
# with 32 values and n = 1,741 a text's locate test still took 5 to 11 s).  16 values spread
# over the byte range keep eight binary wavelet levels, symbols on either side of 128, a symbol
# list filled by more than one wave and terminator 0.  They do not keep the quaternary matrix's
# depth: it codes the present symbols densely (build_qwm), so 17 symbols give three levels, not
# the four of a text with 65 or more (DESIGN §10.2 lists what that leaves uncovered).
_BYTES = np.sort(np.random.default_rng(104).choice(np.arange(1, 255, dtype=np.uint8), 16, replace=False))
assert _BYTES[0] < 64 and _BYTES[-1] >= 192

FAMILIES = {
    # name: (alphabet, terminator, copies, N written over random places, seed)
    # n = copies * 300 + (copies + 1) * 40 + 1: 4,121 with 12 copies, 1,741 with 5.  A search
    # costs (n + 5) * (symbols listed) steps for the pattern longer than the text whatever k
    # is, so the two larger alphabets get the smaller text: one copy per substitution count
    "fam_dna": (_ACGT, b"$", 12, 0, 101),
    "fam_dna_N": (_ACGT, b"$", 12, 30, 102),
    "fam_alpha12": (_A12, b"$", 5, 0, 103),
    "fam_bytes": (_BYTES, b"\x00", 5, 0, 104),
}

# The prefix-table depths the builder gives these texts (fm_structs.hip: the largest k with
# sigma^k <= max(4096, 8 n) entries, sigma counting the terminator and N; none below k = 2),
# and the forced depth 8 of the DNA texts.  The patterns carry a planted pair around m - k for
# each, and the GPU tests assert that info().prefix_k is 0 or one of these.
PREFIX_KS = {"fam_dna": (6, 8), "fam_dna_N": (5, 8), "fam_alpha12": (3,), "fam_bytes": (3,)}


def _other(rng, alphabet, c):
    o = alphabet[alphabet != c]
    return int(o[int(rng.integers(0, len(o)))])


def family_text(name):
    """(text, segment): copies of a random SEG-symbol segment, copy c with c mod 5
    substitutions at random places, random SPACER-symbol spacers before, between and after
    them, then the terminator."""
    alphabet, term, copies, n_N, seed = FAMILIES[name]
    rng = np.random.default_rng(seed)
    seg = alphabet[rng.integers(0, len(alphabet), SEG)]
    parts = []
    for c in range(copies):
        parts.append(alphabet[rng.integers(0, len(alphabet), SPACER)])
        cp = seg.copy()
        for j in rng.choice(SEG, c % 5, replace=False):
            cp[j] = _other(rng, alphabet, cp[j])
        parts.append(cp)
    parts.append(alphabet[rng.integers(0, len(alphabet), SPACER)])
    t = np.concatenate(parts)
    if n_N:  # most land inside the copies (87 % of the text); copy 0 is kept whole, so that a
        # window of every length still has an exact occurrence
        free = np.concatenate([np.arange(SPACER), np.arange(SPACER + SEG, len(t))])
        t[rng.choice(free, n_N, replace=False)] = ord("N")
    text = t.tobytes() + term
    check_scannable(text)
    return text, seg.tobytes()


def planted_sets(m, prefix_ks):
    """The substitution sets a window of length m carries."""
    sets = [(), (m - 1,), (m - 1, m - 2, m - 3), (0,), (0, 1, 2), (0, m // 2, m - 1)]
    # The leaf frame restarts from the table while m - j < prefix_k, j the last substituted
    # position: m - prefix_k + 1 is the first position whose leaf restarts, m - prefix_k the
    # last whose leaf goes on from its range.  The pair holds one of each (its hit's leaf goes
    # on from the range); the single position gives a hit whose leaf restarts at the boundary.
    for pk in prefix_ks:
        if m - pk >= 0:
            sets.append((m - pk, m - pk + 1))
            sets.append((m - pk + 1,))
    return sets


def family_patterns(name, text, seg):
    """The patterns of one family text, in mixed lengths (CSR starts on every byte alignment),
    and per pattern the planted positions (None for the patterns that are not windows of the
    segment)."""
    alphabet = FAMILIES[name][0]
    alphabet = alphabet[np.isin(alphabet, np.frombuffer(text, np.uint8))]  # substitutes: present symbols
    rng = np.random.default_rng(len(text))
    n = len(text)
    pats, planted = [], []

    def add(p, where=None):
        pats.append(bytes(p))
        planted.append(where)

    for m in (1, 3):  # short windows: leaves of many rows
        i = int(rng.integers(0, SEG - m + 1))
        add(seg[i:i + m], ())
    for m in LENGTHS:
        i = int(rng.integers(0, SEG - m + 1))
        for where in planted_sets(m, PREFIX_KS[name]):
            p = bytearray(seg[i:i + m])
            for j in where:
                p[j] = _other(rng, alphabet, p[j])
            add(p, where)
    m = 21  # a byte absent from the text at the last, a middle and the first position
    i = int(rng.integers(0, SEG - m + 1))
    absent = 255 if name == "fam_bytes" else _absent_byte(text)
    assert absent not in set(text)
    for at in (m - 1, m // 2, 0):
        p = bytearray(seg[i:i + m])
        p[at] = absent
        add(p)
    a, b = 12, 15  # through the end of the text: the terminator is pattern byte a - 1
    wrap = bytearray(text[n - a:] + text[:b])
    add(wrap)
    wrap[a - 1] = _other(rng, alphabet, 0)  # its only hit substitutes the terminator, d = 1
    add(wrap)
    add((text * 3)[7:7 + n + 5])  # longer than the text
    add(b"")
    return pats, planted


_FAMILY_CASES = {}


def family_case(name):
    """(text, patterns, planted positions, the scan's k = 3 histogram, the scan's k = 3 pairs),
    computed once per text and shared; the bound k is the first k + 1 columns / the pairs with
    d <= k (_cut)."""
    if name not in _FAMILY_CASES:
        text, seg = family_text(name)
        pats, planted = family_patterns(name, text, seg)
        hist, pairs = scan_hamming(text, pats, KMAX)
        hist.setflags(write=False)
        _FAMILY_CASES[name] = (text, pats, planted, hist, pairs)
    return _FAMILY_CASES[name]
