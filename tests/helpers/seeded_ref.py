"""What the seeded-locate suites share (tests/test_seeded_ref_cpu.py,
tests/test_zz_gpu_mismatch_seeded.py): a numpy restatement of include/cs_fmindex_approx_seeded.h
on the cyclic text — the piece split, the pieces' exact hits, the alignments they propose, the
ownership rule — and the device-call wrappers.

The restatement is checked against the cyclic Hamming scan of tests/helpers/mismatch_ref.py
without a GPU (tests/test_seeded_ref_cpu.py); the GPU tests compare the library with the scan
(the pairs), with the restatement (the candidate count C and, through the exact locate of the
pieces, the raw order) and with the backtracking locate at k <= 3.
"""
import numpy as np

from helpers.mismatch_ref import CANARY, _dev, _split, family_case, scan_distances

SEED_KS = (0, 1, 3, 4, 8)
SEED_KMAX = max(SEED_KS)


def piece_starts(m, k):
    """a_0 .. a_{k+1}: piece p of a pattern of length m is P[a_p, a_{p+1})."""
    return [p * m // (k + 1) for p in range(k + 2)]


def kept(pats, k):
    """The indices of the patterns a call at bound k accepts: m = 0 or m > k."""
    return [q for q, p in enumerate(pats) if len(p) == 0 or len(p) > k]


def piece_hits(text, piece):
    """The sorted starts x in [0, n) at which the cyclic text spells piece (len(piece) >= 1)."""
    n, L = len(text), len(piece)
    if L > n:
        return np.flatnonzero(scan_distances(text, piece) == 0).astype(np.int64)
    cyc = text + text[:L - 1]
    out, i = [], cyc.find(piece)
    while i != -1:
        out.append(i)
        i = cyc.find(piece, i + 1)
    return np.asarray(out, np.int64)


def piece_mismatches(text, pat, k, s):
    """int64 [len(s), k + 1]: the mismatching bytes of each piece of pat in the cyclic windows
    at the starts s."""
    t = np.frombuffer(text, np.uint8)
    p = np.frombuffer(pat, np.uint8)
    n, m = len(t), len(p)
    a = piece_starts(m, k)
    s = np.asarray(s, np.int64)
    out = np.zeros((len(s), k + 1), np.int64)
    step = max(1, (1 << 22) // max(m, 1))  # rows per block: 4 MB of window bytes at a time
    for r0 in range(0, len(s), step):
        rows = s[r0:r0 + step]
        ne = t[(rows[:, None] + np.arange(m)[None, :]) % n] != p[None, :]
        for pp in range(k + 1):
            out[r0:r0 + step, pp] = ne[:, a[pp]:a[pp + 1]].sum(axis=1)
    return out


def restate(text, pat, k):
    """The call's steps for one pattern with m > k: per candidate, in the output's candidate
    order up to the order inside a piece (here by position; the library's is the piece's
    exact-locate row order), the arrays
      piece   the piece it comes from
      x       the hit's text position
      s       the alignment (x - a_p) mod n
      d       the window's distance (all pieces)
      clean_before   whether a piece p' < p is clean at s (the candidate is not the owner)
      keep    owner and d <= k
    as a dict; C = len(piece)."""
    n, m = len(text), len(pat)
    assert m > k
    a = piece_starts(m, k)
    piece, x = [], []
    for p in range(k + 1):
        h = piece_hits(text, pat[a[p]:a[p + 1]])
        piece.append(np.full(len(h), p, np.int64))
        x.append(h)
    piece, x = np.concatenate(piece), np.concatenate(x)
    s = (x - np.asarray(a, np.int64)[piece]) % n
    mm = piece_mismatches(text, pat, k, s)
    assert (mm[np.arange(len(s)), piece] == 0).all()  # the piece that proposed s is clean there
    before = np.arange(k + 1)[None, :] < piece[:, None]
    clean_before = ((mm == 0) & before).any(axis=1)
    d = mm.sum(axis=1)
    return dict(piece=piece, x=x, s=s, d=d, clean_before=clean_before, keep=~clean_before & (d <= k))


def restated_pairs(r):
    """The emitted (pos, d) of a restate() result, as an int64 [count, 2] array in its order."""
    sel = r["keep"]
    return np.stack([r["s"][sel], r["d"][sel]], axis=1).reshape(-1, 2)


_SEEDED_CASES = {}


def seeded_case(name):
    """(text, patterns, d) of a family text (mismatch_ref.family_case's text and committed
    patterns), d[q] = the scan's distance at every start (None for the empty pattern): computed
    once per text and shared, never changed."""
    if name not in _SEEDED_CASES:
        text, pats = family_case(name)[:2]
        dist = []
        for p in pats:
            d = scan_distances(text, p) if p else None
            if d is not None:
                d.setflags(write=False)
            dist.append(d)
        _SEEDED_CASES[name] = (text, pats, dist)
    return _SEEDED_CASES[name]


def scan_pairs(dist, sel, k):
    """The scan's pairs (pos, d), d <= k, sorted by position, of the patterns sel."""
    out = []
    for q in sel:
        d = dist[q]
        if d is None:
            out.append(np.zeros((0, 2), np.int64))
            continue
        pos = np.flatnonzero(d <= k)
        out.append(np.stack([pos.astype(np.int64), d[pos].astype(np.int64)], axis=1).reshape(-1, 2))
    return out


_RESTATED = {}


def restated_case(name, k):
    """Per kept pattern of the family text at bound k its restate() result (None for the empty
    pattern), and the candidate count C of the whole batch; computed once and shared."""
    if (name, k) not in _RESTATED:
        text, pats, _ = seeded_case(name)
        rs = [restate(text, pats[q], k) if pats[q] else None for q in kept(pats, k)]
        _RESTATED[(name, k)] = (rs, sum(len(r["piece"]) for r in rs if r is not None))
    return _RESTATED[(name, k)]


# ---- the device calls ----------------------------------------------------------------------
def seeded_device(g, pats, k, flags=0, fixed_m=None, phases=False, raw=False, pad=0):
    """locate_mismatch_seeded_device (a sizing call with cap = 0 and null outputs, then the
    call) over CSR offsets, or fixed_m with d_offs = NULL -> (offsets, per-pattern sorted pairs,
    candidates); the entries after the last position and distance must come back untouched.
    phases: through the measurement twin (its phase times must come back).  pad: the pattern bytes start
    that many bytes into a larger device buffer.  raw: positions and distances as written."""
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    st = torch.cuda.current_stream().cuda_stream
    buf, offs = pkg.pack_patterns(pats)
    npat = len(pats)
    host = np.full(pad + max(len(buf), 1) + 3, 0xEE, np.uint8)
    host[pad:pad + len(buf)] = buf
    d_p = _dev(host, torch.uint8)
    d_o = _dev(offs.astype(np.int64), torch.int64)
    ms = [] if phases else None
    kw = dict(flags=flags, stream=st, phase_ms=ms)
    if fixed_m is not None:
        kw["fixed_m"] = fixed_m
    p_arg = d_p.data_ptr() + pad
    d_offs_arg = d_o.data_ptr() if fixed_m is None else None
    d_oo = torch.full((npat + 1,), -1, dtype=torch.int64, device="cuda")
    total, cand, written = g.locate_mismatch_seeded_device(p_arg, d_offs_arg, npat, k, d_oo.data_ptr(), None, None,
                                                           0, **kw)
    assert written == (total == 0)
    sized = d_oo.cpu().numpy().copy()
    d_pos = torch.full((total + CANARY,), -1, dtype=torch.int64, device="cuda")
    d_dist = torch.full((total + CANARY,), 0xFF, dtype=torch.uint8, device="cuda")
    d_oo.fill_(-1)
    tot2, cand2, written = g.locate_mismatch_seeded_device(p_arg, d_offs_arg, npat, k, d_oo.data_ptr(),
                                                           d_pos.data_ptr(), d_dist.data_ptr(), total, **kw)
    torch.cuda.synchronize()
    assert written and tot2 == total and cand2 == cand
    if phases:  # the piece search always runs; a call that verifies candidates takes time there
        assert len(ms) == 5 and ms[0] > 0 and (cand == 0 or ms[2] > 0)
    oo = d_oo.cpu().numpy()
    assert oo.tolist() == sized.tolist() and oo[-1] == total
    pos, dist = d_pos.cpu().numpy(), d_dist.cpu().numpy()
    assert (pos[total:] == -1).all() and (dist[total:] == 0xFF).all(), "canary overwritten"
    if raw:
        return oo, pos[:total], dist[:total], cand
    return oo, _split(oo, pos[:total], dist[:total]), cand


def seeded_host(g, pats, k):
    oo, pos, dist = g.locate_mismatches_seeded_batch(pats, k)
    assert pos.dtype == np.uint64 and dist.dtype == np.uint8 and len(pos) == len(dist) == oo[-1]
    return oo, _split(oo, pos, dist)
