"""The LF steps of locate's walks (cs_fm_locate_walk_steps_device, what bench.py reads for its
walk bytes) replayed on the host, and the walk's forms against each other.

A walk from BWT row r follows LF to the first stop row and reports sample + steps (mod n).
The replay applies LF (FMIndex.lf, checked against the oracle's suffix array) to the walk's
row `steps` times: the row it reaches is a stop row, no row before it on the path is one, and
the reported position is the oracle's SA[r].  Stop rows, read off the builder (build_walk_t /
k_walk_pack, fm_build_rank.hip) and the walk (fm_walk.hpp):
  * text-position marks (info().walk_marks == 2): SA[row] % position_stride == 0, or a row the
    reference samples, row % ssa_stride == 0; every walk ends within position_stride - 1 steps;
  * row marks (CS_FM_WALK_MARKS=row, walk_marks == 1): the marked rows are the reference's
    sampled rows, so row % ssa_stride == 0 alone;
  * no walk lines (CS_Q_NO_WALK_LINES, k_walk over the engine's LF): row % ssa_stride == 0.
The patterns are text substrings plus absent ones and the empty pattern, their rows sp + j
of the plain records CS_Q_NO_CONTEXTS gives.
The file is named to collect after every suite that was here before it.
"""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg

pytestmark = pytest.mark.gpu

LIMIT = 100000

# the walk's forms (fm_walk.hip): WalkLine with text-position marks, WalkLineW, the quaternary
# matrix's walk lines (kQ), row marks (k_walk_lines by default)
BUILDS = {
    "nosa": {"CS_FM_FULL_SA": "0"},
    "wide_nosa": {"CS_FM_WIDE": "1", "CS_FM_FULL_SA": "0"},
    "qwm_nosa": {"CS_FM_ENGINE": "qwm", "CS_FM_FULL_SA": "0"},
    "rowmarks": {"CS_FM_WALK_MARKS": "row", "CS_FM_FULL_SA": "0"},
}


def _dna(with_n):
    t = O.gen_dna(20, 20000).copy()  # 20,000 bases, then '$'
    if with_n:  # several rare rows: walk_lf_k's table branch (one, the terminator's: nexc == 1)
        t[np.random.default_rng(20).choice(20000, 20, replace=False)] = ord("N")
    return t.tobytes()


TEXTS = {"dna": lambda: _dna(False), "dna_N": lambda: _dna(True)}

_CASES = {}


def _case(name):
    """(text, patterns, the oracle's suffix array), computed once per text."""
    if name not in _CASES:
        text = TEXTS[name]()
        t = np.frombuffer(text, np.uint8)
        pats = [bytes(p) for p in O.gen_patterns_text(t, 12, 300, seed=3)]
        pats += [bytes(p) for p in O.gen_patterns_text(t, 3, 100, seed=4)]  # ~300 rows each: > kLocSmall
        ref = O.Index(text)
        absent = [bytes(p) for p in O.gen_patterns_unif("dna", 14, 200, seed=5) if ref.count(bytes(p)) == 0][:20]
        assert len(absent) == 20
        pats += absent + [b""]
        _CASES[name] = (text, pats, ref.sa().astype(np.int64))
    return _CASES[name]


def _walks(g, pats, flags):
    """Both phases under `flags`: (records, offsets, steps, positions) as host arrays."""
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    npat = len(pats)
    d_sp = torch.zeros(npat, dtype=torch.int64, device="cuda")
    d_oo = torch.zeros(npat + 1, dtype=torch.int64, device="cuda")
    tot = g.locate_ranges_device(d_buf.data_ptr(), d_offs.data_ptr(), npat, LIMIT, d_sp.data_ptr(),
                                 d_oo.data_ptr(), flags=flags)
    d_steps = torch.full((max(tot, 1),), -1, dtype=torch.int64, device="cuda")
    d_pos = torch.full((max(tot, 1),), -1, dtype=torch.int64, device="cuda")
    g.locate_walk_steps_device(d_sp.data_ptr(), d_oo.data_ptr(), npat, tot, d_steps.data_ptr(), flags=flags)
    g.locate_walk_device(d_sp.data_ptr(), d_oo.data_ptr(), npat, tot, d_pos.data_ptr(), flags=flags)
    torch.cuda.synchronize()
    return (d_sp.cpu().numpy().view(np.uint64), d_oo.cpu().numpy(), d_steps[:tot].cpu().numpy(),
            d_pos[:tot].cpu().numpy())


def _build(pkg, opts, text):
    with pkg.build_options(opts):
        return pkg.FMIndex.build_from_text(text)


def _replay(pkg, g, name, row_marks, no_walk_lines):
    text, pats, sa = _case(name)
    n = len(text)
    flags = pkg.Q_NO_CONTEXTS | (pkg.Q_NO_WALK_LINES if no_walk_lines else 0)
    rec, oo, steps, pos = _walks(g, pats, flags)
    cnt = np.diff(oo)
    assert cnt[-1] == 0 and (cnt[-21:-1] == 0).all() and (cnt[:400] >= 1).all()
    assert (cnt[300:400] > 32).sum() >= 50  # ranges for the wide kernel
    assert not (rec[cnt > 0] >> np.uint64(63)).any()  # plain records: rows sp + j
    rows = np.concatenate([int(rec[q]) + np.arange(cnt[q]) for q in range(len(pats))]).astype(np.int64)
    assert len(rows) == len(steps) == oo[-1]
    # LF of every row, by the oracle's suffix array: SA[LF(r)] = SA[r] - 1 (mod n)
    lf = g.lf(np.arange(n, dtype=np.uint64)).astype(np.int64)
    assert (sa[lf] == (sa - 1) % n).all()
    inf = g.info()
    marks = inf.walk_marks == 2 and not no_walk_lines
    assert inf.walk_marks == (1 if row_marks else 2)
    stop = np.arange(n) % inf.ssa_stride == 0
    if marks:
        stop |= sa % inf.position_stride == 0
        assert steps.max() <= inf.position_stride - 1
    assert steps.min() >= 0 and steps.max() < n
    cur = rows.copy()
    for t in range(int(steps.max()) + 1):
        assert not stop[cur[steps > t]].any(), (name, t)   # no earlier stop row on a path
        assert stop[cur[steps == t]].all(), (name, t)       # the row after steps[i] LF steps is one
        cur = lf[cur]
    assert (pos == sa[rows]).all()


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("build", sorted(BUILDS) + ["nosa_nowalklines"])
def test_exact_replay(build, name):
    pkg = load_pkg()
    opts = BUILDS[build.replace("_nowalklines", "")]
    g = _build(pkg, opts, _case(name)[0])
    _replay(pkg, g, name, build == "rowmarks", build.endswith("_nowalklines"))


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_forms_agree(build, name):
    """Steps and positions element-wise equal under the default flags, CS_QT_WALK_ROWS and
    CS_QT_WALK_PERSISTENT, from plain records and from the default ones (context windows,
    adj > 0), whose rows and positions are the plain records' in the same order."""
    pkg = load_pkg()
    text, pats, _ = _case(name)
    g = _build(pkg, BUILDS[build], text)
    got = {}
    for base in (pkg.Q_NO_CONTEXTS, 0):
        for sel in (0, pkg.QT_WALK_ROWS, pkg.QT_WALK_PERSISTENT):
            rec, oo, steps, pos = _walks(g, pats, base | sel)
            got[base, sel] = (oo, steps, pos)
            if base == 0 and g.info().context_q:
                assert (rec >> np.uint64(63)).any()  # context windows among the records
    want = got[pkg.Q_NO_CONTEXTS, 0]
    for key, (oo, steps, pos) in got.items():
        assert (oo == want[0]).all(), key
        assert (pos == want[2]).all(), key
        if key[0] == pkg.Q_NO_CONTEXTS:  # (a window's walk starts k rows earlier: other steps)
            assert (steps == want[1]).all(), key
        else:
            assert (steps == got[0, 0][1]).all(), key


def test_full_sa_steps_zero():
    pkg = load_pkg()
    text, pats, sa = _case("dna")
    g = _build(pkg, {}, text)
    assert g.info().walk_marks == 0
    for flags in (0, pkg.Q_NO_CONTEXTS):
        rec, oo, steps, pos = _walks(g, pats, flags)
        assert len(steps) == oo[-1] > 20000 and (steps == 0).all()
