"""The routed staged count (k_count_ctx's count forms, csrc/fm_query.hip) at its block, slot
and wave edges against the oracle, count for count, on a standard-DNA index and on two that
are not.

The count codes a standard-DNA index's characters in registers (DevIndex::dna_std, reported
by cs_fm_dna_std) and every other index's through the symbol map in LDS, so the same batches
run on three texts of 1.2 M symbols (the terminator must be rarer than one row in 2^20 to stay
out of the table's alphabet, or no text with a '$' is standard DNA):
  std    seeded DNA + '$'                    -> dna_std, characters coded in registers;
  fifth  DNA with a fifth frequent symbol    -> not dna_std, the index's own count;
  acgu   DNA with T spelled U                -> occurrence lines over a 4-symbol alphabet that
                                                is not A C G T: k_count_ctx through the LDS map.
Batch sizes sit on the block (512 patterns), wave-slot (128) and wave (64) edges, so the
clamp of the last block's indices (qc = npat - 1), the last partial wave and the count
stores' addresses (formed from the lane's first pattern index inside each store's branch) are
hit; every batch goes through one CSR offsets array of mixed lengths (o0 & 3 takes every
value) with lengths around the table depth K and the context reach K + 7, bytes outside the
alphabet (N, a, 0x00, 0xFF) in the table part, the context part and before them, mutated and
random patterns that do not occur; u64 and u32 counts; a zero-filled workspace used by two
consecutive calls, and no workspace."""
import numpy as np
import pytest
import torch

import oracle as O
from conftest import load_pkg
from test_gpu_parity import _count_ex

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025]
SPECIALS = [ord("N"), ord("a"), 0x00, 0xFF]
CTX_Q = 7  # characters before the table part that a context key holds (fm_device.hpp kCtxQ)


def _text(kind):
    t = O.gen_dna(1234, 1_199_999).copy()  # 1,199,999 bases + '$'
    if kind == "fifth":
        rng = np.random.default_rng(5)
        body = t[:-1]
        body[rng.random(len(body)) < 0.2] = ord("N")
    elif kind == "acgu":
        t[t == ord("T")] = ord("U")
    return t.tobytes()


def _lengths(K):
    return [0, 1, K - 1, K] + [K + d for d in range(1, 8)] + [K + 8, 31, 32, 33, 64]


def _batch(text, K, n):
    """n patterns, seeded by n: slices of the text with the lengths cycled, and per pattern
    one of seven treatments cycled (7 and the 16 lengths are coprime: every pairing comes up).
    -> (patterns, coverage) with coverage the set of (special byte, part) pairs placed."""
    t = np.frombuffer(text, np.uint8)
    body = len(t) - 1
    rng = np.random.default_rng(1000 + n)
    lens = _lengths(K)
    alpha = sorted(set(t[:body].tolist()))
    pats, cov = [], set()
    for i in range(n):
        L = lens[(i + n) % len(lens)]
        at = int(rng.integers(0, body - L))
        p = bytearray(t[at:at + L].tobytes())
        kind = i % 7
        sp = SPECIALS[(i // 7) % 4]
        tab0 = max(L - K, 0)                 # table part: [tab0, L)
        ctx0 = max(tab0 - CTX_Q, 0)          # context part: [ctx0, tab0)
        if kind == 1 and L:                  # a mutation: mostly a pattern the text does not hold
            j = int(rng.integers(0, L))
            p[j] = alpha[(alpha.index(p[j]) + 1 + int(rng.integers(0, len(alpha) - 1))) % len(alpha)]
        elif kind == 2 and L:
            p[int(rng.integers(tab0, L))] = sp
            cov.add((sp, "table"))
        elif kind == 3 and tab0 > ctx0:
            p[int(rng.integers(ctx0, tab0))] = sp
            cov.add((sp, "context"))
        elif kind == 4 and ctx0 > 0:
            p[int(rng.integers(0, ctx0))] = sp
            cov.add((sp, "before"))
        elif kind == 5 and L:                # uniform over the alphabet: does not occur when long
            p = bytearray(rng.choice(alpha, L).astype(np.uint8).tobytes())
        pats.append(bytes(p))
    return pats, cov


class _Index:
    def __init__(self, kind, K=None):
        pkg = load_pkg()
        self.text = _text(kind)
        # the headline's layout: compact 16-B context records (the default from a table depth
        # of 15 on, 4 G bases; forced here, every other option at its default)
        with pkg.build_options({"CS_FM_CTX_RECORDS": "16"}):
            self.g = pkg.FMIndex.build_from_text(self.text)
        self.o = O.Index(self.text)
        self.info = self.g.info()
        # (the lengths follow the standard-DNA index's table depth on every index)
        self.K = int(self.info.prefix_k) if K is None else K
        self.batches = {}

    def batch(self, n):
        """(patterns, coverage, oracle counts), made once per size."""
        if n not in self.batches:
            pats, cov = _batch(self.text, self.K, n)
            buf, offs = O.pack_patterns(pats)
            want = np.asarray(self.o.count_batch(buf=buf, offs=offs, nthreads=4), np.uint64)
            self.batches[n] = (pats, cov, want)
        return self.batches[n]


@pytest.fixture(scope="module")
def indexes():
    std = _Index("std")
    return {"std": std, "fifth": _Index("fifth", std.K), "acgu": _Index("acgu", std.K)}


def _count_ws(g, pats, width, ws, wsb):
    buf, offs = O.pack_patterns(pats)
    d_buf = torch.from_numpy(buf.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    dt = {8: torch.int64, 4: torch.int32}[width]
    out = torch.full((len(pats),), -1, dtype=dt, device="cuda")
    g.count_device_ws(d_buf.data_ptr(), d_offs.data_ptr(), len(pats), out.data_ptr(), ws.data_ptr(), wsb,
                      width=width)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64).astype(np.uint64) & np.uint64((1 << (8 * width)) - 1)


def _check(ix, n):
    pats, _, want = ix.batch(n)
    bad = []
    for width in (8, 4):
        wsb = ix.g.workspace_bytes(n)
        ws = torch.zeros(max(wsb, 1), dtype=torch.uint8, device="cuda")
        for call in (1, 2):  # the second call finds the workspace as the first left it
            got = _count_ws(ix.g, pats, width, ws, wsb)
            if not np.array_equal(got, want):
                bad.append((width, "workspace call %d" % call, np.flatnonzero(got != want)[:5].tolist()))
        got, _, _ = _count_ex(ix.g, pats, width=width)
        if not np.array_equal(got, want):
            bad.append((width, "no workspace", np.flatnonzero(got != want)[:5].tolist()))
    assert not bad, (n, bad)


def test_alphabet_forms(indexes):
    """Only the standard-DNA index codes its characters in registers, and the handles report
    the alphabets apart; the table is deep enough for every length class to differ."""
    std, fifth, acgu = indexes["std"], indexes["fifth"], indexes["acgu"]
    assert std.g.dna_std() and not fifth.g.dna_std() and not acgu.g.dna_std()
    assert std.info.engine == 1 and acgu.info.engine == 1  # occurrence lines: k_count_ctx
    assert std.info.prefix_sigma == 4 and acgu.info.prefix_sigma == 4
    codes = {k: bytes(ix.info.prefix_code) for k, ix in indexes.items()}
    assert codes["std"] != codes["acgu"] and codes["std"] != codes["fifth"]
    assert (fifth.info.engine, fifth.info.prefix_sigma) != (1, 4)
    assert 2 <= std.K == std.info.prefix_k and std.K + 8 < 31, std.K
    assert std.info.context_q == CTX_Q and std.info.record_bytes == 16 and std.info.full_sa_bytes


def test_batches_cover_the_cases(indexes):
    """The generator's own promise, on the batches the count tests use."""
    ix = indexes["std"]
    for n in SIZES:
        pats, cov, want = ix.batch(n)
        assert len(pats) == n == len(want)
        if n >= 511:
            assert cov == {(s, part) for s in SPECIALS for part in ("table", "context", "before")}, n
            _, offs = O.pack_patterns(pats)
            assert set((offs[:-1] & np.uint64(3)).tolist()) == {0, 1, 2, 3}
            assert {len(p) for p in pats} == set(_lengths(ix.K))
            assert (want == 0).sum() > n // 8 and (want == 1).sum() > n // 8 and (want > 1).any()
    assert ix.batch(1)[2].tolist() == [ix.o.count(ix.batch(1)[0][0])]


@pytest.mark.parametrize("n", SIZES)
def test_std_count(indexes, n):
    _check(indexes["std"], n)


@pytest.mark.parametrize("n", SIZES)
def test_fifth_symbol_count(indexes, n):
    _check(indexes["fifth"], n)


@pytest.mark.parametrize("n", SIZES)
def test_acgu_count(indexes, n):
    _check(indexes["acgu"], n)
