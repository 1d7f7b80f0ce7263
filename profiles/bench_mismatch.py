"""bench_mismatch.py — count within k mismatches: the backtracking kernel against neighbour
enumeration.

Synthetic DNA of n symbols (default 10^8, bench.py's C2 size) built on the device; 10^6
20-mers sampled from the text with 0-2 substitutions applied (pattern q gets q mod 3).  Timed,
with device events around each call after a warm-up, alternating the two sides:

  (a) cs_fm_count_mismatch_device at k = 1, 2, 3 over the whole batch;
  (b) the path a caller has today: every Hamming neighbour over ACGT built on the device
      outside the timed region, then one cs_fm_count_device over the expanded batch (with a
      caller's workspace) plus the reduction of its counts to histograms, both timed.
      k = 1 runs on the whole batch (61 strings per pattern); k = 2 on the first 1/16 of the
      patterns (1,771 strings each) and its time is scaled by 16 — the output says so.

Before any time is reported (a) is checked against (b) for equality.  (a) also counts the
neighbours that substitute the terminator, which a caller enumerating ACGT leaves out; those
strings are counted separately, outside the timed region, and added to (b) for the check.

The divergence figure: (a) timed again on the same patterns grouped by their number of
substitutions, so that a wave's lanes walk trees of one class.

One JSON line per timed run and a summary line go to --out (default profiles/mismatch/); the
summary is also printed.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

DOLLAR = 3  # a substitute choice: 0-2 = the r-th other base, 3 = the terminator


def neighbour_table(m, k, with_dollar):
    """-> (pos [T, k], choice [T, k], dist [T]) of every neighbour at distance 0..k: the
    substituted positions (padded with position 0 / choice -1) and the choice at each.
    with_dollar: only the neighbours with at least one terminator substitute."""
    pos, ch, dist = [], [], []
    for d in range(k + 1):
        for p in itertools.combinations(range(m), d):
            for c in itertools.product(range(4 if with_dollar else 3), repeat=d):
                if with_dollar and DOLLAR not in c:
                    continue
                pos.append(list(p) + [0] * (k - d))
                ch.append(list(c) + [-1] * (k - d))
                dist.append(d)
    return (np.array(pos, np.int64).reshape(len(dist), k), np.array(ch, np.int64).reshape(len(dist), k),
            np.array(dist, np.int64))


def expand(P, codes, tab, dev):
    """The neighbours of every pattern: uint8 [B, T, m] on the device."""
    pos, ch, _ = tab
    B, m = P.shape
    T = len(pos)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    out = P[:, None, :].repeat(1, T, 1)
    tix = torch.arange(T, device=dev)
    for s in range(pos.shape[1]):
        use = np.nonzero(ch[:, s] >= 0)[0]
        if not len(use):
            continue
        j = torch.from_numpy(pos[use, s]).to(dev)
        c = torch.from_numpy(ch[use, s]).to(dev)
        base = acgt[((codes[:, j].long() + 1 + c[None, :]) & 3)]
        val = torch.where(c[None, :] == DOLLAR, torch.tensor(ord("$"), dtype=torch.uint8, device=dev), base)
        out[:, tix[use], j] = val
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k2-sample", type=int, default=16, help="(b) at k = 2 runs on 1/this of the patterns")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch"))
    ap.add_argument("--tag", default=time.strftime("%Y%m%d_%H%M%S"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mismatch.py needs a GPU"
    pkg = G._load_pkg()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    N, B, m = args.n, args.npat, args.m
    os.makedirs(args.out, exist_ok=True)
    runs = open(os.path.join(args.out, "mismatch_%s.jsonl" % args.tag), "w")

    def record(**kw):
        runs.write(json.dumps(kw) + "\n")
        runs.flush()

    text = torch.empty(N + 16, dtype=torch.uint8, device=dev)
    pkg.synth_text_device("dna", 42, N - 1, text.data_ptr(), sh)
    t0 = time.perf_counter()
    g = pkg.FMIndex.build_from_device_text(text.data_ptr(), N, pkg.BuildParams(ssa_stride=32))
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    info = g.info()

    # the patterns: text 20-mers, pattern q with q mod 3 substitutions at random positions
    P = torch.empty((B, m), dtype=torch.uint8, device=dev)
    pkg.synth_patterns_device(text.data_ptr(), N, m, 0, B, 4242, P.data_ptr(), None, sh)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    lut[torch.tensor(list(b"ACGT"), device=dev)] = torch.arange(4, dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    nsub = torch.arange(B, device=dev) % 3
    where = torch.rand((B, m), generator=gen, device=dev).argsort(dim=1)[:, :2]  # two distinct positions
    shift = torch.randint(1, 4, (B, 2), generator=gen, device=dev)
    for s in range(2):
        rows = torch.nonzero(nsub > s)[:, 0]
        j = where[rows, s]
        P[rows, j] = acgt[(lut[P[rows, j].long()].long() + shift[rows, s]) & 3]
    codes = lut[P.long()]
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def run_a(pats, npat, k):
        h = torch.empty((npat, k + 1), dtype=torch.int64, device=dev)
        return h, lambda: g.count_mismatch_device(pats.data_ptr(), None, npat, k, h.data_ptr(), fixed_m=m, stream=sh)

    def run_b(nb, tab):
        """(b): one exact count over the expanded batch + the reduction to histograms."""
        npat, T = nb.shape[0], nb.shape[1]
        k = tab[0].shape[1]
        cnt = torch.empty(npat * T, dtype=torch.int64, device=dev)
        wb = g.workspace_bytes(npat * T)
        work = torch.zeros(max(wb, 8), dtype=torch.uint8, device=dev)
        hist = torch.empty((npat, k + 1), dtype=torch.int64, device=dev)
        d = tab[2]
        seg = [(int(np.nonzero(d == x)[0][0]), int(np.nonzero(d == x)[0][-1]) + 1) for x in range(k + 1)]

        def fn():
            g.count_device_ws(nb.data_ptr(), None, npat * T, cnt.data_ptr(), work.data_ptr(), wb, fixed_m=m,
                              stream=sh)
            c = cnt.view(npat, T)
            for x, (lo, hi) in enumerate(seg):
                hist[:, x] = c[:, lo:hi].sum(dim=1)
        return hist, fn

    def dollar_hist(sub, k):
        """hist of the neighbours with a terminator substitute (not timed)."""
        tab = neighbour_table(m, k, True)
        out = torch.zeros((len(sub), k + 1), dtype=torch.int64, device=dev)
        step = max(1, (1 << 27) // (len(tab[2]) * m))  # ~128 MB of strings per piece
        dd = torch.from_numpy(tab[2]).to(dev)
        for lo in range(0, len(sub), step):
            nb = expand(sub[lo:lo + step], codes_of(sub[lo:lo + step]), tab, dev)
            npat, T = nb.shape[0], nb.shape[1]
            cnt = torch.empty(npat * T, dtype=torch.int64, device=dev)
            g.count_device_ws(nb.data_ptr(), None, npat * T, cnt.data_ptr(), 0, 0, fixed_m=m, stream=sh)
            out[lo:lo + npat].index_add_(1, dd, cnt.view(npat, T))
        return out

    def codes_of(p):
        return lut[p.long()]

    summary = {"what": "count within k mismatches: (a) cs_fm_count_mismatch_device vs (b) neighbour "
                       "enumeration over ACGT through cs_fm_count_device + reduction",
               "n": N, "patterns": B, "m": m, "pairs": args.pairs, "warmup": args.warmup,
               "engine": int(info.engine), "prefix_k": int(info.prefix_k), "build_s": build_s, "k": {}}

    for k in (1, 2):
        frac = 1 if k == 1 else args.k2_sample
        nb_pat = B // frac
        sub = P[:nb_pat].contiguous()
        tab = neighbour_table(m, k, False)
        nb = expand(sub, codes[:nb_pat], tab, dev)
        ha, fa = run_a(P, B, k)
        hb, fb = run_b(nb, tab)
        fa()
        fb()
        torch.cuda.synchronize()
        want = hb + dollar_hist(sub, k)
        equal = bool(torch.equal(ha[:nb_pat], want))
        acgt_equal = bool(torch.equal(ha[:nb_pat], hb))
        assert equal, "k = %d: (a) differs from (b) + terminator neighbours" % k
        for _ in range(args.warmup):
            fa()
            fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for i in range(args.pairs):  # alternated pairs
            ta.append(timed(fa))
            tb.append(timed(fb) * frac)
            record(k=k, pair=i, a_ms=ta[-1], b_ms=tb[-1], b_scaled_by=frac, b_patterns=nb_pat,
                   b_strings=nb_pat * len(tab[2]))
        summary["k"][str(k)] = {
            "a_ms_median": statistics.median(ta), "a_ms_range": [min(ta), max(ta)],
            "b_ms_median": statistics.median(tb), "b_ms_range": [min(tb), max(tb)],
            "b_measured_on_patterns": nb_pat, "b_time_scaled_by": frac,
            "b_strings_per_pattern": int(len(tab[2])), "equal_with_terminator_neighbours": equal,
            "equal_to_acgt_enumeration_alone": acgt_equal,
            "a_beats_b": max(ta) < min(tb), "hist_column_sums": [int(v) for v in ha.sum(dim=0).tolist()]}
        del nb, hb, want
        torch.cuda.empty_cache()

    # k = 3: (a) only
    ha, fa = run_a(P, B, 3)
    for _ in range(args.warmup):
        fa()
    ta = [timed(fa) for _ in range(args.pairs)]
    for i, t in enumerate(ta):
        record(k=3, pair=i, a_ms=t)
    summary["k"]["3"] = {"a_ms_median": statistics.median(ta), "a_ms_range": [min(ta), max(ta)],
                         "hist_column_sums": [int(v) for v in ha.sum(dim=0).tolist()]}

    # divergence: the same patterns grouped by their number of substitutions
    order = torch.argsort(nsub, stable=True)
    grouped = P[order].contiguous()
    div = {}
    for k in (1, 2, 3):
        hm, fm_ = run_a(P, B, k)
        hg, fg = run_a(grouped, B, k)
        fm_()
        fg()
        torch.cuda.synchronize()
        assert torch.equal(hm[order], hg)
        tm, tg = [], []
        for i in range(args.pairs):
            tm.append(timed(fm_))
            tg.append(timed(fg))
            record(k=k, pair=i, divergence=True, mixed_ms=tm[-1], grouped_ms=tg[-1])
        div[str(k)] = {"mixed_ms_median": statistics.median(tm), "mixed_ms_range": [min(tm), max(tm)],
                       "grouped_ms_median": statistics.median(tg), "grouped_ms_range": [min(tg), max(tg)]}
    summary["divergence"] = div
    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
