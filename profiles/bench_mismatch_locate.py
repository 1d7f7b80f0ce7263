"""bench_mismatch_locate.py — locate within k mismatches: the two-pass kernel against neighbour
enumeration through the exact locate.

Synthetic DNA of n symbols (default 10^8, bench.py's C2 size) built on the device; 10^6
20-mers sampled from the text with 0-2 substitutions applied (pattern q gets q mod 3), the
batch of bench_mismatch.py.  Timed at k = 1 and k = 2, with device events around each call
after a warm-up, alternating the two sides:

  (a) cs_fm_locate_mismatch_device over the whole batch (offsets, positions, distances; the
      output buffers sized beforehand by a sizing call);
  (b) what a caller has without it: every Hamming neighbour over ACGT built on the device
      outside the timed region, with its CSR offsets, then one cs_fm_locate_device over them
      (caller's workspace, limit = n) plus the labelling of each position with its
      neighbour's distance (the per-neighbour counts from the offsets, one repeat), both
      timed.  k = 1 runs on the whole batch (61 strings per pattern); k = 2 on the first
      1/16 of the patterns (1,771 strings each) and its time is scaled by 16 — the output
      says so.

On every timed run the two sides are compared as per-pattern sorted (position, distance) sets.
(a) also reports the neighbours that substitute the terminator, which a caller enumerating
ACGT leaves out; those strings are located separately, outside the timed region, and added to
(b) for the check.

The split of (a) into its phases — sizing traversal, scans with their read-back, emitting
traversal, positions, distances — comes from the measurement twin
cs_fm_locate_mismatch_phases_device (device events inside the call), in runs of their own.

One JSON line per timed run and a summary line go to --out (default profiles/mismatch/); the
summary is also printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import __graft_entry__ as G  # noqa: E402
from bench_mismatch import expand, neighbour_table  # noqa: E402


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
    assert torch.cuda.is_available(), "bench_mismatch_locate.py needs a GPU"
    pkg = G._load_pkg()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    N, B, m = args.n, args.npat, args.m
    assert N < (1 << 30) and B < (1 << 24)  # the check's keys: pattern << 32 | position << 2 | distance
    os.makedirs(args.out, exist_ok=True)
    runs = open(os.path.join(args.out, "mismatch_locate_%s.jsonl" % args.tag), "w")

    def record(**kw):
        runs.write(json.dumps(kw) + "\n")
        runs.flush()

    text = torch.empty(N + 16, dtype=torch.uint8, device=dev)
    pkg.synth_text_device("dna", 42, N - 1, text.data_ptr(), sh)
    g = pkg.FMIndex.build_from_device_text(text.data_ptr(), N, pkg.BuildParams(ssa_stride=32))
    torch.cuda.synchronize()
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

    def keys(offs, pos, dist, npat):
        """Sorted int64 keys pattern << 32 | position << 2 | distance of the first npat patterns."""
        end = int(offs[npat])
        pid = torch.repeat_interleave(torch.arange(npat, device=dev), offs[1:npat + 1] - offs[:npat],
                                      output_size=end)
        return torch.sort((pid << 32) | (pos[:end] << 2) | dist[:end].long())[0]

    class SideA:
        def __init__(self, k):
            self.k = k
            self.offs = torch.empty(B + 1, dtype=torch.int64, device=dev)
            self.total, _ = g.locate_mismatch_device(P.data_ptr(), None, B, k, self.offs.data_ptr(), None, None, 0,
                                                     fixed_m=m, stream=sh)
            self.pos = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)
            self.dist = torch.empty(max(self.total, 1), dtype=torch.uint8, device=dev)

        def __call__(self, phase_ms=None):
            tot, ok = g.locate_mismatch_device(P.data_ptr(), None, B, self.k, self.offs.data_ptr(),
                                               self.pos.data_ptr(), self.dist.data_ptr(), self.total, fixed_m=m,
                                               stream=sh, phase_ms=phase_ms)
            assert ok and tot == self.total

        def keys(self, npat):
            return keys(self.offs, self.pos, self.dist, npat)

    class SideB:
        """One exact locate over the strings nb [npat, T, m] + the labelling with tab's distances."""

        def __init__(self, nb, tab):
            self.npat, self.T = nb.shape[0], nb.shape[1]
            self.nb = nb
            S = self.npat * self.T
            self.S = S
            self.d_offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * m
            self.out_offs = torch.empty(S + 1, dtype=torch.int64, device=dev)
            self.wb = g.workspace_bytes(S)
            self.work = torch.zeros(max(self.wb, 8), dtype=torch.uint8, device=dev)
            self.label = torch.from_numpy(tab[2]).to(dev).to(torch.uint8).repeat(self.npat)  # per string
            self.total, _ = g.locate_device_ws(nb.data_ptr(), self.d_offs.data_ptr(), S, N, self.out_offs.data_ptr(),
                                               None, 0, self.work.data_ptr(), self.wb, stream=sh)
            self.pos = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)
            self.dist = None

        def __call__(self):
            tot, ok = g.locate_device_ws(self.nb.data_ptr(), self.d_offs.data_ptr(), self.S, N,
                                         self.out_offs.data_ptr(), self.pos.data_ptr(), self.total,
                                         self.work.data_ptr(), self.wb, stream=sh)
            assert ok and tot == self.total
            cnt = self.out_offs[1:] - self.out_offs[:-1]
            self.dist = torch.repeat_interleave(self.label, cnt, output_size=self.total)

        def keys(self):
            pat_offs = self.out_offs[::self.T].contiguous()  # a pattern's strings are contiguous
            return keys(pat_offs, self.pos, self.dist, self.npat)

    def dollar_keys(sub, k):
        """The pairs of the neighbours with a terminator substitute (not timed), as keys."""
        tab = neighbour_table(m, k, True)
        step = max(1, (1 << 27) // (len(tab[2]) * m))  # ~128 MB of strings per piece
        out = []
        for lo in range(0, len(sub), step):
            part = sub[lo:lo + step]
            b = SideB(expand(part, lut[part.long()], tab, dev), tab)
            b()
            out.append(b.keys() + (lo << 32))
        return torch.cat(out)

    summary = {"what": "locate within k mismatches: (a) cs_fm_locate_mismatch_device vs (b) neighbour "
                       "enumeration over ACGT through cs_fm_locate_device + distance labels",
               "n": N, "patterns": B, "m": m, "pairs": args.pairs, "warmup": args.warmup,
               "engine": int(info.engine), "prefix_k": int(info.prefix_k), "k": {}}

    for k in (1, 2):
        frac = 1 if k == 1 else args.k2_sample
        nb_pat = B // frac
        sub = P[:nb_pat].contiguous()
        tab = neighbour_table(m, k, False)
        a = SideA(k)
        b = SideB(expand(sub, codes[:nb_pat], tab, dev), tab)
        extra = dollar_keys(sub, k)

        def agree():
            want = torch.sort(torch.cat([b.keys(), extra]))[0]
            return bool(torch.equal(a.keys(nb_pat), want))

        for _ in range(args.warmup):
            a()
            b()
        torch.cuda.synchronize()
        assert agree(), "k = %d: (a) differs from (b) + terminator neighbours" % k
        ta, tb = [], []
        for i in range(args.pairs):  # alternated pairs, checked on every run
            a.pos.fill_(-1)
            ta.append(timed(a))
            tb.append(timed(b) * frac)
            ok = agree()
            record(k=k, pair=i, a_ms=ta[-1], b_ms=tb[-1], b_scaled_by=frac, b_patterns=nb_pat,
                   b_strings=nb_pat * len(tab[2]), equal=ok)
            assert ok, "k = %d pair %d: (a) differs from (b) + terminator neighbours" % (k, i)
        phases = []
        for i in range(args.pairs):  # the split of (a), runs of their own
            ms = []
            a(phase_ms=ms)
            phases.append(ms)
            record(k=k, pair=i, phases=True, size_ms=ms[0], scans_ms=ms[1], emit_ms=ms[2], positions_ms=ms[3],
                   expand_ms=ms[4])
        names = ("size", "scans", "emit", "positions", "expand")
        summary["k"][str(k)] = {
            "a_ms_median": statistics.median(ta), "a_ms_range": [min(ta), max(ta)],
            "b_ms_median": statistics.median(tb), "b_ms_range": [min(tb), max(tb)],
            "b_measured_on_patterns": nb_pat, "b_time_scaled_by": frac,
            "b_strings_per_pattern": int(len(tab[2])), "equal_on_every_run": True,
            "a_beats_b": max(ta) < min(tb), "b_beats_a": max(tb) < min(ta),
            "a_total_pairs": int(a.total), "b_acgt_pairs_measured": int(b.total),
            "terminator_pairs_added_for_the_check": int(len(extra)),
            "a_phase_ms_median": {nm: statistics.median(p[i] for p in phases) for i, nm in enumerate(names)},
            "a_phase_ms_range": {nm: [min(p[i] for p in phases), max(p[i] for p in phases)]
                                 for i, nm in enumerate(names)}}
        del a, b, extra
        torch.cuda.empty_cache()

    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
