"""bench_mismatch_seeded.py — seeded locate within k mismatches against the backtracking locate.

Synthetic DNA of n symbols (default 10^8, bench.py's C2 size; the text of
bench_mismatch_locate.py) built on the device.  Timed with device events around each call after
2 warm-up calls, five alternated pairs in one process:

  (a) cs_fm_locate_mismatch_seeded_device over the whole batch (offsets, positions, distances;
      the output buffers sized beforehand by a sizing call);
  (b) cs_fm_locate_mismatch_device on the same handle, wherever k <= 3.  Where a call of (b)
      over the whole batch would pass 10 s (estimated from 1/64 of the patterns), (b) runs on
      the first 1/4, 1/16 or 1/64 of the patterns and its time is scaled — the output says so.

On every timed run the two sides are compared as per-pattern sorted (position, distance) sets
(over the patterns (b) ran on).

Workloads: bench_mismatch_locate.py's 10^6 20-mers (0-2 substitutions) at k = 1; 10^6 100-mers
and 10^6 150-mers sampled from the text with 0-4 substitutions (pattern q gets q mod 5), at
k = 2 and 3 against (b) and at k = 5 and 8 alone.  For (a) the record holds the candidate count
C and the split into piece search / positions / verify / scan / emit (the measurement twin's
device events, runs of their own).  20-mers at k = 2 and 3 do not fit at 10^6 patterns: their C
is recorded from a sample (sizing calls).  (The committed record mismatch_seeded_c2.jsonl was
made while the verification kernel still had a second form, eight lanes per candidate, and
holds both as "lanes1" and "lanes8", the call's own choice then being lanes8 from m = 64; the
second form lost everywhere and is gone, so "lanes1" is what the call does now.)

One JSON line per timed run and a summary line go to --out (default profiles/mismatch/); the
summary is also printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

B_LIMIT_MS = 10_000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch"))
    ap.add_argument("--tag", default=time.strftime("%Y%m%d_%H%M%S"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mismatch_seeded.py needs a GPU"
    pkg = G._load_pkg()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    N, B = args.n, args.npat
    assert N < (1 << 30) and B < (1 << 24)  # the check's keys: pattern << 36 | position << 4 | distance
    os.makedirs(args.out, exist_ok=True)
    runs = open(os.path.join(args.out, "mismatch_seeded_%s.jsonl" % args.tag), "w")

    def record(**kw):
        runs.write(json.dumps(kw) + "\n")
        runs.flush()

    text = torch.empty(N + 16, dtype=torch.uint8, device=dev)
    pkg.synth_text_device("dna", 42, N - 1, text.data_ptr(), sh)
    g = pkg.FMIndex.build_from_device_text(text.data_ptr(), N, pkg.BuildParams(ssa_stride=32))
    torch.cuda.synchronize()
    info = g.info()
    assert info.text_in_hbm == 1

    lut = torch.zeros(256, dtype=torch.uint8, device=dev)
    lut[torch.tensor(list(b"ACGT"), device=dev)] = torch.arange(4, dtype=torch.uint8, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)

    def patterns(m, nmod, seed):
        """B text m-mers, pattern q with q mod nmod substitutions at distinct random positions."""
        P = torch.empty((B, m), dtype=torch.uint8, device=dev)
        pkg.synth_patterns_device(text.data_ptr(), N, m, 0, B, 4242, P.data_ptr(), None, sh)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        nsub = torch.arange(B, device=dev) % nmod
        where = torch.rand((B, m), generator=gen, device=dev).argsort(dim=1)[:, :nmod - 1]
        shift = torch.randint(1, 4, (B, nmod - 1), generator=gen, device=dev)
        for s in range(nmod - 1):
            rows = torch.nonzero(nsub > s)[:, 0]
            j = where[rows, s]
            P[rows, j] = acgt[(lut[P[rows, j].long()].long() + shift[rows, s]) & 3]
        torch.cuda.synchronize()
        return P

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def keys(offs, pos, dist, npat):
        """Sorted int64 keys pattern << 36 | position << 4 | distance of the first npat patterns."""
        end = int(offs[npat])
        pid = torch.repeat_interleave(torch.arange(npat, device=dev), offs[1:npat + 1] - offs[:npat],
                                      output_size=end)
        return torch.sort((pid << 36) | (pos[:end] << 4) | dist[:end].long())[0]

    class Side:
        """(a) the seeded call (seeded=True) or (b) the backtracking call over the first npat patterns."""

        def __init__(self, P, npat, k, seeded):
            self.P, self.npat, self.k, self.seeded, self.m = P, npat, k, seeded, P.shape[1]
            self.offs = torch.empty(npat + 1, dtype=torch.int64, device=dev)
            self.cand = None
            r = self.call(None, None, 0)
            self.total = r[0]
            self.pos = torch.empty(max(self.total, 1), dtype=torch.int64, device=dev)
            self.dist = torch.empty(max(self.total, 1), dtype=torch.uint8, device=dev)

        def call(self, pos, dist, cap, **kw):
            if self.seeded:
                tot, self.cand, ok = g.locate_mismatch_seeded_device(
                    self.P.data_ptr(), None, self.npat, self.k, self.offs.data_ptr(), pos, dist, cap, fixed_m=self.m,
                    stream=sh, **kw)
            else:
                tot, ok = g.locate_mismatch_device(self.P.data_ptr(), None, self.npat, self.k, self.offs.data_ptr(),
                                                   pos, dist, cap, fixed_m=self.m, stream=sh)
            return tot, ok

        def __call__(self, **kw):
            tot, ok = self.call(self.pos.data_ptr(), self.dist.data_ptr(), self.total, **kw)
            assert ok and tot == self.total

        def keys(self, npat):
            return keys(self.offs, self.pos, self.dist, npat)

    summary = {"what": "locate within k mismatches: (a) cs_fm_locate_mismatch_seeded_device vs "
                       "(b) cs_fm_locate_mismatch_device (k <= 3)",
               "n": N, "patterns": B, "pairs": args.pairs, "warmup": args.warmup, "engine": int(info.engine),
               "prefix_k": int(info.prefix_k), "workloads": {}}
    names = ("pieces", "positions", "verify", "scan", "emit")

    def workload(label, P, k, with_b):
        a = Side(P, B, k, True)
        out = {"m": int(P.shape[1]), "k": k, "a_candidates": int(a.cand), "a_total_pairs": int(a.total)}
        b, frac = None, 1
        if with_b:
            probe = Side(P, B // 64, k, False)
            probe()
            est = timed(probe) * 64
            frac = next(f for f in (1, 4, 16, 64) if est / f < B_LIMIT_MS or f == 64)
            b = probe if frac == 64 else Side(P, B // frac, k, False)
            out.update(b_measured_on_patterns=B // frac, b_time_scaled_by=frac, b_estimate_ms_whole_batch=est)
        nb = B // frac

        def agree():
            return bool(torch.equal(a.keys(nb), b.keys(nb)))

        for _ in range(args.warmup):
            a()
            if b:
                b()
        torch.cuda.synchronize()
        if b:
            assert agree(), "%s: (a) differs from (b)" % label
        ta, tb = [], []
        for i in range(args.pairs):  # alternated pairs, checked on every run
            a.pos.fill_(-1)
            ta.append(timed(a))
            ok = None
            if b:
                b.pos.fill_(-1)
                tb.append(timed(b) * frac)
                ok = agree()
                assert ok, "%s pair %d: (a) differs from (b)" % (label, i)
            record(workload=label, pair=i, a_ms=ta[-1], b_ms=tb[-1] if b else None, b_scaled_by=frac, equal=ok)
        out.update(a_ms_median=statistics.median(ta), a_ms_range=[min(ta), max(ta)])
        if b:
            out.update(b_ms_median=statistics.median(tb), b_ms_range=[min(tb), max(tb)], equal_on_every_run=True,
                       a_beats_b=max(ta) < min(tb), b_beats_a=max(tb) < min(ta))
        phases = []
        for i in range(args.pairs):  # the split of (a), runs of their own
            ms = []
            a(phase_ms=ms)
            phases.append(ms)
            record(workload=label, pair=i, phases=True, **{nm + "_ms": ms[j] for j, nm in enumerate(names)})
        out["a_phase_ms_median"] = {nm: statistics.median(p[j] for p in phases) for j, nm in enumerate(names)}
        out["a_phase_ms_range"] = {nm: [min(p[j] for p in phases), max(p[j] for p in phases)]
                                   for j, nm in enumerate(names)}
        summary["workloads"][label] = out
        record(workload=label, result=out)
        del a, b
        torch.cuda.empty_cache()

    P20 = patterns(20, 3, 7)
    workload("m20_k1", P20, 1, True)
    # 20-mers at k >= 2: the candidate count alone rules the whole batch out; C from a sample
    for k, ns in ((2, 1000), (3, 200)):
        s = Side(P20, ns, k, True)
        summary["workloads"]["m20_k%d_sample" % k] = {
            "m": 20, "k": k, "sample_patterns": ns, "a_candidates": int(s.cand), "a_total_pairs": int(s.total),
            "a_candidates_scaled_to_batch": int(s.cand) * (B // ns),
            "a_temporaries_bytes_scaled_to_batch": int(s.cand) * (B // ns) * 17}
        del s
    del P20
    for m in (100, 150):
        P = patterns(m, 5, 11 + m)
        for k in (2, 3):
            workload("m%d_k%d" % (m, k), P, k, True)
        for k in (5, 8):
            workload("m%d_k%d" % (m, k), P, k, False)
        del P
    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
