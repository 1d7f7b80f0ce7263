"""bench_mismatch_best.py — best stratum: the rounds of cs_fm_best_mismatch_device against the
full histogram plus a reduction.

The index and the batch are bench_mismatch.py's: synthetic DNA of n symbols (default 10^8) built
on the device; 10^6 20-mers sampled from the text with 0-2 substitutions applied (pattern q gets
q mod 3).  Timed with device events around each call, after 2 warm-up calls per side, in five
alternated pairs, at k = 1, 2, 3:

  (a) cs_fm_best_mismatch_device: (best_dist, best_count) per pattern;
  (b) what a caller had: cs_fm_count_mismatch_device at the same k, then the reduction of each
      histogram row to its first non-zero column and that column's value, on the device.

(a) is asserted equal to (b), element for element, after every run.  Each record also holds how
many patterns each round of (a) received (round d: the patterns with no hit below d, from the
result itself).  The records are appended to --out (default
profiles/mismatch/mismatch_best_c2.jsonl), a summary record last; the summary is also printed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--m", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch", "mismatch_best_c2.jsonl"))
    ap.add_argument("--tag", default=time.strftime("%Y%m%d_%H%M%S"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mismatch_best.py needs a GPU"
    pkg = G._load_pkg()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    N, B, m = args.n, args.npat, args.m
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    runs = open(args.out, "a")

    def record(**kw):
        runs.write(json.dumps(dict(kw, tag=args.tag)) + "\n")
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
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    none = torch.tensor(pkg.CS_MM_NONE, dtype=torch.uint8, device=dev)
    summary = {"what": "best stratum: (a) cs_fm_best_mismatch_device vs (b) cs_fm_count_mismatch_device + "
                       "first-non-zero-column reduction on the device",
               "n": N, "patterns": B, "m": m, "pairs": args.pairs, "warmup": args.warmup,
               "engine": int(info.engine), "prefix_k": int(info.prefix_k), "build_s": build_s, "k": {}}

    for k in (1, 2, 3):
        a_dist = torch.empty(B, dtype=torch.uint8, device=dev)
        a_cnt = torch.empty(B, dtype=torch.int64, device=dev)
        hist = torch.empty((B, k + 1), dtype=torch.int64, device=dev)
        b_out = {}

        def fa():
            g.best_mismatch_device(P.data_ptr(), None, B, k, a_dist.data_ptr(), a_cnt.data_ptr(), fixed_m=m,
                                   stream=sh)

        def fb():
            g.count_mismatch_device(P.data_ptr(), None, B, k, hist.data_ptr(), fixed_m=m, stream=sh)
            hit = hist != 0
            first = hit.to(torch.int32).argmax(dim=1)
            found = hit.any(dim=1)
            b_out["dist"] = torch.where(found, first.to(torch.uint8), none)
            b_out["cnt"] = torch.where(found, hist.gather(1, first[:, None])[:, 0], torch.zeros_like(a_cnt))

        def check():
            assert torch.equal(a_dist, b_out["dist"]) and torch.equal(a_cnt, b_out["cnt"]), \
                "k = %d: (a) differs from (b)" % k

        def poison():  # so that a run that wrote nothing cannot pass on the last run's values
            a_dist.fill_(0xEE)
            a_cnt.fill_(-1)

        for _ in range(args.warmup):
            poison()
            fa()
            fb()
            torch.cuda.synchronize()
            check()
        # round d of (a) receives the patterns with no hit below d
        received = [B] + [int((a_dist >= d).sum().item()) for d in range(1, k + 1)]
        resolved = [int((a_dist == d).sum().item()) for d in range(k + 1)] + [int((a_dist == none).sum().item())]
        ta, tb = [], []
        for i in range(args.pairs):  # alternated pairs
            poison()
            torch.cuda.synchronize()
            ta.append(timed(fa))
            tb.append(timed(fb))
            check()
            record(k=k, pair=i, a_ms=ta[-1], b_ms=tb[-1], round_received=received)
        summary["k"][str(k)] = {
            "a_ms_median": statistics.median(ta), "a_ms_range": [min(ta), max(ta)],
            "b_ms_median": statistics.median(tb), "b_ms_range": [min(tb), max(tb)],
            "equal_on_every_run": True, "a_beats_b": max(ta) < min(tb),
            "round_received": received, "resolved_at_0..k_then_none": resolved}
    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
