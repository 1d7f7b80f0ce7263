"""bench_mismatch_best_locate.py — best-stratum locate: cs_fm_locate_best_mismatch_device against
the two routes a caller had before it.

The index and the batch are bench_mismatch.py's: synthetic DNA of n symbols (default 10^8) built
on the device; 10^6 20-mers sampled from the text with 0-2 substitutions applied (pattern q gets
q mod 3).  Timed with device events around each side, after 2 warm-up calls per side, in five
alternated pairs per comparison, at k = 1, 2, 3, every output sized beforehand:

  (a)  cs_fm_locate_best_mismatch_device: best_dist, offsets and the positions of the stratum;
  (b1) cs_fm_locate_mismatch_device at the same k, then a device-side filter of its pairs to each
       pattern's smallest distance (segment minimum, mask, compaction, offsets);
  (b2) cs_fm_best_mismatch_device, a device gather of the patterns by distance, one
       cs_fm_locate_mismatch_device per non-empty group at k = d, and the scatter of the groups'
       positions back into batch order — everything inside the timed region.

(a) is asserted equal to both baselines after every run: the distances element for element, the
positions as per-pattern sorted sets.  The records are appended to --out (default
profiles/mismatch/mismatch_best_locate_c2.jsonl), a summary record last; the summary is also
printed.
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
    ap.add_argument("--ks", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch", "mismatch_best_locate_c2.jsonl"))
    ap.add_argument("--tag", default=time.strftime("%Y%m%d_%H%M%S"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mismatch_best_locate.py needs a GPU"
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

    ar = torch.arange(B, device=dev)

    def keys(oo, pos):
        """The result as one sorted int64 vector: pattern * N + position."""
        own = torch.repeat_interleave(ar, oo[1:] - oo[:-1])
        return (own * N + pos).sort().values

    summary = {"what": "best-stratum locate: (a) cs_fm_locate_best_mismatch_device vs (b1) "
                       "cs_fm_locate_mismatch_device + device filter to the minimum distance and (b2) "
                       "cs_fm_best_mismatch_device + gather by distance + one cs_fm_locate_mismatch_device per "
                       "group + scatter into batch order",
               "n": N, "patterns": B, "m": m, "pairs": args.pairs, "warmup": args.warmup,
               "engine": int(info.engine), "prefix_k": int(info.prefix_k), "build_s": build_s, "k": {}}

    for k in [int(x) for x in args.ks.split(",")]:
        # ---- sizes, beforehand ----
        a_dist = torch.empty(B, dtype=torch.uint8, device=dev)
        a_oo = torch.empty(B + 1, dtype=torch.int64, device=dev)
        tot_a, _ = g.locate_best_mismatch_device(P.data_ptr(), None, B, k, a_dist.data_ptr(), a_oo.data_ptr(), None,
                                                 0, fixed_m=m, stream=sh)
        a_pos = torch.empty(max(tot_a, 1), dtype=torch.int64, device=dev)
        l_oo = torch.empty(B + 1, dtype=torch.int64, device=dev)
        tot_l, _ = g.locate_mismatch_device(P.data_ptr(), None, B, k, l_oo.data_ptr(), None, None, 0, fixed_m=m,
                                            stream=sh)
        l_pos = torch.empty(max(tot_l, 1), dtype=torch.int64, device=dev)
        l_dist = torch.empty(max(tot_l, 1), dtype=torch.uint8, device=dev)
        # (b2)'s buffers: the groups' outputs one after the other (their totals sum to tot_a: a
        # pattern of group d has no pair below d)
        c_dist = torch.empty(B, dtype=torch.uint8, device=dev)
        c_cnt = torch.empty(B, dtype=torch.int64, device=dev)
        g_pos = torch.empty(max(tot_a, 1), dtype=torch.int64, device=dev)
        g_dd = torch.empty(max(tot_a, 1), dtype=torch.uint8, device=dev)
        b1, b2 = {}, {}

        def fa():
            t, ok = g.locate_best_mismatch_device(P.data_ptr(), None, B, k, a_dist.data_ptr(), a_oo.data_ptr(),
                                                  a_pos.data_ptr(), tot_a, fixed_m=m, stream=sh)
            assert ok and t == tot_a

        def fb1():
            t, ok = g.locate_mismatch_device(P.data_ptr(), None, B, k, l_oo.data_ptr(), l_pos.data_ptr(),
                                             l_dist.data_ptr(), tot_l, fixed_m=m, stream=sh)
            assert ok and t == tot_l
            own = torch.repeat_interleave(ar, l_oo[1:] - l_oo[:-1])
            dd = l_dist[:tot_l].to(torch.int32)
            dmin = torch.full((B,), pkg.CS_MM_NONE, dtype=torch.int32, device=dev)
            dmin.scatter_reduce_(0, own, dd, "amin")
            keep = dd == dmin[own]
            dmin = dmin.to(torch.uint8)
            sizes = torch.zeros(B, dtype=torch.int64, device=dev)
            sizes.scatter_add_(0, own, keep.to(torch.int64))
            b1["dist"] = dmin
            b1["oo"] = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
            b1["pos"] = l_pos[:tot_l][keep]

        def fb2():
            g.best_mismatch_device(P.data_ptr(), None, B, k, c_dist.data_ptr(), c_cnt.data_ptr(), fixed_m=m,
                                   stream=sh)
            sizes = torch.zeros(B, dtype=torch.int64, device=dev)
            groups, used = [], 0
            for d in range(k + 1):
                idx = torch.nonzero(c_dist == d)[:, 0]
                if not len(idx):
                    continue
                Pd = P[idx].contiguous()
                oo = torch.empty(len(idx) + 1, dtype=torch.int64, device=dev)
                t, ok = g.locate_mismatch_device(Pd.data_ptr(), None, len(idx), d, oo.data_ptr(),
                                                 g_pos[used:].data_ptr(), g_dd[used:].data_ptr(), tot_a - used,
                                                 fixed_m=m, stream=sh)
                assert ok
                sizes[idx] = oo[1:] - oo[:-1]
                groups.append((idx, oo, used, t))
                used += t
            off = torch.cat([sizes.new_zeros(1), sizes.cumsum(0)])
            out = torch.empty(max(used, 1), dtype=torch.int64, device=dev)
            for idx, oo, at, t in groups:  # the scatter back into batch order
                own = torch.repeat_interleave(torch.arange(len(idx), device=dev), oo[1:] - oo[:-1])
                dest = off[idx][own] + (torch.arange(t, device=dev) - oo[own])
                out[dest] = g_pos[at:at + t]
            b2["dist"] = c_dist
            b2["oo"] = off
            b2["pos"] = out[:used]

        def check(b, name):
            assert torch.equal(a_dist, b["dist"]), "k = %d: (a)'s distances differ from (%s)'s" % (k, name)
            assert torch.equal(a_oo, b["oo"]), "k = %d: (a)'s offsets differ from (%s)'s" % (k, name)
            assert torch.equal(keys(a_oo, a_pos[:tot_a]), keys(b["oo"], b["pos"])), \
                "k = %d: (a)'s positions differ from (%s)'s" % (k, name)

        def poison():  # so that a run that wrote nothing cannot pass on the last run's values
            a_dist.fill_(0xEE)
            a_oo.fill_(-1)
            a_pos.fill_(-1)

        for _ in range(args.warmup):
            poison()
            fa()
            fb1()
            fb2()
            torch.cuda.synchronize()
            check(b1, "b1")
            check(b2, "b2")
        none = pkg.CS_MM_NONE
        resolved = [int((a_dist == d).sum().item()) for d in range(k + 1)] + [int((a_dist == none).sum().item())]
        res = {}
        for name, fb, b in (("b1", fb1, b1), ("b2", fb2, b2)):
            ta, tb = [], []
            for i in range(args.pairs):  # alternated pairs
                poison()
                torch.cuda.synchronize()
                ta.append(timed(fa))
                tb.append(timed(fb))
                check(b, name)
                record(k=k, against=name, pair=i, a_ms=ta[-1], b_ms=tb[-1])
            res[name] = {"a_ms_median": statistics.median(ta), "a_ms_range": [min(ta), max(ta)],
                         "b_ms_median": statistics.median(tb), "b_ms_range": [min(tb), max(tb)],
                         "equal_on_every_run": True, "a_beats_b": max(ta) < min(tb)}
        # the sizing half of (a) alone (cap = 0): the rounds, the scans and the read-back
        ts = []
        for i in range(args.pairs):
            ts.append(timed(lambda: g.locate_best_mismatch_device(P.data_ptr(), None, B, k, a_dist.data_ptr(),
                                                                  a_oo.data_ptr(), None, 0, fixed_m=m, stream=sh)))
        res["a_sizing_only_ms_median"] = statistics.median(ts)
        res["a_sizing_only_ms_range"] = [min(ts), max(ts)]
        res["best_stratum_positions"] = tot_a
        res["pairs_within_k"] = tot_l
        res["resolved_at_0..k_then_none"] = resolved
        record(k=k, result=res)
        summary["k"][str(k)] = res
    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
