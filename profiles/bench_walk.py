"""bench_walk.py — the callers of locate's LF walk (csrc/fm_walk.hpp) at a size no bench.py leg
has: an index without the full suffix array that builds in seconds.

Synthetic DNA of n symbols (default 10^8) built on the device with CS_FM_FULL_SA=0 (walk lines
with text-position marks).  Timed with device events around each call, after --warmup calls,
--pairs times each, the forms taken in turn inside every round:

  count_long     cs_fm_count_device of 10^6 text 64-mers under CS_Q_LONG (k_count_long's
                 walk-verify forms);
  locate_one     the one-call cs_fm_locate_device of 10^6 text 20-mers (the search's
                 lockstep walks, k_locate_emit's listing, k_locate_walks);
  ranges         phase 1 of the two-phase locate of the same 20-mers (it synchronises);
  walk_default   phase 2 under the default flags (k_walk_fused, k_walk_fused_wide),
  walk_rows      CS_QT_WALK_ROWS (k_expand_rows + k_walk_short),
  walk_persist   CS_QT_WALK_PERSISTENT (k_expand_rows + k_walk_lines).

Before any time is reported the three selectors' positions and LF steps are checked equal
element by element, and the one call's offsets and positions equal to the two phases'.  The
summary carries a digest of every output, so two builds of the library can be compared.

One JSON line per timed call and a summary line go to --out (default profiles/walk/); the
summary is also printed.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


def digest(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk"))
    ap.add_argument("--tag", default=time.strftime("%Y%m%d_%H%M%S"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_walk.py needs a GPU"
    pkg = G._load_pkg()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sh = stream.cuda_stream
    N, B = args.n, args.npat
    os.makedirs(args.out, exist_ok=True)
    runs = open(os.path.join(args.out, "walk_%s.jsonl" % args.tag), "w")

    def record(**kw):
        runs.write(json.dumps(kw) + "\n")
        runs.flush()

    text = torch.empty(N + 16, dtype=torch.uint8, device=dev)
    pkg.synth_text_device("dna", 42, N - 1, text.data_ptr(), sh)
    t0 = time.perf_counter()
    with pkg.build_options({"CS_FM_FULL_SA": "0"}):
        g = pkg.FMIndex.build_from_device_text(text.data_ptr(), N, pkg.BuildParams(ssa_stride=32))
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    info = g.info()
    assert info.walk_marks == 2, "the index has no walk lines with text-position marks"

    def patterns(m, seed):
        p = torch.empty((B, m), dtype=torch.uint8, device=dev)
        pkg.synth_patterns_device(text.data_ptr(), N, m, 0, B, seed, p.data_ptr(), None, sh)
        return p, torch.arange(B + 1, dtype=torch.int64, device=dev) * m

    P64, _ = patterns(64, 4242)
    P20, O20 = patterns(20, 4243)
    limit = 100000
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the two phases once, for the sizes and the records the walks take
    sp = torch.zeros(B, dtype=torch.int64, device=dev)
    oo = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    total = g.locate_ranges_device(P20.data_ptr(), O20.data_ptr(), B, limit, sp.data_ptr(), oo.data_ptr(), sh)
    sels = {"walk_default": 0, "walk_rows": pkg.QT_WALK_ROWS, "walk_persist": pkg.QT_WALK_PERSISTENT}
    pos = {k: torch.full((total,), -1, dtype=torch.int64, device=dev) for k in sels}
    steps = {k: torch.full((total,), -1, dtype=torch.int64, device=dev) for k in sels}
    for k, f in sels.items():
        g.locate_walk_steps_device(sp.data_ptr(), oo.data_ptr(), B, total, steps[k].data_ptr(), sh, flags=f)
        g.locate_walk_device(sp.data_ptr(), oo.data_ptr(), B, total, pos[k].data_ptr(), sh, flags=f)
    torch.cuda.synchronize()
    for k in sels:
        assert torch.equal(pos[k], pos["walk_default"]), "positions differ under " + k
        assert torch.equal(steps[k], steps["walk_default"]), "steps differ under " + k
    oo1 = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    pos1 = torch.full((total,), -1, dtype=torch.int64, device=dev)
    cnt = torch.empty(B, dtype=torch.int64, device=dev)

    def f_count():
        g.count_device_ex(P64.data_ptr(), None, B, cnt.data_ptr(), flags=pkg.Q_LONG, fixed_m=64, stream=sh)

    def f_one():
        tot, ok = g.locate_device(P20.data_ptr(), O20.data_ptr(), B, limit, oo1.data_ptr(), pos1.data_ptr(), total,
                                  stream=sh)
        assert ok and tot == total

    def f_ranges():
        g.locate_ranges_device(P20.data_ptr(), O20.data_ptr(), B, limit, sp.data_ptr(), oo.data_ptr(), sh)

    forms = {"count_long": f_count, "locate_one": f_one, "ranges": f_ranges}
    for k, f in sels.items():
        forms[k] = (lambda k=k, f=f: g.locate_walk_device(sp.data_ptr(), oo.data_ptr(), B, total,
                                                           pos[k].data_ptr(), sh, sync=False, flags=f))
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    g.locate_check(sh)
    assert torch.equal(oo1, oo) and torch.equal(pos1, pos["walk_default"]), "one call differs from the two phases"
    assert int(cnt.min()) >= 1, "a text 64-mer counted 0"
    times = {k: [] for k in forms}
    for i in range(args.pairs):
        for k, fn in forms.items():
            times[k].append(timed(fn))
            record(form=k, round=i, ms=times[k][-1])
    g.locate_check(sh)
    summary = {"what": "the walk's callers on an index without the full suffix array",
               "n": N, "patterns": B, "rounds": args.pairs, "warmup": args.warmup, "build_s": build_s,
               "position_stride": int(info.position_stride), "reported_rows": int(total),
               "mean_steps": float(steps["walk_default"].double().mean()),
               "digest": {"count_long": digest(cnt), "offsets": digest(oo), "positions": digest(pos["walk_default"]),
                          "steps": digest(steps["walk_default"])},
               "ms": {k: {"median": statistics.median(v), "range": [min(v), max(v)]} for k, v in times.items()}}
    record(summary=summary)
    runs.close()
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
