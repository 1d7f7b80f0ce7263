"""bench.py's stdout line: the driver keeps only the tail of the run's
output, so the one JSON line must hold the headline in <= 4 KB and parse on its own; the
legs go to the --legs-out file and stderr.  CPU only: compact_line() is fed the full result
of a real round-3 C4 run (profiles/r03/bench_c4_r03z.json, every leg present, 46 KB) and an
inflated synthetic one."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = os.path.join(ROOT, "profiles", "r03", "bench_c4_r03z.json")
REQUIRED = ("metric", "value", "unit", "n_gpus", "ranks_seen", "steps", "warmup", "ms_per_step",
            "dtype", "config", "roofline", "cpu_baseline", "p50_us", "locate")


def _bench():
    import bench
    return bench


def _full():
    with open(FULL) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def test_full_result_compacts_under_4k():
    b = _bench()
    res = _full()
    assert len(json.dumps(res)) > 40000 and len(res["legs"]) > 20  # the round-3 line
    line = b.compact_line(res, "gpurun_out/bench_full_n1_x.json")
    assert len(line.encode()) <= 4096
    got = json.loads(line)
    for k in REQUIRED:
        assert k in got, k
    assert got["value"] == float("%.6g" % res["value"])
    assert got["ms_per_step"] == res["ms_per_step"]
    rf = got["roofline"]
    for k in ("frac", "achieved", "alg_bytes_per_launch", "traffic", "kernel_ms_mean",
              "frac_of_random_access_ceiling"):
        assert k in rf, k
    assert abs(rf["frac"] - res["roofline"]["frac"]) <= 1e-3 * res["roofline"]["frac"]
    cb = got["cpu_baseline"]
    for k in ("value", "kind", "cores_used", "host_cores", "matches_gpu"):
        assert k in cb, k
    assert set(got["locate"]) == {"patterns_per_s", "frac"}
    assert "legs" not in got and got["legs_file"].endswith(".json")


def test_inflated_result_still_fits():
    # every optional field at its largest: long leg-error list, long strings everywhere
    b = _bench()
    res = copy.deepcopy(_full())
    res["leg_errors"] = {"leg%02d" % i: "RuntimeError: " + "x" * 500 for i in range(40)}
    res["config"]["engine"] = "e" * 3000
    res["config"]["workload"] = "w" * 300
    res["cpu_baseline"]["sample"] = "s" * 5000
    res["gather_verified"] = True
    line = b.compact_line(res, "gpurun_out/" + "f" * 300 + ".json")
    assert len(line.encode()) <= 4096
    got = json.loads(line)
    assert got["value"] and got["roofline"]["frac"] and got["gather_verified"] is True


def test_plain_result_compacts_to_the_headline():
    # a plain run (no --full) carries no roofline, CPU baseline, p50 or legs: the line is the
    # contract's fields, the config and the index's size
    b = _bench()
    full = _full()
    res = {k: v for k, v in full.items()
           if k not in ("roofline", "cpu_baseline", "cpu_port", "cpu_locate", "cpu_fast", "locate", "legs")
           and not k.startswith(("p50", "p95", "p99", "max_us"))}
    got = json.loads(b.compact_line(res, None))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "steps", "warmup", "ms_per_step",
              "config"):
        assert k in got, k
    assert got["ms_per_step"] == full["ms_per_step"] and got["value"] == float("%.6g" % full["value"])
    for k in ("roofline", "cpu_baseline", "p50_us", "locate", "legs_file"):
        assert k not in got, k


def test_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: float64 files; every count when they fit the cap, else the counts at a
    fixed sample of positions; the summary covers the whole output either way."""
    import numpy as np
    b = _bench()
    c = (np.arange(100_003, dtype=np.int64) * 7919) % 1000
    c[5] = 2 ** 40 + 1  # exact in float64, not in float32
    b.dump_outputs(str(tmp_path / "a"), c)
    got = np.load(tmp_path / "a" / "counts.npy")
    assert got.dtype == np.float64 and np.array_equal(got, c.astype(np.float64))
    s = np.load(tmp_path / "a" / "counts_summary.npy")
    assert s.dtype == np.float64 and s.tolist() == [c.size, c.sum(), (c >= 1).sum(), c.max()]
    # too large to write whole: the sample, identical from call to call, within the cap
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 256 << 10)
    monkeypatch.setattr(b, "DUMP_SAMPLE", 20_000)
    ix = b.dump_sample_index(c.size, 20_000)
    assert ix.size == 20_000 and int(ix.max()) < c.size and np.array_equal(ix, b.dump_sample_index(c.size, 20_000))
    assert len(set(ix.tolist())) > 15_000  # spread over the output, not a prefix
    b.dump_outputs(str(tmp_path / "b"), c)
    got = np.load(tmp_path / "b" / "counts.npy")
    assert got.dtype == np.float64 and np.array_equal(got, c[ix.astype(np.int64)].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "b" / "counts_summary.npy"), s)
    files = list((tmp_path / "b").iterdir())
    assert sum(f.stat().st_size for f in files) <= 256 << 10 and all(f.suffix == ".npy" for f in files)


def test_only_mode_keeps_the_leg_object():
    b = _bench()
    res = {"only": "count", "workload_key": "k", "count": {"frac": 0.2}, "legs": {}}
    assert json.loads(b.compact_line(res)) == res
