#!/usr/bin/env python3
"""GROUP BY on the device against the only alternative a caller had before it: fetching the rows.

Builds RMAT-22 (the C2 graph), runs `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w,
(bool)(e.w < 50) AS b` from 32 roots once to the device and times, each after warm-up runs and over several
repeats (the median is reported, the spread is kept):
  * nbg_group_by for key b (2 groups: accumulators in LDS) with COUNT(*), SUM($-.w);
  * nbg_group_by for key d (accumulators in HBM) with the same aggregates;
  * nbg_rows_fetch of the same result (a fresh result each time: a fetched one is cached).
(`e.w < 50 AS b` without the cast is an INT column of zeros under the reference's row schema —
one group — so the probe casts it to get the two-group shape.)
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call: what a caller waits for, the HIP launches, copies and allocations included.
Reports rows/s for each and each group_by's fraction of the 8 TB/s HBM peak over its algorithmic
bytes (8 B x referenced columns x rows x passes), and checks both results against numpy over the
fetched rows outside the timed region.  Usage: groupby_probe.py [scale] [roots] [out.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nebula_amd import Engine, expr as E, rmat  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, REPEATS = 3, 9


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    nroots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    src, dst, w = rmat.rmat_edges_fast(scale)
    eng = Engine(100)
    eng.register_edge(1, "e", [("w", 2)])
    eng.load_edges(1, src, dst, [w])
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    del src, dst, w
    ew = E.edge_prop("e", "w")
    yields = [E.edge_prop("e", "_dst").encode(), ew.encode(), E.cast("bool", E.binop("<", ew, E.const(50))).encode()]
    stmt = eng.prepare_go([1], 3, b"", yields)
    names = ["d", "w", "b"]
    aggs = [("COUNT", E.const("*").encode(), "n"), ("SUM", E.input_prop("w").encode(), "s")]
    shapes = {"b": ([E.input_prop("b").encode()], [("", E.input_prop("b").encode(), "b")] + aggs),
              "d": ([E.input_prop("d").encode()], [("", E.input_prop("d").encode(), "d")] + aggs)}
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device", flush=True)

    def timed(fn):
        ts = []
        for i in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            r = fn()
            t1 = time.perf_counter()
            r.free() if r is not None else None
            if i >= WARMUP:
                ts.append(t1 - t0)
        return ts

    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)", "shapes": {}}
    for key, (groups, ys) in shapes.items():
        ts = timed(lambda: eng.group_by(rows, names, groups, ys))
        med = statistics.median(ts)
        algo = 8.0 * 2 * n * 2           # columns {key, w}, key pass + accumulate pass
        out = eng.group_by(rows, names, groups, ys)
        result["shapes"][key] = {"groups": out.count, "seconds_median": med, "seconds_min": min(ts),
                                 "seconds_max": max(ts), "rows_per_s": n / med, "algo_bytes": algo,
                                 "hbm_fraction": algo / med / HBM_PEAK}
        result["shapes"][key]["_out"] = out
        print(key, {k: v for k, v in result["shapes"][key].items() if k != "_out"}, flush=True)

    def fetch_fresh():
        r = stmt.run_device(roots)       # (not timed)
        t0 = time.perf_counter()
        rc = eng.lib.nbg_rows_fetch(r.h)
        t1 = time.perf_counter()
        assert rc == 0
        r.free()
        return t1 - t0
    ft = [fetch_fresh() for _ in range(WARMUP + REPEATS)][WARMUP:]
    fmed = statistics.median(ft)
    result["fetch"] = {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft),
                       "rows_per_s": n / fmed, "bytes": 8.0 * 3 * n, "link_GBps": 8.0 * 3 * n / fmed / 1e9}
    print("fetch", result["fetch"], flush=True)

    # the check, outside the timed region: numpy over the fetched input rows
    d, wv, b = rows.fetch_bits(copy=False)
    for key, col in (("b", b), ("d", d)):
        out = result["shapes"][key].pop("_out")
        got = np.stack(out.fetch_bits(), axis=1)
        out.free()
        got = got[np.argsort(got[:, 0], kind="stable")]
        ks, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)
        sums = np.zeros(len(ks), np.int64)
        np.add.at(sums, inv, wv)
        ok = got.shape[0] == len(ks) and bool((got[:, 0] == ks).all() and (got[:, 1] == cnt).all() and
                                              (got[:, 2] == sums).all())
        result["shapes"][key]["matches_numpy"] = ok
        assert ok, f"group_by over key {key} differs from numpy"
    for key in shapes:
        result["shapes"][key]["faster_than_fetch"] = result["shapes"][key]["seconds_median"] < fmed
    try:
        result["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"],
                                                   stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        result["commit"] = os.environ.get("NBG_COMMIT", "unknown")
    rows.free()
    stmt.free()
    eng.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
