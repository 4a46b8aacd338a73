#!/usr/bin/env python3
"""Piped YIELD ... WHERE on the device against the only alternative a caller had before it:
fetching the rows.

Builds RMAT-22 (the C2 graph), runs `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w` from 32 roots once
to the device and times, each after warm-up runs and over several repeats (the median is reported,
the spread is kept):
  * projection  YIELD $-.d
  * filter      YIELD $-.d WHERE $-.w < 50
  * arithmetic  YIELD $-.d, $-.w * 2 + 1 AS x WHERE $-.w < 50 && $-.d % 3 != 0
  * nbg_rows_fetch of the same input (a fresh result each time: a fetched one is cached);
  * UNION ALL of the input with itself: k_so_copy, a plain row copy on the same chunk walk.
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call: what a caller waits for, the HIP launches, copies and allocations included.  One
more call per shape with nbg_profile on gives each kernel's time, algorithmic bytes (include/nbg.h's
formulas: filter rows x (8 x WHERE columns + 1); emit kept x 8 x (YIELD columns + out columns), plus
rows x 1 when there are keep flags) and achieved bytes/s with its fraction of the 8 TB/s HBM peak
(not part of the timed runs).  Every result is checked against numpy over the fetched input outside
the timed region, never against the device.  Usage: yield_probe.py [scale] [roots] [out.json]"""
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
    stmt = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()])
    names = ["d", "w"]
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device", flush=True)
    d, wv = E.input_prop("d"), E.input_prop("w")
    lt50 = E.binop("<", wv, E.const(50))
    shapes = {
        "projection": ([d], None),
        "filter": ([d], lt50),
        "arithmetic": ([d, E.binop("+", E.binop("*", wv, E.const(2)), E.const(1))],
                       E.binop("&&", lt50, E.binop("!=", E.binop("%", d, E.const(3)), E.const(0)))),
    }

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

    def kernels(prefix):
        prof = {k: v for k, v in eng.profile_read().items() if k.startswith(prefix) and v["launches"]}
        for v in prof.values():
            v["bytes_per_s"] = v["algo_bytes"] / (v["ms"] * 1e-3) if v["ms"] > 0 else None
            v["hbm_fraction"] = v["bytes_per_s"] / HBM_PEAK if v["ms"] > 0 else None
        return prof

    def fetch_fresh():
        r = stmt.run_device(roots)                 # (not timed)
        t0 = time.perf_counter()
        rc = eng.lib.nbg_rows_fetch(r.h)
        t1 = time.perf_counter()
        assert rc == 0
        r.free()
        return t1 - t0
    ft = [fetch_fresh() for _ in range(WARMUP + REPEATS)][WARMUP:]
    fmed = statistics.median(ft)
    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "fetch": {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft), "bytes": 16.0 * n,
                        "link_GBps": 16.0 * n / fmed / 1e9},
              "shapes": {}}
    print("fetch", result["fetch"], flush=True)

    # the plain row copy on the same chunk walk
    ts = timed(lambda: eng.set_op(rows, rows, "UNION"))
    eng.profile(True)
    eng.set_op(rows, rows, "UNION").free()
    copy = kernels("k_so_copy")
    eng.profile(False)
    result["union_all_copy"] = {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts),
                                "kernels": copy}
    print("union_all_copy", result["union_all_copy"], flush=True)

    dv, wvv = rows.fetch_bits()
    for key, (ys, where) in shapes.items():
        yb, wb = [y.encode() for y in ys], where.encode() if where is not None else b""
        ts = timed(lambda: eng.yield_rows(rows, names, yb, wb))
        med = statistics.median(ts)
        eng.profile(True)
        out = eng.yield_rows(rows, names, yb, wb)
        prof = kernels("k_yr_")
        eng.profile(False)
        got = out.fetch_bits()
        n_out = out.count
        out.free()
        # the check, outside the timed region: numpy over the fetched input, in its order
        keep = np.ones(n, bool) if where is None else (wvv < 50) if key == "filter" else (wvv < 50) & (np.fmod(dv, 3) != 0)
        ok = n_out == int(keep.sum()) and bool((got[0] == dv[keep]).all())
        if key == "arithmetic":
            ok = ok and bool((got[1] == wvv[keep] * 2 + 1).all())
        result["shapes"][key] = {"rows_out": n_out, "seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts),
                                 "input_rows_per_s": n / med, "faster_than_fetch": med < fmed, "matches_numpy": ok,
                                 "kernels": prof}
        print(key, result["shapes"][key], flush=True)
        assert ok, f"yield {key} differs from numpy"
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
