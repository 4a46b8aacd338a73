#!/usr/bin/env python3
"""Piped YIELD with aggregates (nbg_yield_agg) on the device against what a caller had before it:
fetching the referenced columns, or, for bare columns, nbg_group_by with a constant key.

Builds RMAT-22 (the C2 graph), runs `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w` from 32 roots once
to the device and times, each after warm-up runs and over several repeats (the median is reported,
the spread is kept):
  * COUNT(*)
  * SUM($-.w)
  * AVG($-.w), SUM($-.w), COUNT(*), MAX($-.w)
  * SUM($-.w * 2 + 1) WHERE $-.w < 50
  * STD($-.w)
  * COUNT_DISTINCT($-.d)
  * for the bare-column statements, nbg_group_by with the constant key abs(5) over the same rows: the
    only device route before this call, which returns the same row;
  * nbg_rows_fetch of a one-column and of the two-column GO result (a fresh result each time: a
    fetched one is cached): the fetch of the referenced columns that the call replaces.
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call.  One more call per statement with nbg_profile on gives each kernel's time and
algorithmic bytes; a statement's reached bytes per second (the referenced columns x 8 x rows over
the call's median) is set against COPY_RATE, the plain row-copy rate DESIGN.md records for k_so_copy
over the same rows.  Every result is checked against numpy over the fetched input outside the timed
region, never against the device.
Usage: yield_agg_probe.py [scale] [roots] [out.json]"""
import json
import math
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
COPY_RATE = 5.48e12          # k_so_copy over the same rows (DESIGN.md "YIELD over device rows")
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
    d_, w_ = E.edge_prop("e", "_dst"), E.edge_prop("e", "w")
    stmt = eng.prepare_go([1], 3, b"", [d_.encode(), w_.encode()])
    stmt_one = eng.prepare_go([1], 3, b"", [w_.encode()])
    names = ["d", "w"]
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device", flush=True)
    W, D, star = E.input_prop("w"), E.input_prop("d"), E.const("*")
    # name: (columns [(fun, expr)], WHERE, referenced columns, bare-column form for nbg_group_by)
    shapes = {
        "count_star": ([("COUNT", star)], None, 0, True),
        "sum_w": ([("SUM", W)], None, 1, True),
        "avg_sum_count_max_w": ([("AVG", W), ("SUM", W), ("COUNT", star), ("MAX", W)], None, 1, True),
        "sum_expr_where": ([("SUM", E.binop("+", E.binop("*", W, E.const(2)), E.const(1)))], E.binop("<", W, E.const(50)), 1, False),
        "std_w": ([("STD", W)], None, 1, True),
        "count_distinct_d": ([("COUNT_DISTINCT", D)], None, 1, True),
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

    def spread(ts):
        return {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}

    def fetch_fresh(st):
        r = st.run_device(roots)                 # (not timed)
        t0 = time.perf_counter()
        rc = eng.lib.nbg_rows_fetch(r.h)
        t1 = time.perf_counter()
        assert rc == 0
        r.free()
        return t1 - t0

    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "copy_rate_bytes_per_s": COPY_RATE, "fetch": {}, "shapes": {}}
    for cols, st in ((1, stmt_one), (2, stmt)):
        ft = [fetch_fresh(st) for _ in range(WARMUP + REPEATS)][WARMUP:]
        result["fetch"][f"{cols}_columns"] = dict(spread(ft), bytes=8.0 * cols * n, link_GBps=8.0 * cols * n / statistics.median(ft) / 1e9)
        print("fetch", cols, result["fetch"][f"{cols}_columns"], flush=True)

    dv, wv = rows.fetch_bits()                   # the check's input, outside every timed region
    keep = wv < 50
    want = {
        "count_star": [n],
        "sum_w": [int(wv.sum())],
        "avg_sum_count_max_w": [float(np.float64(int(wv.sum())) / np.float64(n)), int(wv.sum()), n, int(wv.max())],
        "sum_expr_where": [int((wv[keep] * 2 + 1).sum())],
        "std_w": None,
        "count_distinct_d": [len(np.unique(dv))],
    }
    wf = wv.astype(np.float64)
    std = math.sqrt(float(((wf - np.float64(int(wv.sum())) / np.float64(n)) ** 2).sum()) / n)

    for key, (cols, where, refs, bare) in shapes.items():
        ys, funs = [e.encode() for _, e in cols], [f for f, _ in cols]
        wb = where.encode() if where is not None else b""
        ts = timed(lambda: eng.yield_agg(rows, names, ys, funs, wb))
        med = statistics.median(ts)
        eng.profile(True)
        out = eng.yield_agg(rows, names, ys, funs, wb)
        prof = {k: v for k, v in eng.profile_read().items() if v["launches"]}
        eng.profile(False)
        got = out.fetch()[0]
        out.free()
        ok = abs(got[0] - std) <= n * 2.0 ** -52 * std if key == "std_w" else got == want[key]
        fetch = result["fetch"]["1_columns"]
        per = dict(spread(ts), referenced_columns=refs, result=got, matches_numpy=bool(ok), kernels=prof,
                   bytes_per_s=8.0 * refs * n / med, of_copy_rate=8.0 * refs * n / med / COPY_RATE,
                   fetch_of_referenced_columns_seconds_median=fetch["seconds_median"] if refs else None,
                   beyond_fetch_spread=bool(refs and max(ts) < fetch["seconds_min"]))
        if bare:
            gys = [(f, e.encode(), None) for f, e in cols]
            gkey = [E.Expr(E.K_FUNC, alias="abs", args=[E.const(5)]).encode()]
            gt = timed(lambda: eng.group_by(rows, names, gkey, gys))
            gout = eng.group_by(rows, names, gkey, gys)
            grow = gout.fetch()[0]
            gout.free()
            per["group_by_constant_key"] = dict(spread(gt), result=grow, same_row=bool(grow == got),
                                                beyond_spread=bool(max(ts) < min(gt)))
        result["shapes"][key] = per
        print(key, per, flush=True)
        assert ok, f"{key}: {got} differs from numpy"
    try:
        result["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"],
                                                   stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        result["commit"] = os.environ.get("NBG_COMMIT", "unknown")
    rows.free()
    stmt.free()
    stmt_one.free()
    eng.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
