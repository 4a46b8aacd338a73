#!/usr/bin/env python3
"""ORDER BY / LIMIT on the device against what a caller had before it: fetching every row and
sorting on the host.

Builds RMAT-22 (the C2 graph), runs `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w, (double)e.w AS x`
from 32 roots once to the device and times, each after warm-up runs and over several repeats (the
median is reported, the spread is kept):
  * w_desc_limit10   ORDER BY $-.w DESC | LIMIT 10         (a heavily tied first factor)
  * d_limit10        ORDER BY $-.d | LIMIT 10
  * d_w_page         ORDER BY $-.d, $-.w | LIMIT 100000, 1000
  * full_w_d         ORDER BY $-.w, $-.d                   (every row sorted)
  * nbg_rows_fetch of the same result (a fresh result each time: a fetched one is cached), and
    numpy's argpartition / lexsort over the fetched columns — the host-side route is the fetch
    plus one of them.
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call: what a caller waits for, the HIP launches, copies and allocations included.
One more run per shape with nbg_profile on gives each kernel's time, algorithmic bytes and
fraction of the 8 TB/s HBM peak (event pairs around each launch; not part of the timed runs).
Every result is checked against numpy over the fetched rows outside the timed region.
Usage: orderby_probe.py [scale] [roots] [out.json]"""
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
WARMUP, REPEATS = 2, 7
SHAPES = {
    "w_desc_limit10": ([("w", True)], (0, 10)),
    "d_limit10": ([("d", False)], (0, 10)),
    "d_w_page": ([("d", False), ("w", False)], (100000, 1000)),
    "full_w_d": ([("w", False), ("d", False)], None),
}


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
    yields = [E.edge_prop("e", "_dst").encode(), ew.encode(), E.cast("double", ew).encode()]
    stmt = eng.prepare_go([1], 3, b"", yields)
    names = ["d", "w", "x"]
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device", flush=True)

    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)", "shapes": {}}
    outs = {}
    for key, (factors, limit) in SHAPES.items():
        ts = []
        for i in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            r = eng.order_by(rows, names, factors, limit)
            t1 = time.perf_counter()
            r.free()
            if i >= WARMUP:
                ts.append(t1 - t0)
        med = statistics.median(ts)
        eng.profile(True)
        outs[key] = eng.order_by(rows, names, factors, limit)
        prof = {k: v for k, v in eng.profile_read().items() if "ob_" in k and v["launches"]}
        eng.profile(False)
        for v in prof.values():
            v["hbm_fraction"] = v["algo_bytes"] / (v["ms"] * 1e-3) / HBM_PEAK if v["ms"] > 0 else None
        result["shapes"][key] = {"factors": [f"{nm} {'DESC' if d else 'ASC'}" for nm, d in factors], "limit": limit,
                                 "rows_out": outs[key].count, "seconds_median": med, "seconds_min": min(ts),
                                 "seconds_max": max(ts), "rows_per_s": n / med, "kernels": prof}
        print(key, result["shapes"][key], flush=True)

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

    # the host-side route and the check, outside the timed region: numpy over the fetched input rows
    d, wv, xv = rows.fetch_bits(copy=False)

    def host_time(fn, reps):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return out, statistics.median(ts)
    _, t_part_w = host_time(lambda: np.argpartition(-wv, 10)[:10], 3)
    _, t_part_d = host_time(lambda: np.argpartition(d, 10)[:10], 3)
    by_d_w, t_lex_dw = host_time(lambda: np.lexsort((wv, d)), 1)
    by_w_d, t_lex_wd = host_time(lambda: np.lexsort((d, wv)), 1)
    result["host"] = {"argpartition_w_seconds": t_part_w, "argpartition_d_seconds": t_part_d,
                      "lexsort_d_w_seconds": t_lex_dw, "lexsort_w_d_seconds": t_lex_wd}
    host_route = {"w_desc_limit10": fmed + t_part_w, "d_limit10": fmed + t_part_d, "d_w_page": fmed + t_lex_dw,
                  "full_w_d": fmed + t_lex_wd}

    def present(got):                    # every result row is a row of the input
        return all(bool(((d == r[0]) & (wv == r[1]) & (xv == r[2])).any()) for r in got)
    got = {k: np.stack(o.fetch_bits(), axis=1) for k, o in outs.items()}
    for o in outs.values():
        o.free()
    checks = {
        "w_desc_limit10": bool((got["w_desc_limit10"][:, 1] == np.sort(wv)[::-1][:10]).all()) and present(got["w_desc_limit10"]),
        "d_limit10": bool((got["d_limit10"][:, 0] == np.sort(np.partition(d, 10)[:10])).all()) and present(got["d_limit10"]),
        # (x is a function of w, so (d, w) fixes the whole row: these two compare exactly)
        "d_w_page": bool((got["d_w_page"] == np.stack([d, wv, xv], axis=1)[by_d_w[100000:101000]]).all()),
        "full_w_d": bool((got["full_w_d"][:, 0] == d[by_w_d]).all() and (got["full_w_d"][:, 1] == wv[by_w_d]).all() and
                         (got["full_w_d"][:, 2] == xv[by_w_d]).all()),
    }
    for key in SHAPES:
        s = result["shapes"][key]
        s["matches_numpy"] = checks[key]
        s["faster_than_fetch"] = s["seconds_median"] < fmed
        s["host_route_seconds"] = host_route[key]
        assert checks[key], f"order_by shape {key} differs from numpy"
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
