#!/usr/bin/env python3
"""UNION / INTERSECT / MINUS on the device against what a caller had before them: fetching both
results and combining them on the host.

Builds RMAT-22 (the C2 graph) and runs `GO 3 STEPS ...` twice to the device, from roots 0-15 (left)
and roots 8-23 (right) of the bench root list, in two shapes:
  * wide   YIELD e._dst AS d, e.w AS w                          (many distinct rows)
  * low    YIELD e.w % 7 AS k7, (bool)(e.w < 50) AS b           (a handful of distinct rows)
and times, per shape and operator (UNION ALL, UNION DISTINCT, INTERSECT, MINUS), nbg_set_op after
warm-up runs and over several repeats (the median is reported, the spread is kept), and
nbg_rows_fetch of the two inputs (fresh results each time: a fetched one is cached).  Every call is
synchronous and ends in a stream synchronise, so the times are host-clock times around the call.
One more call per operator with nbg_profile on gives each kernel's time, algorithmic bytes and
fraction of the 8 TB/s HBM peak (not part of the timed runs).  Every result is checked against
numpy over the fetched inputs (multiplicities per distinct row; UNION ALL as an exact list) outside
the timed region, never against the device.
Usage: setops_probe.py [scale] [out.json]"""
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
OPS = {"union_all": ("UNION", False), "union_distinct": ("UNION", True), "intersect": ("INTERSECT", False),
       "minus": ("MINUS", False)}


class RowKeys:
    """One int64 key per row: each column's rank among the distinct cells both inputs hold, in mixed
    radix (a 2-D np.unique over a hundred million rows would take minutes)."""

    def __init__(self, cols_l, cols_r):
        self.cells = [np.unique(np.concatenate([a, b])) for a, b in zip(cols_l, cols_r)]
        self.size = 1
        for c in self.cells:
            self.size *= len(c)
        assert self.size < 1 << 62

    def keys(self, cols):
        """(keys, every cell is one the inputs hold)."""
        key, known = np.zeros(len(cols[0]), np.int64), True
        for c, cells in zip(cols, self.cells):
            at = np.minimum(np.searchsorted(cells, c), len(cells) - 1)
            known = known and bool((cells[at] == c).all())
            key = key * len(cells) + at
        return key, known


def counts_of(keys, uniq):
    """How often each key of the sorted `uniq` occurs in `keys` (None: a key outside it)."""
    at = np.minimum(np.searchsorted(uniq, keys), len(uniq) - 1)
    if len(keys) and not bool((uniq[at] == keys).all()):
        return None
    return np.bincount(at, minlength=len(uniq))


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    src, dst, w = rmat.rmat_edges_fast(scale)
    eng = Engine(100)
    eng.register_edge(1, "e", [("w", 2)])
    eng.load_edges(1, src, dst, [w])
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, 24, 42, verts=sv)]
    del src, dst, w
    ew = E.edge_prop("e", "w")
    shapes = {
        "wide": [E.edge_prop("e", "_dst").encode(), ew.encode()],
        "low": [E.binop("%", ew, E.const(7)).encode(), E.cast("bool", E.binop("<", ew, E.const(50))).encode()],
    }
    result = {"graph": f"RMAT-{scale}", "left_roots": "0-15", "right_roots": "8-23", "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)", "shapes": {}}
    for shape, yields in shapes.items():
        stmt = eng.prepare_go([1], 3, b"", yields)
        left, right = stmt.run_device(roots[:16]), stmt.run_device(roots[8:24])
        nl, nr = left.count, right.count
        print(f"{shape}: {nl} + {nr} rows on the device", flush=True)

        def fetch_fresh():
            a, b = stmt.run_device(roots[:16]), stmt.run_device(roots[8:24])       # (not timed)
            t0 = time.perf_counter()
            rc = eng.lib.nbg_rows_fetch(a.h) or eng.lib.nbg_rows_fetch(b.h)
            t1 = time.perf_counter()
            assert rc == 0
            a.free()
            b.free()
            return t1 - t0
        ft = [fetch_fresh() for _ in range(WARMUP + REPEATS)][WARMUP:]
        fmed = statistics.median(ft)
        entry = {"rows_left": nl, "rows_right": nr,
                 "fetch_both": {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft),
                                "bytes": 16.0 * (nl + nr), "link_GBps": 16.0 * (nl + nr) / fmed / 1e9},
                 "operators": {}}
        cl_cols, cr_cols = left.fetch_bits(), right.fetch_bits()
        rk = RowKeys(cl_cols, cr_cols)
        kl, kr = rk.keys(cl_cols)[0], rk.keys(cr_cols)[0]
        uniq = np.unique(np.concatenate([kl, kr]))
        cl, cr = counts_of(kl, uniq), counts_of(kr, uniq)
        del kl, kr
        want = {"union_all": cl + cr, "union_distinct": np.ones_like(cl), "intersect": np.minimum(cl, cr),
                "minus": np.where(cr == 0, cl, 0)}
        entry["distinct_rows"] = int(len(uniq))
        for key, (op, distinct) in OPS.items():
            ts = []
            for i in range(WARMUP + REPEATS):
                t0 = time.perf_counter()
                r = eng.set_op(left, right, op, distinct)
                t1 = time.perf_counter()
                r.free()
                if i >= WARMUP:
                    ts.append(t1 - t0)
            med = statistics.median(ts)
            eng.profile(True)
            out = eng.set_op(left, right, op, distinct)
            prof = {k: v for k, v in eng.profile_read().items() if k.startswith("k_so_") and v["launches"]}
            eng.profile(False)
            for v in prof.values():
                v["hbm_fraction"] = v["algo_bytes"] / (v["ms"] * 1e-3) / HBM_PEAK if v["ms"] > 0 else None
            got = out.fetch_bits()
            n_out = out.count
            out.free()
            # the check, outside the timed region: every result row's count against numpy's
            gk, known = rk.keys(got) if n_out else (np.zeros(0, np.int64), True)
            cg = counts_of(gk, uniq) if known else None
            ok = cg is not None and bool((cg == want[key]).all())
            if key == "union_all":
                ok = ok and all(bool((g == np.concatenate([a, b])).all()) for g, a, b in zip(got, cl_cols, cr_cols))
            entry["operators"][key] = {"rows_out": n_out, "seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts),
                                       "input_rows_per_s": (nl + nr) / med, "faster_than_fetch_of_both": med < fmed,
                                       "matches_numpy": ok, "kernels": prof}
            print(shape, key, entry["operators"][key], flush=True)
            assert ok, f"set_op {shape} {key} differs from numpy"
        result["shapes"][shape] = entry
        left.free()
        right.free()
        stmt.free()
    try:
        result["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"],
                                                   stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        result["commit"] = os.environ.get("NBG_COMMIT", "unknown")
    eng.close()
    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
