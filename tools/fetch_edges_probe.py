#!/usr/bin/env python3
"""Piped FETCH PROP ON <edge> on the device against what a caller had before it: fetching the key
columns.

Builds RMAT-22 (the C2 graph) with one INT prop `w` on the edges, runs `GO 3 STEPS ... YIELD
e._src AS s, e._dst AS d` from 32 roots once to the device and times, each after warm-up runs and
over several repeats (the median is reported, the spread is kept), side by side in one run:
  1. nbg_rows_fetch of the two key columns, which the stage replaces (a fresh result each time: a
     fetched one is cached);
  2. nbg_yield `YIELD $-.s, $-.d` over the same rows: the no-join floor;
  3. nbg_fetch_vertices over `$-.s` alone (a tag `t` on every vertex): the vertex half of the join;
  4. nbg_fetch_edges `$-.s->$-.d YIELD e.w` (the search that ships: one vid search per row);
  5. (the run-leader variant of the search, one vid search per run of equal src within a wave,
     was measured by this probe alternating call by call with 4, lost and was deleted with its
     knob; profiles/fetch_edges_c2.json and DESIGN.md keep both rows);
  6. `YIELD e.w * 2 + 1` (through the interpreter).
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call: what a caller waits for, the HIP launches, copies and allocations included.  One
more call per shape and variant with nbg_profile on gives each kernel's time and algorithmic bytes.
Every result is checked against numpy over the fetched input outside the timed region, never
against the device: every row of the GO is an edge, so `e.w` must come back for every row, in order.
Usage: fetch_edges_probe.py [scale] [roots] [out.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nebula_amd import Engine, expr as E, kvgen, rmat  # noqa: E402
from tools.fetch_probe import load_tag  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, REPEATS = 3, 10
PARTS, TAG = 100, 7
SHIPPED = "plain"
VARIANTS = (SHIPPED,)        # (the deleted run-leader variant stood beside it, behind an environment knob)


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    nroots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    src, dst, w = rmat.rmat_edges_fast(scale)
    verts = np.union1d(src, dst)
    eng = Engine(PARTS)
    eng.register_edge(1, "e", [("w", kvgen.INT)])
    eng.register_tag(TAG, "t", [("a", kvgen.INT)])
    eng.load_edges(1, src, dst, [w])
    load_tag(eng, verts)
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    # the latest version per (src, dst): what the fetch must return (a bulk load keeps the last write)
    order = np.lexsort((np.arange(len(src)), dst, src))
    s_sorted, d_sorted, w_sorted = src[order], dst[order], np.asarray(w)[order]
    last = np.ones(len(order), bool)
    last[:-1] = (s_sorted[1:] != s_sorted[:-1]) | (d_sorted[1:] != d_sorted[:-1])
    s_u, d_u, w_u = s_sorted[last], d_sorted[last], w_sorted[last]
    nv = len(verts)
    del src, dst, w, order, s_sorted, d_sorted, w_sorted, last
    stmt = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_src").encode(), E.edge_prop("e", "_dst").encode()])
    names = ["s", "d"]
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device, {nv} vertices", flush=True)

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

    def summary(ts):
        return {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}

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
    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "vertices": nv, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "fetch": {**summary(ft), "bytes": 16.0 * n, "link_GBps": 16.0 * n / fmed / 1e9}}
    print("fetch", result["fetch"], flush=True)

    # 2. the no-join floor, 3. the vertex half of the join
    yb = [E.input_prop("s").encode(), E.input_prop("d").encode()]
    result["yield_projection"] = summary(timed(lambda: eng.yield_rows(rows, names, yb)))
    print("yield_projection", result["yield_projection"], flush=True)
    tb = [E.edge_prop("t", "a").encode()]
    os.environ.pop("NBG_FETCH_SEARCH", None)
    result["fetch_vertices_src"] = summary(timed(lambda: eng.fetch_vertices(rows, names, "s", TAG, tb)))
    eng.profile(True)
    eng.fetch_vertices(rows, names, "s", TAG, tb).free()
    result["fetch_vertices_src"]["kernels"] = kernels("k_fv_")
    eng.profile(False)
    print("fetch_vertices_src", result["fetch_vertices_src"], flush=True)

    # the expectation, from numpy over the fetched input: every row is an edge
    s_in, d_in = rows.fetch_bits()[:2]
    key_u = s_u.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ d_u.astype(np.uint64)
    key_in = s_in.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ d_in.astype(np.uint64)
    assert len(np.unique(key_u)) == len(key_u)     # (the mix separates this graph's pairs)
    srt = np.argsort(key_u)
    pos = np.searchsorted(key_u[srt], key_in)
    assert bool((key_u[srt][pos] == key_in).all())
    want = w_u[srt][pos]
    runs = int((s_in[1:] != s_in[:-1]).sum()) + 1
    result["src_runs"] = {"runs": runs, "mean_run_length": n / runs}

    # 4. the search variants, alternating call by call
    wexpr = E.edge_prop("e", "w")
    bare = [wexpr.encode()]

    def call(variant, ys):
        return eng.fetch_edges(rows, names, "s", "d", None, 1, ys)
    ts = {v: [] for v in VARIANTS}
    for i in range(WARMUP + REPEATS):
        for variant in VARIANTS:
            t0 = time.perf_counter()
            r = call(variant, bare)
            t1 = time.perf_counter()
            r.free()
            if i >= WARMUP:
                ts[variant].append(t1 - t0)
    result["shapes"] = {"bare": {}}
    for variant in VARIANTS:
        eng.profile(True)
        out = call(variant, bare)
        prof = kernels("k_fe_")
        eng.profile(False)
        got = out.fetch_bits()[0]
        ok = out.count == n and bool((got == want).all())
        out.free()
        med = statistics.median(ts[variant])
        result["shapes"]["bare"][variant] = {**summary(ts[variant]), "rows_out": n, "input_rows_per_s": n / med,
                                             "faster_than_fetch": med < fmed, "matches_numpy": ok, "kernels": prof}
        print("bare", variant, result["shapes"]["bare"][variant], flush=True)
        assert ok, f"fetch_edges bare ({variant}) differs from numpy"

    # 6. through the interpreter, the shipped variant
    arith = [E.binop("+", E.binop("*", wexpr, E.const(2)), E.const(1)).encode()]
    ta = timed(lambda: call(SHIPPED, arith))
    eng.profile(True)
    out = call(SHIPPED, arith)
    prof = kernels("k_fe_")
    eng.profile(False)
    got = out.fetch_bits()[0]
    ok = out.count == n and bool((got == want * 2 + 1).all())
    out.free()
    result["shapes"]["arithmetic"] = {SHIPPED: {**summary(ta), "rows_out": n, "input_rows_per_s": n / statistics.median(ta),
                                                "faster_than_fetch": statistics.median(ta) < fmed, "matches_numpy": ok,
                                                "kernels": prof}}
    print("arithmetic", result["shapes"]["arithmetic"], flush=True)
    assert ok, "fetch_edges arithmetic differs from numpy"
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
