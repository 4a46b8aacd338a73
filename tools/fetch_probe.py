#!/usr/bin/env python3
"""Piped FETCH PROP ON <tag> on the device against the only alternative a caller had before it:
fetching the ids.

Builds RMAT-22 (the C2 graph) with a tag `t` (one INT prop `a` = vid mod 100) on the vertices with
vid % 4 != 0, runs `GO 3 STEPS ... YIELD e._dst AS id` from 32 roots once to the device and times,
each after warm-up runs and over several repeats (the median is reported, the spread is kept):
  * bare        | FETCH PROP ON t $-.id YIELD t.a
  * arithmetic  | FETCH PROP ON t $-.id YIELD t.a * 2 + 1 AS x
    each as shipped (the plain binary search) and with the join's other search variant
    (NBG_FETCH_SEARCH=two-level);
  * nbg_rows_fetch of the same input, which the stage replaces (a fresh result each time: a
    fetched one is cached);
  * the bare nbg_yield projection `YIELD $-.id` over the same rows: the no-join floor.
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times
around the call: what a caller waits for, the HIP launches, copies and allocations included.  One
more call per shape and variant with nbg_profile on gives each kernel's time and algorithmic bytes
(rows x 13 for k_fv_resolve: the vid cell, the dense id and the keep byte), and for the join the
probe traffic: rows x dependent global probes x 8 bytes per second, to set against the 0.08 TB/s
that 64 lanes reading 64 different lines reach on this device.  Every result is checked against
numpy over the fetched input outside the timed region, never against the device.
Usage: fetch_probe.py [scale] [roots] [out.json]"""
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
from nebula_amd import Engine, expr as E, kvgen, rmat  # noqa: E402

HBM_PEAK = 8.0e12
RANDOM_LINES = 0.08e12       # 64 lanes in 64 different lines, useful bytes per second
WARMUP, REPEATS = 3, 10
PARTS, TAG = 100, 7
FV_PIVOTS = 2048             # csrc/nbg_internal.h


def load_tag(eng, verts):
    """One vertex record of tag TAG per vertex, through the KV path, built with numpy: the key is
    (part << 8 | 1, vid, tag, version), the value a one-column row holding vid mod 100 (one varint
    byte behind the header byte)."""
    ver = kvgen.version_of(1_600_000_000_000_000)
    part = (verts.astype(np.uint64) % np.uint64(PARTS)).astype(np.int64) + 1
    key_t = np.dtype([("h", "<i4"), ("vid", "<i8"), ("tag", "<u4"), ("ver", "<i8")])
    assert key_t.itemsize == 24
    for p in range(1, PARTS + 1):
        v = verts[part == p]
        if not len(v):
            continue
        keys = np.zeros(len(v), key_t)
        keys["h"], keys["vid"], keys["tag"], keys["ver"] = (p << 8) | 1, v, TAG, ver
        vals = np.zeros((len(v), 2), np.uint8)
        vals[:, 1] = np.mod(v, 100)
        ko = np.arange(len(v) + 1, dtype=np.uint64) * np.uint64(24)
        vo = np.arange(len(v) + 1, dtype=np.uint64) * np.uint64(2)
        eng.load_part(p, keys.view(np.uint8).reshape(-1).copy(), ko, vals.reshape(-1).copy(), vo, len(v))


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
    load_tag(eng, verts[np.mod(verts, 4) != 0])
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    nv = len(verts)
    del src, dst, w
    stmt = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_dst").encode()])
    names = ["id"]
    rows = stmt.run_device(roots)
    n = rows.count
    print(f"RMAT-{scale}, {nroots} roots: {n} rows on the device, {nv} vertices", flush=True)
    a = E.edge_prop("t", "a")
    shapes = {"bare": [a], "arithmetic": [E.binop("+", E.binop("*", a, E.const(2)), E.const(1))]}
    probes = {"shipped": math.ceil(math.log2(nv)), "two-level": math.ceil(math.log2(nv / FV_PIVOTS))}

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
    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": n, "vertices": nv, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "fetch": {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft), "bytes": 8.0 * n,
                        "link_GBps": 8.0 * n / fmed / 1e9},
              "random_lines_bytes_per_s": RANDOM_LINES, "shapes": {}}
    print("fetch", result["fetch"], flush=True)

    # the no-join floor: the bare projection over the same rows
    yb = [E.input_prop("id").encode()]
    ts = timed(lambda: eng.yield_rows(rows, names, yb))
    result["yield_projection"] = {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}
    print("yield_projection", result["yield_projection"], flush=True)

    ids = rows.fetch_bits()[0]
    keep = np.mod(ids, 4) != 0
    want = np.mod(ids[keep], 100)
    for key, ys in shapes.items():
        yb = [y.encode() for y in ys]
        per = {}
        for variant in ("shipped", "two-level"):
            if variant == "shipped":
                os.environ.pop("NBG_FETCH_SEARCH", None)
            else:
                os.environ["NBG_FETCH_SEARCH"] = variant
            ts = timed(lambda: eng.fetch_vertices(rows, names, "id", TAG, yb))
            med = statistics.median(ts)
            eng.profile(True)
            out = eng.fetch_vertices(rows, names, "id", TAG, yb)
            prof = kernels("k_fv_")
            eng.profile(False)
            got = out.fetch_bits()[0]
            n_out = out.count
            out.free()
            # the check, outside the timed region: numpy over the fetched input, in its order
            ok = n_out == int(keep.sum()) and bool((got == (want if key == "bare" else want * 2 + 1)).all())
            per[variant] = {"rows_out": n_out, "seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts),
                            "input_rows_per_s": n / med, "faster_than_fetch": med < fmed, "matches_numpy": ok, "kernels": prof}
            if variant in probes and "k_fv_resolve" in prof and prof["k_fv_resolve"]["ms"] > 0:
                bps = n * probes[variant] * 8.0 / (prof["k_fv_resolve"]["ms"] * 1e-3)
                per[variant]["global_probes_per_row"] = probes[variant]
                per[variant]["probe_bytes_per_s"] = bps
                per[variant]["probe_vs_random_lines"] = bps / RANDOM_LINES
            print(key, variant, per[variant], flush=True)
            assert ok, f"fetch {key} ({variant}) differs from numpy"
        os.environ.pop("NBG_FETCH_SEARCH", None)
        result["shapes"][key] = per
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
