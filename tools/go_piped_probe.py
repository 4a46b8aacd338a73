#!/usr/bin/env python3
"""`| GO FROM $-.id` over device rows (nbg_go_piped) against what a caller had before it.

Builds RMAT-22 (the C2 graph) with one INT prop `w` on the edges and runs `GO 3 STEPS ... YIELD
e._dst AS id, e.w AS w` from 32 roots once to the device.  The input of the second GO is the first N
rows of that result (`| LIMIT N`), N = 10^3, 10^5, 10^6, 10^7, and the second GO is
`GO FROM $-.id OVER e WHERE e.w < 1 YIELD [DISTINCT] e._dst` or, with a `$-` column,
`... YIELD [DISTINCT] $-.w, e._dst` (w is uniform in [0, 100): the WHERE keeps the result at a
hundredth of the scanned edges, so that the result's own row buffers do not decide the comparison).
Each shape is timed three ways, after warm-up runs and over several repeats (the median is reported,
the spread is kept), side by side in one run:
  1. device: nbg_go_piped over the rows where they lie;
  2. host:   nbg_rows_fetch of the input (a fresh LIMIT result each time, made outside the timed
             region: a fetched one is cached), then nbg_go_device with `starts' and input_cols from
             the fetched columns — only calls the library had before nbg_go_piped;
  3. floor:  the second GO alone: a prepared statement without $- executed from the fetched start
             list (nbg_go_execute).  With a `$-` column there is no such floor (the index is part
             of the sentence): the shape reports the floor of its `$-`-less twin.
Every call is synchronous and ends in a stream synchronise, so the times are host-clock times around
the call.  Where the start list's entries plus edges reach 2^32 - 1 (nbg_go's own bound, which both
routes answer with NBG_E_UNSUPPORTED) the shape records that instead of a time.  One more device call
per shape with nbg_profile on gives each new kernel's time and algorithmic bytes.  The two routes'
results are compared by their digests outside the timed region.
Usage: go_piped_probe.py [scale] [roots] [out.json]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nebula_amd import Engine, NbgError, _lib as L, expr as E, kvgen, rmat  # noqa: E402
from nebula_amd.engine import DeviceRows  # noqa: E402

HBM_PEAK = 8.0e12
ROW_COPY = 5.5e12             # a plain row copy on this device
WARMUP, REPEATS = 2, 7
PARTS = 100
SIZES = (10**3, 10**5, 10**6, 10**7)
NAMES = ["id", "w"]


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    nroots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    src, dst, w = rmat.rmat_edges_fast(scale)
    eng = Engine(PARTS)
    eng.register_edge(1, "e", [("w", kvgen.INT)])
    eng.load_edges(1, src, dst, [w])
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    del src, dst, w
    first = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()])
    rows = first.run_device(roots)
    print(f"RMAT-{scale}, {nroots} roots: {rows.count} rows on the device", flush=True)
    where = E.binop("<", E.edge_prop("e", "w"), E.const(1)).encode()
    dst_only = [E.edge_prop("e", "_dst").encode()]
    with_input = [E.input_prop("w").encode(), E.edge_prop("e", "_dst").encode()]

    def summary(ts):
        return {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts), "repeats": len(ts)}

    def kernels():
        prof = {k: v for k, v in eng.profile_read().items() if k.startswith("k_gp_") and v["launches"]}
        for v in prof.values():
            v["bytes_per_s"] = v["algo_bytes"] / (v["ms"] * 1e-3) if v["ms"] > 0 else None
            v["of_row_copy"] = v["bytes_per_s"] / ROW_COPY if v["ms"] > 0 else None
        return prof

    def host_route(inp, ys, distinct):
        """nbg_rows_fetch + nbg_go_device with host inputs; the DeviceRows."""
        cols = inp.fetch_bits(copy=False)
        req, keep = eng._go_request(cols[0], [1], 1, where, ys, distinct, False)
        if len(ys) > 1:
            cname = (C.c_char_p * 2)(b"id", b"w")
            ckind = (C.c_uint8 * 2)(0, 0)
            cptr = (C.c_void_p * 2)(cols[0].ctypes.data, cols[1].ctypes.data)
            req.num_input_cols, req.input_names, req.input_kinds = 2, cname, ckind
            req.input_cols, req.num_input_rows, req.input_vid_col = cptr, len(cols[0]), 0
        out = C.c_void_p()
        eng._check(eng.lib.nbg_go_device(eng.h, C.byref(req), C.byref(out)), "go_device")
        return DeviceRows(eng, out)

    result = {"graph": f"RMAT-{scale}", "roots": nroots, "rows": rows.count, "warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "row_copy_bytes_per_s": ROW_COPY, "shapes": []}
    for n in SIZES:
        if n > rows.count:
            continue
        inp = eng.order_by(rows, NAMES, [], (0, n))
        starts = inp.fetch_bits()[0]
        floors = {}
        for use_input in (False, True):
            for distinct in (False, True):
                ys = with_input if use_input else dst_only
                shape = {"n": n, "distinct": distinct, "input_column": use_input}
                try:
                    eng.go_piped(inp, NAMES, "id", [1], 1, where, ys, distinct).free()
                except NbgError as ex:
                    if ex.code != L.E_UNSUPPORTED:
                        raise
                    shape["stopped"] = str(ex)                       # the 2^32 - 1 bound, on both routes
                    try:
                        host_route(inp, ys, distinct).free()
                        shape["host_route_also_stopped"] = False
                    except NbgError as hx:
                        shape["host_route_also_stopped"] = hx.code == L.E_UNSUPPORTED
                    result["shapes"].append(shape)
                    print(shape, flush=True)
                    continue
                dev_t, host_t = [], []
                reps = REPEATS if n < 10**7 else 3
                for i in range(WARMUP + reps):
                    t0 = time.perf_counter()
                    r = eng.go_piped(inp, NAMES, "id", [1], 1, where, ys, distinct)
                    t1 = time.perf_counter()
                    dg = (r.count, r.digest())
                    r.free()
                    fresh = eng.order_by(rows, NAMES, [], (0, n))      # (not timed: an unfetched input)
                    t2 = time.perf_counter()
                    h = host_route(fresh, ys, distinct)
                    t3 = time.perf_counter()
                    same = (h.count, h.digest()) == dg
                    h.free()
                    fresh.free()
                    assert same, f"the two routes differ at {shape}"
                    if i >= WARMUP:
                        dev_t.append(t1 - t0)
                        host_t.append(t3 - t2)
                shape["rows_out"] = dg[0]
                shape["device"] = summary(dev_t)
                shape["host"] = summary(host_t)
                if not use_input:
                    stmt = eng.prepare_go([1], 1, where, ys, distinct)
                    fl = []
                    for i in range(WARMUP + reps):
                        t0 = time.perf_counter()
                        r = stmt.run_device(starts)
                        t1 = time.perf_counter()
                        r.free()
                        if i >= WARMUP:
                            fl.append(t1 - t0)
                    stmt.free()
                    floors[distinct] = summary(fl)
                shape["floor"] = floors[distinct]
                d, hst = shape["device"], shape["host"]
                shape["speedup_median"] = hst["seconds_median"] / d["seconds_median"]
                shape["beats_host_beyond_its_spread"] = d["seconds_max"] < hst["seconds_min"]
                eng.profile(True)
                eng.go_piped(inp, NAMES, "id", [1], 1, where, ys, distinct).free()
                shape["kernels"] = kernels()
                eng.profile(False)
                result["shapes"].append(shape)
                print(json.dumps(shape), flush=True)
        inp.free()
    timed = [s for s in result["shapes"] if "device" in s and s["n"] > 32]
    result["claim_device_beats_host_at_every_n"] = all(s["beats_host_beyond_its_spread"] for s in timed)
    try:
        result["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        result["commit"] = os.environ.get("NBG_COMMIT", "unknown")
    rows.free()
    first.free()
    eng.close()
    print(json.dumps({k: v for k, v in result.items() if k != "shapes"}))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
