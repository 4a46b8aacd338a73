#!/usr/bin/env python3
"""nbg_rows_encode against nbg_rows_fetch of the same rows: what the hand-over of a device result
to graphd costs either way.

Shape "c2": RMAT-22 (the C2 graph), `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w` from 32 roots, run
once to the device.  Shape "strings": RMAT-14 built from KV records whose edges carry a dictionary
string (64 distinct names of 8 to 23 bytes), `GO 3 STEPS ... YIELD e._dst AS d, e.s AS s`.  Per shape,
each after warm-up calls and over several repeats (the median is reported, the spread is kept):
  * nbg_rows_encode of the rows (the nbg_rowset_free after it is outside the timer);
  * nbg_rows_fetch of the same rows (a fresh result of the same statement each time: a fetched one
    is cached; the GO itself is not timed).
Both calls are synchronous and end in a stream synchronise, so the times are host-clock times around
the call: what a caller waits for, the HIP launches, the device allocation of the encoded bytes and
the DMA into pinned memory included.  One more call with nbg_profile on gives each kernel's time,
algorithmic bytes (include/nbg.h) and achieved bytes/s with its fraction of the 8 TB/s HBM peak (not
part of the timed runs).  The bytes are checked outside the timed region against numpy over the
fetched rows (every row's length; the first and last rows byte for byte through kvgen.encode_row),
never against the device.  The host RowWriter loop this call replaces is not timed: the reference's
RowWriter is no part of this build.  Usage: rows_encode_probe.py [scale] [roots] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nebula_amd import Engine, expr as E, kvgen, rmat  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, REPEATS = 3, 9
CHECK_ROWS = 2000


def varint_len(v):
    """folly::encodeVarint's length of int64 payloads taken as uint64 (numpy)."""
    u = v.astype(np.uint64)
    n = np.ones(len(u), np.int64)
    for k in range(1, 10):
        n += (u >= np.uint64(1) << np.uint64(7 * k)).astype(np.int64)
    return n


def rowset(types, rows):
    out = []
    for r in rows:
        b = kvgen.encode_row([("", t) for t in types], r, 0)
        out.append(kvgen._varint(len(b)) + b)
    return b"".join(out)


def measure(eng, stmt, roots, types, cell_bytes):
    """cell_bytes(rows) -> (the cord length of every row (numpy), the first and the last CHECK_ROWS rows)."""
    lib = eng.lib
    rows = stmt.run_device(roots)
    n = rows.count

    def encode_once():
        out = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.nbg_rows_encode(eng.h, rows.h, C.byref(out))
        t1 = time.perf_counter()
        assert rc == 0, rc
        return out, t1 - t0

    ts = []
    for i in range(WARMUP + REPEATS):
        out, dt = encode_once()
        lib.nbg_rowset_free(out)
        if i >= WARMUP:
            ts.append(dt)

    def fetch_fresh():
        r = stmt.run_device(roots)                 # (not timed)
        t0 = time.perf_counter()
        rc = lib.nbg_rows_fetch(r.h)
        t1 = time.perf_counter()
        assert rc == 0
        r.free()
        return t1 - t0
    ft = [fetch_fresh() for _ in range(WARMUP + REPEATS)][WARMUP:]

    eng.profile(True)
    out, _ = encode_once()
    prof = {k: v for k, v in eng.profile_read().items() if k.startswith("k_re_") and v["launches"]}
    eng.profile(False)
    for v in prof.values():
        v["bytes_per_s"] = v["algo_bytes"] / (v["ms"] * 1e-3) if v["ms"] > 0 else None
        v["hbm_fraction"] = v["bytes_per_s"] / HBM_PEAK if v["ms"] > 0 else None
    nbytes = lib.nbg_rowset_len(out)
    data = np.ctypeslib.as_array(lib.nbg_rowset_data(out), shape=(nbytes,))
    # the check, outside the timed region
    cord, first, last = cell_bytes(rows)
    row_len = 1 + cord                              # fewer than 16 columns: no block offsets
    assert int(cord.max()) < 256
    ok = nbytes == int((row_len + varint_len(row_len)).sum())
    head = rowset(types, first)
    tail = rowset(types, last)
    ok = ok and bytes(data[:len(head)]) == head and bytes(data[nbytes - len(tail):]) == tail
    lib.nbg_rowset_free(out)
    rows.free()
    med, fmed = statistics.median(ts), statistics.median(ft)
    res = {"rows": n, "columns": len(types), "encoded_bytes": nbytes, "fetch_bytes": 8.0 * len(types) * n,
           "bytes_per_row": nbytes / n,
           "encode": {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "link_GBps": nbytes / med / 1e9},
           "fetch": {"seconds_median": fmed, "seconds_min": min(ft), "seconds_max": max(ft),
                     "link_GBps": 8.0 * len(types) * n / fmed / 1e9},
           "encode_over_fetch": med / fmed, "fetch_over_encode": fmed / med,
           # a win only when the medians lie outside each other's spread
           "encode_faster_outside_spread": max(ts) < min(ft), "fetch_faster_outside_spread": max(ft) < min(ts),
           "matches_model": ok, "kernels": prof}
    assert ok, "encoded bytes differ from the model"
    return res


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    nroots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    result = {"warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call (ends in a stream synchronise)",
              "not_timed": "the host RowWriter loop nbg_rows_encode replaces (the reference's RowWriter is no part of this build)",
              "shapes": {}}

    # ---- c2: (VID, INT)
    src, dst, w = rmat.rmat_edges_fast(scale)
    eng = Engine(100)
    eng.register_edge(1, "e", [("w", 2)])
    eng.load_edges(1, src, dst, [w])
    eng.finalize()
    sv, _ = rmat.vertex_sets(scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    del src, dst, w
    stmt = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()])
    def int_cells(rows):
        d, wv = rows.fetch_bits()
        ends = lambda a, b: list(zip(a.tolist(), b.tolist()))   # noqa: E731
        return 8 + varint_len(wv), ends(d[:CHECK_ROWS], wv[:CHECK_ROWS]), ends(d[-CHECK_ROWS:], wv[-CHECK_ROWS:])
    res = measure(eng, stmt, roots, [kvgen.VID, kvgen.INT], int_cells)
    res["graph"] = f"RMAT-{scale}"
    res["roots"] = nroots
    result["shapes"]["c2"] = res
    print("c2", res, flush=True)
    stmt.free()
    eng.close()

    # ---- strings: (VID, STRING) over a dictionary of 64 names
    s_scale = min(scale, 14)
    src, dst, w = rmat.rmat_edges_fast(s_scale)
    names = [f"name-{k:02d}" + "x" * (k % 16) for k in range(64)]
    schema = [("w", kvgen.INT), ("s", kvgen.STRING)]
    kb = kvgen.KVBuilder(8)
    for s_, d_, w_ in zip(src.tolist(), dst.tolist(), w.tolist()):
        kb.insert_edge(s_, d_, 1, 0, schema, [w_, names[(s_ ^ d_) % 64]], 1_600_000_000_000_000)
    eng = Engine(8)
    eng.register_edge(1, "e", schema)
    eng.load_builder(kb)
    sv, _ = rmat.vertex_sets(s_scale)
    roots = [int(x) for x in rmat.pick_roots(src, nroots, 42, verts=sv)]
    stmt = eng.prepare_go([1], 3, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "s").encode()])
    def string_cells(rows):
        d, ids = rows.fetch_bits()                  # (string cells: ids into the result's string table)
        text = {int(i): eng.lib.nbg_rows_string(rows.h, int(i)).decode() for i in np.unique(ids)}
        lens = np.zeros(max(text) + 1, np.int64)
        for i, t in text.items():
            lens[i] = len(t.encode())
        ends = lambda a, b: [(x, text[y]) for x, y in zip(a.tolist(), b.tolist())]   # noqa: E731
        return 8 + 1 + lens[ids], ends(d[:CHECK_ROWS], ids[:CHECK_ROWS]), ends(d[-CHECK_ROWS:], ids[-CHECK_ROWS:])
    res = measure(eng, stmt, roots, [kvgen.VID, kvgen.STRING], string_cells)
    res["graph"] = f"RMAT-{s_scale} (KV records, 64 dictionary strings)"
    res["roots"] = nroots
    result["shapes"]["strings"] = res
    print("strings", res, flush=True)
    stmt.free()
    eng.close()

    print(json.dumps(result))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
