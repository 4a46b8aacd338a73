#!/usr/bin/env python3
"""nbg_rows_decode of the RowSetWriter bytes of a device result: what the way back onto the device
costs, and where the time goes.

Shape "c2": RMAT-22 (the C2 graph), `GO 3 STEPS ... YIELD e._dst AS d, e.w AS w` from 32 roots, run
once to the device and encoded with nbg_rows_encode.  Shape "strings": RMAT-14 built from KV records
whose edges carry a dictionary string (64 distinct names of 8 to 23 bytes), `GO 3 STEPS ... YIELD
e._dst AS d, e.s AS s`.  Per shape, each after warm-up calls and over several repeats (the median is
reported, min and max are kept):
  * nbg_rows_decode of the bytes, which lie in ordinary (pageable) host memory as a caller's would
    (the nbg_rows_free after it is outside the timer);
  * for comparison, a plain hipMemcpy host-to-device of the same number of bytes from the same
    pageable buffer and from pinned memory (the floor: what any route onto the device pays), and
    nbg_rows_encode of the same rows (the inverse).
All calls are synchronous, so the times are host-clock times around the call.  One more decode with
nbg_profile on gives the breakdown (not part of the timed runs; with the profile on the call waits
for the upload before it launches): rd_host_walk, the host walk of the length prefixes;
rd_host_upload, the copy into the pinned block plus the DMA of bytes, chunk starts and row offsets;
k_rd_cells, the kernel's event time with its algorithmic bytes (include/nbg.h) and the fraction of
the 8 TB/s HBM peak they come to.  What is left of the call beside the three (allocating the result
and the device copy, the pinned block, the record's read-back) is reported as "rest".
The decoded rows are checked outside the timed region: their digest (nbg_rows_digest, computed in
HBM) and their re-encoded bytes equal the original's.
Usage: rows_decode_probe.py [scale] [roots] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nebula_amd import Engine, _lib as L, expr as E, kvgen, rmat  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, REPEATS = 3, 9
PARTS = ("rd_host_walk", "rd_host_upload", "k_rd_cells")


def timed(fn, after=None):
    ts = []
    for i in range(WARMUP + REPEATS):
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        if after:
            after(r)
        if i >= WARMUP:
            ts.append(t1 - t0)
    return {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}


def memcpy_floor(buf):
    """hipMemcpy host-to-device of buf's bytes: from buf itself (pageable) and from pinned memory."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipHostFree.argtypes = [C.c_void_p]
    n = len(buf)
    dev, pin = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), n) == 0 and hip.hipHostMalloc(C.byref(pin), n, 0) == 0
    C.memmove(pin, buf.ctypes.data, n)
    H2D = 1

    def copy(src):
        assert hip.hipMemcpy(dev, src, n, H2D) == 0
    out = {"pageable": timed(lambda: copy(buf.ctypes.data)), "pinned": timed(lambda: copy(pin))}
    for v in out.values():
        v["GBps"] = n / v["seconds_median"] / 1e9
    hip.hipFree(dev)
    hip.hipHostFree(pin)
    return out


def measure(eng, stmt, roots):
    lib = eng.lib
    rows = stmt.run_device(roots)
    n = rows.count
    data, types = rows.encode()
    buf = np.frombuffer(data, np.uint8)
    t = (C.c_int32 * len(types))(*types)
    view = L.nbg_rowset_view(buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), t, len(types))

    def decode():
        out = C.c_void_p()
        rc = lib.nbg_rows_decode(eng.h, C.byref(view), C.byref(out))
        assert rc == 0, (rc, lib.nbg_last_error(eng.h))
        return out
    dec = timed(decode, lib.nbg_rows_free)

    def encode():
        out = C.c_void_p()
        assert lib.nbg_rows_encode(eng.h, rows.h, C.byref(out)) == 0
        return out
    enc = timed(encode, lib.nbg_rowset_free)
    floor = memcpy_floor(buf)

    eng.profile(True)
    t0 = time.perf_counter()
    out = decode()
    profiled = time.perf_counter() - t0
    prof = {k: v for k, v in eng.profile_read().items() if k in PARTS}
    eng.profile(False)
    k = prof["k_rd_cells"]
    k["bytes_per_s"] = k["algo_bytes"] / (k["ms"] * 1e-3)
    k["hbm_fraction"] = k["bytes_per_s"] / HBM_PEAK
    parts = {p: prof[p]["ms"] * 1e-3 for p in PARTS}
    parts["rest"] = profiled - sum(parts.values())
    # the check, outside the timed region
    from nebula_amd.engine import DeviceRows
    back = DeviceRows(eng, out)
    ok = back.count == n and back.digest() == rows.digest() and back.encode() == (data, types)
    back.free()
    rows.free()
    med = dec["seconds_median"]
    res = {"rows": n, "columns": len(types), "encoded_bytes": len(buf), "bytes_per_row": len(buf) / n,
           "uploaded_bytes": prof["rd_host_upload"]["algo_bytes"],
           "decode": dict(dec, rows_per_s=n / med, GBps=len(buf) / med / 1e9),
           "encode": enc, "hipMemcpy_h2d_same_bytes": floor,
           "decode_over_pinned_memcpy": med / floor["pinned"]["seconds_median"],
           "decode_over_pageable_memcpy": med / floor["pageable"]["seconds_median"],
           "decode_over_encode": med / enc["seconds_median"],
           "profiled_call_seconds": profiled, "breakdown_seconds": parts,
           "breakdown_fraction": {p: v / profiled for p, v in parts.items()},
           "largest_part": max(parts, key=parts.get),
           "walk_ns_per_row": parts["rd_host_walk"] / n * 1e9,
           "kernel_over_upload": parts["k_rd_cells"] / parts["rd_host_upload"],
           "kernels": prof, "matches_original": ok}
    assert ok, "the decoded rows differ from the original"
    return res


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    nroots = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    result = {"warmup": WARMUP, "repeats": REPEATS,
              "timing": "host clock around each synchronous call; the breakdown from one more call with nbg_profile on",
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
    res = measure(eng, stmt, roots)
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
    res = measure(eng, stmt, roots)
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
