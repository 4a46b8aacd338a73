"""nbg_fetch_edges at the C ABI: the symbol, its signature and the request struct, the header text,
and the null-argument checks that need no rows (run on an engine that is not finalized, as
tests/test_fetch_abi.py does).  Every check that needs a result object is in
tests/test_gpu_fetch_edges.py."""
import ctypes as C
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine

FIELDS = ["input_names", "src_col", "dst_col", "rank_col", "srcs", "dsts", "ranks", "num_keys", "edge_type",
          "yield_exprs", "yield_lens", "num_yields", "distinct"]


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_fetch_edges")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_fetch_edges"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 4
    R = _lib.nbg_fetch_edges_request
    assert [f for f, _ in R._fields_] == FIELDS
    # seven pointers, a uint64, an int32 (padded), two pointers, two int32
    assert C.sizeof(R) == 96
    assert R.src_col.offset == 8 and R.dst_col.offset == 16 and R.rank_col.offset == 24
    assert R.srcs.offset == 32 and R.dsts.offset == 40 and R.ranks.offset == 48 and R.num_keys.offset == 56
    assert R.edge_type.offset == 64 and R.yield_exprs.offset == 72 and R.yield_lens.offset == 80
    assert R.num_yields.offset == 88 and R.distinct.offset == 92
    assert hasattr(Engine, "fetch_edges")


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("} nbg_fetch_edges_request;",
                   "int32_t nbg_fetch_edges(nbg_engine* e, const nbg_rows* in, const nbg_fetch_edges_request* req, "
                   "nbg_rows** out);",
                   "nbg_fetch_edges ≙ FetchEdgesExecutor (src/graph/FetchEdgesExecutor.cpp:17-384, "
                   "src/graph/FetchExecutor.cpp:14-131, src/storage/QueryEdgePropsProcessor.cpp:17-101)",
                   "const char* src_col;", "const char* dst_col;", "const char* rank_col;",
                   "const int64_t* srcs;", "const int64_t* ranks;", "int32_t edge_type;",
                   " * nbg_fetch_edges (tests/test_gpu_fetch_edges.py holds one test per limit",
                   "Unspecified in the reference: an edge whose value does not decode.",
                   "Statuses, in this order:", "k_fe_resolve, k_fe_emit"):
        assert needle in text, needle
    # the struct's members in the header's order are the ctypes fields
    body = text[text.index("typedef struct {", text.index("FetchEdgesExecutor) ------")):text.index("} nbg_fetch_edges_request;")]
    members = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln.split("/*")[0]]
    assert members == FIELDS


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_fetch_edges_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_fetch_edges(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_fetch_edges(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_fetch_edges(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        req.num_keys = 3                      # in == NULL, srcs == dsts == NULL, num_keys > 0
        assert L.nbg_fetch_edges(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        keys = (C.c_int64 * 3)(1, 2, 3)
        req.srcs = keys                       # ... dsts still NULL
        assert L.nbg_fetch_edges(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        req.srcs, req.num_keys, req.num_yields = None, 0, 2   # YIELDs announced, none given
        assert L.nbg_fetch_edges(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
