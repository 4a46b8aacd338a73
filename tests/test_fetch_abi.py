"""nbg_fetch_vertices at the C ABI: the symbol, its signature and the request struct, the header
text, and the null-argument checks that need no rows (run on an engine that is not finalized, as
tests/test_yield_abi.py does).  Every check that needs a result object is in
tests/test_gpu_fetch.py."""
import ctypes as C
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_fetch_vertices")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_fetch_vertices"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 4
    R = _lib.nbg_fetch_request
    assert [f for f, _ in R._fields_] == [
        "input_names", "vid_col", "vids", "num_vids", "tag_id", "yield_exprs", "yield_lens", "num_yields", "distinct"]
    # three pointers, a uint64, an int32 (padded), two pointers, two int32
    assert C.sizeof(R) == 64
    assert R.vid_col.offset == 8 and R.vids.offset == 16 and R.num_vids.offset == 24
    assert R.tag_id.offset == 32 and R.yield_exprs.offset == 40 and R.yield_lens.offset == 48
    assert R.num_yields.offset == 56 and R.distinct.offset == 60
    assert hasattr(Engine, "fetch_vertices")


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("} nbg_fetch_request;",
                   "int32_t nbg_fetch_vertices(nbg_engine* e, const nbg_rows* in, const nbg_fetch_request* req, "
                   "nbg_rows** out);",
                   "nbg_fetch_vertices         ≙ FetchVerticesExecutor",
                   "const char* vid_col;",
                   "const int64_t* vids;",
                   "int32_t distinct;",
                   " * nbg_fetch_vertices (tests/test_gpu_fetch.py holds one test per limit",
                   "k_fv_resolve"):
        assert needle in text, needle
    # the struct's members in the header's order are the ctypes fields
    body = text[text.index("typedef struct {", text.index("FetchVerticesExecutor) ------")):text.index("} nbg_fetch_request;")]
    members = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln.split("/*")[0]]
    assert members == [f for f, _ in _lib.nbg_fetch_request._fields_]


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_fetch_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_fetch_vertices(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_fetch_vertices(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_fetch_vertices(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        req.num_vids = 3                      # in == NULL, vids == NULL, num_vids > 0
        assert L.nbg_fetch_vertices(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        req.num_vids, req.num_yields = 0, 2   # YIELDs announced, none given
        assert L.nbg_fetch_vertices(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
