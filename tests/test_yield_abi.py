"""nbg_yield at the C ABI: the symbol, its signature and the request struct, the header text, and
the null-argument checks that need no rows (run on an engine that is not finalized, as
tests/test_setops_abi.py does).  Every check that needs a result object is in
tests/test_gpu_yield.py."""
import ctypes as C
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_yield")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_yield"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 4
    assert [f for f, _ in _lib.nbg_yield_request._fields_] == [
        "input_names", "where", "where_len", "yield_exprs", "yield_lens", "yield_funs", "num_yields"]
    # three pointers, a uint32 (padded), three pointers, an int32 (padded)
    assert C.sizeof(_lib.nbg_yield_request) == 56
    assert _lib.nbg_yield_request.where_len.offset == 16
    assert _lib.nbg_yield_request.num_yields.offset == 48
    assert hasattr(Engine, "yield_rows")


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("} nbg_yield_request;",
                   "int32_t nbg_yield(nbg_engine* e, const nbg_rows* in, const nbg_yield_request* req, nbg_rows** out);",
                   "nbg_yield                  ≙ YieldExecutor",
                   "const int32_t* yield_funs;",
                   " * nbg_yield (tests/test_gpu_yield.py holds one test per limit",
                   "k_yr_filter"):
        assert needle in text, needle


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_yield_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_yield(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
