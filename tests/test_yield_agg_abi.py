"""nbg_yield_agg at the C ABI: the symbol and its signature, the header text, the binding, and the
null-argument checks that need no rows (run on an engine that is not finalized, as
tests/test_yield_abi.py does).  Every check that needs a result object is in
tests/test_gpu_yield_agg.py."""
import ctypes as C
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_yield_agg")
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["nbg_yield_agg"]
    assert ret is _lib.i32 and len(args) == 4
    assert args == sigs["nbg_yield"][1]                 # the same request struct
    assert hasattr(Engine, "yield_agg") and hasattr(Engine, "yield_rows")


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("int32_t nbg_yield_agg(nbg_engine* e, const nbg_rows* in, const nbg_yield_request* req, nbg_rows** out);",
                   "nbg_yield_agg              ≙ YieldExecutor",
                   " * nbg_yield_agg (tests/test_gpu_yield_agg.py holds one test per limit",
                   "k_ya_reduce", "k_ya_finish"):
        assert needle in text, needle


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_yield_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_yield_agg(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield_agg(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield_agg(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_yield_agg(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
