"""nbg_set_op at the C ABI: the symbol, its signature and the request struct, and the null-argument
checks that need no rows (run on an engine that is not finalized, as tests/test_orderby_abi.py
does).  Every check that needs a result object is in tests/test_gpu_setops.py."""
import ctypes as C

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_set_op")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_set_op"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 5
    assert [f for f, _ in _lib.nbg_set_request._fields_] == ["op", "distinct"]
    assert C.sizeof(_lib.nbg_set_request) == 8
    assert (_lib.SET_UNION, _lib.SET_INTERSECT, _lib.SET_MINUS) == (1, 2, 3)
    assert _lib.SET_BY_NAME == {"UNION": 1, "INTERSECT": 2, "MINUS": 3}
    assert hasattr(Engine, "set_op")


def test_header_declares_it():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("#define NBG_SET_UNION     1", "#define NBG_SET_INTERSECT 2", "#define NBG_SET_MINUS     3",
                   "} nbg_set_request;", "int32_t nbg_set_op(nbg_engine* e, const nbg_rows* left, const nbg_rows* right,"):
        assert needle in text, needle


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_set_request(_lib.SET_UNION, 0)
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_set_op(None, None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_set_op(e.h, None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_set_op(e.h, None, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_set_op(e.h, None, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
