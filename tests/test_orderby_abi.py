"""nbg_order_by at the C ABI: the symbol, its signature and the request struct, and the argument
checks that need no rows (run on an engine that is not finalized, as tests/test_abi.py does).
Negative offsets / counts and host-only rows need a result object, which only exists after a
query ran: those checks are in tests/test_gpu_orderby.py."""
import ctypes as C

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_order_by")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_order_by"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 4
    fields = [f for f, _ in _lib.nbg_order_request._fields_]
    assert fields == ["input_names", "factor_names", "factor_desc", "num_factors", "has_limit", "offset", "count"]
    # the header's struct: three pointers, two int32, two int64
    assert C.sizeof(_lib.nbg_order_request) == 3 * 8 + 2 * 4 + 2 * 8
    assert _lib.nbg_order_request.offset.offset == 32 and _lib.nbg_order_request.count.offset == 40
    assert hasattr(Engine, "order_by")


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_order_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_order_by(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_order_by(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_order_by(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_order_by(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
