"""nbg_group_by at the C ABI: the symbol and its signature, argument checks that need no rows (run
on an engine that is not finalized, as tests/test_abi.py does), and the rejection of a host-only
result.  A result object only exists after a query ran, so that last check needs the device and
is marked gpu; the others are CPU tests."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import _lib, expr as E, kvgen
from nebula_amd.engine import Engine, NbgError


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_group_by")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_group_by"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 4
    fields = [f for f, _ in _lib.nbg_group_request._fields_]
    assert fields == ["input_names", "group_exprs", "group_lens", "num_groups", "yield_exprs", "yield_lens",
                      "yield_funs", "yield_aliases", "num_yields"]
    # the header's struct: three pointers, an int32 (padded), four pointers, an int32 (padded)
    assert C.sizeof(_lib.nbg_group_request) == 9 * 8
    assert _lib.E_SYNTAX_ERROR == -7
    assert [_lib.AGG_BY_NAME[n] for n in ("", "COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MAX", "MIN", "STD",
                                          "BIT_AND", "BIT_OR", "BIT_XOR")] == list(range(11))


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_group_request()
        out = C.c_void_p()
        L = e.lib
        assert L.nbg_group_by(None, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_group_by(e.h, None, C.byref(req), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_group_by(e.h, None, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_group_by(e.h, None, C.byref(req), None) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()


@pytest.mark.gpu
def test_host_only_rows_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    e.load_edges(1, np.array([1, 1]), np.array([2, 3]), [np.array([5, 6])])
    e.finalize()
    try:
        req, keep = e._go_request([1], [1], 1, b"", [E.edge_prop("e", "w").encode()], False, False)
        rows = C.c_void_p()
        assert e.lib.nbg_go(e.h, C.byref(req), C.byref(rows)) == _lib.OK     # rows copied to the host
        from nebula_amd.engine import DeviceRows
        with pytest.raises(NbgError) as ex:
            e.group_by(DeviceRows(e, rows), ["w"], [E.input_prop("w").encode()],
                       [("COUNT", E.const("*").encode(), None)])
        assert ex.value.code == _lib.E_INVALID_ARGUMENT
    finally:
        e.close()
