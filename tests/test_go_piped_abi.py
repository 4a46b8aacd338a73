"""nbg_go_piped at the C ABI: the symbol and its signature, the header text, and the null-argument
checks that need no rows (run on an engine that is not finalized, as tests/test_fetch_edges_abi.py
does).  Every check that needs a result object is in tests/test_gpu_go_piped.py."""
import ctypes as C
import inspect
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_go_piped")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_go_piped"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 5
    assert L.nbg_go_piped.restype is _lib.i32 and len(L.nbg_go_piped.argtypes) == 5
    # the request is nbg_go's, unchanged
    assert sig[1][2] is C.POINTER(_lib.nbg_go_request)
    assert [f for f, _ in _lib.nbg_go_request._fields_][-6:] == [
        "num_input_cols", "input_names", "input_kinds", "input_cols", "num_input_rows", "input_vid_col"]
    assert hasattr(Engine, "go_piped")
    params = list(inspect.signature(Engine.go_piped).parameters)
    assert params == ["self", "rows", "input_names", "vid_col", "etypes", "steps", "where", "yields", "distinct",
                      "over_all", "device"]
    assert inspect.signature(Engine.go_piped).parameters["device"].default is True


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("int32_t nbg_go_piped(nbg_engine* e, const nbg_rows* in, const nbg_go_request* req, int32_t device, "
                   "nbg_rows** out);",
                   "nbg_go_piped               ≙ GoExecutor::setupStarts",
                   " * nbg_go_piped (tests/test_gpu_go_piped.py holds one test per limit",
                   "k_gp_resolve, k_gp_table, k_gp_degrees, k_gp_emit, k_gp_compact"):
        assert needle in text, needle
    # the call's own comment: its statuses, numbered 1 to 7, between its title and its prototype
    body = text[text.index("GO FROM $-.col / $var.col over a device-resident result"):text.index("int32_t nbg_go_piped(")]
    assert "Statuses, in this order:" in body
    statuses = body[body.index("Statuses, in this order:"):]
    for k in range(1, 8):
        assert f" *  {k}. " in statuses, k
    assert "Device limits" in statuses
    # the Device-limits paragraph names every limit of the call
    limits = text[text.index(" * nbg_go_piped (tests/test_gpu_go_piped.py"):text.index("(A storage filter with a function call")]
    for needle in ("a partitioned engine", "a misaligned or FLOAT column", "col_kind == -1",
                   "strings outside the dictionary", "an input of 2^32 rows or more", "2^32 - 1"):
        assert needle in limits, needle


def test_null_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        req = _lib.nbg_go_request()
        out = C.c_void_p()
        L = e.lib
        fake = C.c_void_p(8)   # (never dereferenced: every call below fails on a null argument first)
        assert L.nbg_go_piped(None, fake, C.byref(req), 1, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_go_piped(e.h, None, C.byref(req), 1, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_go_piped(e.h, fake, None, 1, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_go_piped(e.h, fake, C.byref(req), 1, None) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_go_piped(e.h, None, C.byref(req), 0, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert not out.value
    finally:
        e.close()
