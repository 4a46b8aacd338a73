"""nbg_rows_decode at the C ABI: the symbol, its signature and the view struct, the header text, and
the argument checks that need no rows (run on an engine that is not finalized, as
tests/test_yield_abi.py does).  Every check that needs a device is in tests/test_gpu_rows_decode.py."""
import ctypes as C
import os

from nebula_amd import _lib, kvgen
from nebula_amd.engine import Engine


def test_symbol_and_signature():
    L = _lib.load()
    assert hasattr(L, "nbg_rows_decode")
    sig = {n: (r, a) for n, r, a in _lib.SIGNATURES}["nbg_rows_decode"]
    assert sig[0] is _lib.i32 and len(sig[1]) == 3
    assert [f for f, _ in _lib.nbg_rowset_view._fields_] == ["data", "len", "col_types", "num_cols"]
    # a pointer, a uint64, a pointer, an int32 (padded)
    assert C.sizeof(_lib.nbg_rowset_view) == 32
    assert _lib.nbg_rowset_view.len.offset == 8
    assert _lib.nbg_rowset_view.col_types.offset == 16
    assert _lib.nbg_rowset_view.num_cols.offset == 24
    assert hasattr(Engine, "rows_decode")


def test_header_declares_it():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbg.h")).read()
    for needle in ("} nbg_rowset_view;",
                   "int32_t nbg_rows_decode(nbg_engine* e, const nbg_rowset_view* rs, nbg_rows** out);",
                   "nbg_rows_decode ≙ InterimResult::getRows / RowSetReader + RowReader",
                   "const uint8_t* data;",
                   "const int32_t* col_types;",
                   " * nbg_rows_decode (tests/test_gpu_rows_decode.py holds one test per limit",
                   "k_rd_cells"):
        assert needle in text, needle
    # the struct's fields in the header's order are the ctypes fields
    body = text[text.index("typedef struct {\n  const uint8_t* data;"):text.index("} nbg_rowset_view;")]
    names = [line.split(";")[0].split()[-1].lstrip("*") for line in body.splitlines()[1:] if ";" in line]
    assert names == [f for f, _ in _lib.nbg_rowset_view._fields_]


def test_arguments_rejected():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    try:
        L = e.lib
        types = (C.c_int32 * 2)(kvgen.VID, kvgen.INT)
        data = (C.c_uint8 * 4)(3, 0, 1, 2)
        out = C.c_void_p()

        def view(d=data, n=4, t=types, nc=2):
            return _lib.nbg_rowset_view(d, n, t, nc)

        v = view()
        assert L.nbg_rows_decode(None, C.byref(v), C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_rows_decode(e.h, None, C.byref(out)) == _lib.E_INVALID_ARGUMENT
        assert L.nbg_rows_decode(e.h, C.byref(v), None) == _lib.E_INVALID_ARGUMENT
        for bad in (view(t=None), view(nc=0), view(nc=-1), view(d=None),
                    view(t=(C.c_int32 * 2)(kvgen.VID, 0)), view(t=(C.c_int32 * 2)(8, kvgen.INT))):
            assert L.nbg_rows_decode(e.h, C.byref(bad), C.byref(out)) == _lib.E_INVALID_ARGUMENT
            assert not out.value
        # good arguments reach the next check: the engine is not finalized
        assert L.nbg_rows_decode(e.h, C.byref(v), C.byref(out)) == _lib.E_STATE
        assert not out.value
    finally:
        e.close()
