"""The GO driver's argument checks, by status code, exact nbg_last_error text and order: the request
checks of nbg_go_prepare (engine state, steps, OVER, WHERE / YIELD decoding, the YIELD limit, the
`$-` input) and the null-argument checks of nbg_go_execute / nbg_go_submit / nbg_go_wait.  Where two
checks could both fire, the case names the one that comes first.

One single-GPU engine over a 6-edge graph with one INT property, and a second engine that is
registered but not finalized.  The library is called directly where the Python wrapper would reject
the request first.  Every call fails in its checks, before any kernel is launched; the last test
runs one one-step query to show the engine is still usable."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import _lib as L, expr as E, kvgen
from nebula_amd.engine import Engine

pytestmark = pytest.mark.gpu

W = E.edge_prop("e", "w").encode()
BAD = E.const(1).encode() + b"\x00"   # a whole expression and one byte more: undecodable
MAX_YIELDS = 32                        # NBG_MAX_YIELDS (include/nbg.h)


def _engine(finalize):
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    if finalize:
        e.load_edges(1, np.array([1, 1, 1, 2, 2, 3]), np.array([2, 3, 4, 3, 4, 4]), [np.array([5, 6, 7, 8, 9, 10])])
        e.finalize()
    return e


@pytest.fixture(scope="module")
def engines():
    good, raw = _engine(True), _engine(False)
    yield good, raw
    good.close()
    raw.close()


def _prepare(eng, etypes=(1,), steps=1, where=b"", yields=()):
    """nbg_go_prepare called directly: (status, nbg_last_error)."""
    req, keep = eng._go_request([1], list(etypes), steps, where, list(yields), False, False)
    out = C.c_void_p()
    rc = eng.lib.nbg_go_prepare(eng.h, C.byref(req), C.byref(out))
    if rc == L.OK:
        eng.lib.nbg_go_stmt_free(out)
    return rc, eng.lib.nbg_last_error(eng.h).decode()


# (id, the unfinalized engine?, request, status, text; a text ending in "..." is a prefix)
PREPARE = [
    ("unfinalized", True, {}, L.E_STATE, "engine not finalized"),
    ("unfinalized_before_steps", True, {"steps": 0}, L.E_STATE, "engine not finalized"),
    ("steps_0", False, {"steps": 0}, L.E_INVALID_ARGUMENT, "steps must be >= 1"),
    ("steps_before_over", False, {"steps": 0, "etypes": (99,)}, L.E_INVALID_ARGUMENT, "steps must be >= 1"),
    ("reversely", False, {"etypes": (-1,)}, L.E_EXECUTION_ERROR, "`REVERSELY' not supported yet"),
    ("unknown_edge", False, {"etypes": (99,)}, L.E_EXECUTION_ERROR, "edge type not found"),
    ("empty_over", False, {"etypes": ()}, L.E_EXECUTION_ERROR, "empty OVER clause"),
    ("where_bytes", False, {"where": BAD}, L.E_INVALID_ARGUMENT, "WHERE: ..."),
    ("yield_bytes", False, {"yields": [BAD]}, L.E_INVALID_ARGUMENT, "YIELD: ..."),
    ("too_many_yields", False, {"yields": [W] * (MAX_YIELDS + 1)}, L.E_UNSUPPORTED, "too many YIELD columns"),
    ("input_prop_without_input", False, {"yields": [E.input_prop("w").encode()]}, L.E_EXECUTION_ERROR,
     "$- / $var props need the piped or variable input"),
]


@pytest.mark.parametrize("raw,request_,code,text", [c[1:] for c in PREPARE], ids=[c[0] for c in PREPARE])
def test_prepare_guards(engines, raw, request_, code, text):
    rc, msg = _prepare(engines[1] if raw else engines[0], **request_)
    assert rc == code
    if text.endswith("..."):
        assert msg.startswith(text[:-3]) and len(msg) > len(text) - 3
    else:
        assert msg == text


def _execute(eng, starts, out):
    """nbg_go_execute on a good statement with num_starts = 1, after a failure with another text."""
    st = eng.prepare_go([1], 1)
    try:
        assert _prepare(eng, steps=0)[1] == "steps must be >= 1"
        rc = eng.lib.nbg_go_execute(st.h, starts, 1, 0, out)
        return rc, eng.lib.nbg_last_error(eng.h).decode()
    finally:
        st.free()


def test_execute_null_starts(engines):
    out = C.c_void_p()
    assert _execute(engines[0], None, C.byref(out)) == (L.E_INVALID_ARGUMENT, "null argument")
    assert not out.value


def test_execute_null_out(engines):
    starts = (C.c_int64 * 1)(1)
    assert _execute(engines[0], starts, None) == (L.E_INVALID_ARGUMENT, "null argument")


def test_submit_null_statement(engines):
    starts = (C.c_int64 * 1)(1)
    out = C.c_void_p()
    assert engines[0].lib.nbg_go_submit(None, starts, 1, 0, C.byref(out)) == L.E_INVALID_ARGUMENT


def test_wait_null_ticket(engines):
    out = C.c_void_p()
    assert engines[0].lib.nbg_go_wait(None, C.byref(out)) == L.E_INVALID_ARGUMENT


def test_engine_still_usable(engines):
    """After every failure above (the module's tests run in file order), GO 1 STEP from vertex 1."""
    assert sorted(engines[0].go([1], [1], 1, b"", [W])) == [[5], [6], [7]]
