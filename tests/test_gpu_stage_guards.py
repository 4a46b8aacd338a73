"""The guards every stage over device-resident rows shares, by their texts: rows of another engine
and a host-only result are both NBG_E_INVALID_ARGUMENT, and nbg_last_error names the stage.  The
statuses are tested per stage (tests/test_gpu_groupby.py ... test_gpu_fetch.py); here the label of
each stage is matched literally, for either side of nbg_set_op too.

Two single-GPU engines over the same 6-edge graph with one INT property; one nbg_go_device result
and one host-only nbg_go result from each.  Every call fails in its argument checks: no stage
kernel is launched."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import _lib as L, expr as E, kvgen
from nebula_amd.engine import DeviceRows, Engine, NbgError

pytestmark = pytest.mark.gpu

OTHER = "{}: the rows belong to another engine"
HOST = "{}: the rows are host-only (not a device result)"
W = E.input_prop("w").encode()


def _engine():
    e = Engine(num_parts=3)
    e.register_edge(1, "e", [("w", kvgen.INT)])
    e.load_edges(1, np.array([1, 1, 1, 2, 2, 3]), np.array([2, 3, 4, 3, 4, 4]), [np.array([5, 6, 7, 8, 9, 10])])
    e.finalize()
    return e


class Side:
    def __init__(self):
        self.eng = _engine()
        ys = [E.edge_prop("e", "w").encode()]
        self.dev = self.eng.go_device([1], [1], 1, b"", ys)
        req, keep = self.eng._go_request([1], [1], 1, b"", ys, False, False)
        h = C.c_void_p()
        assert self.eng.lib.nbg_go(self.eng.h, C.byref(req), C.byref(h)) == L.OK     # rows copied to the host
        self.host = DeviceRows(self.eng, h)
        assert self.dev.count == 3 and self.host.count == 3

    def close(self):
        self.dev.free()
        self.host.free()
        self.eng.close()


@pytest.fixture(scope="module")
def sides():
    a, b = Side(), Side()
    yield a, b
    a.close()
    b.close()


# (stage label, Engine method name in the error text, the call given the engine, the rows under test and good rows)
STAGES = [
    ("GROUP BY", "group_by", lambda e, bad, good: e.group_by(bad, ["w"], [W], [("COUNT", E.const("*").encode(), None)])),
    ("ORDER BY", "order_by", lambda e, bad, good: e.order_by(bad, ["w"], [("w", False)])),
    ("set operation", "set_op", lambda e, bad, good: e.set_op(bad, good, "UNION")),
    ("set operation", "set_op", lambda e, bad, good: e.set_op(good, bad, "UNION")),   # the right-hand side
    ("YIELD", "yield_rows", lambda e, bad, good: e.yield_rows(bad, ["w"], [W])),
    ("FETCH", "fetch_vertices", lambda e, bad, good: e.fetch_vertices(bad, ["w"], "w", 7, [W])),
]
IDS = ["group_by", "order_by", "set_op_left", "set_op_right", "yield", "fetch_vertices"]


def _fails(call, what, text):
    with pytest.raises(NbgError) as ex:
        call().free()
    assert ex.value.code == L.E_INVALID_ARGUMENT
    assert str(ex.value) == f"nbg error {L.E_INVALID_ARGUMENT}: {what}: {text}"


@pytest.mark.parametrize("label,what,call", STAGES, ids=IDS)
def test_rows_of_another_engine(sides, label, what, call):
    a, b = sides
    _fails(lambda: call(a.eng, b.dev, a.dev), what, OTHER.format(label))


@pytest.mark.parametrize("label,what,call", STAGES, ids=IDS)
def test_host_only_rows(sides, label, what, call):
    a, _ = sides
    _fails(lambda: call(a.eng, a.host, a.dev), what, HOST.format(label))
