"""The final step's `WHERE <int col> <cmp> <const>` on every route of tests/support/finalwhere.py:
columns that fill their stored width (1, 2, 4 and 8 bytes, negative cells included), constants at
and beyond the ends of every width, at the int32 and int64 extremes and with low 32 bits that equal
a stored cell, all six operators, the constant on either side.  Rows are compared with the numpy
model (which test_final_where_model.py holds against the storage oracle), edges_scanned and the
per-step statistics with step_model: the WHERE must not change them.

Every (column, route) case runs all of the column's WHEREs, the constant-on-the-left variants of
every constant included."""
import functools

import numpy as np
import pytest

from nebula_amd import NbgError
from tests.support import finalwhere as FW

pytestmark = pytest.mark.gpu

_device_error = []


def stops_after_a_device_error(test):
    """A device error ends the module: the tests after it fail without another launch."""
    @functools.wraps(test)
    def run(*a, **kw):
        if _device_error:
            pytest.fail("not run: device error in %s" % _device_error[0])
        try:
            return test(*a, **kw)
        except NbgError:
            _device_error.append(test.__name__)
            raise
    return run


@pytest.fixture(scope="module")
def graph():
    return FW.Graph()


@pytest.fixture(scope="module")
def engine(graph):
    eng = graph.engine()
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def restored(graph, engine, tmp_path_factory):
    """A fresh engine loaded from `engine`'s snapshot file: its narrow copies are made on the host
    (Engine::upload_type), the writer's by k_narrow."""
    from nebula_amd import Engine
    path = str(tmp_path_factory.mktemp("finalwhere") / "snap.nbg")
    engine.snapshot_save(path)
    eng = Engine(100)
    try:
        eng.snapshot_load(path)
        yield eng
    finally:
        eng.close()


@pytest.fixture(scope="module")
def kv_engine(graph):
    eng = graph.kv_engine()
    yield eng
    eng.close()


def report(n, bad):
    print("%d statements, %d mismatches" % (n, len(bad)))
    assert not bad, "%d of %d: %s" % (len(bad), n, "; ".join(bad[:6]))


@pytest.mark.parametrize("route", list(FW.ROUTES))
@pytest.mark.parametrize("col", FW.COLUMNS)
@stops_after_a_device_error
def test_where_edges(graph, engine, col, route):
    tiny = engine.stats()["tiny_queries"]
    n, bad = FW.run_route(graph, engine, route, col)
    if route == "tiny":
        assert engine.stats()["tiny_queries"] == tiny + n   # (fails if the path was never taken)
    else:
        assert engine.stats()["tiny_queries"] == tiny
    report(n, bad)


@pytest.mark.parametrize("route", ["fast_cols", "wide_cols"])
@stops_after_a_device_error
def test_yield_reads_narrow_columns(graph, engine, route):
    """Without a WHERE and with two per column (one passes most rows, one a few), the column-reading
    kernels return every cell of every column exactly: each width's min and max and the negative
    one-byte cells among them."""
    yields = {"fast_cols": [("_dst", "a8", "a16"), ("_dst", "a32", "a64"), ("_dst", "a16", "a8")],
              "wide_cols": [("_dst",) + FW.COLUMNS, ("_dst",) + FW.COLUMNS[::-1]]}[route]
    wheres = [(None, None, None, False)] + [(c, "!=", 5, False) for c in FW.COLUMNS] + \
             [(c, ">", FW.width_range(c)[0] + 1, True) for c in FW.COLUMNS]
    n = 0
    for v0 in FW.ROUTES[route].variants:
        for ys in yields:
            v = FW.Variant(v0.steps, v0.starts, ys)
            all_rows = graph.rows(v.starts, ys)
            for y, name in enumerate(ys[1:], 1):   # (what "every cell" means here)
                lo, hi = FW.width_range(name)
                assert all_rows[:, y].min() == lo and all_rows[:, y].max() == hi
                assert name != "a8" or np.count_nonzero(all_rows[:, y] < 0) > 100
            for col, op, k, left in wheres:
                n += 1
                got = FW.run_variant(graph, engine, v, col, op, k, left)
                assert not got, (route, ys, col, op, k, left, got)
    assert n == len(FW.ROUTES[route].variants) * len(yields) * 9


@pytest.mark.parametrize("col", FW.COLUMNS)
@stops_after_a_device_error
def test_snapshot_restored_engine(graph, restored, col):
    """lean_dst, index_copy, fast_cols and wide_cols over the engine restored from a snapshot, with
    the width-edge constants: the host-made narrow copies against the model."""
    n, bad = 0, []
    for route in ("lean_dst", "index_copy", "fast_cols", "wide_cols"):
        k, b = FW.run_route(graph, restored, route, col, FW.width_edge_constants(col))
        n, bad = n + k, bad + b
    report(n, bad)


@pytest.mark.parametrize("col", FW.COLUMNS)
@stops_after_a_device_error
def test_kv_loaded_engine(graph, kv_engine, col):
    """The same graph loaded as KV records: lean_dst and index_copy with the width-edge constants."""
    n, bad = 0, []
    for route in ("lean_dst", "index_copy"):
        k, b = FW.run_route(graph, kv_engine, route, col, FW.width_edge_constants(col))
        n, bad = n + k, bad + b
    report(n, bad)
