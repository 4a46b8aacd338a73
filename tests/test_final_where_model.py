"""The numpy model of tests/support/finalwhere.py against the storage oracle, for every (column,
constant, operator, operand order) the GPU tests of test_gpu_final_where.py use, and the
properties of the graph and the constants that keep those tests from passing vacuously.  No GPU."""
import numpy as np
import pytest

from tests.support import finalwhere as FW


@pytest.fixture(scope="module")
def world():
    g = FW.Graph()
    orc = g.oracle()
    yield g, orc
    orc.close()


def test_constant_sets():
    assert [len(FW.constants(c)) for c in FW.COLUMNS] == [21, 21, 17, 15]
    for c in FW.COLUMNS:
        lo, hi = FW.width_range(c)
        ks = FW.constants(c)
        assert set(FW.width_edge_constants(c)) <= set(ks)
        for k in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, -1, 0, 1, 5, FW.I32_MIN - 1, FW.I32_MIN, FW.I32_MAX,
                  FW.I32_MAX + 1, 2 ** 32, -2 ** 32, FW.LOW5, FW.I64_MIN, FW.I64_MIN + 1, FW.I64_MAX - 1, FW.I64_MAX):
            assert (k in ks) == (FW.I64_MIN <= k <= FW.I64_MAX), (c, k)
        assert len(FW.cases(c)) == len(ks) * 12


def test_graph_shape(world):
    g, _ = world
    assert len(g.src) == 10 + 3 + sum(FW.DEGS) + sum(FW.DEGS2) == 1719
    assert g.step_stats("R", 2) == ([1, 10], [10, sum(FW.DEGS)])
    assert g.step_stats("mids", 1) == ([10], [sum(FW.DEGS)])
    assert g.step_stats("R2", 2) == ([1, 3], [3, sum(FW.DEGS2)])
    finals = np.concatenate([g.final["R"], g.final["R2"]])
    assert len(np.unique(g.dst[finals])) == len(finals) and g.dst[finals].min() >= FW.LEAF
    for c in FW.COLUMNS:
        assert not g.cols[c][:13].any()   # (the first hop's edges carry 0: they widen no column)


@pytest.mark.parametrize("col", FW.COLUMNS)
def test_columns_fill_their_width(world, col):
    """Both loaders choose the stored width from a column's min and max: each column holds its
    width's min and max and nothing outside it (a64: the int64 extremes, so no narrow copy)."""
    g, _ = world
    lo, hi = FW.width_range(col)
    cells = g.cols[col]
    assert int(cells.min()) == lo and int(cells.max()) == hi
    for starts in ("R", "R2"):
        assert set(FW.base_cells(col)) <= set(cells[g.final[starts]].tolist()), starts
    assert (cells[g.final["R"]] < 0).any() and (cells[g.final["R"]] > 0).any()


@pytest.mark.parametrize("col", FW.COLUMNS)
def test_model_against_oracle(world, col):
    """GO 2 STEPS FROM R WHERE ... YIELD _dst, e.<col>: the model's rows are the storage oracle's,
    and the case list holds WHEREs that pass no row, every row and a strict subset."""
    g, orc = world
    ys = FW.yield_bytes(("_dst", col))
    total = len(g.final["R"])
    seen = set()
    for op, k, left in FW.cases(col):
        exp = g.rows("R", ("_dst", col), col, op, k, left)
        got = sorted(tuple(r) for r in orc.go([FW.R], [FW.E_TYPE], 2, FW.where_bytes(col, op, k, left), ys))
        assert got == [tuple(r) for r in exp.tolist()], (col, op, k, left, len(got), len(exp))
        seen.add("none" if len(exp) == 0 else "all" if len(exp) == total else "some")
    assert seen == {"none", "all", "some"}
    lo, hi = FW.width_range(col)
    for k in (lo, hi):
        assert len(g.rows("R", ("_dst",), col, "==", k)) >= 1, k
        assert len(g.rows("R2", ("_dst",), col, "==", k)) >= 1, k
    # 2^32 + 5 is a cell of a64 only; 5 is a cell of every column
    assert len(g.rows("R", ("_dst",), col, "==", 5)) >= 1
    assert (len(g.rows("R", ("_dst",), col, "==", FW.LOW5)) >= 1) == (col == "a64")
    assert (len(g.rows("R", ("_dst",), col, "==", FW.LOW5, True)) >= 1) == (col == "a64")


def test_model_against_oracle_other_shapes(world):
    """The statements of the other routes over the oracle, one WHERE per column: GO FROM <mids>,
    the small root, the interpreter's wrapped WHERE, constant and many-column YIELDs."""
    g, orc = world
    for col in FW.COLUMNS:
        lo, hi = FW.width_range(col)
        for op, k, left in (("<", hi, False), (">=", lo + 1, True), ("!=", 5, False)):
            for route in FW.ROUTES.values():
                for v in route.variants:
                    exp = g.rows(v.starts, v.yields, col, op, k, left)
                    got = sorted(tuple(r) for r in orc.go(g.starts[v.starts], [FW.E_TYPE], v.steps,
                                                          FW.where_bytes(col, op, k, left, v.interp),
                                                          FW.yield_bytes(v.yields)))
                    assert got == [tuple(r) for r in exp.tolist()], (route.name, col, op, k, left)
