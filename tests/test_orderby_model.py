"""Pins the ORDER BY / LIMIT checker (tests/support/orderby.py: parser, model, session) to the
reference's own OrderByTest and GroupByLimitTest vectors before it judges the device: over the CPU
oracle's GO rows the model reproduces every case of tests/golden/orderby_golden.json — statuses,
column names and row counts where the reference asserts them, rows in order where the reference
compares them unsorted.  CPU only."""
import pytest

from nebula_amd import _lib
from tests.support import golden, groupby, orderby
from tests.support.ngql import Interim
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("orderby_golden.json")
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def test_golden_file_shape():
    assert len(CASES) == 27
    assert sum(c["source"].endswith("OrderByTest.cpp") for c in CASES) == 16
    assert sum(c["status"] == "E_SYNTAX_ERROR" for c in CASES) == 4
    assert sum(c["status"] == "E_EXECUTION_ERROR" for c in CASES) == 1
    assert sum(bool(c.get("ordered")) for c in CASES) == 16
    assert sum(c.get("match") is False for c in CASES) == 1
    # every GroupByLimitTest case groupby_golden.json skipped for its ORDER BY / LIMIT is here
    skipped = [s["query"] for s in golden.load("groupby_golden.json")["skipped"] if "ORDER BY" in s["reason"]]
    assert skipped and set(skipped) <= {c["query"] for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, case):
    ok, msg = orderby.run_case(orderby.Session(orc), case)
    assert ok, msg


def test_parser_forms():
    s = orderby.parse_sentence("ORDER BY $-.a, b DESC, $-.c ASC")
    assert s.factors == [("a", False), ("b", True), ("c", False)]
    assert orderby.parse_sentence("LIMIT 7") == orderby.LimitSentence(0, 7)
    assert orderby.parse_sentence("LIMIT 3, 7") == orderby.LimitSentence(3, 7)
    assert orderby.parse_sentence("LIMIT 3 OFFSET 7") == orderby.LimitSentence(3, 7)   # parser.yy:875
    for bad in ("ORDER BY ", "ORDER BY $-.$$.team.name", "LIMIT", "LIMIT a"):
        with pytest.raises(Exception):
            orderby.parse_sentence(bad)


def test_model_order_and_windows():
    inp = Interim(["z", "i", "s", "b"], [[0.0, 3, "b", True], [-0.0, -5, "a", False], [1.5, 3, "B", True],
                                        [-2.0, 1 << 62, "", False]])
    # -0.0 and 0.0 do not decide: the next factor does
    assert [r[1] for r in orderby.order_model(inp, [("z", False), ("i", False)]).rows] == [1 << 62, -5, 3, 3]
    assert [r[1] for r in orderby.order_model(inp, [("z", True), ("i", True)]).rows] == [3, 3, -5, 1 << 62]
    assert [r[2] for r in orderby.order_model(inp, [("s", False)]).rows] == ["", "B", "a", "b"]   # by bytes
    assert [r[3] for r in orderby.order_model(inp, [("b", False), ("i", False)]).rows] == [False, False, True, True]
    with pytest.raises(groupby.GroupError) as ex:
        orderby.order_model(inp, [("nope", False)])
    assert ex.value.code == _lib.E_EXECUTION_ERROR
    assert orderby.order_model(Interim(["z"], []), [("nope", False)]).rows == []
    n = len(inp.rows)
    assert orderby.window(n, 0, 0) == (0, 0) and orderby.window(n, n, 5) == (0, 0)
    assert orderby.window(n, 1, 2) == (1, 3) and orderby.window(n, 1, 3) == (1, 4) and orderby.window(n, 1, 4) == (1, 4)
    assert orderby.window(n, 2, (1 << 63) - 1) == (2, 4)
    for off, cnt in ((-1, 2), (1, -2)):
        with pytest.raises(groupby.GroupError) as ex:
            orderby.limit_model(inp, off, cnt)
        assert ex.value.code == _lib.E_SYNTAX_ERROR
    assert orderby.limit_model(inp, 1, 2).rows == inp.rows[1:3]


def test_check_window_rejects_wrong_rows():
    inp = Interim(["k", "v"], [[1, 10], [1, 11], [2, 20], [2, 21], [3, 30]])
    f = [("k", False)]
    orderby.check_window([[1, 11], [1, 10], [2, 21]], inp, f, (0, 3))      # the cut key: any of its rows
    with pytest.raises(AssertionError):
        orderby.check_window([[1, 11], [1, 11], [2, 21]], inp, f, (0, 3))  # a whole key must be the input's
    with pytest.raises(AssertionError):
        orderby.check_window([[1, 11], [1, 10], [2, 22]], inp, f, (0, 3))  # a cut key's rows come from the input
    with pytest.raises(AssertionError):
        orderby.check_window([[1, 11], [2, 20], [1, 10]], inp, f, (0, 3))
