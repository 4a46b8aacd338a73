"""Pins the set-operation checker (tests/support/setops.py: parser, model, session) to the
reference's own SetTest vectors before it judges the device: over the CPU oracle's GO rows the
model reproduces every case of tests/golden/setop_golden.json — statuses, column names and rows
where the reference asserts them — and it follows include/nbg.h's multiplicity and cast tables on
hand-made rows.  CPU only."""
import math

import pytest

from nebula_amd import _lib
from tests.support import golden, groupby, setops
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID
from tests.support.ngql import Interim, ParseError
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("setop_golden.json")
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def test_golden_file_shape():
    assert len(CASES) == 19 and not GOLDEN["skipped"]
    by_test = {}
    for c in CASES:
        by_test[c["test"]] = by_test.get(c["test"], 0) + 1
    assert by_test == {"UnionAllTest": 9, "UnionDistinct": 2, "Minus": 1, "Intersect": 1, "Mix": 1, "NoInput": 1,
                       "SyntaxError": 1, "ExecutionError": 3}
    assert sum(c["status"] == "E_EXECUTION_ERROR" for c in CASES) == 3
    assert sum(bool(c.get("no_rows")) for c in CASES) == 1
    # two blocks fill `expected` without comparing it: status and column names only
    assert sum(c["status"] == "SUCCEEDED" and "expected" not in c and not c.get("no_rows") for c in CASES) == 2


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, case):
    ok, msg = setops.run_case(setops.Session(orc), case)
    assert ok, msg


def test_parser_forms():
    go = "GO FROM 1 OVER like YIELD like._dst AS id"
    t = setops.parse_statement(f"{go} UNION {go} union all {go} INTERSECT ({go} MINUS {go} | LIMIT 3) UNION DISTINCT {go}")
    ops = []
    while isinstance(t, setops.SetNode):       # one priority, left-associative
        ops.append((t.op, t.distinct))
        assert isinstance(t.right, setops.PipeNode)
        t = t.left
    assert ops == [("UNION", True), ("INTERSECT", False), ("UNION", False), ("UNION", True)]
    inner = setops.parse_statement(f"{go} INTERSECT ({go} MINUS {go} | LIMIT 3)").right.parts[0]
    assert isinstance(inner, setops.SetNode) and inner.op == "MINUS" and len(inner.right.parts) == 2
    # a keyword inside a string or a longer name is no operator
    one = setops.parse_statement('GO FROM 1 OVER like YIELD "a UNION b" AS unions, like._dst AS minus_x')
    assert isinstance(one, setops.PipeNode) and len(one.parts) == 1
    piped = setops.parse_statement(f"({go} UNION ALL {go}) | GO FROM $-.id OVER like")
    assert isinstance(piped, setops.PipeNode) and isinstance(piped.parts[0], setops.SetNode)
    for bad in (f"{go} UNION", f"UNION {go}", f"{go} | ({go} UNION {go})", f"{go} MINUS ({go}", f"{go} INTERSECT LIMIT"):
        with pytest.raises(ParseError):
            setops.parse_statement(bad)


def _ms(rows):
    return groupby.multiset(rows)


def _model(lrows, rrows, op, distinct=False, lt=None, rt=None, ncols=1):
    cols = [f"c{i}" for i in range(ncols)]
    return setops.set_model(Interim(cols, lrows), Interim(cols, rrows), op, distinct, lt, rt)


def test_multiplicity_table():
    # value: (cL, cR): 1: left only; 2: cL > cR >= 1; 3: cR > cL >= 1; 4: equal; 5: right only
    counts = {1: (2, 0), 2: (3, 1), 3: (1, 4), 4: (2, 2), 5: (0, 3)}
    left = [[v, v * 1.5] for v, (cl, _) in counts.items() for _ in range(cl)]
    right = [[v, v * 1.5] for v, (_, cr) in counts.items() for _ in range(cr)]

    def copies(rows):
        out = {}
        for r in rows:
            assert r[1] == r[0] * 1.5
            out[r[0]] = out.get(r[0], 0) + 1
        return out
    res, types = _model(left, right, "UNION", ncols=2)
    assert res.rows == left + right and types == [INT, DOUBLE]          # UNION ALL: the left's rows, then the right's
    assert copies(res.rows) == {v: cl + cr for v, (cl, cr) in counts.items()}
    assert copies(_model(left, right, "UNION", True, ncols=2)[0].rows) == {v: 1 for v in counts}
    assert copies(_model(left, right, "INTERSECT", ncols=2)[0].rows) == {2: 1, 3: 1, 4: 2}        # min(cL, cR)
    assert copies(_model(left, right, "MINUS", ncols=2)[0].rows) == {1: 2}                      # cL if cR == 0
    assert copies(_model(left, left, "INTERSECT", ncols=2)[0].rows) == copies(left)
    assert _model(left, left, "MINUS", ncols=2)[0].rows == []


def test_empty_shortcuts_and_field_count():
    a = [[1, "x"], [1, "x"], [2, "y"]]
    e = Interim(["p", "q"], [])
    A = Interim(["p", "q"], a)
    B = Interim(["r", "s"], [[1.5, True]])
    for op, d in (("UNION", False), ("UNION", True), ("INTERSECT", False), ("MINUS", False)):
        assert setops.set_model(e, e, op, d)[0].rows == []
        with pytest.raises(groupby.GroupError) as ex:              # even with both inputs empty
            setops.set_model(e, Interim(["p"], []), op, d)
        assert ex.value.code == _lib.E_EXECUTION_ERROR
    # the other side as it is: not de-duplicated, its own types, the left's names
    res, types = setops.set_model(A, e, "UNION", True)
    assert res.rows == a and res.columns == ["p", "q"] and types == [INT, STRING]
    res, types = setops.set_model(e, B, "UNION", True, [INT, STRING], None)
    assert res.rows == B.rows and res.columns == ["p", "q"] and types == [DOUBLE, BOOL]
    assert setops.set_model(A, e, "INTERSECT")[0].rows == [] and setops.set_model(e, A, "INTERSECT")[0].rows == []
    assert setops.set_model(e, A, "MINUS")[0].rows == []
    assert setops.set_model(A, e, "MINUS")[0].rows == a
    # the shortcut comes before the cast check: a STRING / INT pair passes with an empty side
    assert setops.set_model(A, Interim(["p", "q"], []), "UNION", False, None, [STRING, INT])[0].rows == a


def test_cast_table():
    c = setops.cast_value
    for t in (INT, VID, TIMESTAMP):
        for f in (INT, VID, TIMESTAMP):
            assert c(-7, f, t) == -7
        assert c(-2.75, DOUBLE, t) == -2 and c(2.75, DOUBLE, t) == 2 and c(-0.5, DOUBLE, t) == 0     # toward zero
        assert c(True, BOOL, t) == 1 and c(False, BOOL, t) == 0 and type(c(True, BOOL, t)) is int
        assert c(2 ** 53, t, DOUBLE) == c(2 ** 53 + 1, t, DOUBLE) == 9007199254740992.0          # nearest even
        assert c(2 ** 53 + 3, t, DOUBLE) == 9007199254740996.0
        assert c(5, t, BOOL) is True and c(0, t, BOOL) is False
        assert c(-12, t, STRING) == "-12"
        with pytest.raises(groupby.GroupError):
            c(float("nan"), DOUBLE, t)
        with pytest.raises(groupby.GroupError):
            c(2.0 ** 63, DOUBLE, t)
    assert c(True, BOOL, DOUBLE) == 1.0 and c(False, BOOL, DOUBLE) == 0.0 and type(c(True, BOOL, DOUBLE)) is float
    assert c(0.5, DOUBLE, BOOL) is True and c(-0.0, DOUBLE, BOOL) is False and c(float("nan"), DOUBLE, BOOL) is True
    with pytest.raises(groupby.GroupError) as ex:
        c("12", STRING, INT)
    assert ex.value.code == _lib.E_UNSUPPORTED
    # the casts run on every right row, before any comparison, in all three operators
    left, right = [[-2], [3], [3]], [[-2.75], [3.9], [4.0]]
    assert _ms(_model(left, right, "UNION", lt=[INT], rt=[DOUBLE])[0].rows) == _ms([[-2], [3], [3], [-2], [3], [4]])
    assert _ms(_model(left, right, "UNION", True, lt=[INT], rt=[DOUBLE])[0].rows) == _ms([[-2], [3], [4]])
    assert _ms(_model(left, right, "INTERSECT", lt=[INT], rt=[DOUBLE])[0].rows) == _ms([[-2], [3]])
    assert _model(left, right, "MINUS", lt=[INT], rt=[DOUBLE])[0].rows == []
    # the result takes the left's types; a VID column stays a VID
    assert _model([[1]], [[2]], "UNION", lt=[VID], rt=[INT])[1] == [VID]


def test_equality_zeros_and_nans():
    nan, nnan = float("nan"), -float("nan")
    left, right = [[0.0], [-0.0], [nan], [nnan], [nan]], [[-0.0], [nan]]
    inter = _model(left, right, "INTERSECT")[0].rows
    assert len(inter) == 1 and inter[0][0] == 0.0                       # one zero for the one right zero; no NaN
    minus = _model(left, right, "MINUS")[0].rows
    assert len(minus) == 3 and all(math.isnan(r[0]) for r in minus)      # a NaN row always survives
    uni = _model(left, right, "UNION", True)[0].rows
    assert sorted(setops.bits_cell(r[0])[1] & ~(1 << 63) if r[0] == 0.0 else setops.bits_cell(r[0])[1] for r in uni) == \
        sorted([0, setops.bits_cell(nan)[1], setops.bits_cell(nnan)[1]])   # NaNs by their bits, the zeros as one
