"""Pins the YIELD checker (tests/support/yieldpipe.py: parser, evaluator, model, session) before it
judges the device: over the CPU oracle's GO rows the model reproduces every case of
tests/golden/yield_golden.json (the reference's own YieldTest vectors), its evaluator agrees with
every case of tests/golden/expression_cases.json inside its stated subset, and it follows
include/nbg.h's status order on hand-made rows.  CPU only."""
import math

import pytest

from nebula_amd import _lib, expr as E
from tests.support import golden, groupby, yieldpipe
from tests.support.groupby import BOOL, DOUBLE, TIMESTAMP, GroupError
from tests.support.ngql import Interim, ParseError
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("yield_golden.json")
CASES = GOLDEN["cases"]
EXPR_CASES = golden.load("expression_cases.json")


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def test_golden_file_shape():
    assert len(CASES) == 23 and len(GOLDEN["skipped"]) == 1
    by_test = {}
    for c in CASES:
        by_test[c["test"]] = by_test.get(c["test"], 0) + 1
    assert by_test == {"yieldPipe": 6, "yieldVar": 6, "error": 7, "AggCall": 4}
    assert sum(c["status"] == "E_EXECUTION_ERROR" for c in CASES) == 4
    assert sum(c["status"] == "E_SYNTAX_ERROR" for c in CASES) == 4
    assert all("expected" in c for c in CASES if c["status"] == "SUCCEEDED")


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, case):
    ok, msg = yieldpipe.run_case(yieldpipe.Session(orc), case)
    assert ok, msg


def _expr(text):
    p = yieldpipe.Parser(text)
    e = p.expression()
    assert p.peek()[0] == "eof", text
    return e


def test_evaluator_against_expression_cases():
    """Every expression_cases.json vector whose operators the evaluator covers: the value and its
    kind, or the evaluation error.  The others (functions, string building) raise ModelScope."""
    ran = 0
    for c in EXPR_CASES:
        try:
            e = _expr(c["expr"])
        except ParseError:
            continue
        try:
            v = yieldpipe.evaluate(e)
        except yieldpipe.ModelScope:
            continue
        except yieldpipe.EvalError:
            assert c.get("error"), c
            ran += 1
            continue
        assert not c.get("error"), c
        ran += 1
        if c.get("function"):
            want = float(c["expect"]) if c["kind"] == "Double" else int(c["expect"])
            rel = {"EQ": "==", "LT": "<", "LE": "<=", "GT": ">", "GE": ">="}[c["op"]]
            assert yieldpipe.evaluate(E.binop(rel, E.const(v), E.const(want))) is True, c
            continue
        kind = "Bool" if isinstance(v, bool) else "Int" if isinstance(v, int) else "Double" if isinstance(v, float) else "String"
        assert kind == c["kind"], c
        if kind == "Double":
            assert abs(v - c["expect"]) < 1e-8, c
        else:
            assert v == c["expect"], c
    assert ran == EVALUATED and ran > 0


# every vector of the literal (11), arithmetic (45), relational (88), logical (44) and
# invalid-expression (17) blocks; the FunctionCall / StringFunctionCall vectors are outside the subset
EVALUATED = 205


def test_parser_forms():
    s = yieldpipe.parse_sentence("YIELD $-.d AS id, $-.w * 2 AS w2 WHERE $-.w > 50")
    assert isinstance(s, yieldpipe.YieldSentence) and [c.name() for c in s.yields] == ["id", "w2"]
    assert s.where.to_string() == "($-.w>50)" and s.uses_input() and not s.variables()
    s = yieldpipe.parse_sentence("YIELD $-.*, hash(123) AS h")
    assert s.yields[0].expr.prop == "*" and s.where is None
    s = yieldpipe.parse_sentence("yield AVG($v.age), COUNT(*), 1+1")
    assert [c.fun for c in s.yields] == ["AVG", "COUNT", ""] and s.variables() == ["v"]
    assert yieldpipe.parse_sentence("YIELD 1+1").is_constant()
    assert yieldpipe.split_statements(" $a = GO FROM 1 OVER e; YIELD $a.x WHERE $a.y == \";\" ;") == \
        [("a", " GO FROM 1 OVER e"), (None, "YIELD $a.x WHERE $a.y == \";\"")]
    go = "GO FROM 1 OVER like YIELD like._dst AS id"
    t = yieldpipe.parse_statement(f"({go} | YIELD $-.id) UNION {go} | YIELD $-.id | LIMIT 3")
    assert isinstance(t, yieldpipe.SetNode) and len(t.right.parts) == 3
    for bad in ("YIELD", "YIELD $-.a WHERE", "YIELD DISTINCT $-.a,", f"{go} | YIELD $-.id UNION"):
        with pytest.raises(ParseError):
            yieldpipe.parse_statement(bad)


def _model(cols, rows, text, types=None):
    return yieldpipe.yield_model(Interim(cols, rows), yieldpipe.parse_sentence(text), types)


def _code(fn):
    with pytest.raises(GroupError) as ex:
        fn()
    return ex.value.code


def test_filter_first_order_kept_and_expansion():
    rows = [[i, (i * 7) % 5, float(i) / 2, i % 2 == 0] for i in range(10)]
    res, types = _model(["pos", "w", "x", "b"], rows, "YIELD $-.pos, $-.w * 2 + 1 AS y WHERE $-.w < 3 && $-.pos % 3 != 0")
    assert res.columns == ["$-.pos", "y"] and types == [None, None]
    assert res.rows == [[r[0], r[1] * 2 + 1] for r in rows if r[1] < 3 and r[0] % 3 != 0]       # the input's order
    res, types = _model(["pos", "w", "x", "b"], rows, "YIELD $-.*, (double)$-.pos AS d, (timestamp)$-.x AS t, (bool)$-.w")
    assert res.columns == ["$-.pos", "$-.w", "$-.x", "$-.b", "d", "t", "(bool)$-.w"]
    assert types == [None, None, None, None, DOUBLE, TIMESTAMP, BOOL]
    assert res.rows[3] == [3, 1, 1.5, False, 3.0, 1, True] and type(res.rows[3][4]) is float
    # with duplicate names the first match wins
    assert _model(["a", "a"], [[1, 2]], "YIELD $-.a")[0].rows == [[1]]
    # a YIELD error on a row the WHERE rejects is not an error; on a passing row, or in the WHERE, it is
    assert _model(["pos", "i"], [[0, 5], [3, 6]], "YIELD $-.i / ($-.pos - 3) WHERE $-.pos != 3")[0].rows == [[-1]]
    assert _code(lambda: _model(["pos", "i"], [[0, 5], [3, 6]], "YIELD $-.i / ($-.pos - 3)")) == _lib.E_EXECUTION_ERROR
    assert _code(lambda: _model(["pos", "i"], [[0, 5], [3, 6]], "YIELD $-.i WHERE $-.i / ($-.pos - 3) > 0")) == _lib.E_EXECUTION_ERROR
    # a constant YIELD is a constant column; a constant-false WHERE keeps nothing
    assert _model(["a"], [[1], [2]], "YIELD 7, $-.a")[0].rows == [[7, 1], [7, 2]]
    assert _model(["a"], [[1], [2]], "YIELD $-.a WHERE 1 == 2")[0].rows == []


def test_status_order():
    rows = [[1, 2]]
    # 3 before 4: an edge property beside `$-' and `$var'
    assert _code(lambda: _model(["a", "b"], rows, "YIELD $-.a, $v.b, e.w")) == _lib.E_SYNTAX_ERROR
    assert _code(lambda: _model(["a", "b"], rows, "YIELD $^.t.p")) == _lib.E_SYNTAX_ERROR
    assert _code(lambda: _model(["a", "b"], rows, "YIELD COUNT(*), $-.a")) == _lib.E_SYNTAX_ERROR
    # 4 before 5 and 6
    assert _code(lambda: _model(["a", "b"], [], "YIELD $-.a WHERE $v.zz > 1")) == _lib.E_EXECUTION_ERROR
    assert _code(lambda: _model(["a", "b"], rows, "YIELD $v.a WHERE $w.b > 1")) == _lib.E_EXECUTION_ERROR
    # 5 before 6: no rows, no name check, one column per YIELD after expansion
    res, _ = _model(["a", "b"], [], "YIELD $-.*, $-.zz")
    assert res.rows == [] and len(res.columns) == 3
    # 6
    assert _code(lambda: _model(["a", "b"], rows, "YIELD $-.zz")) == _lib.E_EXECUTION_ERROR
    assert _code(lambda: _model(["a", "b"], rows, "YIELD $-.a WHERE $-.zz == 1")) == _lib.E_EXECUTION_ERROR
    # no input at all: an empty result; executeConstant: one row
    assert yieldpipe.yield_model(None, yieldpipe.parse_sentence("YIELD $-.a"))[0].rows == []
    assert yieldpipe.yield_model(None, yieldpipe.parse_sentence("YIELD 1+1, COUNT(*)"))[0].rows == [[2, 1]]


def test_evaluator_rules():
    ev = lambda t: yieldpipe.evaluate(_expr(t))       # noqa: E731
    big = (1 << 63) - 1
    assert ev(f"{big} + 1") == -(1 << 63) and ev(f"{big} * 2") == -2 and ev(f"-{big} - 2") == big
    assert ev("-7 / 2") == -3 and ev("-7 % 2") == -1 and ev("7 / -2") == -3 and ev("7 % -2") == 1    # toward zero
    for bad in ("1 / 0", "1 % 0", f"(-{big} - 1) / -1", f"(-{big} - 1) % -1", "true + 1", "-true", '"a" < 1'):
        with pytest.raises(yieldpipe.EvalError):
            ev(bad)
    assert ev("1 / 0.0") == math.inf and ev("-1 / 0.0") == -math.inf and math.isnan(ev("0.0 / 0.0"))
    assert math.isnan(ev("1.5 % 0.0")) and ev("7.5 % 2") == 1.5
    assert ev("0.1 + 0.2 == 0.3") is True and ev("1.0 == 1.00000002") is False                  # |a - b| < 1e-8
    nan = "(0.0 / 0.0)"
    assert ev(f"{nan} < 1") is False and ev(f"{nan} <= 1") is True and ev(f"{nan} >= 1") is True and ev(f"{nan} > 1") is False
    assert ev(f"{nan} == {nan}") is False and ev(f"{nan} != {nan}") is True
    assert ev("true == 1") is True and ev("true < 2.5") is True and ev("false < true") is True
    assert ev('"abc" < "abd"') is True and ev('"Z" < "a"') is True and ev('"é" > "z"') is True    # bytes
    assert ev("2 XOR 0") is True and ev("!0.0") is True and ev("1 && 0.5") is True and ev("5 ^ 3") == 6
    assert ev("(int)-2.75") == -2 and ev("(double)true") == 1.0 and ev("(bool)-0.0") is False and ev("(timestamp)3.9") == 3
    assert ev("hash(-5)") == -5 and ev('hash("Tim Duncan")') == golden_vid("Tim Duncan")
    with pytest.raises(yieldpipe.EvalError):
        ev("(bigint)1")
    # both operands are evaluated, the left one's error first: no short circuit
    with pytest.raises(yieldpipe.EvalError):
        ev("false && 1 / 0 == 1")
    for out in ('"a" + "b"', "(string)1", 'upper("a")', "(int)(0.0 / 0.0)", '!"a"'):
        with pytest.raises(yieldpipe.ModelScope):
            ev(out)


def golden_vid(name):
    from nebula_amd.vidhash import std_hash
    return std_hash(name)


def test_session_pipes_sets_and_variables(orc):
    s = yieldpipe.Session(orc)
    tim = golden_vid("Tim Duncan")
    go = f"GO FROM {tim} OVER like YIELD like._dst AS id, like.likeness AS w"
    base = s.execute(go).rows
    assert base
    got = s.execute(f"{go} | YIELD $-.id, $-.w + 1 AS w1 WHERE $-.w >= 90 | ORDER BY $-.w1 | LIMIT 1")
    want = sorted(([r[0], r[1] + 1] for r in base if r[1] >= 90), key=lambda r: r[1])[:1]
    assert got.columns == ["$-.id", "w1"] and [r[1] for r in got.rows] == [r[1] for r in want]
    both = s.execute(f"({go} | YIELD $-.id) UNION ALL ({go} | YIELD $-.id WHERE $-.w < 0)")
    assert groupby.multiset(both.rows) == groupby.multiset([[r[0]] for r in base])
    var = s.execute(f"$a = {go}; YIELD $a.w AS w WHERE $a.w != 0 | GROUP BY $-.w YIELD $-.w, COUNT(*)")
    assert sum(r[1] for r in var.rows) == len([r for r in base if r[1] != 0])
    assert s.status("YIELD $nope.x")[0] == "E_EXECUTION_ERROR"
    assert s.status(f"{go} | YIELD 1 + 1 AS two")[1].rows == [[2]]                # executeConstant: one row
