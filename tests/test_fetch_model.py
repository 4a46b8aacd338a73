"""Pins the FETCH checker (tests/support/fetchpipe.py: parser, model, session) before it judges the
device: over the CPU oracle's GO rows and tests/golden/nba.json's tag data the model reproduces
every non-skipped case of tests/golden/fetch_golden.json (the reference's own FetchVerticesTest
vectors), and it follows include/nbg.h's status order on hand-made rows.  CPU only."""
import pytest

from nebula_amd import _lib, kvgen
from tests.support import fetchpipe, golden
from tests.support.fetchpipe import TagTable
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID, GroupError
from tests.support.ngql import Interim, ParseError
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("fetch_golden.json")
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def test_golden_file_shape():
    assert len(CASES) == 16 and len(GOLDEN["skipped"]) == 2
    assert all("uuid(" in s["query"] for s in GOLDEN["skipped"])
    by_test = {}
    for c in CASES:
        by_test[c["test"]] = by_test.get(c["test"], 0) + 1
    assert by_test == {"base": 6, "noYield": 2, "distinct": 2, "syntaxError": 3, "executionError": 1, "nonExistVertex": 2}
    assert sum(c["status"] == "E_SYNTAX_ERROR" for c in CASES) == 3
    assert sum(c["status"] == "E_EXECUTION_ERROR" for c in CASES) == 1
    assert all("expected" in c for c in CASES if c["status"] == "SUCCEEDED")
    assert sum(bool(c.get("ordered")) for c in CASES) == 1


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, nba_data, case):
    ses = fetchpipe.Session(orc, fetchpipe.nba_tables(nba_data, kvgen.NBA_TAGS))
    ok, msg = fetchpipe.run_case(ses, case)
    assert ok, msg


def test_parser_forms():
    s = fetchpipe.parse_sentence("FETCH PROP ON player 1, -2, hash(\"x\") YIELD DISTINCT player.name AS n, player.age + 1")
    assert isinstance(s, fetchpipe.FetchSentence) and s.label == "player" and s.vids[:2] == [1, -2] and len(s.vids) == 3
    assert s.ref is None and s.distinct and [c.name() for c in s.yields] == ["n", "(player.age+1)"]
    s = fetchpipe.parse_sentence("fetch prop on t $-.id")
    assert s.ref == ("$-", "id") and s.yields is None and not s.distinct and not s.variables()
    s = fetchpipe.parse_sentence("FETCH PROP ON t $v.dst YIELD t.a")
    assert s.ref == ("v", "dst") and s.variables() == ["v"]
    assert fetchpipe.parse_sentence("FETCH PROP ON team $-").ref == ("$-", "id")
    t = fetchpipe.parse_statement("GO FROM 1 OVER like YIELD like._dst AS id | FETCH PROP ON player $-.id "
                                  "YIELD player.age AS age | ORDER BY $-.age | LIMIT 3")
    assert len(t.parts) == 4
    for bad in ("FETCH PROP player 1", "FETCH PROP ON player", "FETCH PROP ON player 1 YIELD",
                "FETCH PROP ON player 1 YIELD COUNT(player.age)", "FETCH PROP ON 5 1", "FETCH PROP ON player 1.5"):
        with pytest.raises(ParseError):
            fetchpipe.parse_statement(bad)


T = {"t": TagTable(9, [("i", INT), ("x", DOUBLE), ("b", BOOL), ("ts", TIMESTAMP), ("s", STRING)],
                   {1: [10, 0.5, True, 100, "a"], 2: [20, -0.0, False, 200, "b"], -3: [30, 0.0, True, 300, "c"],
                    4: [0, 2.5, False, 400, "a"]})}


def _model(text, inp=None, types=None):
    return fetchpipe.fetch_model(fetchpipe.parse_sentence(text), T, inp, types)


def _code(fn):
    with pytest.raises(GroupError) as ex:
        fn()
    return ex.value.code


def test_rows_order_duplicates_and_schema():
    res, types = _model("FETCH PROP ON t 2, 7, 1, 2, -3, 99, 2 YIELD t.i, t.x * 2 AS x2, (timestamp)t.i AS c, t.b, 5 AS k")
    assert res.columns == ["t.i", "x2", "c", "t.b", "k"] and types == [INT, None, TIMESTAMP, BOOL, None]
    # the input's order with the missing vids removed; every occurrence of a duplicate kept
    assert [r[0] for r in res.rows] == [20, 10, 20, 30, 20]
    assert res.rows[1] == [10, 1.0, 10, True, 5]
    # no YIELD clause: every column of the schema, with the schema's types
    res, types = _model("FETCH PROP ON t -3")
    assert res.columns == ["t.i", "t.x", "t.b", "t.ts", "t.s"] and res.rows == [[30, 0.0, True, 300, "c"]]
    assert types == [INT, DOUBLE, BOOL, TIMESTAMP, STRING]
    # a piped input: the named column, whatever else the rows hold
    inp = Interim(["w", "id"], [[5, 4], [6, 8], [7, 1]])
    assert _model("FETCH PROP ON t $-.id YIELD t.s, t.i", inp)[0].rows == [["a", 0], ["a", 10]]
    assert _model("FETCH PROP ON t $v.id YIELD t.s", inp)[0].rows == [["a"], ["a"]]
    # every vid missing: no rows, no error
    assert _model("FETCH PROP ON t 5, 6")[0].rows == []


def test_distinct_rows_not_vids():
    assert _model("FETCH PROP ON t 1, 4, 1 YIELD DISTINCT t.s")[0].rows == [["a"]]          # two vids, one row
    assert _model("FETCH PROP ON t 1, 4, 1 YIELD DISTINCT t.s, t.i")[0].rows == [["a", 10], ["a", 0]]
    assert len(_model("FETCH PROP ON t 2, -3 YIELD DISTINCT t.x")[0].rows) == 1             # -0.0 is 0.0
    assert len(_model("FETCH PROP ON t 2, -3 YIELD t.x")[0].rows) == 2


def test_status_order():
    one = Interim(["id", "d", "f", "s", "ts"], [[1, 2, 1.5, "a", 3]])
    none = Interim(["id"], [])
    types = [VID, INT, DOUBLE, STRING, TIMESTAMP]
    # 3: the tag, then `*'
    assert _code(lambda: _model("FETCH PROP ON nope 1 YIELD $^.t.i")) == _lib.E_EXECUTION_ERROR
    assert _code(lambda: _model("FETCH PROP ON t $-.* YIELD $^.t.i", one)) == _lib.E_EXECUTION_ERROR
    # 4, for an empty input too, before 5 and 6
    for y in ("$^.t.i", "$$.t.i", "$-.id", "$v.id", "u.i", "t.i + u.i"):
        assert _code(lambda: _model(f"FETCH PROP ON t $-.zz YIELD {y}", none)) == _lib.E_SYNTAX_ERROR, y
        assert _code(lambda: _model(f"FETCH PROP ON t 1 YIELD {y}")) == _lib.E_SYNTAX_ERROR, y
    # 5 before 6: no rows, no column check, one column per YIELD
    res, _ = _model("FETCH PROP ON t $-.zz YIELD t.nope, 1 + 1", none)
    assert res.rows == [] and len(res.columns) == 2
    assert _model("FETCH PROP ON t $-.zz", None)[0].columns == ["t.i", "t.x", "t.b", "t.ts", "t.s"]
    # 6: the vid column, then the props
    assert _code(lambda: _model("FETCH PROP ON t $-.zz YIELD 1 + 1", one, types)) == _lib.E_EXECUTION_ERROR
    for col in ("f", "s", "ts"):
        assert _code(lambda: _model(f"FETCH PROP ON t $-.{col} YIELD t.i", one, types)) == _lib.E_EXECUTION_ERROR, col
    assert _model("FETCH PROP ON t $-.d YIELD t.i", one, types)[0].rows == [[20]]
    assert _code(lambda: _model("FETCH PROP ON t 1 YIELD 1 + 1")) == _lib.E_EXECUTION_ERROR     # "No props declared."
    assert _code(lambda: _model("FETCH PROP ON t 1 YIELD t.i, t.nope")) == _lib.E_EXECUTION_ERROR
    # 8: an evaluation error in a found row only
    assert _code(lambda: _model("FETCH PROP ON t 1, 4 YIELD 7 / t.i")) == _lib.E_EXECUTION_ERROR
    assert _model("FETCH PROP ON t 1, 44 YIELD 70 / t.i")[0].rows == [[7]]


def test_session_pipes_variables_and_stages(orc, nba_data):
    from nebula_amd.vidhash import std_hash
    ses = fetchpipe.Session(orc, fetchpipe.nba_tables(nba_data, kvgen.NBA_TAGS))
    age = {p["vid"]: p["age"] for p in nba_data["players"]}
    name = {p["vid"]: p["name"] for p in nba_data["players"]}
    tim = std_hash("Tim Duncan")
    go = f"GO FROM {tim} OVER like YIELD like._dst AS id"
    ids = [r[0] for r in ses.execute(go).rows]
    assert len(ids) >= 2
    got = ses.execute(f"{go} | FETCH PROP ON player $-.id YIELD player.name AS n, player.age AS age")
    assert got.columns == ["n", "age"] and got.rows == [[name[v], age[v]] for v in ids]          # the input's order
    got = ses.execute(f"{go} | FETCH PROP ON player $-.id YIELD player.age AS age | ORDER BY $-.age DESC | LIMIT 1")
    assert got.rows == [[max(age[v] for v in ids)]]
    got = ses.execute(f"$a = {go}; FETCH PROP ON player $a.id YIELD player.age AS age | YIELD $-.age + 1 AS a1")
    assert [r[0] for r in got.rows] == [age[v] + 1 for v in ids]
    # a team is no player: a vertex without the tag yields no row
    assert ses.execute(f"GO FROM {tim} OVER serve YIELD serve._dst AS id | FETCH PROP ON player $-.id").rows == []
    assert ses.status("FETCH PROP ON player $nope.id")[0] == "E_EXECUTION_ERROR"
    assert ses.status("FETCH PROP ON player $nope.id YIELD $^.player.age")[0] == "E_SYNTAX_ERROR"
