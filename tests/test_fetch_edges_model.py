"""Pins the edge FETCH checker (tests/support/fetchedges.py: parser, model, session) before it judges
the device: over the CPU oracle's GO rows and tests/golden/nba.json's serve edges the model
reproduces every non-skipped case of tests/golden/fetch_edges_golden.json (the reference's own
FetchEdgesTest vectors), the parser tells the two FETCH sentences apart, and the model follows
include/nbg.h's status order on hand-made rows.  CPU only."""
import pytest

from nebula_amd import _lib, kvgen
from tests.support import fetchedges, fetchpipe, golden
from tests.support.fetchedges import EdgeTable
from tests.support.groupby import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID, GroupError
from tests.support.ngql import Interim, ParseError
from tests.support.oracle import nba_oracle

GOLDEN = golden.load("fetch_edges_golden.json")
CASES = GOLDEN["cases"]


@pytest.fixture(scope="module")
def orc(nba_data):
    o = nba_oracle(nba_data)
    yield o
    o.close()


def _tables(nba_data):
    return {**fetchpipe.nba_tables(nba_data, kvgen.NBA_TAGS), **fetchedges.nba_edge_tables(nba_data, kvgen.NBA_EDGES)}


def test_golden_file_shape():
    assert len(CASES) == 19 and len(GOLDEN["skipped"]) == 3
    assert all("uuid(" in s["query"] for s in GOLDEN["skipped"])
    by_test = {}
    for c in CASES:
        by_test[c["test"]] = by_test.get(c["test"], 0) + 1
    assert by_test == {"base": 7, "noYield": 3, "distinct": 4, "noInput": 1, "syntaxError": 3, "nonExistEdge": 1}
    assert sum(c["status"] == "E_SYNTAX_ERROR" for c in CASES) == 3
    assert all("expected" in c for c in CASES if c["status"] == "SUCCEEDED")


@pytest.mark.parametrize("case", CASES, ids=[f"{c['test']}-{i}" for i, c in enumerate(CASES)])
def test_model_reproduces_golden(orc, nba_data, case):
    ses = fetchedges.Session(orc, _tables(nba_data))
    ok, msg = fetchedges.run_case(ses, case)
    assert ok, msg


def test_parser_tells_the_two_fetch_sentences_apart():
    s = fetchedges.parse_sentence('FETCH PROP ON serve 1->2@3, -4 -> hash("x"), 5->-6@-7 YIELD DISTINCT serve.a AS n, serve._dst')
    assert isinstance(s, fetchedges.FetchEdgesSentence) and s.label == "serve" and s.ref is None and s.distinct
    assert s.keys[0] == (1, 2, 3) and s.keys[1][0] == -4 and s.keys[1][2] == 0 and s.keys[2] == (5, -6, -7)
    assert [c.name() for c in s.yields] == ["n", "serve._dst"]
    s = fetchedges.parse_sentence("fetch prop on e $-.s->$-.d")
    assert isinstance(s, fetchedges.FetchEdgesSentence) and s.ref == ("$-", "s", "d", None) and s.yields is None
    s = fetchedges.parse_sentence("FETCH PROP ON e $v.s->$v.d@$v.k YIELD e.w")
    assert s.ref == ("v", "s", "d", "k") and s.variables() == ["v"]
    # the vertex sentence through the same parser: no `->' after the first key
    for text in ('FETCH PROP ON player 1, -2, hash("x") YIELD player.name', "FETCH PROP ON t $-.id", "FETCH PROP ON t $v.dst YIELD t.a",
                 "FETCH PROP ON team $-", "FETCH PROP ON p -1, - 2"):
        s = fetchedges.parse_sentence(text)
        assert isinstance(s, fetchpipe.FetchSentence) and not isinstance(s, fetchedges.FetchEdgesSentence), text
    assert fetchedges.parse_sentence("FETCH PROP ON p -1, - 2").vids == [-1, -2]
    assert fetchedges.parse_sentence('FETCH PROP ON e hash("a->b")->2 YIELD e.w').keys[0][1] == 2      # an arrow inside a string
    t = fetchedges.parse_statement("GO FROM 1 OVER e YIELD e._src AS s, e._dst AS d | FETCH PROP ON e $-.s->$-.d YIELD e.w AS w "
                                   "| ORDER BY $-.w | LIMIT 3")
    assert len(t.parts) == 4
    assert [v for v, _ in fetchedges.split_statements("$a = GO FROM 1 OVER e; FETCH PROP ON e $a.s->$a.d@$a.k")] == ["a", None]
    with pytest.raises(ParseError, match="Only support single data source."):
        fetchedges.parse_statement("FETCH PROP ON e $a.s->$b.d YIELD e.w")
    for bad in ("FETCH PROP ON e 1->", "FETCH PROP ON e 1->2@", "FETCH PROP ON e 1->2, 3", "FETCH PROP ON e $-.s->$v.d",
                "FETCH PROP ON e $-.s->2", "FETCH PROP ON e 1->2 YIELD", "FETCH PROP ON e 1->2 YIELD COUNT(e.w)",
                "FETCH PROP ON e 1.5->2", "FETCH PROP ON e 1->2@$-.k", "FETCH PROP ON 5 1->2"):
        with pytest.raises(ParseError):
            fetchedges.parse_statement(bad)


T = {"e": EdgeTable(7, [("i", INT), ("x", DOUBLE), ("b", BOOL), ("ts", TIMESTAMP), ("s", STRING)],
                    {(1, 2, 0): [10, 0.5, True, 100, "a"], (1, 2, 5): [20, -0.0, False, 200, "b"],
                     (1, -3, 0): [30, 0.0, True, 300, "c"], (4, 1, -1): [0, 2.5, False, 400, "a"]})}


def _model(text, inp=None, types=None):
    return fetchedges.fetch_edges_model(fetchedges.parse_sentence(text), T, inp, types)


def _code(fn):
    with pytest.raises(GroupError) as ex:
        fn()
    return ex.value.code


def test_rows_order_duplicates_and_schema():
    res, types = _model("FETCH PROP ON e 1->2@5, 2->1, 1->2, 1->2@5, 1->-3, 4->1, 4->1@-1 "
                        "YIELD e.i, e.x * 2 AS x2, (timestamp)e.i AS c, e.b, 5 AS k, e._src, e._dst AS d, e._rank, e._type")
    assert res.columns == ["e.i", "x2", "c", "e.b", "k", "e._src", "d", "e._rank", "e._type"]
    # a bare prop: the schema's type; a root cast: the cast's; the key pseudo-props: the value's own
    assert types == [INT, None, TIMESTAMP, BOOL, None, None, None, None, None]
    # the input's order with the missing keys removed; every occurrence of a duplicate kept; the
    # rank is part of the key (1->2 is 1->2@0, 4->1 is not 4->1@-1)
    assert [r[0] for r in res.rows] == [20, 10, 20, 30, 0]
    assert res.rows[0] == [20, -0.0, 20, False, 5, 1, 2, 5, "e"] and res.rows[4][5:] == [4, 1, -1, "e"]
    # no YIELD clause: every column of the schema, with the schema's types
    res, types = _model("FETCH PROP ON e 1->-3")
    assert res.columns == ["e.i", "e.x", "e.b", "e.ts", "e.s"] and res.rows == [[30, 0.0, True, 300, "c"]]
    assert types == [INT, DOUBLE, BOOL, TIMESTAMP, STRING]
    # a piped input: the named columns, whatever else the rows hold; without `@' every rank is 0
    inp = Interim(["w", "a", "b", "k"], [[5, 1, 2, 5], [6, 8, 1, 0], [7, 4, 1, -1]])
    assert _model("FETCH PROP ON e $-.a->$-.b@$-.k YIELD e.s, e.i", inp)[0].rows == [["b", 20], ["a", 0]]
    assert _model("FETCH PROP ON e $-.a->$-.b YIELD e.s", inp)[0].rows == [["a"]]
    assert _model("FETCH PROP ON e $v.a->$v.b YIELD e.s", inp)[0].rows == [["a"]]
    # every key missing: no rows, no error
    assert _model("FETCH PROP ON e 5->6, 2->1 YIELD e.i")[0].rows == []


def test_distinct_rows_not_keys():
    assert _model("FETCH PROP ON e 1->2, 4->1@-1, 1->2 YIELD DISTINCT e.s")[0].rows == [["a"]]          # two keys, one row
    assert _model("FETCH PROP ON e 1->2, 4->1@-1, 1->2 YIELD DISTINCT e.s, e.i")[0].rows == [["a", 10], ["a", 0]]
    assert len(_model("FETCH PROP ON e 1->2@5, 1->-3 YIELD DISTINCT e.x")[0].rows) == 1                 # -0.0 is 0.0
    assert len(_model("FETCH PROP ON e 1->2@5, 1->-3 YIELD e.x")[0].rows) == 2


def test_status_order():
    one = Interim(["a", "b", "f", "s", "ts", "k"], [[1, 2, 1.5, "a", 3, 5]])
    none = Interim(["a"], [])
    types = [VID, INT, DOUBLE, STRING, TIMESTAMP, INT]
    # 3: the edge, then `*' in any of the three columns
    assert _code(lambda: _model("FETCH PROP ON nope 1->2 YIELD $^.e.i")) == _lib.E_EXECUTION_ERROR
    for ref in ("$-.*->$-.b", "$-.a->$-.*", "$-.a->$-.b@$-.*"):
        assert _code(lambda: _model(f"FETCH PROP ON e {ref} YIELD $^.e.i", one)) == _lib.E_EXECUTION_ERROR, ref
    # 4, for an empty input too, before 5 and 6
    for y in ("$^.e.i", "$$.e.i", "$-.a", "$v.a", "u.i", "e.i + u.i", "u._dst"):
        assert _code(lambda: _model(f"FETCH PROP ON e $-.zz->$-.b YIELD {y}", none)) == _lib.E_SYNTAX_ERROR, y
        assert _code(lambda: _model(f"FETCH PROP ON e 1->2 YIELD {y}")) == _lib.E_SYNTAX_ERROR, y
    # 5 before 6: no rows, no column check, one column per YIELD
    res, _ = _model("FETCH PROP ON e $-.zz->$-.b YIELD e.nope, 1 + 1", none)
    assert res.rows == [] and len(res.columns) == 2
    assert _model("FETCH PROP ON e $-.zz->$-.b", None)[0].columns == ["e.i", "e.x", "e.b", "e.ts", "e.s"]
    # 6: the key columns (src, dst, then rank), then the props
    with pytest.raises(GroupError, match="Column `zz' not found"):
        _model("FETCH PROP ON e $-.zz->$-.f YIELD 1 + 1", one, types)
    with pytest.raises(GroupError, match="Column `f' not found"):
        _model("FETCH PROP ON e $-.a->$-.f@$-.zz YIELD e.i", one, types)
    for col in ("f", "s", "ts"):
        for ref in (f"$-.{col}->$-.b", f"$-.a->$-.{col}", f"$-.a->$-.b@$-.{col}"):
            assert _code(lambda: _model(f"FETCH PROP ON e {ref} YIELD e.i", one, types)) == _lib.E_EXECUTION_ERROR, ref
    assert _model("FETCH PROP ON e $-.a->$-.b@$-.k YIELD e.i", one, types)[0].rows == [[20]]
    assert _code(lambda: _model("FETCH PROP ON e 1->2 YIELD 1 + 1")) == _lib.E_EXECUTION_ERROR     # "No props declared."
    assert _code(lambda: _model("FETCH PROP ON e 1->2 YIELD e.i, e.nope")) == _lib.E_EXECUTION_ERROR
    assert _model("FETCH PROP ON e 1->2 YIELD e._dst")[0].rows == [[2]]                            # a key prop is a prop
    # 8: an evaluation error in a found row only
    assert _code(lambda: _model("FETCH PROP ON e 1->2, 4->1@-1 YIELD 7 / e.i")) == _lib.E_EXECUTION_ERROR
    assert _model("FETCH PROP ON e 1->2, 4->1 YIELD 70 / e.i")[0].rows == [[7]]


def test_session_pipes_variables_and_stages(orc, nba_data):
    from nebula_amd.vidhash import std_hash
    ses = fetchedges.Session(orc, _tables(nba_data))
    tony, tim = std_hash("Tony Parker"), std_hash("Tim Duncan")
    serves = {(w, t): (s, e) for w, t, s, e in nba_data["serve"]}
    go = f"GO FROM {tony}, {tim} OVER serve YIELD serve._src AS s, serve._dst AS d"
    keys = [tuple(r) for r in ses.execute(go).rows]
    assert len(keys) == 3
    tables = _tables(nba_data)
    want = [tables["serve"].rows[(s, d, 0)] for s, d in keys]
    got = ses.execute(f"{go} | FETCH PROP ON serve $-.s->$-.d YIELD serve.start_year AS a, serve.end_year AS b")
    assert got.columns == ["a", "b"] and got.rows == want                                     # the input's order
    assert sorted(map(tuple, want)) == sorted(serves[k] for k in (("Tony Parker", "Spurs"), ("Tony Parker", "Hornets"), ("Tim Duncan", "Spurs")))
    got = ses.execute(f"{go} | FETCH PROP ON serve $-.s->$-.d YIELD serve.end_year AS b | ORDER BY $-.b DESC | LIMIT 1")
    assert got.rows == [[2019]]
    got = ses.execute(f"$a = {go}; FETCH PROP ON serve $a.s->$a.d YIELD serve.end_year AS b | YIELD $-.b + 1 AS b1")
    assert [r[0] for r in got.rows] == [w[1] + 1 for w in want]
    # an edge FETCH feeding a vertex FETCH
    got = ses.execute(f"{go} | FETCH PROP ON serve $-.s->$-.d YIELD DISTINCT serve._dst AS id | FETCH PROP ON team $-.id")
    assert sorted(r[0] for r in got.rows) == ["Hornets", "Spurs"]
    # the reversed keys are no serve edges
    assert ses.execute(f"{go} | FETCH PROP ON serve $-.d->$-.s").rows == []
    assert ses.status("FETCH PROP ON serve $nope.s->$nope.d")[0] == "E_EXECUTION_ERROR"
    assert ses.status("FETCH PROP ON serve $nope.s->$nope.d YIELD $^.serve.start_year")[0] == "E_SYNTAX_ERROR"
    assert ses.status("FETCH PROP ON serve $a.s->$b.d")[0] == "E_SYNTAX_ERROR"
