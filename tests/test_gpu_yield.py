"""nbg_yield on the MI355X: piped YIELD ... WHERE over device-resident rows, judged by the
plain-Python model of tests/support/yieldpipe.py (pinned to the reference's YieldTest vectors and to
tests/golden/expression_cases.json by tests/test_yield_model.py) — never by the device itself.

The graph, GO and columns are those of tests/test_gpu_orderby.py (seeded RMAT-10): k7, d (vids), s
(dictionary strings), w (100 values of both signs), x (nearly unique doubles), z (both zeros) and
b2 (a BOOL); the GO's 4,452 rows lie in several segments.  The model's input is the GO's rows in
their fetch order (asserted to be the CPU oracle's rows as a multiset), so its output is the
expected result row for row: nbg_yield keeps the input's order.

Cells these rows never hold, the row counts at the wave / workgroup / chunk edges, the register
limit and the input of more chunks than workgroups are the subject of
tests/test_gpu_values_yield.py.

Three NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
column whose kind differs between OVER types, a passed-through string column whose OVER types
spell different constants, and the input of 2^32 rows."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E
from nebula_amd.engine import DeviceRows, nba_engine
from tests.support import golden, graphs, groupby, ngql, orderby, setops, yieldpipe
from tests.support.oracle import Oracle
from tests.test_gpu_orderby import E_SCHEMA, GO_COLS, PARTS, ROOTS, T_SCHEMA, _kv

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("yield_golden.json")["cases"]
EMPTY_SRC = 123                       # no such vertex: a GO from it has no rows
YR_KERNELS = ("k_yr_filter", "k_yr_scan", "k_yr_emit")


class Fixture:
    pass


@pytest.fixture(scope="module")
def yf():
    """Engine, oracle, the GO's rows on the device and, fetched, as the model's input: computed
    once and left unchanged."""
    src, kb = _kv()
    assert set(ROOTS) <= set(src.tolist()) and EMPTY_SRC not in set(src.tolist())
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.load_builder(kb)
    f.orc = Oracle(PARTS)
    f.orc.register(True, 1, "e", E_SCHEMA)
    f.orc.register(False, 7, "t", T_SCHEMA)
    f.orc.load_builder(kb)
    f.go = f"GO 2 STEPS FROM {ROOTS[0]}, {ROOTS[1]} OVER e YIELD {GO_COLS}"
    f.sent = ngql.Parser(f.go).go()
    f.names = [c.name() for c in f.sent.yields]
    f.rows = f.eng.go_device(ROOTS, [1], 2, b"", [c.expr.encode() for c in f.sent.yields])
    assert f.eng.lib.nbg_rows_num_segments(f.rows.h) >= 2 and f.rows.count >= 2048
    f.digest = f.rows.digest()
    f.inp = ngql.Interim(f.names, f.rows.fetch())             # the input's own segment order
    oracle_rows = orderby.Session(f.orc).execute(f.go).rows
    assert groupby.multiset(f.inp.rows) == groupby.multiset(oracle_rows)
    f.types = groupby.go_column_types(f.sent, f.inp.rows)
    yield f
    f.rows.free()
    f.eng.close()
    f.orc.close()


@pytest.fixture(scope="module")
def nba(nba_data):
    eng = nba_engine(nba_data)
    yield eng
    eng.close()


def _take(rows):
    try:
        return rows.fetch()
    finally:
        rows.free()


def _bits(rows):
    return [tuple(setops.bits_cell(v) for v in r) for r in rows]


def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def _args(text):
    """(yields, where, funs) of a `YIELD ... [WHERE ...]` text for Engine.yield_rows."""
    st = yieldpipe.parse_sentence(text)
    funs = [c.fun if c.fun else 0 for c in st.yields] if any(c.fun for c in st.yields) else None
    return [c.expr.encode() for c in st.yields], st.where.encode() if st.where is not None else b"", funs


def _yield(eng, rows, names, text):
    ys, where, funs = _args(text)
    return eng.yield_rows(rows, names, ys, where, funs)


def _model(inp, text, types=None):
    return yieldpipe.yield_model(inp, yieldpipe.parse_sentence(text), types)


def _go(eng, yields, root=ROOTS[0], steps=1):
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {yields}").go()
    rows = eng.go_device([root], [1], steps, b"", [c.expr.encode() for c in sent.yields])
    return rows, [c.name() for c in sent.yields]


# ------------------------------------------------------------------------------ 1. golden cases
def _is_agg_over_input(case):
    return case["test"] == "AggCall" and case["status"] == "SUCCEEDED" and ("$-." in case["query"] or "$var." in case["query"])


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, case):
    """Every GO in front of a YIELD with go_device, the YIELD with nbg_yield, one fetch.  The two
    whole-input aggregate cases must report NBG_E_UNSUPPORTED and still match through the model."""
    ses = yieldpipe.Session(nba, device=True)
    ok, msg = yieldpipe.run_case(ses, case)
    assert ok, msg
    if case["status"] != "SUCCEEDED":
        return
    if _is_agg_over_input(case):
        assert ses.fallbacks == [("YieldSentence", L.E_UNSUPPORTED)] and ses.yield_calls == 0
    elif "$-." in case["query"] or "$var." in case["query"]:
        assert not ses.fallbacks and ses.yield_calls == 1
    else:
        assert not ses.fallbacks and ses.yield_calls == 0      # executeConstant: no input, one row


def test_golden_has_the_two_aggregate_cases():
    assert sum(_is_agg_over_input(c) for c in GOLDEN) == 2


# ------------------------------------------------------------------------------ 2. parity, in order
TEXTS = {
    "filter_arith": "YIELD $-.d, $-.w * 2 + 1 AS y WHERE $-.w < 3 && $-.d % 3 != 0",
    "star": "YIELD $-.*",
    "star_and_more": "YIELD $-.w AS w0, $-.*, $-.w - 1 AS w1 WHERE $-.k7 != 0",
    "strings": 'YIELD $-.s, $-.s == "n5" AS is5, $-.s < "n2" AS lt, $-.s >= "zz" AS ge WHERE $-.s != "n7"',
    "casts": "YIELD (double)$-.w / 3 AS q, (int)$-.x AS xi, (bool)$-.k7 AS bk, !$-.b2 AS nb, -$-.x AS nx, "
             "(timestamp)$-.w AS t, (double)$-.b2 AS bd WHERE $-.x >= -1000.5 || $-.b2",
    "constants": 'YIELD 7 AS c, "no such name" AS s2, 2.5 AS h, true AS b, "n3" AS known, $-.w WHERE true',
    "logic": "YIELD $-.w % 7 AS m, $-.w / 7 AS q, $-.w ^ 5 AS xr, $-.b2 XOR ($-.w > 0) AS lx, $-.z == 0 AS zz "
             "WHERE !($-.w == 0) && ($-.x < 0.0 || $-.k7 >= 2)",
    "variable": "YIELD $v.d, $v.x * 0.5 AS hx WHERE $v.w > 0",
    "keeps_one": "YIELD $-.d, $-.x WHERE $-.x == {X} && $-.d == {D}",      # (the middle row's x and d)
    "hash": "YIELD hash($-.d) AS h, hash($-.w) AS hw WHERE hash($-.w) < 10",
}


@pytest.mark.parametrize("name", list(TEXTS))
def test_parity_in_input_order(yf, name):
    mid = yf.inp.rows[len(yf.inp.rows) // 2]
    text = TEXTS[name].replace("{X}", repr(mid[4])).replace("{D}", str(mid[1]))
    want, types = _model(yf.inp, text, yf.types)
    out = _yield(yf.eng, yf.rows, yf.names, text)
    assert out.count == len(want.rows)
    assert out.count == 0 or yf.eng.lib.nbg_rows_num_segments(out.h) == 1
    assert yf.eng.lib.nbg_rows_num_cols(out.h) == len(want.columns)
    dev = _take(out)
    assert _bits(dev) == _bits(want.rows)                       # row for row: the input's order, filtered
    if name == "keeps_one":
        assert 1 <= len(dev) <= 4
    else:
        assert 0 < len(dev) and (name in ("star", "constants") or len(dev) < len(yf.inp.rows))
    assert yf.rows.digest() == yf.digest                        # `in` stays unchanged


def test_constant_where(yf):
    yf.eng.profile(True)
    none = _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d, $-.w + 1 WHERE 1 == 2")
    prof = yf.eng.profile_read()
    assert none.count == 0 and yf.eng.lib.nbg_rows_num_cols(none.h) == 2 and _take(none) == []
    assert all(prof[k]["launches"] == 0 for k in YR_KERNELS)   # a constant-false WHERE: no launch
    yf.eng.profile(True)
    every = _take(_yield(yf.eng, yf.rows, yf.names, "YIELD $-.d WHERE 2 > 1"))
    prof = yf.eng.profile_read()
    yf.eng.profile(False)
    assert _bits(every) == _bits([[r[1]] for r in yf.inp.rows])
    assert [prof[k]["launches"] for k in YR_KERNELS] == [0, 0, 1]


def test_path_coverage_and_bytes(yf):
    n = len(yf.inp.rows)
    yf.eng.profile(True)
    _take(_yield(yf.eng, yf.rows, yf.names, "YIELD $-.d"))
    prof = yf.eng.profile_read()
    assert [prof[k]["launches"] for k in YR_KERNELS] == [0, 0, 1]
    assert prof["k_yr_emit"]["algo_bytes"] == n * 8 * (1 + 1) and prof["k_yr_emit"]["ms"] > 0
    yf.eng.profile(True)
    kept = len(_take(_yield(yf.eng, yf.rows, yf.names, "YIELD $-.d, $-.w * 2 + $-.d AS y WHERE $-.w < 0 && $-.k7 != 1")))
    prof = yf.eng.profile_read()
    yf.eng.profile(False)
    assert [prof[k]["launches"] for k in YR_KERNELS] == [1, 1, 1] and 0 < kept < n
    assert prof["k_yr_filter"]["algo_bytes"] == n * (8 * 2 + 1)                    # w and k7, one flag byte
    assert prof["k_yr_emit"]["algo_bytes"] == n + kept * 8 * (2 + 2)               # flags; d and w in, 2 columns out
    assert all(prof[k]["launches"] == 0 for k in prof if k.startswith("k_so_") or k.startswith("k_ob_"))


# ------------------------------------------------------------------------------ 3. statuses, in nbg.h's order
def test_status_1_invalid_arguments(yf, nba):
    rows, names = yf.rows, yf.names
    assert _code(lambda: yf.eng.yield_rows(rows, names, [])) == L.E_INVALID_ARGUMENT                   # num_yields < 1
    good = E.input_prop("w").encode()
    for bad in (b"\xff", good[:-1], good + b"\x00", E.cast("int", E.input_prop("w")).encode()[:1] + b"\x09" + good):
        assert _code(lambda: yf.eng.yield_rows(rows, names, [bad])) == L.E_INVALID_ARGUMENT
        assert _code(lambda: yf.eng.yield_rows(rows, names, [good], bad)) == L.E_INVALID_ARGUMENT
    # ... before the syntax check of another column
    assert _code(lambda: yf.eng.yield_rows(rows, names, [E.edge_prop("e", "w").encode(), b"\xff"])) == L.E_INVALID_ARGUMENT
    # rows of another engine
    sent = ngql.Parser("GO FROM 1 OVER like YIELD like._dst AS d").go()
    other = nba.go_device([5662213458193308137], [nba.edge_types["like"]], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        assert _code(lambda: yf.eng.yield_rows(other, ["d"], [E.input_prop("d").encode()])) == L.E_INVALID_ARGUMENT
    finally:
        other.free()
    # host-only rows
    req, keep = yf.eng._go_request([ROOTS[0]], [1], 1, b"", [E.edge_prop("e", "w").encode()], False, False)
    h = C.c_void_p()
    assert yf.eng.lib.nbg_go(yf.eng.h, C.byref(req), C.byref(h)) == L.OK
    host = DeviceRows(yf.eng, h)
    try:
        assert _code(lambda: yf.eng.yield_rows(host, ["w"], [good])) == L.E_INVALID_ARGUMENT
    finally:
        host.free()


def test_status_2_partitioned_engine():
    """A LocalCluster of 2 in-process ranks: its rows live on several ranks.  Before the syntax check."""
    src, kb = _kv()
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.register_tag(7, "t", T_SCHEMA)
        c.load_builder(kb)
        ys = [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()]
        rows = c.each(lambda e: e.go_device([ROOTS[0]], [1], 1, b"", ys))
        assert sum(r.count for r in rows) > 0
        for e, r in zip(c.engines, rows):
            assert _code(lambda: _yield(e, r, ["d", "w"], "YIELD $-.d")) == L.E_UNSUPPORTED
            assert _code(lambda: _yield(e, r, ["d", "w"], "YIELD e.w")) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()


@pytest.mark.parametrize("text", ["YIELD $^.t.name", "YIELD $$.t.name", "YIELD e.w", "YIELD e._dst", "YIELD $-.d WHERE e.w > 1",
                                  "YIELD $-.d WHERE $$.t.name == \"n1\"", "YIELD COUNT(*), $-.d", "YIELD SUM($-.w), $v.d"])
def test_status_3_syntax_errors(yf, text):
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, text)) == L.E_SYNTAX_ERROR


def test_status_3_comes_before_4_5_6(yf):
    empty, names = _go(yf.eng, "e._dst AS d, e.w AS w", EMPTY_SRC)
    try:
        assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d, $v.w, e.w")) == L.E_SYNTAX_ERROR
        assert _code(lambda: _yield(yf.eng, empty, names, "YIELD $^.t.name")) == L.E_SYNTAX_ERROR           # even without rows
        assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.zz, $$.t.name")) == L.E_SYNTAX_ERROR
    finally:
        empty.free()


def test_status_4_input_and_variable(yf):
    empty, names = _go(yf.eng, "e._dst AS d, e.w AS w", EMPTY_SRC)
    try:
        for text in ("YIELD $v.d WHERE $-.w > 1", "YIELD $-.d, $v.w", "YIELD $v.d WHERE $u.w > 1", "YIELD $v.d, $u.w"):
            assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, text)) == L.E_EXECUTION_ERROR
            assert _code(lambda: _yield(yf.eng, empty, names, text)) == L.E_EXECUTION_ERROR                # before 5
        with pytest.raises(NbgError, match="Not support both input and variable."):
            _yield(yf.eng, yf.rows, yf.names, "YIELD $v.d WHERE $-.w > 1")
        with pytest.raises(NbgError, match="Only one variable allowed to use."):
            _yield(yf.eng, yf.rows, yf.names, "YIELD $v.d WHERE $u.zz > 1")                                # before 6
    finally:
        empty.free()


def test_status_5_zero_input_rows(yf):
    empty, names = _go(yf.eng, "e._dst AS d, e.w AS w, $$.t.name AS s", EMPTY_SRC)
    assert empty.count == 0
    try:
        for text, ncols in (("YIELD $-.d", 1), ("YIELD $-.*, $-.w + 1", 4), ("YIELD $-.zz, $-.*", 4),      # before 6
                            ("YIELD $-.s + \"x\" WHERE $-.zz == 1", 1), ("YIELD AVG($-.w), COUNT(*)", 2)):  # before 7
            out = _yield(yf.eng, empty, names, text)
            assert out.count == 0 and yf.eng.lib.nbg_rows_num_cols(out.h) == ncols and _take(out) == []
    finally:
        empty.free()


def test_status_6_unknown_column(yf):
    with pytest.raises(NbgError, match="column `zz' not exist in input.") as ex:
        _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d WHERE $-.zz > 1")
    assert ex.value.code == L.E_EXECUTION_ERROR
    with pytest.raises(NbgError, match="column `abc' not exist in variable.") as ex:
        _yield(yf.eng, yf.rows, yf.names, "YIELD $v.abc")
    assert ex.value.code == L.E_EXECUTION_ERROR
    # before 7: with an aggregate, with a string-building column
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD SUM($-.zz)")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, 'YIELD $-.s + "x", $-.zz')) == L.E_EXECUTION_ERROR
    # with duplicate names the first match wins
    dup = ["a", "a"] + yf.names[2:]
    assert _bits(_take(_yield(yf.eng, yf.rows, dup, "YIELD $-.a"))) == _bits([[r[0]] for r in yf.inp.rows])


def test_status_8_evaluation_errors(yf):
    """`$-.w / ($-.w + 7)`: the rows with w == -7 fail.  In the WHERE of any row, or in a YIELD of a
    passing row, the call fails with no result; in a YIELD of a rejected row it does not."""
    assert any(r[3] == -7 for r in yf.inp.rows)
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d WHERE $-.w / ($-.w + 7) > 0")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.w / ($-.w + 7)")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.w % ($-.w + 7) WHERE $-.w < 0")) == L.E_EXECUTION_ERROR
    text = "YIELD $-.d, $-.w / ($-.w + 7) AS q WHERE $-.w != -7"
    assert _bits(_take(_yield(yf.eng, yf.rows, yf.names, text))) == _bits(_model(yf.inp, text)[0].rows)
    # a statically ill-typed node is an error of every row that evaluates it
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.b2 + 1")) == L.E_EXECUTION_ERROR
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, 'YIELD $-.d WHERE $-.s < 1')) == L.E_EXECUTION_ERROR
    assert _take(_yield(yf.eng, yf.rows, yf.names, "YIELD $-.b2 + 1 WHERE $-.w > 1000")) == []
    assert yf.rows.digest() == yf.digest


# ------------------------------------------------------------------------------ 4. device limits
def test_limit_aggregates(yf):
    for text in ("YIELD COUNT(*)", "YIELD AVG($-.w), SUM($-.x), COUNT(*), 1 + 1", "YIELD MAX($v.w)"):
        assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, text)) == L.E_UNSUPPORTED


@pytest.mark.parametrize("text", ['YIELD $-.s + "!"', "YIELD (string)$-.w", "YIELD upper($-.s)", "YIELD $-.d, (string)$-.b2 AS t",
                                  'YIELD lpad(left($-.s, 2), 5, $-.s) WHERE $-.w > 0'])
def test_limit_string_building(yf, text):
    """A YIELD that stores a string it built (the programs with OP_SOUT / OP_SMAT)."""
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, text)) == L.E_UNSUPPORTED


def test_limit_strings_outside_the_dictionary(yf):
    """A derived table or a constant outside the dictionary: the column passes through (and the
    result spells it), any other use is out of scope."""
    for ys in ('$$.t.name + "!" AS s, e.w AS w', '"no such name" AS s, e.w AS w'):
        rows, names = _go(yf.eng, ys, ROOTS[0], 2)
        inp = ngql.Interim(names, rows.fetch())
        try:
            assert inp.rows and all(r[0].endswith("!") or r[0] == "no such name" for r in inp.rows)
            text = "YIELD $-.w, $-.s WHERE $-.w > 0"
            assert _bits(_take(_yield(yf.eng, rows, names, text))) == _bits(_model(inp, text)[0].rows)
            assert _code(lambda: _yield(yf.eng, rows, names, 'YIELD $-.s == "n1"')) == L.E_UNSUPPORTED
            assert _code(lambda: _yield(yf.eng, rows, names, 'YIELD $-.w WHERE $-.s < "n1"')) == L.E_UNSUPPORTED
            assert _code(lambda: _yield(yf.eng, rows, names, "YIELD hash($-.s)")) == L.E_UNSUPPORTED
        finally:
            rows.free()


def test_limit_float_and_misaligned_inputs(yf):
    for ys in ("e._dst AS d, e.f AS f", "e._dst AS d, e.x + e.w AS m, e.w AS w"):
        rows, names = _go(yf.eng, ys)
        try:
            assert _code(lambda: _yield(yf.eng, rows, names, "YIELD $-.d")) == L.E_UNSUPPORTED
        finally:
            rows.free()


def test_limit_too_many_columns(yf):
    rows, names = _go(yf.eng, ", ".join(f"e.w + {k} AS c{k}" for k in range(17)), ROOTS[0])
    inp = ngql.Interim(names, rows.fetch())
    try:
        assert _code(lambda: _yield(yf.eng, rows, names, "YIELD $-.*, $-.*")) == L.E_UNSUPPORTED           # 34 after expansion
        text = "YIELD $-.*, " + ", ".join(f"$-.c{k} * 2" for k in range(15))                               # 32: answered
        assert _bits(_take(_yield(yf.eng, rows, names, text))) == _bits(_model(inp, text)[0].rows)
    finally:
        rows.free()


def _balanced_sum(terms):
    while len(terms) > 1:
        terms = [f"({a} + {b})" if b else a for a, b in zip(terms[0::2], terms[1::2] + [None])]
    return terms[0]


def test_limit_program_length(yf):
    long_ = "YIELD " + _balanced_sum([f"$-.w * {k}" for k in range(100)])                                    # > 256 instructions
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, long_)) == L.E_UNSUPPORTED
    assert _code(lambda: _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d WHERE " + long_[6:] + " > 0")) == L.E_UNSUPPORTED
    ok = "YIELD " + _balanced_sum([f"$-.w * {k}" for k in range(20)])
    assert _bits(_take(_yield(yf.eng, yf.rows, yf.names, ok))) == _bits(_model(yf.inp, ok)[0].rows)


# ------------------------------------------------------------------------------ 5. chaining
def test_output_feeds_every_stage(yf):
    text = "YIELD $-.k7 AS k, $-.w + 1 AS w1, $-.x AS x WHERE $-.w % 2 == 0"
    mid, _ = _model(yf.inp, text, yf.types)
    out = _yield(yf.eng, yf.rows, yf.names, text)
    names = mid.columns
    try:
        gs = groupby.parse_sentence("GROUP BY $-.k YIELD $-.k, COUNT(*), SUM($-.w1)")
        got = _take(yf.eng.group_by(out, names, [c.expr.encode() for c in gs.groups],
                                    [(c.fun, c.expr.encode(), c.alias) for c in gs.yields]))
        assert groupby.multiset(got) == groupby.multiset(groupby.group_model(mid, gs.groups, gs.yields).rows)
        top = _take(yf.eng.order_by(out, names, [("w1", True), ("x", False)], (0, 10)))
        orderby.check_window(top, mid, [("w1", True), ("x", False)], (0, 10))
        both = _take(yf.eng.set_op(out, out, "UNION"))
        assert _bits(both) == _bits(mid.rows + mid.rows)
        again_text = "YIELD $-.w1 * 2 AS w2, $-.k WHERE $-.x < 0.0"
        again = _take(_yield(yf.eng, out, names, again_text))
        assert _bits(again) == _bits(_model(mid, again_text)[0].rows) and again
    finally:
        out.free()


def test_inputs_from_every_stage(yf):
    gs = groupby.parse_sentence("GROUP BY $-.k7 YIELD $-.k7 AS k7, COUNT(*) AS n")
    grouped = yf.eng.group_by(yf.rows, yf.names, [c.expr.encode() for c in gs.groups],
                              [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    ordered = yf.eng.order_by(yf.rows, yf.names, [("x", False)], (3, 700))
    united = yf.eng.set_op(ordered, ordered, "UNION")
    try:
        for rows, names, text in ((grouped, ["k7", "n"], "YIELD $-.n * 2 AS n2, $-.k7 WHERE $-.k7 > -3"),
                                  (ordered, yf.names, "YIELD $-.x, $-.s WHERE $-.b2"),
                                  (united, yf.names, "YIELD $-.d WHERE $-.w > 0")):
            inp = ngql.Interim(names, rows.fetch())
            assert inp.rows
            assert _bits(_take(_yield(yf.eng, rows, names, text))) == _bits(_model(inp, text)[0].rows)
    finally:
        grouped.free()
        ordered.free()
        united.free()


def test_order_by_yield_limit_is_exact(yf):
    """`ORDER BY $-.x DESC | YIELD $-.d | LIMIT 5`: the first five rows of the ordered input."""
    ordered = yf.eng.order_by(yf.rows, yf.names, [("x", True), ("d", False)])
    try:
        first = ordered.fetch()[:5]
        y = _yield(yf.eng, ordered, yf.names, "YIELD $-.d")
        top = _take(yf.eng.order_by(y, ["d"], [], (0, 5)))
        y.free()
        assert _bits(top) == _bits([[r[1]] for r in first])
        mod = orderby.order_model(yf.inp, [("x", True), ("d", False)]).rows[:5]
        assert _bits(top) == _bits([[r[1]] for r in mod])
    finally:
        ordered.free()
    # the same through the session: every stage on the device
    ses = yieldpipe.Session(yf.eng, device=True)
    dev = ses.execute(f"{yf.go} | ORDER BY $-.x DESC, $-.d | YIELD $-.d | LIMIT 5")
    assert ses.yield_calls == 1 and not ses.fallbacks and _bits(dev.rows) == _bits([[r[1]] for r in mod])


def test_session_keeps_the_pipe_on_the_device(yf):
    text = (f"(({yf.go} | YIELD $-.d AS d, $-.w AS w WHERE $-.w > 40) UNION ({yf.go} | YIELD $-.d AS d, $-.w AS w WHERE $-.w < -45))"
            " | YIELD $-.w AS w, $-.d % 5 AS m | GROUP BY $-.w YIELD $-.w, COUNT(*), SUM($-.m)")
    mod = yieldpipe.Session(yf.orc).execute(text)
    ses = yieldpipe.Session(yf.eng, device=True)
    dev = ses.execute(text)
    assert ses.yield_calls == 3 and ses.set_calls == [("UNION", True)] and not ses.fallbacks
    assert mod.rows and groupby.multiset(dev.rows) == groupby.multiset(mod.rows)


def test_col_types_through_union(yf):
    """The result's col_types, seen through nbg_set_op's implicit cast to a DOUBLE left side: a VID
    column passed through is INT (cast by (double)), and `(double)$-.w` is DOUBLE (no cast).  AVG
    over a passed-through VID column is accepted where nbg_group_by refuses the GO's own."""
    left = _yield(yf.eng, yf.rows, yf.names, "YIELD $-.x AS a")
    vid = _yield(yf.eng, yf.rows, yf.names, "YIELD $-.d AS a")
    dbl = _yield(yf.eng, yf.rows, yf.names, "YIELD (double)$-.w AS a")
    try:
        n = len(yf.inp.rows)
        u = _take(yf.eng.set_op(left, vid, "UNION"))
        assert all(type(r[0]) is float for r in u)
        assert _bits(u[n:]) == _bits([[float(r[1])] for r in yf.inp.rows])
        u = _take(yf.eng.set_op(left, dbl, "UNION"))
        assert _bits(u[n:]) == _bits([[float(r[3])] for r in yf.inp.rows])
        assert yf.eng.lib.nbg_rows_col_kind(dbl.h, 0) == L.V_DOUBLE and yf.eng.lib.nbg_rows_col_kind(vid.h, 0) == L.V_INT
        gs = groupby.parse_sentence("GROUP BY $-.a YIELD AVG($-.a)")
        args = (["a"], [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
        d_only, _ = _go(yf.eng, "e._dst AS a")
        assert _code(lambda: yf.eng.group_by(d_only, *args)) == L.E_UNSUPPORTED
        d_only.free()
        yf.eng.group_by(vid, *args).free()
    finally:
        left.free()
        vid.free()
        dbl.free()


# ------------------------------------------------------------------------------ 6. fusion equivalence
def test_fusion_equivalence_against_the_oracle():
    """GO | YIELD ... WHERE on the device against the oracle's one GO with the WHERE and YIELD fused."""
    src, dst, w = graphs.rmat_graph(10)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    try:
        for r in graphs.roots(src, 2):
            rows = eng.go_device([r], [1], 2, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()])
            out = _yield(eng, rows, ["d", "w"], "YIELD $-.d, $-.w * 2 + 1 AS x WHERE $-.w < 50 && $-.d % 3 != 0")
            got = out.digest()
            out.free()
            rows.free()
            g = ngql.Parser("GO FROM 1 OVER e WHERE e.w < 50 && e._dst % 3 != 0 YIELD e._dst, e.w * 2 + 1").go()
            exp = orc.go([r], [1], 2, g.where.encode(), [c.expr.encode() for c in g.yields])
            assert exp
            want = graphs.multiset_digest([np.array([x[0] for x in exp], np.int64), np.array([x[1] for x in exp], np.int64)])
            assert tuple(got) == want
    finally:
        eng.close()
        orc.close()
