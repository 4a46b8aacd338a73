"""nbg_set_op on the MI355X: UNION / INTERSECT / MINUS over device-resident rows, judged by the
plain-Python model of tests/support/setops.py (pinned to the reference's SetTest vectors by
tests/test_setops_model.py) over the CPU oracle's rows — never by the device itself.

The random-parity graph, GO and columns are those of tests/test_gpu_orderby.py (seeded RMAT-10).
The left operand is the 2-step GO from ROOTS[0]; the right one is the 2-step GO from RIGHT, another
root of the same graph: the GO from test_gpu_orderby's ROOTS[1] has 853 rows against the left's
4386, so over the 26 values of shape (a) no value occurs more often on the right than on the left.
From RIGHT both sides have some 4,400 rows in several segments.  The shapes:
  a  k7, b2    at most 26 distinct rows: heavy duplicates, the two sides' counts differ
  b  d, w, x   nearly unique rows (a GO visits an edge once, so every count is 0 or 1)
  c  s, z      dictionary strings and both zeros
  d  w, k7     the right side is the 1-step GO from RIGHT (80 rows): duplicates AND a difference
What each shape can show is asserted from the oracle's rows in the fixture (WANT).  No shape of
thousands of rows over 26 values has a value missing on one side, so (a) and (c) have an empty
difference (their MINUS is the empty result); (d) is there for a duplicate-heavy MINUS that keeps
rows.  Together the shapes cover every row of the multiplicity table.

Cells these rows never hold, the wrap of the row table and the inputs of more chunks than
workgroups are the subject of tests/test_gpu_values_setops.py.

Two NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
column whose kind differs between OVER types, and the row-count limits."""
import ctypes as C
from collections import Counter

import pytest

from nebula_amd import LocalCluster, NbgError, _lib as L, expr as E
from nebula_amd.engine import DeviceRows, nba_engine
from tests.support import golden, groupby, ngql, orderby, setops
from tests.support.oracle import Oracle
from tests.test_gpu_orderby import E_SCHEMA, PARTS, ROOTS, T_SCHEMA, _kv

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("setop_golden.json")["cases"]
RIGHT = 5449003421900272633
EMPTY_SRC = 123                       # no such vertex: a GO from it has no rows
OPS = [("UNION", False), ("UNION", True), ("INTERSECT", False), ("MINUS", False)]
OP_IDS = ["union_all", "union_distinct", "intersect", "minus"]
SHAPES = {
    "a": ("e.w % 7 AS k7, (bool)(e.w % 2 == 0) AS b2", 2),
    "b": ("e._dst AS d, e.w AS w, e.x AS x", 2),
    "c": ("$$.t.name AS s, e.x * 0.0 AS z", 2),
    "d": ("e.w AS w, e.w % 7 AS k7", 1),
}
# what the oracle's rows of a shape must show: (intersection, difference, cL > cR >= 1, cR > cL >= 1, duplicates)
WANT = {"a": (True, False, True, True, True), "b": (True, True, False, False, True),
        "c": (True, False, True, True, True), "d": (True, True, True, False, True)}


class Side:
    """One operand: its GO text, the oracle's rows and types, the same rows on the device."""

    def __init__(self, f, root, yields, steps):
        self.text = f"GO {steps} STEPS FROM {root} OVER e YIELD {yields}"
        s = orderby.Session(f.orc)
        self.inp = s.execute(self.text)
        self.sent = ngql.Parser(self.text).go()
        self.types = groupby.go_column_types(self.sent, self.inp.rows)
        self.names = [c.name() for c in self.sent.yields]
        self.rows = f.eng.go_device([root], [1], steps, b"", [c.expr.encode() for c in self.sent.yields])
        assert self.rows.count == len(self.inp.rows)
        self.digest = self.rows.digest()
        self.fetched = self.rows.fetch()


class Fixture:
    pass


@pytest.fixture(scope="module")
def so():
    """Engine, oracle and, per shape, both operands: computed once and left unchanged."""
    src, kb = _kv()
    assert {ROOTS[0], RIGHT} <= set(src.tolist()) and EMPTY_SRC not in set(src.tolist())
    f = Fixture()
    from nebula_amd import Engine
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.load_builder(kb)
    f.orc = Oracle(PARTS)
    f.orc.register(True, 1, "e", E_SCHEMA)
    f.orc.register(False, 7, "t", T_SCHEMA)
    f.orc.load_builder(kb)
    f.left, f.right = {}, {}
    for name, (ys, rsteps) in SHAPES.items():
        f.left[name] = Side(f, ROOTS[0], ys, 2)
        f.right[name] = Side(f, RIGHT, ys, rsteps)
        lt, rt = f.left[name], f.right[name]
        assert len(lt.inp.rows) >= 2048 and f.eng.lib.nbg_rows_num_segments(lt.rows.h) >= 2
        if rsteps == 2:
            assert len(rt.inp.rows) >= 2048 and f.eng.lib.nbg_rows_num_segments(rt.rows.h) >= 2
        cl = Counter(setops.row_key(r) for r in lt.inp.rows)
        cr = Counter(setops.row_key(r) for r in rt.inp.rows)
        have = (any(k in cr for k in cl), any(k not in cr for k in cl),
                any(cl[k] > cr.get(k, 0) >= 1 for k in cl), any(cr.get(k, 0) > cl[k] >= 1 for k in cl),
                any(v > 1 for v in (cl + cr).values()))
        assert have == WANT[name], (name, have)
    assert all(any(WANT[s][i] for s in WANT) for i in range(5))     # every property somewhere
    yield f
    for side in list(f.left.values()) + list(f.right.values()):
        side.rows.free()
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


def _ms(rows):
    return groupby.multiset(rows)


def _model(lt, rt, op, distinct):
    return setops.set_model(lt.inp, rt.inp, op, distinct, lt.types, rt.types)[0].rows


def _unchanged(*sides):
    for s in sides:
        assert s.rows.digest() == s.digest


# ------------------------------------------------------------------------------ 1. golden cases
FALLBACK_QUERY_PART = "$$.team.name as player UNION ALL"      # name / team name UNION ALL name / start_year


@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, case):
    """Every operand's last GO with go_device, every set operation with nbg_set_op, one fetch.  The
    one case that may complete through the model is the `$$.team.name` UNION ALL `serve.start_year`
    block: its int-to-string cast is out of device scope (NBG_E_UNSUPPORTED)."""
    ses = setops.Session(nba, device=True)
    ok, msg = setops.run_case(ses, case)
    assert ok, msg
    if case["status"] != "SUCCEEDED":
        return
    n_ops = sum(case["query"].upper().count(f" {w} ") for w in ("UNION", "INTERSECT", "MINUS"))
    if FALLBACK_QUERY_PART in case["query"]:
        assert ses.fallbacks == [("UNION", L.E_UNSUPPORTED)] and not ses.set_calls
    else:
        assert not ses.fallbacks and len(ses.set_calls) == n_ops >= 1


def test_golden_has_the_one_fallback_case():
    assert sum(FALLBACK_QUERY_PART in c["query"] and c["status"] == "SUCCEEDED" for c in GOLDEN) == 1


# ------------------------------------------------------------------------------ 2. random parity
@pytest.mark.parametrize("op,distinct", OPS, ids=OP_IDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_parity(so, shape, op, distinct):
    lt, rt = so.left[shape], so.right[shape]
    out = so.eng.set_op(lt.rows, rt.rows, op, distinct)
    assert out.count == 0 or so.eng.lib.nbg_rows_num_segments(out.h) == 1
    dev = _take(out)
    want = _model(lt, rt, op, distinct)
    assert len(dev) == len(want)
    assert _ms(dev) == _ms(want)
    if op == "UNION" and not distinct:          # exact: the left's fetch order, then the right's
        assert _bits(dev) == _bits(lt.fetched + rt.fetched)
    if op == "MINUS" and not WANT[shape][1]:
        assert dev == []
    _unchanged(lt, rt)


def test_limit_of_union_all_is_exact(so):
    lt, rt = so.left["b"], so.right["b"]
    u = so.eng.set_op(lt.rows, rt.rows, "UNION")
    n = len(lt.fetched)
    got = _take(so.eng.order_by(u, lt.names, [], (n - 5, 12)))
    u.free()
    assert _bits(got) == _bits((lt.fetched + rt.fetched)[n - 5:n + 7])


# ------------------------------------------------------------------------------ 3. casts
def _go(eng, yields, root=ROOTS[0], steps=1):
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {yields}").go()
    rows = eng.go_device([root], [1], steps, b"", [c.expr.encode() for c in sent.yields])
    return rows, sent


def _oracle(orc, yields, root=ROOTS[0], steps=1):
    text = f"GO {steps} STEPS FROM {root} OVER e YIELD {yields}"
    inp = orderby.Session(orc).execute(text)
    return inp, groupby.go_column_types(ngql.Parser(text).go(), inp.rows)


CASTS = {
    "int_from_double": ("e.w AS a", "e.x AS a"),                 # DOUBLE -> INT: truncation
    "double_from_int": ("e.x AS a", "e.w AS a"),
    "bool_from_int": ("(bool)(e.w % 2 == 0) AS a", "e.w % 3 AS a"),
    "int_from_bool": ("e.w % 3 AS a", "(bool)(e.w % 2 == 0) AS a"),
    "vid_from_int": ("e._dst AS a", "e.w AS a"),
    "bool_from_double": ("(bool)(e.w % 2 == 0) AS a", "e.x * 0.0 AS a"),
    "double_from_bool": ("e.x * 0.0 AS a", "(bool)(e.w % 2 == 0) AS a"),
}


@pytest.mark.parametrize("op,distinct", OPS, ids=OP_IDS)
@pytest.mark.parametrize("cast", list(CASTS))
def test_casts(so, cast, op, distinct):
    ly, ry = CASTS[cast]
    ly, ry = ly + ", e.w % 5 AS g", ry + ", e.w % 5 AS g"
    li, lt = _oracle(so.orc, ly, ROOTS[0], 2)
    ri, rt = _oracle(so.orc, ry, RIGHT, 2)
    assert lt[0] != rt[0] and lt[1] == rt[1]
    lrows, _ = _go(so.eng, ly, ROOTS[0], 2)
    rrows, _ = _go(so.eng, ry, RIGHT, 2)
    try:
        out = so.eng.set_op(lrows, rrows, op, distinct)
        kind = so.eng.lib.nbg_rows_col_kind(out.h, 0) if out.count else None
        dev = _take(out)
    finally:
        lrows.free()
        rrows.free()
    want = setops.set_model(li, ri, op, distinct, lt, rt)[0].rows
    assert _ms(dev) == _ms(want)
    if dev:                                       # the result takes the left's kind
        assert kind == {groupby.DOUBLE: L.V_DOUBLE, groupby.BOOL: L.V_BOOL}.get(lt[0], L.V_INT)
        assert all(type(r[0]) is type(li.rows[0][0]) for r in dev)


def test_cast_result_column_is_a_vid(so):
    """VID against INT: the result's column is a VID, so AVG over it is what nbg_group_by refuses
    for VID columns (and accepts for the INT column of the reverse call)."""
    lrows, _ = _go(so.eng, "e._dst AS a")
    rrows, _ = _go(so.eng, "e.w AS a", RIGHT)
    gs = groupby.parse_sentence("GROUP BY $-.a YIELD AVG($-.a)")
    args = (["a"], [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    try:
        u = so.eng.set_op(lrows, rrows, "UNION")
        with pytest.raises(NbgError) as ex:
            so.eng.group_by(u, *args)
        assert ex.value.code == L.E_UNSUPPORTED
        u.free()
        u = so.eng.set_op(rrows, lrows, "UNION")
        so.eng.group_by(u, *args).free()
        u.free()
    finally:
        lrows.free()
        rrows.free()


# ------------------------------------------------------------------------------ 4. empty shortcuts
@pytest.mark.parametrize("op,distinct", OPS, ids=OP_IDS)
def test_empty_shortcuts(so, op, distinct):
    lt = so.left["a"]
    empty, _ = _go(so.eng, SHAPES["a"][0], EMPTY_SRC)
    other, _ = _go(so.eng, "e.x AS k7, e.x AS b2", EMPTY_SRC)         # other types: no schema check
    assert empty.count == 0
    try:
        a_e = _take(so.eng.set_op(lt.rows, empty, op, distinct))
        e_a = _take(so.eng.set_op(empty, lt.rows, op, distinct))
        e_e = so.eng.set_op(empty, other, op, distinct)
        assert e_e.count == 0 and so.eng.lib.nbg_rows_num_cols(e_e.h) == 2 and _take(e_e) == []
        as_it_is = _bits(_take(so.eng.order_by(lt.rows, lt.names, [])))
        assert as_it_is == _bits(lt.fetched)
        if op == "UNION":       # the other side as it is: its duplicates kept, even under DISTINCT
            assert _bits(a_e) == as_it_is and _bits(e_a) == as_it_is and len(set(as_it_is)) < len(as_it_is)
        elif op == "INTERSECT":
            assert a_e == [] and e_a == []
        else:
            assert _bits(a_e) == as_it_is and e_a == []
        assert _take(so.eng.set_op(lt.rows, other, op, distinct)) == a_e
    finally:
        empty.free()
        other.free()
    _unchanged(lt)


def test_empty_union_keeps_the_right_sides_types(so):
    empty, _ = _go(so.eng, "e.w AS a", EMPTY_SRC)
    right, _ = _go(so.eng, "e.x AS a")
    try:
        out = so.eng.set_op(empty, right, "UNION", True)
        assert so.eng.lib.nbg_rows_col_kind(out.h, 0) == L.V_DOUBLE
        assert _bits(_take(out)) == _bits(right.fetch())
    finally:
        empty.free()
        right.free()


def test_field_count_even_when_both_are_empty(so):
    one, _ = _go(so.eng, "e.w AS a", EMPTY_SRC)
    two, _ = _go(so.eng, "e.w AS a, e.w AS b", EMPTY_SRC)
    try:
        for op, d in OPS:
            assert _code(lambda: so.eng.set_op(one, two, op, d)) == L.E_EXECUTION_ERROR
            assert _code(lambda: so.eng.set_op(so.left["a"].rows, one, op, d)) == L.E_EXECUTION_ERROR
        with pytest.raises(NbgError, match="Field count not match."):
            so.eng.set_op(one, two, "UNION")
    finally:
        one.free()
        two.free()


def test_pass_through_keeps_order_bys_limits(so):
    """`As it is` is nbg_order_by without factors and LIMIT, its NBG_E_UNSUPPORTED cases included."""
    empty, _ = _go(so.eng, "e._dst AS d, e.w AS f", EMPTY_SRC)
    flt, _ = _go(so.eng, "e._dst AS d, e.f AS f")
    try:
        assert _code(lambda: so.eng.order_by(flt, ["d", "f"], [])) == L.E_UNSUPPORTED
        assert _code(lambda: so.eng.set_op(flt, empty, "UNION")) == L.E_UNSUPPORTED
        assert _code(lambda: so.eng.set_op(flt, empty, "MINUS")) == L.E_UNSUPPORTED
        assert _take(so.eng.set_op(flt, empty, "INTERSECT")) == []
    finally:
        empty.free()
        flt.free()


# ------------------------------------------------------------------------------ 5. chaining and inputs
@pytest.mark.parametrize("shape", ["a", "b"])
def test_left_is_right(so, shape):
    lt = so.left[shape]
    for op, d in OPS:
        dev = _take(so.eng.set_op(lt.rows, lt.rows, op, d))
        assert _ms(dev) == _ms(_model(lt, lt, op, d)), (op, d)
    assert _take(so.eng.set_op(lt.rows, lt.rows, "MINUS")) == []
    assert _ms(_take(so.eng.set_op(lt.rows, lt.rows, "INTERSECT"))) == _ms(lt.inp.rows)
    _unchanged(lt)


def test_chain_on_the_device(so):
    """(A MINUS B) UNION C INTERSECT D, left-associative, every step on the device."""
    ys = SHAPES["b"][0]
    roots = {"A": ROOTS[0], "B": RIGHT, "C": ROOTS[1], "D": RIGHT}
    text = (f"(GO 2 STEPS FROM {roots['A']} OVER e YIELD {ys} MINUS GO 2 STEPS FROM {roots['B']} OVER e YIELD {ys})"
            f" UNION GO 2 STEPS FROM {roots['C']} OVER e YIELD {ys} INTERSECT GO 2 STEPS FROM {roots['D']} OVER e YIELD {ys}")
    mod = setops.Session(so.orc).execute(text)
    ses = setops.Session(so.eng, device=True)
    dev = ses.execute(text)
    assert ses.set_calls == [("MINUS", False), ("UNION", True), ("INTERSECT", False)] and not ses.fallbacks
    assert dev.columns == mod.columns and len(mod.rows) > 0
    assert _ms(dev.rows) == _ms(mod.rows)


def test_output_feeds_group_by_and_order_by(so):
    lt, rt = so.left["a"], so.right["a"]
    gs = groupby.parse_sentence("GROUP BY $-.k7, $-.b2 YIELD $-.k7, $-.b2, COUNT(*)")
    args = (lt.names, [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    for op, d in OPS[:3]:
        out = so.eng.set_op(lt.rows, rt.rows, op, d)
        want = ngql.Interim(lt.names, _model(lt, rt, op, d))
        got = _take(so.eng.group_by(out, *args))
        assert _ms(got) == _ms(groupby.group_model(want, gs.groups, gs.yields, lt.types).rows)
        top = _take(so.eng.order_by(out, lt.names, [("k7", True), ("b2", False)], (0, 10)))
        orderby.check_window(top, want, [("k7", True), ("b2", False)], (0, 10))
        out.free()
    _unchanged(lt, rt)


def test_inputs_from_group_by_and_order_by(so):
    lt, rt = so.left["a"], so.right["a"]
    gs = groupby.parse_sentence("GROUP BY $-.k7, $-.b2 YIELD $-.k7 AS k7, $-.b2 AS b2")
    args = (lt.names, [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    grouped = so.eng.group_by(lt.rows, *args)                      # the left's distinct rows
    ordered = so.eng.order_by(rt.rows, rt.names, [("k7", False)], (0, 700))
    g_int = ngql.Interim(lt.names, grouped.fetch())
    o_int = ngql.Interim(rt.names, ordered.fetch())
    assert len(g_int.rows) == len({setops.row_key(r) for r in lt.inp.rows}) and len(o_int.rows) == 700
    for op, d in OPS:
        dev = _take(so.eng.set_op(grouped, ordered, op, d))
        assert _ms(dev) == _ms(setops.set_model(g_int, o_int, op, d, lt.types, rt.types)[0].rows), (op, d)
        dev = _take(so.eng.set_op(ordered, grouped, op, d))
        assert _ms(dev) == _ms(setops.set_model(o_int, g_int, op, d, rt.types, lt.types)[0].rows), (op, d)
    # a set operation's output is an input of the next
    inter = so.eng.set_op(lt.rows, rt.rows, "INTERSECT")
    again = _take(so.eng.set_op(inter, grouped, "MINUS"))
    assert again == []
    inter.free()
    grouped.free()
    ordered.free()
    _unchanged(lt, rt)


# ------------------------------------------------------------------------------ 6. statuses and limits
def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def test_bad_operator(so):
    lt = so.left["a"]
    for op in (0, 4, -1):
        assert _code(lambda: so.eng.set_op(lt.rows, lt.rows, op)) == L.E_INVALID_ARGUMENT
    with pytest.raises(KeyError):
        so.eng.set_op(lt.rows, lt.rows, "EXCEPT")


def test_rows_of_another_engine(so, nba):
    sent = ngql.Parser("GO FROM 1 OVER like YIELD like._dst AS d, like.likeness AS b2").go()
    other = nba.go_device([5662213458193308137], [nba.edge_types["like"]], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        assert _code(lambda: so.eng.set_op(so.left["a"].rows, other, "UNION")) == L.E_INVALID_ARGUMENT
        assert _code(lambda: so.eng.set_op(other, so.left["a"].rows, "MINUS")) == L.E_INVALID_ARGUMENT
    finally:
        other.free()


def test_host_only_rows_rejected(so):
    req, keep = so.eng._go_request([ROOTS[0]], [1], 1, b"", [E.edge_prop("e", "w").encode()], False, False)
    rows = C.c_void_p()
    assert so.eng.lib.nbg_go(so.eng.h, C.byref(req), C.byref(rows)) == L.OK     # rows copied to the host
    host = DeviceRows(so.eng, rows)
    dev, _ = _go(so.eng, "e.w AS w")
    try:
        assert _code(lambda: so.eng.set_op(host, dev, "UNION")) == L.E_INVALID_ARGUMENT
        assert _code(lambda: so.eng.set_op(dev, host, "INTERSECT")) == L.E_INVALID_ARGUMENT
    finally:
        host.free()
        dev.free()


def test_partitioned_engine():
    """A LocalCluster of 2 in-process ranks: its rows live on several ranks."""
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
            assert _code(lambda: e.set_op(r, r, "UNION")) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()


def _pair_code(so, ly, ry, op="INTERSECT"):
    lrows, _ = _go(so.eng, ly)
    rrows, _ = _go(so.eng, ry, RIGHT)
    try:
        return _code(lambda: so.eng.set_op(lrows, rrows, op))
    finally:
        lrows.free()
        rrows.free()


def test_limit_float_and_misaligned_inputs(so):
    assert _pair_code(so, "e._dst AS d, e.f AS f", "e._dst AS d, e.x AS f") == L.E_UNSUPPORTED
    assert _pair_code(so, "e._dst AS d, e.x AS f", "e._dst AS d, e.f AS f", "UNION") == L.E_UNSUPPORTED
    # a DOUBLE value in a column typed INT by its last getter: the reference re-reads shifted rows
    assert _pair_code(so, "e._dst AS d, e.x + e.w AS m", "e._dst AS d, e.w AS m", "MINUS") == L.E_UNSUPPORTED


def test_limit_string_against_int(so):
    for op in ("UNION", "INTERSECT", "MINUS"):
        assert _pair_code(so, "$$.t.name AS s", "e.w AS s", op) == L.E_UNSUPPORTED
        assert _pair_code(so, "e.w AS s", "$$.t.name AS s", op) == L.E_UNSUPPORTED


def test_limit_string_constant_outside_the_dictionary(so):
    assert _pair_code(so, '"no such name" AS s, e.w AS w', "$$.t.name AS s, e.w AS w") == L.E_UNSUPPORTED
    assert _pair_code(so, "$$.t.name AS s, e.w AS w", '"no such name" AS s, e.w AS w', "UNION") == L.E_UNSUPPORTED
    assert _pair_code(so, '"no such name" AS s, e.w AS w', '"another" AS s, e.w AS w', "MINUS") == L.E_UNSUPPORTED


def test_derived_strings_compare_across_results(so):
    """Derived codes are content hashes: the same text from two GOs is one value, and the result
    spells it."""
    ys = '$$.t.name + "!" AS s'
    li, lt = _oracle(so.orc, ys, ROOTS[0], 2)
    ri, rt = _oracle(so.orc, ys, RIGHT, 2)
    lrows, _ = _go(so.eng, ys, ROOTS[0], 2)
    rrows, _ = _go(so.eng, ys, RIGHT, 2)
    try:
        for op, d in OPS[1:]:
            dev = _take(so.eng.set_op(lrows, rrows, op, d))
            assert _ms(dev) == _ms(setops.set_model(li, ri, op, d, lt, rt)[0].rows), (op, d)
            assert all(r[0].endswith("!") for r in dev)
    finally:
        lrows.free()
        rrows.free()


# ------------------------------------------------------------------------------ 7. which path ran
SO_KERNELS = ("k_so_insert", "k_so_probe", "k_so_emit", "k_so_copy")


def _profiled(so, op, distinct, shape="a"):
    lt, rt = so.left[shape], so.right[shape]
    so.eng.profile(True)
    n = len(_take(so.eng.set_op(lt.rows, rt.rows, op, distinct)))
    prof = so.eng.profile_read()
    so.eng.profile(False)
    return {k: prof[k]["launches"] for k in SO_KERNELS}, prof, n


def test_path_coverage(so):
    launches, prof, n = _profiled(so, "UNION", False)
    assert launches == {"k_so_insert": 0, "k_so_probe": 0, "k_so_emit": 0, "k_so_copy": 2}
    assert prof["k_so_copy"]["algo_bytes"] == n * 2 * 16 and prof["k_so_copy"]["ms"] > 0
    assert all(prof[k]["launches"] == 0 for k in prof if k.startswith("k_ob_"))
    launches, prof, _ = _profiled(so, "UNION", True)               # both sides inserted, both emitted
    assert launches == {"k_so_insert": 2, "k_so_probe": 0, "k_so_emit": 2, "k_so_copy": 0}
    launches, prof, _ = _profiled(so, "INTERSECT", False)
    assert launches == {"k_so_insert": 1, "k_so_probe": 1, "k_so_emit": 1, "k_so_copy": 0}
    assert prof["k_so_insert"]["algo_bytes"] > 0 and prof["k_so_probe"]["ms"] > 0
    launches, _, n = _profiled(so, "MINUS", False)                 # (a)'s difference is empty: nothing to emit
    assert n == 0 and launches == {"k_so_insert": 1, "k_so_probe": 1, "k_so_emit": 0, "k_so_copy": 0}
    launches, _, n = _profiled(so, "MINUS", False, "b")
    assert n > 0 and launches == {"k_so_insert": 1, "k_so_probe": 1, "k_so_emit": 1, "k_so_copy": 0}
