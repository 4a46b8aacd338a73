"""nbg_group_by on the MI355X: GROUP BY with aggregates over device-resident GO rows, judged by the
plain-Python model of tests/support/groupby.py (pinned to the reference's GroupByLimitTest vectors
by tests/test_groupby_model.py) over the CPU oracle's rows — never by the device itself.

The random-parity graph is a seeded RMAT-10 with an int prop w in [-50, 50), a double prop
x = k / 8 with |k| < 2^20 (every double sum is then exact in any order: partial sums stay below
2^43 in units of 1/8, so SUM and AVG compare exactly) and a string tag prop.  STD is compared
relative to the model within n * 2^-52 for a group of n rows: both sides sum the same
non-negative terms in different orders, each within (n - 1) * 2^-53 of the true sum.

`e.w % 2 == 0 AS b` is an INT column of zeros under the reference's row schema (the column takes
the type of the last prop getter, GoExecutor.cpp:707-748, and RowWriter writes a bool into an INT
column as its default), so key `b` is ONE group on both sides; `(bool)(e.w % 2 == 0) AS b2` is the
BOOL column that gives the two-group shape (accumulators in LDS, worst contention).

Two NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
column whose kind differs between OVER types (go_prepare coerces every OVER type's value to the
column's type) and 2^32 groups.

The cells these rows never hold (the int64 and double extremes, NaNs, negative VIDs, TIMESTAMPs,
strings with bytes >= 0x80, values equal to an accumulator's identity) are the subject of
tests/test_gpu_values_groupby.py; the LDS limit, the waves' group counts and probe chains that wrap
are that of tests/test_gpu_rowtable_scale.py."""
import math

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen, rmat
from nebula_amd.engine import nba_engine
from tests.support import golden, groupby, ngql
from tests.support.oracle import Oracle

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("groupby_golden.json")["cases"]
BLOCK = 256            # csrc/ws.h: rows a workgroup walks per step

SEED = 11
E_SCHEMA = [("w", kvgen.INT), ("x", kvgen.DOUBLE), ("f", kvgen.FLOAT)]
T_SCHEMA = [("name", kvgen.STRING)]
PARTS = 5


def _kv():
    src, dst, _ = rmat.rmat_edges(10, seed=SEED)
    rng = np.random.default_rng(SEED)
    w = rng.integers(-50, 50, len(src))
    k = rng.integers(-(1 << 20) + 1, 1 << 20, len(src))
    kb = kvgen.KVBuilder(PARTS)
    now = 1_600_000_000_000_000
    for v in np.unique(np.concatenate([src, dst])).tolist():
        kb.insert_vertex(v, 7, T_SCHEMA, [f"n{v % 23}"], now)
    for s, d, a, b in zip(src.tolist(), dst.tolist(), w.tolist(), k.tolist()):
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, [a, b / 8.0, 0.5], now + 1)
    return src, kb


GO_COLS = ("e.w % 2 == 0 AS b, e.w % 7 AS k7, e._dst AS d, $$.t.name AS s, e.w AS w, e.x AS x, "
           "e.x * 0.0 AS z, (bool)(e.w % 2 == 0) AS b2")
ROOTS = [5760179112236117641, 7046348246087443434]     # two well-connected sources of this seed's graph


@pytest.fixture(scope="module")
def gb():
    """(engine, oracle, GO text, the oracle's rows as the model's input): computed once."""
    src, kb = _kv()
    assert set(ROOTS) <= set(src.tolist())
    eng = Engine(PARTS)
    eng.register_edge(1, "e", E_SCHEMA)
    eng.register_tag(7, "t", T_SCHEMA)
    eng.load_builder(kb)
    orc = Oracle(PARTS)
    orc.register(True, 1, "e", E_SCHEMA)
    orc.register(False, 7, "t", T_SCHEMA)
    orc.load_builder(kb)
    go = f"GO 2 STEPS FROM {ROOTS[0]}, {ROOTS[1]} OVER e YIELD {GO_COLS}"
    s = groupby.Session(orc)
    inp = s.execute(go)
    yield eng, orc, go, inp, s.last_types
    eng.close()
    orc.close()


@pytest.fixture(scope="module")
def nba(nba_data):
    eng = nba_engine(nba_data)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, case):
    """go_device -> group_by -> fetch (and the piped follow-on GO of "Output next") against the
    reference's expected status, column names and rows with their kinds."""
    ok, msg = groupby.run_case(groupby.Session(nba, device=True), case)
    assert ok, msg


# ------------------------------------------------------------------------------ 2. random parity
AGGS = ("COUNT(*) AS n, COUNT_DISTINCT($-.k7), COUNT_DISTINCT($-.s), COUNT_DISTINCT($-.z), "
        "SUM($-.w), SUM($-.x), SUM($-.d), SUM($-.s), AVG($-.w), AVG($-.x), AVG($-.b2), "
        "MAX($-.w), MIN($-.w), MAX($-.x), MIN($-.x), MAX($-.s), MIN($-.s), MAX($-.b2), MAX($-.d), "
        "STD($-.w) AS std_w, STD($-.x) AS std_x, STD($-.d), BIT_AND($-.w), BIT_OR($-.w), BIT_XOR($-.w), "
        "BIT_OR($-.x), SUM(1.5), BIT_XOR(3), 1+1")
STD_COLS = ("std_w", "std_x")
# (GROUP BY list, the key columns also yielded, expected path)
SHAPES = {
    "const": ("abs(5)", []),
    "b": ("$-.b", ["b"]),
    "b2": ("$-.b2", ["b2"]),
    "k7": ("$-.k7", ["k7"]),
    "d": ("$-.d", ["d"]),
    "k7_s": ("$-.k7, $-.s", ["k7", "s"]),
    "d_b2": ("$-.d, $-.b2", ["d", "b2"]),
    "z": ("$-.z", ["z"]),
}


def _compare(dev: ngql.Interim, mod: ngql.Interim, keys):
    assert dev.columns == mod.columns
    kidx = [dev.columns.index(k) for k in keys]
    n_at = dev.columns.index("n")
    std = [dev.columns.index(c) for c in STD_COLS if c in dev.columns]

    def index(rows):
        out = {}
        for r in rows:
            out[tuple(groupby.cell(r[i]) for i in kidx)] = r
        assert len(out) == len(rows)
        return out
    d, m = index(dev.rows), index(mod.rows)
    assert d.keys() == m.keys()
    for key, mr in m.items():
        dr = d[key]
        for c, (a, b) in enumerate(zip(dr, mr)):
            if c in std:
                assert isinstance(a, float) and isinstance(b, float)
                assert abs(a - b) <= mr[n_at] * 2.0 ** -52 * abs(b), (dev.columns[c], a, b)
            else:
                assert groupby.cell(a) == groupby.cell(b), (dev.columns[c], key, a, b)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_parity(gb, shape):
    eng, orc, go, inp, types = gb
    groups, keys = SHAPES[shape]
    ylist = ", ".join([f"$-.{k} AS {k}" for k in keys] + [AGGS])
    gtext = f"GROUP BY {groups} YIELD {ylist}"
    sent = groupby.parse_sentence(gtext)
    mod = groupby.group_model(inp, sent.groups, sent.yields, types)
    want_groups = {"const": 1, "b": 1, "b2": 2, "z": 1}.get(shape)
    if want_groups:
        assert len(mod.rows) == want_groups
    if shape in ("d", "d_b2", "k7_s"):
        assert len(mod.rows) > 64          # the accumulators outgrow the LDS: the global path
    if shape == "z":
        zs = {math.copysign(1.0, r[inp.columns.index("z")]) for r in inp.rows}
        assert zs == {1.0, -1.0}           # the key column holds both zeros
    dev = groupby.Session(eng, device=True).execute(f"{go} | {gtext}")
    _compare(dev, mod, keys)


# ------------------------------------------------------------------------------ 3. the row walk
# Start lists whose one-step results have exactly this many rows (found once with the oracle on
# this seed's graph); 0 rows: a vid the graph does not hold.
WALK_STARTS = {
    0: [123],
    1: [49051440398009915],
    63: [6057085510246920549, 49051440398009915],
    64: [6057085510246920549, 80406610535911986],
    65: [6530207483761974300],
    BLOCK - 1: [5695472266747893962, 3777942062627175311, 16752852696591014],
    BLOCK: [5695472266747893962, 3777942062627175311, 379632324886679683],
    BLOCK + 1: [5695472266747893962, 3777942062627175311, 1293712517449765244],
}


@pytest.mark.parametrize("rows", list(WALK_STARTS))
def test_row_walk_edges(gb, rows):
    eng, orc, _, _, _ = gb
    go = f"GO FROM {', '.join(map(str, WALK_STARTS[rows]))} OVER e YIELD e._dst AS d, e.w AS w"
    assert len(groupby.Session(orc).execute(go).rows) == rows
    for gtext, keys in (("GROUP BY abs(5) YIELD COUNT(*) AS n, SUM($-.w)", []),
                        ("GROUP BY $-.d YIELD $-.d AS d, COUNT(*) AS n, SUM($-.w)", ["d"])):
        mod = groupby.Session(orc).execute(f"{go} | {gtext}")
        dev = groupby.Session(eng, device=True).execute(f"{go} | {gtext}")
        assert len(dev.rows) == len(mod.rows)
        if rows:
            _compare(dev, mod, keys)


def test_row_walk_several_segments(gb):
    eng, orc, go, inp, types = gb
    rows = eng.go_device(ROOTS, [1], 2, b"", [E.edge_prop("e", "_dst").encode(), E.edge_prop("e", "w").encode()])
    try:
        assert eng.lib.nbg_rows_num_segments(rows.h) > 1
        for groups, keys in (([E.Expr(E.K_FUNC, alias="abs", args=[E.const(5)])], []), ([E.input_prop("d")], ["d"])):
            ys = [("", E.input_prop(k).encode(), k) for k in keys] + \
                 [("COUNT", E.const("*").encode(), "n"), ("SUM", E.input_prop("w").encode(), None)]
            out = eng.group_by(rows, ["d", "w"], [g.encode() for g in groups], ys)
            dev = ngql.Interim(keys + ["n", "SUM($-.w)"], out.fetch())
            out.free()
            sent = groupby.parse_sentence("GROUP BY " + ("$-.d" if keys else "abs(5)") + " YIELD " +
                                          ("$-.d AS d, " if keys else "") + "COUNT(*) AS n, SUM($-.w)")
            d_at, w_at = inp.columns.index("d"), inp.columns.index("w")
            sub = ngql.Interim(["d", "w"], [[r[d_at], r[w_at]] for r in inp.rows])
            _compare(dev, groupby.group_model(sub, sent.groups, sent.yields, ["VID", "INT"]), keys)
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 4. limits
def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def _gb(eng, go_yields, groups, yields, starts=(ROOTS[0],)):
    """go_device over `e` with the named yields, then group_by; everything freed."""
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {go_yields}").go()
    rows = eng.go_device(list(starts), [1], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        gs = groupby.parse_sentence(f"GROUP BY {groups} YIELD {yields}")
        out = eng.group_by(rows, [c.name() for c in sent.yields], [c.expr.encode() for c in gs.groups],
                           [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
        try:
            return out.fetch()
        finally:
            out.free()
    finally:
        rows.free()


def test_limit_expression_not_foldable(gb):
    eng = gb[0]
    assert _code(lambda: _gb(eng, "e._dst AS d, e.w AS w", "$-.d", "SUM($-.w + 1)")) == L.E_UNSUPPORTED
    assert _code(lambda: _gb(eng, "e._dst AS d, e.w AS w", "$-.d, rand32(5)", "COUNT(*)")) == L.E_UNSUPPORTED


def test_limit_misaligned_and_float_inputs(gb):
    eng = gb[0]
    # a DOUBLE value in a column typed INT by its last getter: the reference re-reads shifted rows
    assert _code(lambda: _gb(eng, "e._dst AS d, e.x + e.w AS m", "$-.d", "COUNT(*)")) == L.E_UNSUPPORTED
    assert _code(lambda: _gb(eng, "e._dst AS d, e.f AS f", "$-.d", "COUNT(*)")) == L.E_UNSUPPORTED


def test_limit_avg_over_vid(gb):
    eng = gb[0]
    assert _code(lambda: _gb(eng, "e._dst AS d, e.w AS w", "$-.w", "AVG($-.d)")) == L.E_UNSUPPORTED


def test_limit_max_over_strings_outside_the_dictionary(gb):
    eng = gb[0]
    go = '$$.t.name + "!" AS s, e.w AS w'
    assert _code(lambda: _gb(eng, go, "$-.w", "MAX($-.s)")) == L.E_UNSUPPORTED
    assert _code(lambda: _gb(eng, go, "$-.w", "MIN($-.s)")) == L.E_UNSUPPORTED
    # the same column as a key and under COUNT_DISTINCT is served (derived codes compare as strings do)
    got = _gb(eng, go, "$-.s", "$-.s AS s, COUNT(*), COUNT_DISTINCT($-.w)")
    assert got and all(r[0].endswith("!") for r in got)


def test_limit_too_many_columns(gb):
    eng = gb[0]
    many = ", ".join(["COUNT(*)"] * (32 + 1))
    assert _code(lambda: _gb(eng, "e._dst AS d", "$-.d", many)) == L.E_UNSUPPORTED
    keys = ", ".join(["$-.d"] * (32 + 1))
    assert _code(lambda: _gb(eng, "e._dst AS d", keys, "COUNT(*)")) == L.E_UNSUPPORTED
    assert len(_gb(eng, "e._dst AS d", "$-.d", ", ".join(["COUNT(*)"] * 32))) > 0


def test_limit_partitioned_engine():
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
            assert _code(lambda: e.group_by(r, ["d", "w"], [E.input_prop("d").encode()],
                                            [("COUNT", E.const("*").encode(), None)])) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()


# ------------------------------------------------------------------------------ 5. input untouched
def test_input_untouched_and_repeatable(gb):
    eng, orc, go, inp, types = gb
    sent = ngql.Parser(go).go()
    names = [c.name() for c in sent.yields]
    gs = groupby.parse_sentence(
        "GROUP BY $-.k7, $-.s YIELD $-.k7, $-.s, COUNT(*), SUM($-.w), MAX($-.x), MIN($-.s), COUNT_DISTINCT($-.d), "
        "BIT_XOR($-.w)")       # no double SUM / AVG / STD: the result is the same to the last bit
    args = (names, [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    for free_input_first in (True, False):
        rows = eng.go_device(ROOTS, [1], 2, b"", [c.expr.encode() for c in sent.yields])
        before = rows.digest()
        assert before[0] == len(inp.rows)
        a = eng.group_by(rows, *args)
        assert rows.digest() == before
        b = eng.group_by(rows, *args)
        assert rows.digest() == before
        assert a.digest() == b.digest() and a.count == b.count > 1
        if free_input_first:
            rows.free()
            got = a.fetch()
            a.free()
        else:
            got = a.fetch()
            a.free()
            assert rows.digest() == before
            rows.free()
        assert groupby.multiset(got) == groupby.multiset(groupby.group_model(inp, gs.groups, gs.yields, types).rows)
        assert groupby.multiset(b.fetch()) == groupby.multiset(got)
        b.free()


def test_empty_input_runs_no_check(gb):
    """Zero rows: NBG_OK and no rows, whatever the clause names (GroupByExecutor.cpp:184-188)."""
    eng = gb[0]
    assert _gb(eng, "e._dst AS d", "$-.nonexistent", "SUM(*)", starts=(123,)) == []
