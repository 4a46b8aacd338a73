"""nbg_order_by on the MI355X: ORDER BY and LIMIT over device-resident rows, judged by the
plain-Python model of tests/support/orderby.py (pinned to the reference's OrderByTest and
GroupByLimitTest vectors by tests/test_orderby_model.py) over the CPU oracle's rows — never by the
device itself.

The random-parity graph, GO and columns are those of tests/test_gpu_groupby.py (seeded RMAT-10):
k7 (13 values of both signs), d (vids; this graph's are positive, the golden cases' are negative
too), s (dictionary strings), w (100 values of both signs: many ties), x (nearly unique doubles of
both signs), z (x * 0.0: both zeros and nothing else) and b2 (a BOOL).  The GO's 4452 rows lie
in several segments and exceed 8 workgroups' rows, so every kernel of csrc/orderby.hip runs more
than one workgroup and more than one step of its row loop.

Rows that tie under every factor come in unspecified order (the reference's std::sort is not
stable), so orderby.check_window compares what the reference fixes: the sequence of factor keys
exactly, the rows of every key wholly inside the window as a multiset, and the rows of a key the
window's edge cuts as a sub-multiset of the input's.

One NBG_E_UNSUPPORTED case of include/nbg.h has no test because no GO result reaches it: a column
whose kind differs between OVER types (go_prepare coerces every OVER type's value to the column's
type); nor has the 2^32-row result.

The cells these rows never hold (the int64 and double extremes, ints whose middle bytes differ,
NaNs, negative VIDs, TIMESTAMPs, strings with bytes >= 0x80) are the subject of
tests/test_gpu_values_orderby.py; more chunks than workgroups and segments longer than a chunk are
that of tests/test_gpu_rowtable_scale.py."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen, rmat
from nebula_amd.engine import DeviceRows, nba_engine
from tests.support import golden, groupby, ngql, orderby
from tests.support.oracle import Oracle

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("orderby_golden.json")["cases"]
BLOCK = 256            # csrc/ws.h: rows a workgroup walks per step
SELECT_RATIO = 8       # csrc/nbg_internal.h OB_SELECT_RATIO: selection when K * 8 <= rows
SELECT_KERNELS = ("k_ob_hist", "k_ob_pick", "k_ob_compact")

SEED = 11
E_SCHEMA = [("w", kvgen.INT), ("x", kvgen.DOUBLE), ("f", kvgen.FLOAT)]
T_SCHEMA = [("name", kvgen.STRING)]
PARTS = 5
GO_COLS = ("e.w % 7 AS k7, e._dst AS d, $$.t.name AS s, e.w AS w, e.x AS x, e.x * 0.0 AS z, "
           "(bool)(e.w % 2 == 0) AS b2")
ROOTS = [5760179112236117641, 7046348246087443434]     # two well-connected sources of this seed's graph


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


class Fixture:
    pass


@pytest.fixture(scope="module")
def ob():
    """Engine, oracle, the GO text, the oracle's rows (the model's input) and the same GO's rows
    left on the device: computed once and left unchanged."""
    src, kb = _kv()
    assert set(ROOTS) <= set(src.tolist())
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
    s = orderby.Session(f.orc)
    f.inp = s.execute(f.go)
    f.types = s.last_types
    f.n = len(f.inp.rows)
    assert f.n >= 8 * BLOCK
    f.sent = ngql.Parser(f.go).go()
    f.names = [c.name() for c in f.sent.yields]
    f.rows = f.eng.go_device(ROOTS, [1], 2, b"", [c.expr.encode() for c in f.sent.yields])
    assert f.rows.count == f.n
    assert f.eng.lib.nbg_rows_num_segments(f.rows.h) >= 2
    f.digest = f.rows.digest()
    f.fetched = f.rows.fetch()           # the input's own segment order
    yield f
    f.rows.free()
    f.eng.close()
    f.orc.close()


@pytest.fixture(scope="module")
def nba(nba_data):
    eng = nba_engine(nba_data)
    yield eng
    eng.close()


def _order(f, factors, limit=None, rows=None):
    out = f.eng.order_by(rows if rows is not None else f.rows, f.names, factors, limit)
    try:
        return out.fetch()
    finally:
        out.free()


def _cells(rows):
    return [tuple(groupby.cell(v) for v in r) for r in rows]


# ------------------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, case):
    """go_device -> group_by / order_by stages -> one fetch (and the piped follow-on GO) against
    the reference's expected status, column names and rows, in order where it compares them so."""
    ok, msg = orderby.run_case(orderby.Session(nba, device=True), case)
    assert ok, msg


# ------------------------------------------------------------------------------ 2. random parity
SHAPES = {
    "k7": [("k7", False)], "k7_desc": [("k7", True)],
    "d": [("d", False)], "d_desc": [("d", True)],
    "s": [("s", False)], "s_desc": [("s", True)],
    "w": [("w", False)], "w_desc": [("w", True)],
    "x": [("x", False)], "x_desc": [("x", True)],
    "b2": [("b2", False)], "b2_desc": [("b2", True)],
    "z_wdesc_d": [("z", False), ("w", True), ("d", False)],       # the zeros must not decide
    "sdesc_x": [("s", True), ("x", False)],
    "four": [("b2", True), ("k7", False), ("s", True), ("w", False)],
}
ALL_COLUMNS = [("k7", False), ("d", True), ("s", False), ("w", True), ("x", False), ("z", False), ("b2", True)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_parity(ob, shape):
    factors = SHAPES[shape]
    if shape == "z_wdesc_d":
        zs = {str(r[ob.inp.columns.index("z")]) for r in ob.inp.rows}
        assert zs == {"0.0", "-0.0"}          # the column holds both zeros and nothing else
    if shape.startswith("w"):
        assert min(r[3] for r in ob.inp.rows) < 0 < max(r[3] for r in ob.inp.rows)   # both signs
    dev = _order(ob, factors)
    assert len(dev) == ob.n
    orderby.check_window(dev, ob.inp, factors)


def test_all_columns_exact(ob):
    """Every column a factor: the order is fixed up to identical rows, so the lists are equal."""
    dev = _order(ob, ALL_COLUMNS)
    assert _cells(dev) == _cells(orderby.order_model(ob.inp, ALL_COLUMNS).rows)


# ------------------------------------------------------------------------------ 3. LIMIT windows
FIRST = {"x": [("x", False)], "x_desc_w": [("x", True), ("w", False)],
         "b2": [("b2", True), ("w", False)], "b2_only": [("b2", False)]}


def _windows(n):
    cut = n // SELECT_RATIO                     # the largest K the selection takes
    return {"k1": (0, 1), "k10": (0, 10), "inside": (100, 50), "to_rows_minus_1": (7, n - 1 - 7),
            "to_rows": (7, n - 7), "to_rows_plus_1": (7, n + 1 - 7), "offset_is_rows": (n, 5),
            "count_0": (3, 0), "switch_select": (cut - 20, 20), "switch_sort": (cut - 20, 21),
            "saturate": (5, (1 << 63) - 1)}


@pytest.mark.parametrize("first", list(FIRST))
@pytest.mark.parametrize("win", list(_windows(4452)))
def test_limit_windows(ob, first, win):
    off, cnt = _windows(ob.n)[win]
    factors = FIRST[first]
    ob.eng.profile(True)
    dev = _order(ob, factors, (off, cnt))
    prof = ob.eng.profile_read()
    ob.eng.profile(False)
    lo, hi = orderby.window(ob.n, off, cnt)
    assert len(dev) == hi - lo
    orderby.check_window(dev, ob.inp, factors, (off, cnt))
    if hi > lo:                                 # which path ran: the selection iff K * ratio <= rows
        selected = hi * SELECT_RATIO <= ob.n
        assert (prof["k_ob_hist"]["launches"] == 8) == selected
        assert (prof["k_ob_compact"]["launches"] == 1) == selected
        assert prof["k_ob_gather"]["launches"] == 1
    else:
        assert all(prof[k]["launches"] == 0 for k in prof if k.startswith("k_ob_"))
    if win == "switch_select":
        assert hi * SELECT_RATIO <= ob.n < (hi + 1) * SELECT_RATIO


def test_limit_without_order_is_the_inputs_slice(ob):
    n = ob.n
    ob.eng.profile(True)
    for off, cnt in ((0, 1), (5, 3000), (n - 3, 10), (n, 1), (0, n), (0, n + 5), (1234, 0), (BLOCK - 1, 2 * BLOCK + 3)):
        assert _cells(_order(ob, [], (off, cnt))) == _cells(ob.fetched[off:off + cnt])
    prof = ob.eng.profile_read()
    ob.eng.profile(False)
    assert prof["k_ob_copy"]["launches"] == 6 and prof["k_ob_copy"]["algo_bytes"] > 0
    assert all(prof[k]["launches"] == 0 for k in SELECT_KERNELS + ("k_ob_image", "ob_radix_sort", "k_ob_gather"))


def test_path_coverage(ob):
    """nbg_profile_read tells the paths apart: the selection kernels run for ORDER BY x | LIMIT 10
    and do not run without a LIMIT."""
    ob.eng.profile(True)
    _order(ob, [("x", False)], (0, 10))
    prof = ob.eng.profile_read()
    assert prof["k_ob_hist"]["launches"] == 8 and prof["k_ob_pick"]["launches"] == 8
    assert prof["k_ob_compact"]["launches"] == 1 and prof["k_ob_iota"]["launches"] == 0
    assert prof["k_ob_hist"]["algo_bytes"] == 8 * 8 * ob.n and prof["k_ob_hist"]["ms"] > 0
    assert prof["ob_radix_sort"]["launches"] == 1 and prof["k_ob_image"]["launches"] == 1
    ob.eng.profile(True)                        # (enabling again resets the counters)
    _order(ob, [("x", False), ("w", True)])
    prof = ob.eng.profile_read()
    ob.eng.profile(False)
    assert all(prof[k]["launches"] == 0 for k in SELECT_KERNELS)
    assert prof["k_ob_iota"]["launches"] == 1 and prof["ob_radix_sort"]["launches"] == 2
    assert prof["k_ob_gather"]["launches"] == 1


# ------------------------------------------------------------------------------ 4. chaining
def test_pipeline_stays_on_the_device(ob):
    text = f"{ob.go} | GROUP BY $-.k7 YIELD $-.k7 AS k, SUM($-.w) AS s | ORDER BY $-.s DESC, $-.k | LIMIT 3"
    mod = orderby.Session(ob.orc).execute(text)
    ses = orderby.Session(ob.eng, device=True)
    dev = ses.execute(text)
    assert ses.device_calls == ["group_by", "order_by"]        # ORDER BY | LIMIT fused into one call
    assert dev.columns == mod.columns == ["k", "s"]
    assert len(mod.rows) == 3 and _cells(dev.rows) == _cells(mod.rows)   # (k is unique per group)
    # the three clauses as three calls give the same rows
    text3 = f"{ob.go} | ORDER BY $-.w | GROUP BY $-.k7 YIELD $-.k7 AS k, SUM($-.w) AS s | LIMIT 100 | ORDER BY $-.s DESC, $-.k"
    ses = orderby.Session(ob.eng, device=True)
    dev3 = ses.execute(text3)
    assert ses.device_calls == ["order_by", "group_by", "order_by", "order_by"]
    mod3 = orderby.Session(ob.orc).execute(text3)
    assert len(mod3.rows) > 3 and _cells(dev3.rows) == _cells(mod3.rows) and _cells(dev3.rows)[:3] == _cells(mod.rows)


def test_output_feeds_group_by_and_order_by(ob):
    gs = groupby.parse_sentence("GROUP BY $-.k7, $-.s YIELD $-.k7, $-.s, COUNT(*), SUM($-.w), MAX($-.x), MIN($-.d)")
    args = (ob.names, [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    direct = ob.eng.group_by(ob.rows, *args)
    ordered = ob.eng.order_by(ob.rows, ob.names, [("x", True)])
    assert ordered.count == ob.n and ob.eng.lib.nbg_rows_num_segments(ordered.h) == 1
    via = ob.eng.group_by(ordered, *args)
    want = groupby.multiset(groupby.group_model(ob.inp, gs.groups, gs.yields, ob.types).rows)
    assert groupby.multiset(via.fetch()) == groupby.multiset(direct.fetch()) == want
    # the output of order_by is an input of order_by: LIMIT only keeps its order
    ordered_rows = ordered.fetch()
    assert _cells(_order(ob, [], (10, 300), rows=ordered)) == _cells(ordered_rows[10:310])
    again = _order(ob, [("w", False), ("d", False)], (0, 40), rows=ordered)
    orderby.check_window(again, ob.inp, [("w", False), ("d", False)], (0, 40))
    for r in (direct, via, ordered):
        r.free()
    assert ob.rows.digest() == ob.digest


def test_input_unchanged(ob):
    assert ob.rows.digest() == ob.digest
    assert _cells(ob.rows.fetch()) == _cells(ob.fetched)
    assert groupby.multiset(ob.fetched) == groupby.multiset(ob.inp.rows)


# ------------------------------------------------------------------------------ 5. statuses and limits
def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def _go_order(eng, go_yields, factors, limit=None, starts=(ROOTS[0],)):
    """go_device over `e` with the named yields, then order_by; everything freed."""
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {go_yields}").go()
    rows = eng.go_device(list(starts), [1], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        out = eng.order_by(rows, [c.name() for c in sent.yields], factors, limit)
        try:
            return out.fetch()
        finally:
            out.free()
    finally:
        rows.free()


def test_negative_limit_is_a_syntax_error(ob):
    assert _code(lambda: _order(ob, [("x", False)], (-1, 2))) == L.E_SYNTAX_ERROR
    assert _code(lambda: _order(ob, [], (1, -2))) == L.E_SYNTAX_ERROR
    # checked first, even for an empty input and before the factor is looked up
    assert _code(lambda: _go_order(ob.eng, "e._dst AS d", [("nope", False)], (-1, 2), starts=(123,))) == L.E_SYNTAX_ERROR
    assert _code(lambda: _order(ob, [("nope", False)], (0, -1))) == L.E_SYNTAX_ERROR


def test_unknown_factor(ob):
    assert _code(lambda: _order(ob, [("x", False), ("nope", True)])) == L.E_EXECUTION_ERROR
    assert _code(lambda: _order(ob, [("nope", False)], (0, 0))) == L.E_EXECUTION_ERROR   # before the LIMIT
    # zero input rows: no factor check, no rows (OrderByExecutor.cpp:137-139)
    assert _go_order(ob.eng, "e._dst AS d, e.w AS w", [("nope", False)], starts=(123,)) == []
    assert _go_order(ob.eng, "e._dst AS d, e.w AS w", [("nope", False)], (0, 5), starts=(123,)) == []


def test_duplicate_column_names_first_match(ob):
    got = _go_order(ob.eng, "e.w AS a, e._dst AS a", [("a", False)])
    assert len(got) > 1 and [r[0] for r in got] == sorted(r[0] for r in got)


def test_host_only_rows_rejected(ob):
    req, keep = ob.eng._go_request([ROOTS[0]], [1], 1, b"", [E.edge_prop("e", "w").encode()], False, False)
    rows = C.c_void_p()
    assert ob.eng.lib.nbg_go(ob.eng.h, C.byref(req), C.byref(rows)) == L.OK     # rows copied to the host
    host = DeviceRows(ob.eng, rows)
    try:
        assert _code(lambda: ob.eng.order_by(host, ["w"], [("w", False)])) == L.E_INVALID_ARGUMENT
    finally:
        host.free()


def test_limit_misaligned_and_float_inputs(ob):
    # a DOUBLE value in a column typed INT by its last getter: the reference re-reads shifted rows
    assert _code(lambda: _go_order(ob.eng, "e._dst AS d, e.x + e.w AS m", [("d", False)])) == L.E_UNSUPPORTED
    assert _code(lambda: _go_order(ob.eng, "e._dst AS d, e.f AS f", [("d", False)])) == L.E_UNSUPPORTED
    assert _code(lambda: _go_order(ob.eng, "e._dst AS d, e.f AS f", [], (0, 3))) == L.E_UNSUPPORTED


def test_limit_string_factor_outside_the_dictionary(ob):
    go = '$$.t.name + "!" AS s, e.w AS w'
    assert _code(lambda: _go_order(ob.eng, go, [("s", False)])) == L.E_UNSUPPORTED
    assert _code(lambda: _go_order(ob.eng, go, [("w", False), ("s", True)], (0, 3))) == L.E_UNSUPPORTED
    # the column is carried over when it is no factor (the result keeps the derived-string table)
    got = _go_order(ob.eng, go, [("w", True)], (0, 5))
    assert len(got) == 5 and all(r[0].endswith("!") for r in got)
    assert [r[1] for r in got] == sorted((r[1] for r in got), reverse=True)


def test_limit_too_many_factors(ob):
    assert _code(lambda: _order(ob, [("w", False)] * 33)) == L.E_UNSUPPORTED
    dev = _order(ob, [("w", False)] * 32, (0, 600))
    orderby.check_window(dev, ob.inp, [("w", False)], (0, 600))


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
            assert _code(lambda: e.order_by(r, ["d", "w"], [("w", False)], (0, 3))) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()
