"""nbg_fetch_edges on the MI355X: piped FETCH PROP ON <edge> over device-resident rows, judged by the
plain-Python model of tests/support/fetchedges.py (pinned to the reference's FetchEdgesTest vectors
by tests/test_fetch_edges_model.py) — never by the device itself.

The graph, parts and roots are those of tests/test_gpu_orderby.py (seeded RMAT-10, 5 parts), with
the same E_SCHEMA on type `e`, whose ranks are all 0 (its device rank array is absent).  This
file's own KV builder adds:
  * a second type `r` (INT i, DOUBLE x, BOOL b, TIMESTAMP ts, STRING s) whose edges are parallel
    edges between the same endpoints with ranks from {-(2^63)+1, -1, 0, 1, 255, 256, 2^40}: 255
    against 256 and the negative values order differently in the key's byte order than in signed
    order;
  * edges of both types to negative-vid destinations, so the same holds for dst;
  * a few `r` edges written twice, the newer version with another value (the newer comes back),
    once with the older version loaded after the newer;
  * a vertex (R_ONLY) with out-edges of `r` only, and a hub with 320 out-edges of `e`, more than
    BLOCK, so the in-row search has depth.
The model's edge tables hold the latest version per key; its input is the GO's rows in their
fetch order, so its output is the expected result row for row: nbg_fetch_edges keeps the input's
order.

Three NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
key column whose kind differs between OVER types, an edge type without a device CSR, and the
input of 2^32 rows."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen, rmat
from nebula_amd.engine import DeviceRows, nba_engine
from tests.support import fetchedges, fetchpipe, golden, groupby, ngql, orderby, setops, yieldpipe
from tests.support.fetchedges import EdgeTable
from tests.support.fetchpipe import TagTable
from tests.test_gpu_orderby import E_SCHEMA, PARTS, ROOTS, SEED, T_SCHEMA

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("fetch_edges_golden.json")["cases"]
BLOCK = 256                           # csrc/ws.h: rows a workgroup walks per step
OB_CHUNK = 2048                       # csrc/nbg_internal.h
FE_KERNELS = ("k_fe_resolve", "k_fe_emit")
EMPTY_SRC = 123                       # no such vertex: a GO from it has no rows
R_ONLY, HUB = 77, 99                  # a vertex with out-edges of r only; a source of 320 e edges
RANKS = [-(1 << 63) + 1, -1, 0, 1, 255, 256, 1 << 40]
E_TYPES = [("w", groupby.INT), ("x", groupby.DOUBLE), ("f", groupby.DOUBLE)]
R_SCHEMA = [("i", kvgen.INT), ("x", kvgen.DOUBLE), ("b", kvgen.BOOL), ("ts", kvgen.TIMESTAMP), ("s", kvgen.STRING)]
R_TYPES = [("i", groupby.INT), ("x", groupby.DOUBLE), ("b", groupby.BOOL), ("ts", groupby.TIMESTAMP), ("s", groupby.STRING)]
NOW = 1_600_000_000_000_000
GO_E = "e._src AS s, e._dst AS d, e._rank AS k, e.w AS w"
GO_R = "r._src AS s, r._dst AS d, r._rank AS k, r.i AS w"


def _r_row(s, d, k, gen=0):
    n = (s + 3 * d + 7 * (k % 1000) + gen) % 1009
    x = (n % 17 - 8) * 0.25
    if x == 0.0 and n % 2:
        x = -0.0
    return [n - 500 + gen * 100_000, x, n % 2 == 0, 1_500_000_000 + n, f"r{n % 11}"]


def _kv():
    """tests/test_gpu_orderby.py's graph (each (src, dst) once) plus what the module docstring
    lists; returns (builder, {(s, d, 0): e row}, {(s, d, k): r row}, the graph's vertices)."""
    src, dst, _ = rmat.rmat_edges(10, seed=SEED)
    rng = np.random.default_rng(SEED)
    w = rng.integers(-50, 50, len(src))
    k = rng.integers(-(1 << 20) + 1, 1 << 20, len(src))
    kb = kvgen.KVBuilder(PARTS)
    verts = np.unique(np.concatenate([src, dst])).tolist()
    for v in verts:
        kb.insert_vertex(v, 7, T_SCHEMA, [f"n{v % 23}"], NOW)
    etab, rtab = {}, {}

    def add_e(s, d, a, b):
        if (s, d, 0) not in etab:
            etab[(s, d, 0)] = [a, b / 8.0, 0.5]
            kb.insert_edge(s, d, 1, 0, E_SCHEMA, etab[(s, d, 0)], NOW + 1)
    for s, d, a, b in zip(src.tolist(), dst.tolist(), w.tolist(), k.tolist()):
        add_e(s, d, a, b)
    for root in ROOTS:
        outs = sorted({d for (s, d, _) in etab if s == root})[:40]
        for n, d in enumerate(outs):
            for rk in RANKS:                                      # parallel edges, every rank
                rtab[(root, d, rk)] = _r_row(root, d, rk)
            if n < 12:                                            # negative destinations, three ranks
                add_e(root, -d, n, n)
                for rk in (255, 256, -1):
                    rtab[(root, -d, rk)] = _r_row(root, -d, rk)
    for d in (ROOTS[0], -5, 6):
        rtab[(R_ONLY, d, 0)] = _r_row(R_ONLY, d, 0)
    for key, row in rtab.items():
        kb.insert_edge(key[0], key[1], 2, key[2], R_SCHEMA, row, NOW + 1)
    # newer versions with another value: the newer comes back, whichever was loaded last
    keys = [key for key in rtab if key[0] == ROOTS[0]][3:9]
    for n, key in enumerate(keys):
        newer = _r_row(*key, gen=1)
        if n % 2:
            kb.insert_edge(key[0], key[1], 2, key[2], R_SCHEMA, newer, NOW + 9)
        else:                                                     # an older version loaded after
            kb.insert_edge(key[0], key[1], 2, key[2], R_SCHEMA, _r_row(*key, gen=2), NOW - 5)
            newer = rtab[key]
        rtab[key] = newer
    hub_dsts = [v if n % 3 else -v for n, v in enumerate(verts[:320])]
    for n, d in enumerate(hub_dsts):
        add_e(HUB, d, n - 160, n)
    return kb, etab, rtab, verts


class Fixture:
    pass


def _go_rows(f, text, roots, etype, steps):
    sent = ngql.Parser(text).go()
    rows = f.eng.go_device(roots, [etype], steps, b"", [c.expr.encode() for c in sent.yields])
    inp = ngql.Interim([c.name() for c in sent.yields], rows.fetch())
    return sent, rows, inp, groupby.go_column_types(sent, inp.rows)


@pytest.fixture(scope="module")
def ff():
    """Engine, the model's edge tables, the two GOs' rows on the device and, fetched, as the model's
    input: computed once and left unchanged.  The conditions the tests rely on are asserted on the
    CPU before any FETCH call."""
    kb, etab, rtab, verts = _kv()
    assert not {EMPTY_SRC, R_ONLY, HUB} & set(verts)
    deg = {}
    for (s, d, _) in etab:
        deg.setdefault(s, []).append(d)
    assert max(len(v) for v in deg.values()) >= 300                           # the in-row search has depth
    assert any(v < 0 for v in deg[HUB]) and any(v > 0 for v in deg[HUB])      # a row with dsts of both signs
    r_rows = {}
    for (s, d, rk) in rtab:
        r_rows.setdefault(s, []).append((rk, d))
    assert any({255, 256} <= {rk for rk, _ in v} for v in r_rows.values())    # a row holding rank 255 and rank 256
    assert any(any(d < 0 for _, d in v) and any(d > 0 for _, d in v) for v in r_rows.values())
    assert not any(s == R_ONLY for (s, _, _) in etab) and len(r_rows[R_ONLY]) == 3          # out-edges of r only
    f = Fixture()
    f.verts, f.etab, f.rtab = verts, etab, rtab
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_edge(2, "r", R_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"e": EdgeTable(1, E_TYPES, etab), "r": EdgeTable(2, R_TYPES, rtab),
                "t": TagTable(7, [("name", groupby.STRING)], {v: [f"n{v % 23}"] for v in verts})}
    f.go = f"GO 2 STEPS FROM {ROOTS[0]}, {ROOTS[1]} OVER e YIELD {GO_E}"
    f.sent, f.rows, f.inp, f.types = _go_rows(f, f.go, ROOTS, 1, 2)
    f.names = f.inp.columns
    assert f.eng.lib.nbg_rows_num_segments(f.rows.h) >= 2 and f.rows.count >= 2200
    f.digest = f.rows.digest()
    f.go_r = f"GO FROM {ROOTS[0]}, {ROOTS[1]} OVER r YIELD {GO_R}"
    _, f.rrows, f.rinp, f.rtypes = _go_rows(f, f.go_r, ROOTS, 2, 1)
    # (the type's first record carries rank -(2^63)+1: the loader keeps the rank of a first record too)
    assert len(f.rinp.rows) == sum(len(r_rows[r]) for r in ROOTS) >= 400
    back = sum((r[1], r[0], 0) in etab for r in f.inp.rows)
    assert 0 < back < len(f.inp.rows)                                         # reversed keys: hits and misses
    yield f
    f.rows.free()
    f.rrows.free()
    f.eng.close()


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


def _st(text):
    return fetchedges.parse_sentence(text)


def _fetch(f, rows, names, text):
    """Engine.fetch_edges for a `FETCH PROP ON ...` text: over `rows`, or over its key list."""
    st = _st(text)
    etype = f.tables[st.label].edge_type if isinstance(f.tables.get(st.label), EdgeTable) else 999
    ys = [c.expr.encode() for c in st.yields] if st.yields is not None else []
    if st.ref is None:
        return f.eng.fetch_edges(st.keys, [], "", "", None, etype, ys, st.distinct)
    return f.eng.fetch_edges(rows, names, st.ref[1], st.ref[2], st.ref[3], etype, ys, st.distinct)


def _model(f, inp, text, types=None):
    return fetchedges.fetch_edges_model(_st(text), f.tables, inp, types)


def _yield(eng, rows, names, text):
    st = yieldpipe.parse_sentence(text)
    return eng.yield_rows(rows, names, [c.expr.encode() for c in st.yields], st.where.encode() if st.where is not None else b"")


def _check(f, rows, names, inp, text, types=None):
    """The device's rows are the model's, row for row, with the model's kinds; returns them."""
    want, _ = _model(f, inp, text, types)
    out = _fetch(f, rows, names, text)
    assert out.count == len(want.rows)
    assert out.count == 0 or f.eng.lib.nbg_rows_num_segments(out.h) == 1
    assert f.eng.lib.nbg_rows_num_cols(out.h) == len(want.columns)
    if want.rows:
        kind = {groupby.INT: L.V_INT, groupby.DOUBLE: L.V_DOUBLE, groupby.BOOL: L.V_BOOL, groupby.STRING: L.V_STRING}
        assert [f.eng.lib.nbg_rows_col_kind(out.h, c) for c in range(len(want.columns))] == \
            [kind[groupby.type_of_value(v)] for v in want.rows[0]]
    dev = _take(out)
    assert _bits(dev) == _bits(want.rows)
    return dev


# ------------------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, nba_data, case):
    """Every GO with go_device, the FETCH with nbg_fetch_edges, one fetch at the end: the
    reference's status, column names and rows.  A FETCH behind a GO gets the GO's device handle as
    `in` (path "rows"), a key list goes through in == NULL (path "list")."""
    tables = {**fetchpipe.nba_tables(nba_data, kvgen.NBA_TAGS), **fetchedges.nba_edge_tables(nba_data, kvgen.NBA_EDGES)}
    ses = fetchedges.Session(nba, tables, device=True)
    ok, msg = fetchedges.run_case(ses, case)
    assert ok, msg
    assert not ses.fallbacks
    if case["status"] == "SUCCEEDED":
        assert ses.edge_calls == 1 and ses.fetch_calls == 0
        assert ses.edge_paths == (["rows"] if "GO FROM" in case["query"] else ["list"])


# ------------------------------------------------------------------------------ 2. identity, hits and misses
def test_identity_over_e(ff):
    """Every row of the GO is an edge: the fetched e.w is the input's w column, in order."""
    dev = _check(ff, ff.rows, ff.names, ff.inp, "FETCH PROP ON e $-.s->$-.d@$-.k YIELD e.w", ff.types)
    assert [r[0] for r in dev] == [r[3] for r in ff.inp.rows]
    assert ff.rows.digest() == ff.digest                        # `in` stays unchanged


def test_identity_over_r_with_ranks(ff):
    dev = _check(ff, ff.rrows, ff.rinp.columns, ff.rinp, "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.i, r._rank", ff.rtypes)
    assert [r[0] for r in dev] == [r[3] for r in ff.rinp.rows] and [r[1] for r in dev] == [r[2] for r in ff.rinp.rows]
    assert {r[1] for r in dev} == set(RANKS)
    # the newer version answers: the rewritten keys carry generation 1's value
    assert sum(r[0] >= 50_000 for r in dev) == 3 and not any(r[0] >= 150_000 for r in dev)
    # without `@' every key has rank 0: only the rank-0 parallel edge of each pair is found
    dev = _check(ff, ff.rrows, ff.rinp.columns, ff.rinp, "FETCH PROP ON r $-.s->$-.d YIELD r._rank, r.i", ff.rtypes)
    assert dev and {r[0] for r in dev} == {0} and len(dev) == sum((r[0], r[1], 0) in ff.rtab for r in ff.rinp.rows)


def test_reversed_keys_hit_and_miss(ff):
    dev = _check(ff, ff.rows, ff.names, ff.inp, "FETCH PROP ON e $-.d->$-.s YIELD e._src, e._dst, e.w, e.x", ff.types)
    assert 0 < len(dev) < len(ff.inp.rows)
    # the r rows looked up under e, whose rank array is absent: the rows of rank 0 only
    dev = _check(ff, ff.rrows, ff.rinp.columns, ff.rinp, "FETCH PROP ON e $-.s->$-.d@$-.k YIELD e.w, e._dst", ff.rtypes)
    assert len(dev) == sum(r[2] == 0 for r in ff.rinp.rows) > 0
    dev = _check(ff, ff.rrows, ff.rinp.columns, ff.rinp, "FETCH PROP ON e $-.s->$-.d YIELD e.w", ff.rtypes)
    assert len(dev) == len(ff.rinp.rows)                        # every (root, d) pair is an e edge


# ------------------------------------------------------------------------------ 3. literal keys
def test_literal_keys(ff):
    r0 = ROOTS[0]
    d_pos = sorted(d for (s, d, k) in ff.rtab if s == r0 and k == 255 and d > 0)[0]
    d_neg = sorted(d for (s, d, k) in ff.rtab if s == r0 and k == 255 and d < 0)[0]
    e_only = next(key for key in ff.etab if (key[0], key[1], 0) not in ff.rtab and key[0] not in (HUB,))
    leaf = next(v for v in ff.verts if not any(s == v for (s, _, _) in ff.rtab) and any(s == v for (s, _, _) in ff.etab))
    keys = [(r0, d_pos, 255), (r0, d_pos, 256), (r0, d_neg, 255), (r0, d_neg, -1), (r0, d_pos, RANKS[0]), (r0, d_pos, 1 << 40),
            (EMPTY_SRC, d_pos, 0),                               # a src that is no vertex
            (leaf, d_pos, 0),                                    # a vertex with no out-edge of the type
            (e_only[0], e_only[1], 0),                           # an edge that exists under the other type only
            (r0, d_pos, 2), (r0, d_pos, 254), (r0, d_neg, 0),    # the right endpoints with the wrong rank
            (r0, d_pos, 255), (r0, d_pos, 255),                  # duplicates are kept
            (R_ONLY, -5, 0), (R_ONLY, 6, 0), (R_ONLY, 5, 0), ((1 << 63) - 1, 0, 0), (-(1 << 63) + 1, 0, 0)]
    text = "FETCH PROP ON r " + ", ".join(f"{s}->{d}@{k}" for s, d, k in keys) + " YIELD r.i, r._src, r._dst, r._rank, r.s"
    dev = _check(ff, None, None, None, text)
    assert len(dev) == 10 and [tuple(r[1:4]) for r in dev[:6]] == keys[:6]
    # type e has no rank array: a rank other than 0 is a miss, rank 0 and no rank are the edge
    s, d, _ = e_only
    dev = _check(ff, None, None, None, f"FETCH PROP ON e {s}->{d}@1, {s}->{d}@0, {s}->{d}@-1, {s}->{d}, {R_ONLY}->6 YIELD e.w, e._rank")
    assert dev == [[ff.etab[e_only][0], 0]] * 2
    # every out-edge of the hub (320, dsts of both signs), in key order and reversed, a miss beside each
    hub = [x for (s, d, _) in ff.etab if s == HUB for x in ((s, d, 0), (s, d + 1, 0))]
    for lst in (hub, hub[::-1]):
        dev = _check(ff, None, None, None, "FETCH PROP ON e " + ", ".join(f"{s}->{d}" for s, d, _ in lst) + " YIELD e._dst, e.w")
        assert len(dev) >= 320
    # the empty list (the binding's: the grammar has none) and an all-miss list
    out = ff.eng.fetch_edges([], [], "", "", None, 2, [E.edge_prop("r", "i").encode(), E.edge_prop("r", "s").encode()])
    assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == 2 and _take(out) == []
    out = _fetch(ff, None, None, "FETCH PROP ON r 5->6, 6->7@3 YIELD r.i, r.s, r.x")
    assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == 3 and _take(out) == []


# ------------------------------------------------------------------------------ 4. input shapes
@pytest.mark.parametrize("window", [(0, 1), (0, BLOCK + 1), (0, 2048), (0, 2049), (37, 2100)])
def test_input_shapes(ff, window):
    """1 row, the chunk boundary, and a window whose first chunk starts inside a segment."""
    rows = ff.eng.order_by(ff.rows, ff.names, [], window)
    try:
        inp = ngql.Interim(ff.names, rows.fetch())
        assert len(inp.rows) == window[1] and inp.rows[0] == ff.inp.rows[window[0]]
        _check(ff, rows, ff.names, inp, "FETCH PROP ON e $-.s->$-.d YIELD e.w, e.x * 2 AS x2, e._dst", ff.types)
        _check(ff, rows, ff.names, inp, "FETCH PROP ON e $-.d->$-.s YIELD e.w", ff.types)
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 5. expressions, result schema
TEXTS = {
    "bare": "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.i, r.x, r.b, r.ts, r.s",
    "keys": "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r._src, r._dst AS d, r._rank, r._type, r.i",
    "exprs": "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.i * 2 + 1 AS a, (double)r.i / 3 AS q, (int)r.x AS xi, r.x < 0.0 AS neg, "
             "r.ts - 1500000000 AS dt, !r.b AS nb, r.s == \"r3\" AS is3, (timestamp)r.i AS t, r._rank % 7 AS m, "
             "r._dst + r._src AS sum, -r.x AS nx, r.b XOR (r.i > 0) AS lx",
    "constants": 'FETCH PROP ON r $-.s->$-.d@$-.k YIELD 7 AS c, r.i, "no such name" AS s2, 2.5 AS h, true AS b, "r3" AS known',
    "no_yield": "FETCH PROP ON r $-.s->$-.d@$-.k",
    "variable": "FETCH PROP ON r $v.s->$v.d@$v.k YIELD r.s, r.i + 1 AS i1",
    "float_inside": "FETCH PROP ON e $-.s->$-.d YIELD e.f * 2 AS f2, e.w, (double)e.f AS fd",
}


@pytest.mark.parametrize("name", list(TEXTS))
def test_expressions_equal_the_model(ff, name):
    over_e = name == "float_inside"
    rows, inp, types = (ff.rows, ff.inp, ff.types) if over_e else (ff.rrows, ff.rinp, ff.rtypes)
    dev = _check(ff, rows, inp.columns, inp, TEXTS[name], types)
    assert len(dev) == len(inp.rows)


def test_col_types(ff):
    """The result's col_types, seen through what RowReader::getVid accepts as a key column of a
    second FETCH: a bare TIMESTAMP prop and a root (timestamp) cast are refused, arithmetic over
    the prop and the key pseudo-props (`_dst', `_rank': the value's natural type, INT) are taken."""
    text = ("FETCH PROP ON r $-.s->$-.d@$-.k YIELD r._src AS s, r._dst AS d, r._rank AS k, r.ts AS ts, r.ts + 0 AS ti, "
            "(timestamp)r.i AS tc, r.i AS i")
    mid, mtypes = _model(ff, ff.rinp, text, ff.rtypes)
    assert mtypes == [None, None, None, groupby.TIMESTAMP, None, groupby.TIMESTAMP, groupby.INT]
    out = _fetch(ff, ff.rrows, ff.rinp.columns, text)
    try:
        for col, ok in (("k", True), ("ts", False), ("ti", True), ("tc", False), ("i", True)):
            again = f"FETCH PROP ON r $-.s->$-.d@$-.{col} YIELD r.i"
            if ok:
                _check(ff, out, mid.columns, mid, again, [t or groupby.INT for t in mtypes])
            else:
                assert _code(lambda: _fetch(ff, out, mid.columns, again)) == L.E_EXECUTION_ERROR
        _check(ff, out, mid.columns, mid, "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.i, r._rank", [t or groupby.INT for t in mtypes])
    finally:
        out.free()


@pytest.mark.parametrize("ys", ["r._dst", "r.x", "r.s, r.b", "r.i % 3 AS m, r.x * 0.0 AS z", "7 AS k, r._rank"])
def test_distinct(ff, ys):
    text = f"FETCH PROP ON r $-.s->$-.d@$-.k YIELD DISTINCT {ys}"
    want, _ = _model(ff, ff.rinp, text, ff.rtypes)
    dev = _take(_fetch(ff, ff.rrows, ff.rinp.columns, text))
    assert len(dev) == len(want.rows) < len(ff.rinp.rows) and groupby.multiset(dev) == groupby.multiset(want.rows)
    if ys == "r.x":
        xs = [v[1] for v in ff.rtab.values()]
        assert any(str(x) == "0.0" for x in xs) and any(str(x) == "-0.0" for x in xs)   # both zeros
        assert sum(r[0] == 0.0 for r in dev) == 1


def test_profile_entries(ff):
    n = len(ff.inp.rows)
    found = sum((r[1], r[0], 0) in ff.etab for r in ff.inp.rows)
    ff.eng.profile(True)
    _take(_fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.d->$-.s@$-.k YIELD e.w"))
    prof = ff.eng.profile_read()
    ff.eng.profile(False)
    assert [prof[k]["launches"] for k in FE_KERNELS] == [1, 1]
    assert prof["k_fe_resolve"]["algo_bytes"] == n * (3 * 8 + 4 + 1) and prof["k_fe_resolve"]["ms"] > 0
    assert prof["k_fe_emit"]["algo_bytes"] == n + found * (4 + 8 * 2) and prof["k_fe_emit"]["ms"] > 0


# ------------------------------------------------------------------------------ 6. chaining
def test_go_order_by_fetch_limit_is_exact(ff):
    """`GO | ORDER BY | FETCH edges | ORDER BY | LIMIT`: every stage on the device, the rows the
    model's, in order."""
    fetch = "FETCH PROP ON e $-.d->$-.s YIELD e._dst AS back, e.w AS w, e.x AS x"
    ses = fetchedges.Session(ff.eng, ff.tables, device=True)
    dev = ses.execute(f"{ff.go} | ORDER BY $-.w DESC, $-.d, $-.s | {fetch} | LIMIT 9")
    assert ses.edge_calls == 1 and ses.edge_paths == ["rows"] and not ses.fallbacks
    ordered = orderby.order_model(ff.inp, [("w", True), ("d", False), ("s", False)])
    want, _ = _model(ff, ordered, fetch, ff.types)
    assert dev.columns == ["back", "w", "x"] and len(dev.rows) == 9 and _bits(dev.rows) == _bits(want.rows[:9])
    ses = fetchedges.Session(ff.eng, ff.tables, device=True)
    dev = ses.execute(f"$v = {ff.go_r}; FETCH PROP ON r $v.s->$v.d@$v.k YIELD r.ts AS ts, r.i AS i | ORDER BY $-.ts, $-.i | LIMIT 5")
    want, _ = _model(ff, ff.rinp, "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.ts AS ts, r.i AS i", ff.rtypes)
    assert ses.edge_calls == 1 and not ses.fallbacks
    assert _bits(dev.rows) == _bits(sorted(want.rows, key=lambda r: (r[0], r[1]))[:5])


def test_output_feeds_every_stage(ff):
    text = "FETCH PROP ON r $-.s->$-.d@$-.k YIELD r.i % 5 AS g, r.ts AS ts, r.x AS x, r._dst AS id, r._src AS s"
    mid, mtypes = _model(ff, ff.rinp, text, ff.rtypes)
    out = _fetch(ff, ff.rrows, ff.rinp.columns, text)
    names = mid.columns
    try:
        gs = groupby.parse_sentence("GROUP BY $-.g YIELD $-.g, COUNT(*), SUM($-.g)")
        got = _take(ff.eng.group_by(out, names, [c.expr.encode() for c in gs.groups],
                                    [(c.fun, c.expr.encode(), c.alias) for c in gs.yields]))
        assert groupby.multiset(got) == groupby.multiset(groupby.group_model(mid, gs.groups, gs.yields).rows)
        ytext = "YIELD $-.ts + 1 AS t1, $-.g WHERE $-.x < 0.0"
        again = _take(_yield(ff.eng, out, names, ytext))
        assert again and _bits(again) == _bits(yieldpipe.yield_model(mid, yieldpipe.parse_sentence(ytext))[0].rows)
        # the edge FETCH's `_dst' column feeds the vertex FETCH (negative dsts carry no tag)
        vst = fetchpipe.parse_sentence("FETCH PROP ON t $-.id YIELD t.name")
        tags = _take(ff.eng.fetch_vertices(out, names, "id", 7, [c.expr.encode() for c in vst.yields]))
        want, _ = fetchpipe.fetch_model(vst, ff.tables, mid, [t or groupby.INT for t in mtypes])
        assert 0 < len(tags) < len(mid.rows) and _bits(tags) == _bits(want.rows)
        # ... and an edge FETCH again: its own output's (s, id) under type e
        _check(ff, out, names, mid, "FETCH PROP ON e $-.s->$-.id YIELD e.w, e._dst", [t or groupby.INT for t in mtypes])
        # a set operator over two edge FETCHes
        other_text = "FETCH PROP ON e $-.d->$-.s YIELD e.w % 5 AS g, e.w + 1500000000 AS ts, e.x AS x, e._dst AS id, e._src AS s"
        other_want, _ = _model(ff, ff.inp, other_text, ff.types)
        other = _fetch(ff, ff.rows, ff.names, other_text)
        try:
            both = _take(ff.eng.set_op(out, other, "UNION"))
            assert other_want.rows and _bits(both) == _bits(mid.rows + other_want.rows)
        finally:
            other.free()
    finally:
        out.free()


def test_inputs_from_every_stage(ff):
    gs = groupby.parse_sentence("GROUP BY $-.s, $-.d YIELD $-.s AS s, $-.d AS d, COUNT(*) AS n")
    grouped = ff.eng.group_by(ff.rows, ff.names, [c.expr.encode() for c in gs.groups],
                              [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    ordered = ff.eng.order_by(ff.rows, ff.names, [("w", False)], (3, 700))
    united = ff.eng.set_op(ordered, ordered, "UNION")
    yielded = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.w AS w, $-.d AS s, $-.s AS d WHERE $-.w > 0")
    try:
        for rows, names in ((grouped, ["s", "d", "n"]), (ordered, ff.names), (united, ff.names), (yielded, ["w", "s", "d"])):
            inp = ngql.Interim(names, rows.fetch())
            assert inp.rows
            _check(ff, rows, names, inp, "FETCH PROP ON e $-.s->$-.d YIELD e.w * 2 AS w2, e._dst",
                   [groupby.INT if n in ("s", "d") else None for n in names])
    finally:
        for r in (grouped, ordered, united, yielded):
            r.free()


# ------------------------------------------------------------------------------ 7. statuses, in nbg.h's order
def _fails(ff, code, text, rows=None, names=None):
    rows = ff.rows if rows is None else rows
    assert _code(lambda: _fetch(ff, rows, ff.names if names is None else names, text)) == code, text
    assert ff.rows.digest() == ff.digest


def test_status_1_invalid_arguments(ff, nba):
    good = E.edge_prop("e", "w").encode()
    for bad in (b"\xff", good[:-1], good + b"\x00"):
        assert _code(lambda: ff.eng.fetch_edges(ff.rows, ff.names, "s", "d", None, 1, [bad])) == L.E_INVALID_ARGUMENT
        assert _code(lambda: ff.eng.fetch_edges([(1, 2, 0)], [], "", "", None, 1, [good, bad])) == L.E_INVALID_ARGUMENT
    # ... before the edge and syntax checks
    assert _code(lambda: ff.eng.fetch_edges(ff.rows, ff.names, "*", "d", None, 999, [E.src_prop("p", "i").encode(), b"\xff"])) == \
        L.E_INVALID_ARGUMENT
    # in != NULL with a null dst_col; in == NULL with srcs == NULL and num_keys > 0
    names = (C.c_char_p * len(ff.names))(*[n.encode() for n in ff.names])
    req = L.nbg_fetch_edges_request(names, b"s", None, None, None, None, None, 0, 1, None, None, 0, 0)
    out = C.c_void_p()
    assert ff.eng.lib.nbg_fetch_edges(ff.eng.h, ff.rows.h, C.byref(req), C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    req = L.nbg_fetch_edges_request()
    req.num_keys, req.edge_type = 3, 1
    assert ff.eng.lib.nbg_fetch_edges(ff.eng.h, None, C.byref(req), C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    # rows of another engine
    sent = ngql.Parser("GO FROM 1 OVER like YIELD like._src AS s, like._dst AS d").go()
    other = nba.go_device([5662213458193308137], [nba.edge_types["like"]], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        assert _code(lambda: ff.eng.fetch_edges(other, ["s", "d"], "s", "d", None, 1, [good])) == L.E_INVALID_ARGUMENT
    finally:
        other.free()
    # host-only rows
    req, keep = ff.eng._go_request([ROOTS[0]], [1], 1, b"", [E.edge_prop("e", "_src").encode(), E.edge_prop("e", "_dst").encode()],
                                   False, False)
    h = C.c_void_p()
    assert ff.eng.lib.nbg_go(ff.eng.h, C.byref(req), C.byref(h)) == L.OK
    host = DeviceRows(ff.eng, h)
    try:
        assert _code(lambda: ff.eng.fetch_edges(host, ["s", "d"], "s", "d", None, 1, [good])) == L.E_INVALID_ARGUMENT
    finally:
        host.free()
    assert ff.rows.digest() == ff.digest


def test_status_2_partitioned_engine():
    """A LocalCluster of 2 in-process ranks: its rows live on several ranks.  Before the edge check."""
    kb = kvgen.KVBuilder(PARTS)
    for s, d in ((10, 11), (11, 12), (12, 10), (13, 10)):
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, [s, 0.5, 0.5], NOW)
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.load_builder(kb)
        ys = [E.edge_prop("e", "_src").encode(), E.edge_prop("e", "_dst").encode()]
        rows = c.each(lambda e: e.go_device([10, 11], [1], 1, b"", ys))
        assert sum(r.count for r in rows) > 0
        good = [E.edge_prop("e", "w").encode()]
        for e, r in zip(c.engines, rows):
            assert _code(lambda: e.fetch_edges(r, ["s", "d"], "s", "d", None, 1, good)) == L.E_UNSUPPORTED
            assert _code(lambda: e.fetch_edges(r, ["s", "d"], "s", "d", None, 999, good)) == L.E_UNSUPPORTED
            assert _code(lambda: e.fetch_edges([(10, 11, 0)], [], "", "", None, 1, good)) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()


def test_status_3_unknown_edge_and_star(ff):
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope $-.s->$-.d YIELD nope.i")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope 1->2")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON t $-.s->$-.d")                 # a tag is no edge
    for ref in ("$-.*->$-.d", "$-.s->$-.*", "$-.s->$-.d@$-.*"):
        _fails(ff, L.E_EXECUTION_ERROR, f"FETCH PROP ON e {ref} YIELD e.w")
        _fails(ff, L.E_EXECUTION_ERROR, f"FETCH PROP ON e {ref} YIELD $$.t.name")      # before 4
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope $-.s->$-.d YIELD $^.t.name")
    with pytest.raises(NbgError, match="schema not exist"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON nope $-.s->$-.d")


@pytest.mark.parametrize("ys", ["$^.t.name", "$$.t.name, e.w", "e.w, $-.d", "$v.d + e.w", "r.i, e.w", "e.w + q.i", "r._dst"])
def test_status_4_syntax_errors(ff, ys):
    _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON e $-.s->$-.d YIELD {ys}")
    _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON e 1->2 YIELD {ys}")


def test_status_4_comes_before_5_and_6(ff):
    _, empty, einp, _ = _go_rows(ff, f"GO FROM {EMPTY_SRC} OVER e YIELD {GO_E}", [EMPTY_SRC], 1, 1)
    try:
        assert empty.count == 0
        for ys in ("$^.t.name", "$-.d", "r.i"):
            _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON e $-.s->$-.d YIELD {ys}", empty, einp.columns)    # on an empty input
            _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON e $-.zz->$-.d YIELD {ys}")                        # before the key column check
        assert _code(lambda: ff.eng.fetch_edges([], [], "", "", None, 1, [E.src_prop("t", "name").encode()])) == L.E_SYNTAX_ERROR
    finally:
        empty.free()


def test_status_5_zero_input_rows(ff):
    _, empty, einp, _ = _go_rows(ff, f"GO FROM {EMPTY_SRC} OVER e YIELD {GO_E}", [EMPTY_SRC], 1, 1)
    try:
        for text, ncols in (("FETCH PROP ON e $-.s->$-.d YIELD e.w", 1), ("FETCH PROP ON r $-.s->$-.d", 5),
                            ("FETCH PROP ON e $-.s->$-.d", 3),                                      # before 7: e.f is a FLOAT
                            ("FETCH PROP ON e $-.zz->$-.d YIELD e.nope, 1 + 1", 2),                 # before 6
                            ("FETCH PROP ON r $-.s->$-.d YIELD r.s + \"x\"", 1)):                   # before 6 and 7
            out = _fetch(ff, empty, einp.columns, text)
            assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == ncols and _take(out) == []
    finally:
        empty.free()


def test_status_6_key_columns_and_props(ff):
    with pytest.raises(NbgError, match="Column `zz' not found") as ex:
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.zz->$-.yy YIELD e.w")
    assert ex.value.code == L.E_EXECUTION_ERROR
    with pytest.raises(NbgError, match="Column `yy' not found"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.s->$-.yy@$-.zz YIELD e.w")
    with pytest.raises(NbgError, match="Column `zz' not found"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.s->$-.d@$-.zz YIELD e.w")
    mixed = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.s AS s, $-.d AS d, (double)$-.w AS x, $-.w > 0 AS b, (timestamp)$-.d AS t")
    try:
        names = ["s", "d", "x", "b", "t"]
        for col in ("x", "b", "t"):                             # DOUBLE, BOOL, TIMESTAMP: getVid refuses them
            for ref in (f"$-.{col}->$-.d", f"$-.s->$-.{col}", f"$-.s->$-.d@$-.{col}"):
                _fails(ff, L.E_EXECUTION_ERROR, f"FETCH PROP ON e {ref} YIELD e.w", mixed, names)
        inp = ngql.Interim(names, mixed.fetch())
        _check(ff, mixed, names, inp, "FETCH PROP ON e $-.s->$-.d YIELD e.w", [groupby.VID, groupby.VID, None, None, groupby.TIMESTAMP])
    finally:
        mixed.free()
    with pytest.raises(NbgError, match="No props declared."):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.s->$-.d YIELD 1 + 1, 7")
    with pytest.raises(NbgError, match="Get props failed"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON e $-.s->$-.d YIELD e.w, e.nope + 1")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON e 1->2 YIELD e.nope")
    # before 7: with a string-building column, with the bare FLOAT prop
    _fails(ff, L.E_EXECUTION_ERROR, 'FETCH PROP ON r $-.zz->$-.d YIELD r.s + "x"')
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON e $-.s->$-.d YIELD e.f, e.nope")


def test_status_8_evaluation_errors(ff):
    """`7 / e.w`: the found edges with w == 0 fail the call; an expression that fails nowhere, or
    only where no edge is found, does not."""
    assert any(r[3] == 0 for r in ff.inp.rows)
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON e $-.s->$-.d YIELD e._dst, 7 / e.w")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON r $-.s->$-.d YIELD r.b + 1", ff.rrows, ff.rinp.columns)   # ill-typed: every found row
    _check(ff, ff.rows, ff.names, ff.inp, "FETCH PROP ON e $-.s->$-.d YIELD e._dst, 7 / (e.w + 100) AS q", ff.types)
    assert _take(_fetch(ff, None, None, "FETCH PROP ON r 5->6 YIELD r.b + 1")) == []               # nothing found: nothing evaluated


def test_undecodable_value_and_record_in_another_part():
    """An edge whose value does not decode: a YIELD that reads a schema prop of it fails the call
    (bare or inside an expression), its key pseudo-props still evaluate, and keys that do not
    touch it are answered.  An edge record loaded into a part other than src % parts + 1 is not
    found: the storage client asks the hash part."""
    kb = kvgen.KVBuilder(PARTS)
    tab = {}
    for s, d in ((10, 11), (10, 12), (11, 10), (12, -14)):
        tab[(s, d, 0)] = [s + d, 0.5, 0.5]
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, tab[(s, d, 0)], NOW)
    part = kvgen.part_of(10, PARTS)
    kb.put(part, kvgen.edge_key(part, 10, 1, 0, 13, kvgen.version_of(NOW)), kvgen.encode_row(E_SCHEMA, [1, 0.5, 0.5])[:-3])
    wrong = kvgen.part_of(15, PARTS) % PARTS + 1
    assert wrong != kvgen.part_of(15, PARTS)
    kb.put(wrong, kvgen.edge_key(wrong, 15, 1, 0, 10, kvgen.version_of(NOW)), kvgen.encode_row(E_SCHEMA, [2, 0.5, 0.5]))
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"e": EdgeTable(1, E_TYPES, tab)}
    try:
        lst = "10->11, 15->10, 10->12, 11->10, 12->-14, 10->14"
        dev = _check(f, None, None, None, f"FETCH PROP ON e {lst} YIELD e.w, e._dst, e.x + 1 AS x1")
        assert [r[1] for r in dev] == [11, 12, 10, -14]
        for ys in ("e.w", "e.w + 1", "e._dst, e.x"):
            assert _code(lambda: _fetch(f, None, None, f"FETCH PROP ON e 10->11, 10->13 YIELD {ys}")) == L.E_EXECUTION_ERROR
        got = _take(_fetch(f, None, None, "FETCH PROP ON e 10->11, 10->13, 10->12 YIELD e._src, e._dst, e._rank, e._type"))
        assert [list(r) for r in got] == [[10, 11, 0, "e"], [10, 13, 0, "e"], [10, 12, 0, "e"]]
    finally:
        f.eng.close()


# ------------------------------------------------------------------------------ 8. device limits
def test_limit_float_and_misaligned_inputs(ff):
    for ys in ("e._src AS s, e._dst AS d, e.f AS f", "e._src AS s, e._dst AS d, e.x + e.w AS m, e.w AS w"):
        sent = ngql.Parser(f"GO FROM {ROOTS[0]} OVER e YIELD {ys}").go()
        rows = ff.eng.go_device([ROOTS[0]], [1], 1, b"", [c.expr.encode() for c in sent.yields])
        try:
            assert rows.count > 0
            _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD e.w", rows, [c.name() for c in sent.yields])
        finally:
            rows.free()


def test_limit_bare_float_prop(ff):
    """A bare FLOAT prop would make a FLOAT result column, whose rows no later stage can re-read."""
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD e.f")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD e.w, e.f AS f, e.f + 1")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD DISTINCT e.f")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d")                    # no YIELD: every column, f among them
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON e {ROOTS[0]}->5 YIELD e.f")


@pytest.mark.parametrize("ys", ['r.s + "!"', "(string)r.i", "upper(r.s)", "r.i, (string)r.b AS t"])
def test_limit_string_building(ff, ys):
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON r $-.s->$-.d YIELD {ys}")


def test_limit_too_many_columns(ff):
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD " + ", ".join(f"e.w + {k}" for k in range(33)))
    text = "FETCH PROP ON e $-.s->$-.d YIELD " + ", ".join(f"e.w + {k}" if k % 2 else "e.x" for k in range(32))   # 32: answered
    _check(ff, ff.rows, ff.names, ff.inp, text, ff.types)


def _balanced_sum(terms):
    while len(terms) > 1:
        terms = [f"({a} + {b})" if b else a for a, b in zip(terms[0::2], terms[1::2] + [None])]
    return terms[0]


def test_limit_program_length_and_registers(ff):
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON e $-.s->$-.d YIELD " + _balanced_sum([f"e.w * {k}" for k in range(100)]))
    ok = "FETCH PROP ON e $-.s->$-.d YIELD " + _balanced_sum([f"e.w * {k}" for k in range(20)])
    _check(ff, ff.rows, ff.names, ff.inp, ok, ff.types)
    deep = "e.w"
    for k in range(60):                                         # right-nested: one live register per level
        deep = f"(e._dst % {k + 2} + {deep})"
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON e $-.s->$-.d YIELD {deep}")
