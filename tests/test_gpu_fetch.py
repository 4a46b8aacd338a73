"""nbg_fetch_vertices on the MI355X: piped FETCH PROP ON <tag> over device-resident rows, judged by
the plain-Python model of tests/support/fetchpipe.py (pinned to the reference's FetchVerticesTest
vectors by tests/test_fetch_model.py) — never by the device itself.

The graph, GO and columns are those of tests/test_gpu_orderby.py (seeded RMAT-10, 5 parts, the
4,452-row GO in several segments).  This file's own KV builder adds a second tag `p` with INT (i,
nb), DOUBLE (x, both zeros), BOOL (b), TIMESTAMP (ts) and STRING (s) props on the vertices with
v % 3 != 0 only, so found and tagless vids both occur; nb holds another vertex's vid, so a FETCH's
output can feed a FETCH.  The graph's own vids are positive: the builder also adds tagged vertices
with negative vids (-v for v % 7 == 0) and two near the int64 extremes, so the sorted vid table has
both signs.  The model's table is cross-checked once against the CPU oracle's `$$.p.prop`.  A
third tag `pf` (FLOAT f, INT i) on the same graph vertices reaches the FLOAT limit: a bare `pf.f`
is NBG_E_UNSUPPORTED, `pf.f` inside an expression reads the cell widened to a double.

The model's input is the GO's rows in their fetch order, so its output is the expected result row
for row: nbg_fetch_vertices keeps the input's order.

Three NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a
vid column whose kind differs between OVER types, a tag without device tables, and the input of
2^32 rows."""
import ctypes as C
import struct

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen, rmat
from nebula_amd.engine import DeviceRows, nba_engine
from tests.support import fetchpipe, golden, groupby, ngql, orderby, setops
from tests.support.fetchpipe import TagTable
from tests.support.oracle import Oracle
from tests.test_gpu_orderby import E_SCHEMA, GO_COLS, PARTS, ROOTS, SEED, T_SCHEMA

pytestmark = pytest.mark.gpu

GOLDEN = golden.load("fetch_golden.json")["cases"]
BLOCK = 256                           # csrc/ws.h: rows a workgroup walks per step
OB_CHUNK, STAGE_GRID = 2048, 2048     # csrc/nbg_internal.h, csrc/stage.h
EMPTY_SRC = 123                       # no such vertex: a GO from it has no rows
FV_KERNELS = ("k_fv_resolve", "k_fv_emit")
P_TAG = 9
P_SCHEMA = [("i", kvgen.INT), ("x", kvgen.DOUBLE), ("b", kvgen.BOOL), ("ts", kvgen.TIMESTAMP), ("s", kvgen.STRING),
            ("nb", kvgen.INT)]
P_TYPES = [("i", groupby.INT), ("x", groupby.DOUBLE), ("b", groupby.BOOL), ("ts", groupby.TIMESTAMP),
           ("s", groupby.STRING), ("nb", groupby.INT)]
PF_TAG = 10                           # a tag with a FLOAT prop, on the graph's vertices with v % 3 != 0
PF_SCHEMA = [("f", kvgen.FLOAT), ("i", kvgen.INT)]
PF_TYPES = [("f", groupby.DOUBLE), ("i", groupby.INT)]    # (a FLOAT cell reads as its double, RowReader::getFloat)
LOW, HIGH = -(1 << 63) + 5, (1 << 63) - 6
NOW = 1_600_000_000_000_000


def _p_row(v, nb):
    x = (v % 17 - 8) * 0.25
    if x == 0.0 and v % 2:
        x = -0.0
    return [v % 41 - 20, x, v % 2 == 0, 1_500_000_000 + v % 100_000, f"p{v % 11}", nb]


def _pf_row(v):
    """f is no float32 for most v: the model holds what the 4-byte cell widens to."""
    return [struct.unpack("<f", struct.pack("<f", (v % 13 - 6) * 0.1))[0], v % 5]


def _kv(pf=False):
    """tests/test_gpu_orderby.py's records plus tag p (and, with pf, tag pf); returns (sources,
    builder, {vid: p row}, the graph's vertices)."""
    src, dst, _ = rmat.rmat_edges(10, seed=SEED)
    rng = np.random.default_rng(SEED)
    w = rng.integers(-50, 50, len(src))
    k = rng.integers(-(1 << 20) + 1, 1 << 20, len(src))
    kb = kvgen.KVBuilder(PARTS)
    verts = np.unique(np.concatenate([src, dst])).tolist()
    for v in verts:
        kb.insert_vertex(v, 7, T_SCHEMA, [f"n{v % 23}"], NOW)
    tagged = [v for v in verts if v % 3 != 0] + [-v for v in verts if v % 7 == 0] + [LOW, HIGH]
    table = {}
    for n, v in enumerate(tagged):
        table[v] = _p_row(v, tagged[(n + 1) % len(tagged)])
        kb.insert_vertex(v, P_TAG, P_SCHEMA, table[v], NOW)
    if pf:
        for v in verts:
            if v % 3 != 0:
                kb.insert_vertex(v, PF_TAG, PF_SCHEMA, _pf_row(v), NOW)
    for s, d, a, b in zip(src.tolist(), dst.tolist(), w.tolist(), k.tolist()):
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, [a, b / 8.0, 0.5], NOW + 1)
    return src, kb, table, verts


class Fixture:
    pass


@pytest.fixture(scope="module")
def ff():
    """Engine, oracle, the model's tag table, the GO's rows on the device and, fetched, as the
    model's input: computed once and left unchanged."""
    src, kb, table, verts = _kv(pf=True)
    assert set(ROOTS) <= set(src.tolist()) and EMPTY_SRC not in set(verts)
    f = Fixture()
    f.verts, f.table = verts, table
    f.all_vids = sorted(set(verts) | set(table))
    assert f.all_vids[0] == LOW and f.all_vids[-1] == HIGH                       # the vid table has both signs
    assert sum(v < 0 for v in f.all_vids) > 50 and sum(v > 0 for v in f.all_vids) > 500
    f.eng = Engine(PARTS)
    f.orc = Oracle(PARTS)
    for be, reg_e, reg_t in ((f.eng, f.eng.register_edge, f.eng.register_tag),
                             (f.orc, lambda *a: f.orc.register(True, *a), lambda *a: f.orc.register(False, *a))):
        reg_e(1, "e", E_SCHEMA)
        reg_t(7, "t", T_SCHEMA)
        reg_t(P_TAG, "p", P_SCHEMA)
        reg_t(PF_TAG, "pf", PF_SCHEMA)
        be.load_builder(kb)
    f.tables = {"p": TagTable(P_TAG, P_TYPES, table),
                "pf": TagTable(PF_TAG, PF_TYPES, {v: _pf_row(v) for v in verts if v % 3 != 0}),
                "t": TagTable(7, [("name", groupby.STRING)], {v: [f"n{v % 23}"] for v in verts})}
    f.go = f"GO 2 STEPS FROM {ROOTS[0]}, {ROOTS[1]} OVER e YIELD {GO_COLS}"
    f.sent = ngql.Parser(f.go).go()
    f.names = [c.name() for c in f.sent.yields]
    f.rows = f.eng.go_device(ROOTS, [1], 2, b"", [c.expr.encode() for c in f.sent.yields])
    assert f.eng.lib.nbg_rows_num_segments(f.rows.h) >= 2 and f.rows.count >= 2048
    f.digest = f.rows.digest()
    f.inp = ngql.Interim(f.names, f.rows.fetch())             # the input's own segment order
    f.types = groupby.go_column_types(f.sent, f.inp.rows)
    found = sum(r[1] in table for r in f.inp.rows)
    assert 0 < found < len(f.inp.rows)                        # found and tagless vids both occur
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


def _st(text):
    return fetchpipe.parse_sentence(text)


def _fetch(f, rows, names, text):
    """Engine.fetch_vertices for a `FETCH PROP ON ...` text: over `rows`, or over its vid list."""
    st = _st(text)
    tag_id = f.tables[st.label].tag_id if st.label in f.tables else 999
    ys = [c.expr.encode() for c in st.yields] if st.yields is not None else []
    if st.ref is None:
        return f.eng.fetch_vertices(st.vids, [], "", tag_id, ys, st.distinct)
    return f.eng.fetch_vertices(rows, names, st.ref[1], tag_id, ys, st.distinct)


def _model(f, inp, text, types=None):
    return fetchpipe.fetch_model(_st(text), f.tables, inp, types)


def _yield(eng, rows, names, text):
    from tests.support import yieldpipe
    st = yieldpipe.parse_sentence(text)
    return eng.yield_rows(rows, names, [c.expr.encode() for c in st.yields], st.where.encode() if st.where is not None else b"")


def _go(eng, yields, root=ROOTS[0], steps=1):
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {yields}").go()
    rows = eng.go_device([root], [1], steps, b"", [c.expr.encode() for c in sent.yields])
    return rows, [c.name() for c in sent.yields]


def _check(f, rows, names, inp, text, types=None):
    """The device's rows are the model's, row for row; returns them."""
    want, _ = _model(f, inp, text, types)
    out = _fetch(f, rows, names, text)
    assert out.count == len(want.rows)
    assert out.count == 0 or f.eng.lib.nbg_rows_num_segments(out.h) == 1
    assert f.eng.lib.nbg_rows_num_cols(out.h) == len(want.columns)
    dev = _take(out)
    assert _bits(dev) == _bits(want.rows)
    return dev


# ------------------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize("case", GOLDEN, ids=[f"{c['test']}-{i}" for i, c in enumerate(GOLDEN)])
def test_golden_on_device(nba, nba_data, case):
    """Every GO with go_device where the device path takes it, the FETCH with nbg_fetch_vertices,
    one fetch at the end: the reference's status, column names and rows.  A FETCH behind a GO gets
    the GO's device handle as `in`, never the host's copy of its rows sent as a list; the one GO
    without a YIELD clause (nonExistVertex, no rows) is not go_device's, so the host holds it."""
    ses = fetchpipe.Session(nba, fetchpipe.nba_tables(nba_data, kvgen.NBA_TAGS), device=True)
    ok, msg = fetchpipe.run_case(ses, case)
    assert ok, msg
    assert not ses.fallbacks
    if case["status"] == "SUCCEEDED":
        assert ses.fetch_calls == 1
        go = case["query"].upper().split("|")[0].split(";")[0]
        assert ses.fetch_paths == (["list"] if "GO FROM" not in go else ["rows"] if " YIELD " in go else ["host rows"])


# ------------------------------------------------------------------------------ 2. parity, in order
TEXTS = {
    "bare": "FETCH PROP ON p $-.d YIELD p.i, p.x, p.b, p.ts, p.s, p.nb",
    "one_bare": "FETCH PROP ON p $-.d YIELD p.s",
    "exprs": "FETCH PROP ON p $-.d YIELD p.i * 2 + 1 AS a, (double)p.i / 3 AS q, (int)p.x AS xi, p.x < 0.0 AS neg, "
             "p.ts - 1500000000 AS dt, (bool)p.i AS bi, !p.b AS nb, p.s == \"p3\" AS is3, p.i % 7 AS m, "
             "(timestamp)p.i AS t, hash(p.nb) AS h, -p.x AS nx, p.b XOR (p.i > 0) AS lx",
    "constants": 'FETCH PROP ON p $-.d YIELD 7 AS c, p.i, "no such name" AS s2, 2.5 AS h, true AS b, "p3" AS known',
    "no_yield": "FETCH PROP ON p $-.d",
    "variable": "FETCH PROP ON p $v.d YIELD p.s, p.i + 1 AS i1",
    "other_tag": "FETCH PROP ON t $-.d YIELD t.name, t.name < \"n2\" AS lt",
}


@pytest.mark.parametrize("name", list(TEXTS))
def test_parity_in_input_order(ff, name):
    dev = _check(ff, ff.rows, ff.names, ff.inp, TEXTS[name], ff.types)
    assert dev and (name == "other_tag" or len(dev) < len(ff.inp.rows))
    assert ff.rows.digest() == ff.digest                        # `in` stays unchanged


def test_table_against_the_oracle(ff):
    """The model's {vid: row} table is what the CPU oracle's `$$.p.prop` reads over the same GO."""
    go = (f"GO 2 STEPS FROM {ROOTS[0]}, {ROOTS[1]} OVER e YIELD e._dst AS d, $$.p.i AS i, $$.p.x AS x, $$.p.b AS b, "
          "$$.p.ts AS ts, $$.p.s AS s, $$.p.nb AS nb")
    rows = orderby.Session(ff.orc).execute(go).rows
    assert len(rows) == len(ff.inp.rows)
    hit = 0
    for r in rows:
        if r[0] in ff.table:
            assert _bits([r[1:]]) == _bits([ff.table[r[0]]])
            hit += 1
        else:
            assert r[0] % 3 == 0 and _bits([r[1:]]) == _bits([[0, 0.0, False, 0, "", 0]])    # the schema's defaults
    assert 0 < hit < len(rows)


def test_profile_entries(ff):
    n = len(ff.inp.rows)
    found = sum(r[1] in ff.table for r in ff.inp.rows)
    ff.eng.profile(True)
    _take(_fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD p.i"))
    prof = ff.eng.profile_read()
    ff.eng.profile(False)
    assert [prof[k]["launches"] for k in FV_KERNELS] == [1, 1]
    assert prof["k_fv_resolve"]["algo_bytes"] == n * 13 and prof["k_fv_resolve"]["ms"] > 0
    assert prof["k_fv_emit"]["algo_bytes"] == n + found * (4 + 8 * 2)


# ------------------------------------------------------------------------------ 3. join edge cases
def test_join_edges_through_lists(ff):
    vids = ff.all_vids
    mid = len(vids) // 2
    gap = next(v + 1 for v in vids[mid:] if v + 1 not in set(vids))              # absent between neighbours
    tagless = next(v for v in ff.verts if v % 3 == 0)
    probe = [LOW - 1, LOW, HIGH, HIGH + 1, -(1 << 63) + 1, (1 << 63) - 1, gap, tagless, vids[1], vids[-2], 0, -1, 1, vids[mid]]
    text = "FETCH PROP ON p " + ", ".join(str(v) for v in probe) + " YIELD p.nb, p.i, p.s"
    dev = _check(ff, None, None, None, text)
    assert [r[0] for r in dev[:2]] == [ff.table[LOW][5], ff.table[HIGH][5]] and len(dev) < len(probe)
    # every vid of the table, in order and reversed, with a miss after each
    every = [x for v in vids for x in (v, v + 1)]
    for lst in (every, every[::-1]):
        _check(ff, None, None, None, "FETCH PROP ON p " + ", ".join(map(str, lst)) + " YIELD p.nb, p.ts")
    # every vid missing: zero rows, NBG_OK
    out = _fetch(ff, None, None, "FETCH PROP ON p 5, 6, 7 YIELD p.i, p.s")
    assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == 2 and _take(out) == []


def test_join_edges_through_a_yield_in_front(ff):
    from tests.support import yieldpipe
    # (a YIELD without any `$-' is the reference's executeConstant, one row: the constants ride on a column)
    for ytext in ("YIELD $-.d + 1 AS id", "YIELD 0 - $-.d AS id", f"YIELD $-.d * 0 + {LOW} AS id", "YIELD $-.d * 0 + 5 AS id",
                  f"YIELD $-.d AS id, {HIGH} AS hi"):
        st = yieldpipe.parse_sentence(ytext)
        mid, types = yieldpipe.yield_model(ff.inp, st, ff.types)
        rows = _yield(ff.eng, ff.rows, ff.names, ytext)
        try:
            for col in mid.columns:
                dev = _check(ff, rows, mid.columns, mid, f"FETCH PROP ON p $-.{col} YIELD p.nb, p.x", types)
                if str(LOW) in ytext:
                    assert len(dev) == len(ff.inp.rows)                              # one vid, every row
                if ytext == "YIELD $-.d * 0 + 5 AS id":
                    assert dev == []
        finally:
            rows.free()
    assert any(-r[1] in ff.table for r in ff.inp.rows)                               # the negated vids hit


def test_heavy_duplicates(ff):
    v = next(r[1] for r in ff.inp.rows if r[1] in ff.table)
    lst = ", ".join([str(v)] * 3000)
    dev = _check(ff, None, None, None, f"FETCH PROP ON p {lst} YIELD p.i, p.s, p.x")
    assert len(dev) == 3000 and len(set(map(tuple, dev))) == 1
    out = _take(_fetch(ff, None, None, f"FETCH PROP ON p {lst} YIELD DISTINCT p.i, p.s, p.x"))
    assert _bits(out) == _bits([ff.table[v][:1] + ff.table[v][4:5] + ff.table[v][1:2]])


def test_record_in_another_part_is_not_found():
    """A tag record loaded into a part other than vid % parts + 1: the storage client asks the hash
    part and finds nothing.  (Explicit parts also give the snapshot its visibility bytes.)"""
    kb = kvgen.KVBuilder(PARTS)
    table = {}
    for v in (10, 11, 12, -14):
        table[v] = _p_row(v, v)
        kb.insert_vertex(v, P_TAG, P_SCHEMA, table[v], NOW)
    wrong = kvgen.part_of(13, PARTS) % PARTS + 1
    assert wrong != kvgen.part_of(13, PARTS)
    kb.put(wrong, kvgen.vertex_key(wrong, 13, P_TAG, kvgen.version_of(NOW)), kvgen.encode_row(P_SCHEMA, _p_row(13, 13)))
    kb.insert_edge(10, 11, 1, 0, E_SCHEMA, [1, 0.5, 0.5], NOW + 1)
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(P_TAG, "p", P_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"p": TagTable(P_TAG, P_TYPES, table)}
    try:
        dev = _check(f, None, None, None, "FETCH PROP ON p 13, 12, 13, -14, 10, 9, 11, 13 YIELD p.nb, p.s")
        assert [r[0] for r in dev] == [12, -14, 10, 11]
    finally:
        f.eng.close()


def test_undecodable_record_is_not_found():
    """A live tag record whose value does not decode (truncated, garbage, a bare header) is no record: the
    reference's collectProps skips every bad value, so no tag_data comes back and no row is made.
    The live record is the newest version: a good older version behind a bad one does not count,
    a bad older version behind a good one does not hurt.  Another tag of the same vertices, whose
    records all decode, still finds them."""
    kb = kvgen.KVBuilder(PARTS)
    table = {}
    for v in (10, 11, 12, -14, 16):
        table[v] = _p_row(v, v)
        kb.insert_vertex(v, P_TAG, P_SCHEMA, table[v], NOW)

    def put(v, val, now):
        part = kvgen.part_of(v, PARTS)
        kb.put(part, kvgen.vertex_key(part, v, P_TAG, kvgen.version_of(now)), val)
    good13 = kvgen.encode_row(P_SCHEMA, _p_row(13, 13))
    put(13, good13[:-3], NOW)                                   # truncated inside the string
    put(-15, b"\xff\xff\xff\xff\xff", NOW)                      # garbage
    put(17, b"\x00", NOW)                                       # a header and no columns
    put(15, kvgen.encode_row(P_SCHEMA, _p_row(15, 15)), NOW)    # a good version, superseded by ...
    put(15, good13[:4], NOW + 1)                                # ... a bad one
    put(16, good13[:4], NOW - 1)                                # a bad version, superseded by the good one
    for v in (13, -15, 17, 15, 16):
        kb.insert_vertex(v, 7, T_SCHEMA, [f"n{v % 23}"], NOW)
    kb.insert_edge(10, 13, 1, 0, E_SCHEMA, [1, 0.5, 0.5], NOW + 1)
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.register_tag(P_TAG, "p", P_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"p": TagTable(P_TAG, P_TYPES, table),
                "t": TagTable(7, [("name", groupby.STRING)], {v: [f"n{v % 23}"] for v in (13, -15, 17, 15, 16)})}
    try:
        lst = "13, 12, -15, 16, 17, 15, 13, -14, 10, 11"
        dev = _check(f, None, None, None, f"FETCH PROP ON p {lst} YIELD p.nb, p.s, p.i + 1 AS i1")
        assert [r[0] for r in dev] == [12, 16, -14, 10, 11]
        _check(f, None, None, None, f"FETCH PROP ON p {lst}")
        assert _take(_fetch(f, None, None, "FETCH PROP ON p 13, -15, 17, 15 YIELD p.i")) == []
        dev = _check(f, None, None, None, f"FETCH PROP ON t {lst} YIELD t.name")
        assert len(dev) == 6
        # through a pipe: the GO's one row leads to 13
        rows, names = _go(f.eng, "e._dst AS d", 10)
        try:
            assert [list(r) for r in rows.fetch()] == [[13]]
            assert _take(_fetch(f, rows, names, "FETCH PROP ON p $-.d YIELD p.i")) == []
            assert [list(r) for r in _take(_fetch(f, rows, names, "FETCH PROP ON t $-.d YIELD t.name"))] == [["n13"]]
        finally:
            rows.free()
    finally:
        f.eng.close()


def test_undecodable_record_on_a_partitioned_engine():
    """An undecodable tag record in the parts of one rank only: the decoded-record table is a single
    engine's, so both ranks of a LocalCluster make the same collectives in finalize whatever their
    own records hold, the load ends, and `$$.p.i` reads what it read before (the schema's default
    for the undecodable record, the value for the good one)."""
    kb = kvgen.KVBuilder(PARTS)
    for v in (10, 11, 12):
        kb.insert_vertex(v, P_TAG, P_SCHEMA, _p_row(v, v), NOW)
    part = kvgen.part_of(13, PARTS)
    kb.put(part, kvgen.vertex_key(part, 13, P_TAG, kvgen.version_of(NOW)), kvgen.encode_row(P_SCHEMA, _p_row(13, 13))[:-3])
    for d in (11, 13):
        kb.insert_edge(10, d, 1, 0, E_SCHEMA, [1, 0.5, 0.5], NOW + 1)
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.register_tag(P_TAG, "p", P_SCHEMA)
        c.load_builder(kb)                                      # finalize: the tag tables are all-gathered
        ys = [E.edge_prop("e", "_dst").encode(), E.dst_prop("p", "i").encode()]
        rows = c.each(lambda e: e.go_device([10], [1], 1, b"", ys))
        got = sorted(tuple(r) for part_rows in rows for r in _take(part_rows))
        assert got == [(11, _p_row(11, 11)[0]), (13, 0)]
        for e in c.engines:
            assert _code(lambda: e.fetch_vertices([13], [], "", P_TAG, [E.edge_prop("p", "i").encode()])) == L.E_UNSUPPORTED
    finally:
        c.close()


def test_single_vertex_engine():
    kb = kvgen.KVBuilder(PARTS)
    kb.insert_vertex(42, P_TAG, P_SCHEMA, _p_row(42, 42), NOW)
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(P_TAG, "p", P_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"p": TagTable(P_TAG, P_TYPES, {42: _p_row(42, 42)})}
    try:
        dev = _check(f, None, None, None, "FETCH PROP ON p 41, 42, 43, 42, -42 YIELD p.nb, p.i + 1")
        assert len(dev) == 2
    finally:
        f.eng.close()


@pytest.mark.parametrize("search", ["", "two-level"])
def test_both_search_variants_over_many_vertices(monkeypatch, search):
    """5,000 vertices of both signs, more than twice the pivot count, so NBG_FETCH_SEARCH=two-level
    takes the LDS-pivot search (fewer vertices fall back to the plain one): every vid, first and
    last included, with a miss beside each, in a shuffled order, as a list and through a pipe."""
    rng = np.random.default_rng(3)
    vids = sorted(set(rng.integers(-(1 << 62), 1 << 62, 5000).tolist()) | {LOW, HIGH})
    assert len(vids) >= 2 * 2048 and vids[0] < 0 < vids[-1]
    kb = kvgen.KVBuilder(PARTS)
    table = {}
    for n, v in enumerate(vids):
        if n % 5:                                               # every fifth vertex lacks the tag
            table[v] = _p_row(v, vids[(n + 1) % len(vids)])
            kb.insert_vertex(v, P_TAG, P_SCHEMA, table[v], NOW)
        else:
            kb.insert_vertex(v, 7, T_SCHEMA, ["n"], NOW)
    f = Fixture()
    f.eng = Engine(PARTS)
    f.eng.register_edge(1, "e", E_SCHEMA)
    f.eng.register_tag(7, "t", T_SCHEMA)
    f.eng.register_tag(P_TAG, "p", P_SCHEMA)
    f.eng.load_builder(kb)
    f.tables = {"p": TagTable(P_TAG, P_TYPES, table)}
    if search:
        monkeypatch.setenv("NBG_FETCH_SEARCH", search)
    try:
        probe = [x for v in vids for x in (v, v + 1, v - 1)]
        rng.shuffle(probe)
        st = _st("FETCH PROP ON p 1 YIELD p.nb, p.i, p.s")
        st.vids = [int(v) for v in probe]
        want, _ = fetchpipe.fetch_model(st, f.tables, None)
        ys = [c.expr.encode() for c in st.yields]
        lst = f.eng.fetch_vertices(st.vids, [], "", P_TAG, ys)
        try:
            assert lst.count == len(want.rows) == sum(v in table for v in probe) > 3000
            piped = f.eng.fetch_vertices(lst, ["nb", "i", "s"], "nb", P_TAG, ys)         # nb: the next vertex's vid
            st.vids = [r[0] for r in want.rows]
            assert _bits(_take(piped)) == _bits(fetchpipe.fetch_model(st, f.tables, None)[0].rows)
            assert _bits(lst.fetch()) == _bits(want.rows)
        finally:
            lst.free()
    finally:
        f.eng.close()


# ------------------------------------------------------------------------------ 4. row-count edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2047, 2048, 2049])
def test_row_count_edges(ff, n):
    rows = ff.eng.order_by(ff.rows, ff.names, [], (0, n))
    try:
        inp = ngql.Interim(ff.names, rows.fetch())
        assert len(inp.rows) == n
        _check(ff, rows, ff.names, inp, "FETCH PROP ON p $-.d YIELD p.nb, p.ts + p.i AS t, p.s", ff.types)
    finally:
        rows.free()


def test_more_chunks_than_workgroups(ff):
    """The GO's d column doubled ten times by UNION ALL: one segment of more chunks than STAGE_GRID
    workgroups, so the grid stride runs.  Every base row occurs 1,024 times, so the model's digest
    is the base result's: the count and the sum times 1,024, the xor of an even multiplicity 0."""
    cur = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.d AS id")
    try:
        for _ in range(10):
            nxt = ff.eng.set_op(cur, cur, "UNION")
            cur.free()
            cur = nxt
        assert cur.count == len(ff.inp.rows) * 1024 and -(-cur.count // OB_CHUNK) > STAGE_GRID
        text = "FETCH PROP ON p $-.id YIELD p.nb, p.ts + p.i AS t"
        base, _ = _model(ff, ngql.Interim(["id"], [[r[1]] for r in ff.inp.rows]), text, [groupby.INT])
        from tests.support.oracle import row_digest
        cnt, _, total = row_digest(base.rows)
        out = _fetch(ff, cur, ["id"], text)
        try:
            assert out.count == cnt * 1024
            assert out.digest() == (cnt * 1024, 0, (total * 1024) & ((1 << 64) - 1))
        finally:
            out.free()
    finally:
        cur.free()


# ------------------------------------------------------------------------------ 5. DISTINCT
@pytest.mark.parametrize("ys", ["p.x", "p.s, p.b", "p.i % 3 AS m, p.x * 0.0 AS z", "p.nb", "7 AS k, p.b"])
def test_distinct(ff, ys):
    text = f"FETCH PROP ON p $-.d YIELD DISTINCT {ys}"
    want, _ = _model(ff, ff.inp, text, ff.types)
    dev = _take(_fetch(ff, ff.rows, ff.names, text))
    assert len(dev) == len(want.rows) and groupby.multiset(dev) == groupby.multiset(want.rows)
    if ys == "p.x":
        xs = [ff.table[r[1]][1] for r in ff.inp.rows if r[1] in ff.table]
        assert any(x == 0.0 and str(x) == "0.0" for x in xs) and any(str(x) == "-0.0" for x in xs)   # both zeros
        assert sum(r[0] == 0.0 for r in dev) == 1


# ------------------------------------------------------------------------------ 6. statuses, in nbg.h's order
def _fails(ff, code, text, rows=None, names=None):
    rows = ff.rows if rows is None else rows
    assert _code(lambda: _fetch(ff, rows, ff.names if names is None else names, text)) == code, text
    assert ff.rows.digest() == ff.digest


def test_status_1_invalid_arguments(ff, nba):
    good = E.edge_prop("p", "i").encode()
    for bad in (b"\xff", good[:-1], good + b"\x00"):
        assert _code(lambda: ff.eng.fetch_vertices(ff.rows, ff.names, "d", P_TAG, [bad])) == L.E_INVALID_ARGUMENT
        assert _code(lambda: ff.eng.fetch_vertices([1, 2], [], "", P_TAG, [good, bad])) == L.E_INVALID_ARGUMENT
    # ... before the tag and syntax checks
    assert _code(lambda: ff.eng.fetch_vertices(ff.rows, ff.names, "*", 999, [E.src_prop("p", "i").encode(), b"\xff"])) == \
        L.E_INVALID_ARGUMENT
    # in == NULL with vids == NULL and num_vids > 0
    req = L.nbg_fetch_request()
    req.num_vids, req.tag_id = 3, P_TAG
    out = C.c_void_p()
    assert ff.eng.lib.nbg_fetch_vertices(ff.eng.h, None, C.byref(req), C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    # rows of another engine
    sent = ngql.Parser("GO FROM 1 OVER like YIELD like._dst AS d").go()
    other = nba.go_device([5662213458193308137], [nba.edge_types["like"]], 1, b"", [c.expr.encode() for c in sent.yields])
    try:
        assert _code(lambda: ff.eng.fetch_vertices(other, ["d"], "d", P_TAG, [good])) == L.E_INVALID_ARGUMENT
    finally:
        other.free()
    # host-only rows
    req, keep = ff.eng._go_request([ROOTS[0]], [1], 1, b"", [E.edge_prop("e", "_dst").encode()], False, False)
    h = C.c_void_p()
    assert ff.eng.lib.nbg_go(ff.eng.h, C.byref(req), C.byref(h)) == L.OK
    host = DeviceRows(ff.eng, h)
    try:
        assert _code(lambda: ff.eng.fetch_vertices(host, ["d"], "d", P_TAG, [good])) == L.E_INVALID_ARGUMENT
    finally:
        host.free()
    assert ff.rows.digest() == ff.digest


def test_status_2_partitioned_engine():
    """A LocalCluster of 2 in-process ranks: its rows live on several ranks.  Before the tag check."""
    src, kb, table, verts = _kv()
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.register_tag(7, "t", T_SCHEMA)
        c.register_tag(P_TAG, "p", P_SCHEMA)
        c.load_builder(kb)
        ys = [E.edge_prop("e", "_dst").encode()]
        rows = c.each(lambda e: e.go_device([ROOTS[0]], [1], 1, b"", ys))
        assert sum(r.count for r in rows) > 0
        good = [E.edge_prop("p", "i").encode()]
        for e, r in zip(c.engines, rows):
            assert _code(lambda: e.fetch_vertices(r, ["d"], "d", P_TAG, good)) == L.E_UNSUPPORTED
            assert _code(lambda: e.fetch_vertices(r, ["d"], "d", 999, good)) == L.E_UNSUPPORTED
            assert _code(lambda: e.fetch_vertices([1, 2], [], "", P_TAG, good)) == L.E_UNSUPPORTED
            r.free()
    finally:
        c.close()


def test_status_3_unknown_tag_and_star(ff):
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope $-.d YIELD nope.i")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope 1, 2")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p $-.* YIELD p.i")
    # before 4: a `$^' beside them
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON nope $-.d YIELD $^.p.i")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p $-.* YIELD $$.p.i")
    with pytest.raises(NbgError, match="schema not exist"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON nope $-.d")


@pytest.mark.parametrize("ys", ["$^.p.i", "$$.p.i, p.i", "p.i, $-.d", "$v.d + p.i", "t.name, p.i", "e.w", "p.i + q.i"])
def test_status_4_syntax_errors(ff, ys):
    _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON p $-.d YIELD {ys}")
    _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON p 1, 2 YIELD {ys}")


def test_status_4_comes_before_5_and_6(ff):
    empty, names = _go(ff.eng, "e._dst AS d, e.w AS w", EMPTY_SRC)
    try:
        assert empty.count == 0
        for ys in ("$^.p.i", "$-.d", "t.name"):
            _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON p $-.d YIELD {ys}", empty, names)        # a syntax error on an empty input
            _fails(ff, L.E_SYNTAX_ERROR, f"FETCH PROP ON p $-.zz YIELD {ys}")                     # before the vid column check
        assert _code(lambda: ff.eng.fetch_vertices([], [], "", P_TAG, [E.src_prop("p", "i").encode()])) == L.E_SYNTAX_ERROR
    finally:
        empty.free()


def test_status_5_zero_input_rows(ff):
    empty, names = _go(ff.eng, "e._dst AS d, e.w AS w, $$.t.name AS s", EMPTY_SRC)
    try:
        for text, ncols in (("FETCH PROP ON p $-.d YIELD p.i", 1), ("FETCH PROP ON p $-.d", 6),
                            ("FETCH PROP ON p $-.zz YIELD p.nope, 1 + 1", 2),                      # before 6
                            ("FETCH PROP ON p $-.s YIELD p.s + \"x\"", 1)):                        # before 6 and 7
            out = _fetch(ff, empty, names, text)
            assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == ncols and _take(out) == []
        out = ff.eng.fetch_vertices([], [], "", P_TAG, [])
        assert out.count == 0 and ff.eng.lib.nbg_rows_num_cols(out.h) == 6 and _take(out) == []
    finally:
        empty.free()


def test_status_6_vid_column_and_props(ff):
    with pytest.raises(NbgError, match="Column `zz' not found") as ex:
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.zz YIELD p.i")
    assert ex.value.code == L.E_EXECUTION_ERROR
    for col in ("s", "x", "b2"):                                # STRING, DOUBLE, BOOL: getVid refuses them
        _fails(ff, L.E_EXECUTION_ERROR, f"FETCH PROP ON p $-.{col} YIELD p.i")
    ts = _yield(ff.eng, ff.rows, ff.names, "YIELD (timestamp)$-.d AS t, $-.d AS d")
    try:
        _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p $-.t YIELD p.i", ts, ["t", "d"])          # TIMESTAMP
        inp = ngql.Interim(["t", "d"], ts.fetch())
        _check(ff, ts, ["t", "d"], inp, "FETCH PROP ON p $-.d YIELD p.nb")                         # INT
    finally:
        ts.free()
    with pytest.raises(NbgError, match="No props declared."):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD 1 + 1, 7")
    with pytest.raises(NbgError, match="Get props failed"):
        _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD p.i, p.nope + 1")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p 1 YIELD p.nope")
    # before 7: with a string-building column
    _fails(ff, L.E_EXECUTION_ERROR, 'FETCH PROP ON p $-.zz YIELD p.s + "x"')
    _fails(ff, L.E_EXECUTION_ERROR, 'FETCH PROP ON p $-.d YIELD p.s + "x", p.nope')


def test_status_8_evaluation_errors(ff):
    """`7 / p.i`: the found vertices with i == 0 fail the call; an expression that fails nowhere, or
    only where no vertex is found, does not."""
    assert any(ff.table[r[1]][0] == 0 for r in ff.inp.rows if r[1] in ff.table)
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p $-.d YIELD p.nb, 7 / p.i")
    _fails(ff, L.E_EXECUTION_ERROR, "FETCH PROP ON p $-.d YIELD p.b + 1")                          # ill-typed: every found row
    _check(ff, ff.rows, ff.names, ff.inp, "FETCH PROP ON p $-.d YIELD p.nb, 7 / (p.i + 100) AS q", ff.types)
    out = _fetch(ff, None, None, "FETCH PROP ON p 5, 6 YIELD p.b + 1")                             # nothing found: nothing evaluated
    assert _take(out) == []


# ------------------------------------------------------------------------------ 7. device limits
def test_limit_float_and_misaligned_inputs(ff):
    for ys in ("e._dst AS d, e.f AS f", "e._dst AS d, e.x + e.w AS m, e.w AS w"):
        rows, names = _go(ff.eng, ys)
        try:
            _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON p $-.d YIELD p.i", rows, names)
        finally:
            rows.free()


def test_limit_bare_float_prop(ff):
    """A bare FLOAT prop would make a FLOAT result column, whose rows no later stage can re-read."""
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON pf $-.d YIELD pf.f")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON pf $-.d YIELD pf.i, pf.f AS f, pf.f + 1")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON pf $-.d YIELD DISTINCT pf.f")
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON pf $-.d")                        # no YIELD: every column, f among them
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON pf {ROOTS[0]}, 5 YIELD pf.f")
    _check(ff, ff.rows, ff.names, ff.inp, "FETCH PROP ON pf $-.d YIELD pf.i", ff.types)          # the tag's other prop


def test_float_prop_inside_an_expression(ff):
    """`pf.f` below the root is the 4-byte cell widened to a double (RowReader::getFloat), so the
    column is a DOUBLE one: by kind, and by the cast nbg_set_op gives an INT column unioned to it."""
    text = ("FETCH PROP ON pf $-.d YIELD pf.f * 2 AS f2, pf.f + pf.i AS s, pf.f < 0.0 AS neg, (int)(pf.f * 10) AS fi, "
            "(double)pf.f AS fd, -pf.f AS nf, pf.i")
    dev = _check(ff, ff.rows, ff.names, ff.inp, text, ff.types)
    want = [ff.tables["pf"].rows[r[1]] for r in ff.inp.rows if r[1] in ff.tables["pf"].rows]
    assert dev and _bits([[r[4]] for r in dev]) == _bits([[w[0]] for w in want])                  # the widened cell itself
    assert len({r[4] for r in dev}) > 5 and any(r[4] != round(r[4], 1) for r in dev)             # no short decimals
    out = _fetch(ff, ff.rows, ff.names, "FETCH PROP ON pf $-.d YIELD pf.f * 2 AS a")
    ints = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.w AS a")
    try:
        assert ff.eng.lib.nbg_rows_col_kind(out.h, 0) == L.V_DOUBLE
        both = _take(ff.eng.set_op(out, ints, "UNION"))
        assert _bits(both) == _bits([[w[0] * 2] for w in want] + [[float(r[3])] for r in ff.inp.rows])
    finally:
        out.free()
        ints.free()


@pytest.mark.parametrize("ys", ['p.s + "!"', "(string)p.i", "upper(p.s)", "p.i, (string)p.b AS t"])
def test_limit_string_building(ff, ys):
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON p $-.d YIELD {ys}")


def test_limit_too_many_columns(ff):
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON p $-.d YIELD " + ", ".join(f"p.i + {k}" for k in range(33)))
    text = "FETCH PROP ON p $-.d YIELD " + ", ".join(f"p.i + {k}" if k % 2 else "p.nb" for k in range(32))   # 32: answered
    _check(ff, ff.rows, ff.names, ff.inp, text, ff.types)


def _balanced_sum(terms):
    while len(terms) > 1:
        terms = [f"({a} + {b})" if b else a for a, b in zip(terms[0::2], terms[1::2] + [None])]
    return terms[0]


def test_limit_program_length_and_registers(ff):
    _fails(ff, L.E_UNSUPPORTED, "FETCH PROP ON p $-.d YIELD " + _balanced_sum([f"p.i * {k}" for k in range(100)]))
    ok = "FETCH PROP ON p $-.d YIELD " + _balanced_sum([f"p.i * {k}" for k in range(20)])
    _check(ff, ff.rows, ff.names, ff.inp, ok, ff.types)
    deep = "p.i"
    for k in range(60):                                         # right-nested: one live register per level
        deep = f"(p.nb % {k + 2} + {deep})"
    _fails(ff, L.E_UNSUPPORTED, f"FETCH PROP ON p $-.d YIELD {deep}")


# ------------------------------------------------------------------------------ 8. chaining
def test_output_feeds_every_stage(ff):
    from tests.support import yieldpipe
    text = "FETCH PROP ON p $-.d YIELD p.i % 5 AS k, p.ts AS ts, p.x AS x, p.nb AS nb"
    mid, mtypes = _model(ff, ff.inp, text, ff.types)
    out = _fetch(ff, ff.rows, ff.names, text)
    names = mid.columns
    try:
        gs = groupby.parse_sentence("GROUP BY $-.k YIELD $-.k, COUNT(*), SUM($-.k)")
        got = _take(ff.eng.group_by(out, names, [c.expr.encode() for c in gs.groups],
                                    [(c.fun, c.expr.encode(), c.alias) for c in gs.yields]))
        assert groupby.multiset(got) == groupby.multiset(groupby.group_model(mid, gs.groups, gs.yields).rows)
        top = _take(ff.eng.order_by(out, names, [("ts", True), ("nb", False)], (0, 10)))
        orderby.check_window(top, mid, [("ts", True), ("nb", False)], (0, 10))
        both = _take(ff.eng.set_op(out, out, "UNION"))
        assert _bits(both) == _bits(mid.rows + mid.rows)
        ytext = "YIELD $-.ts + 1 AS t1, $-.k WHERE $-.x < 0.0"
        again = _take(_yield(ff.eng, out, names, ytext))
        assert _bits(again) == _bits(yieldpipe.yield_model(mid, yieldpipe.parse_sentence(ytext))[0].rows) and again
        _check(ff, out, names, mid, "FETCH PROP ON p $-.nb YIELD p.s, p.nb", mtypes)                # FETCH again
    finally:
        out.free()


def test_inputs_from_every_stage(ff):
    gs = groupby.parse_sentence("GROUP BY $-.d YIELD $-.d AS d, COUNT(*) AS n")
    grouped = ff.eng.group_by(ff.rows, ff.names, [c.expr.encode() for c in gs.groups],
                              [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    ordered = ff.eng.order_by(ff.rows, ff.names, [("x", False)], (3, 700))
    united = ff.eng.set_op(ordered, ordered, "UNION")
    yielded = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.w AS w, $-.d AS d WHERE $-.w > 0")
    fetched = _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD p.s AS s, p.nb AS d")
    try:
        for rows, names in ((grouped, ["d", "n"]), (ordered, ff.names), (united, ff.names), (yielded, ["w", "d"]),
                            (fetched, ["s", "d"])):
            inp = ngql.Interim(names, rows.fetch())
            assert inp.rows
            assert _check(ff, rows, names, inp, "FETCH PROP ON p $-.d YIELD p.nb, p.i * 2 AS i2, p.s",
                          [groupby.INT if n == "d" else None for n in names])
    finally:
        for r in (grouped, ordered, united, yielded, fetched):
            r.free()


def test_go_order_by_fetch_limit_is_exact(ff):
    """`GO | ORDER BY $-.x DESC, $-.d | FETCH ... | LIMIT 7`: every stage on the device, the rows the
    model's, in order."""
    text = f"{ff.go} | ORDER BY $-.x DESC, $-.d | FETCH PROP ON p $-.d YIELD p.nb AS nb, p.s AS s, p.i + 1 AS i1 | LIMIT 7"
    ordered = orderby.order_model(ff.inp, [("x", True), ("d", False)])
    want, _ = _model(ff, ordered, "FETCH PROP ON p $-.d YIELD p.nb AS nb, p.s AS s, p.i + 1 AS i1", ff.types)
    ses = fetchpipe.Session(ff.eng, ff.tables, device=True)
    dev = ses.execute(text)
    assert ses.fetch_calls == 1 and not ses.fallbacks
    assert dev.columns == ["nb", "s", "i1"] and _bits(dev.rows) == _bits(want.rows[:7]) and len(dev.rows) == 7
    # the host session (the models over the oracle's GO) agrees on the unordered pipe
    mod = fetchpipe.Session(ff.orc, ff.tables).execute(f"{ff.go} | FETCH PROP ON p $-.d YIELD p.nb AS nb, p.i AS i")
    dev = fetchpipe.Session(ff.eng, ff.tables, device=True).execute(f"{ff.go} | FETCH PROP ON p $-.d YIELD p.nb AS nb, p.i AS i")
    assert mod.rows and groupby.multiset(dev.rows) == groupby.multiset(mod.rows)
    # `$var' input through the session
    ses = fetchpipe.Session(ff.eng, ff.tables, device=True)
    dev = ses.execute(f"$v = {ff.go}; FETCH PROP ON p $v.d YIELD p.s, p.ts AS ts | YIELD $-.ts + 1 AS t1")
    assert ses.fetch_calls == 1 and ses.yield_calls == 1 and not ses.fallbacks
    # (this GO ran again: its segments, hence its fetch order, need not be ff.rows')
    assert sorted(r[0] for r in dev.rows) == sorted(ff.table[r[1]][3] + 1 for r in ff.inp.rows if r[1] in ff.table)


def test_col_types_through_union(ff):
    """The result's col_types, seen through nbg_set_op (the result takes the left side's types): a
    bare TIMESTAMP prop unioned with an INT column stays TIMESTAMP, which RowReader::getVid refuses
    as a vid column; the INT column unioned with the TIMESTAMP prop is INT and is accepted; a root
    cast gives its type; arithmetic over the prop is INT."""
    ts = _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD p.ts AS a")
    cast = _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD (timestamp)p.nb AS a")
    arith = _fetch(ff, ff.rows, ff.names, "FETCH PROP ON p $-.d YIELD p.ts + 0 AS a")
    ints = _yield(ff.eng, ff.rows, ff.names, "YIELD $-.w AS a")
    good = [E.edge_prop("p", "i").encode()]
    made = []
    try:
        n_ts = ts.count
        for left, right, accepted in ((ts, ints, False), (ints, ts, True), (cast, ints, False), (arith, ints, True)):
            u = ff.eng.set_op(left, right, "UNION")
            made.append(u)
            assert u.count == left.count + right.count
            if accepted:
                ff.eng.fetch_vertices(u, ["a"], "a", P_TAG, good).free()
            else:
                assert _code(lambda: ff.eng.fetch_vertices(u, ["a"], "a", P_TAG, good)) == L.E_EXECUTION_ERROR
        rows = made[0].fetch()
        assert [r[0] for r in rows[:n_ts]] == [ff.table[r[1]][3] for r in ff.inp.rows if r[1] in ff.table]
        assert [r[0] for r in rows[n_ts:]] == [r[3] for r in ff.inp.rows]
        assert ff.eng.lib.nbg_rows_col_kind(ts.h, 0) == L.V_INT
    finally:
        for r in [ts, cast, arith, ints] + made:
            r.free()
