"""nbg_rows_encode: the RowSetWriter bytes of a device-resident result, byte for byte.

Every case runs a GO or a stage over a small hand-built graph, encodes the device rows
(DeviceRows.encode) and compares with tests/support/rowsetenc.encode_rowset over the same rows as
nbg_rows_fetch delivers them, by column types written out here from the reference's rule
(Collector::getSchema: `e._dst' is a VID, an INT prop an INT, a root cast the cast's type, ...).
The model is pinned to the reference's vectors in tests/test_rowset_model.py.

The graph (type e = 1, g = 2; tags t = 7, p = 9), every hub a source of its own GO:
  HUB   2,100 e-edges whose props walk through the varint widths, the special doubles and a few
        short strings, and 5 g-edges
  EDGE  e-edges whose strings put the cord and the row length on their width boundaries
  LONG  70 e-edges that all carry one 40,000-byte string (no LDS tile holds such a row)
  MIX   2,001 e-edges with short strings and the long one in the middle
Three NBG_E_UNSUPPORTED guards have no test because no GO result reaches them: a column whose kind
differs between OVER types (or from its type's reader), an input of 2^32 rows, and a row that
could encode to 4 GiB."""
import ctypes as C
import struct

import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen
from nebula_amd.engine import DeviceRows
from nebula_amd.kvgen import BOOL, DOUBLE, INT, STRING, TIMESTAMP, VID
from tests.support import fetchpipe, groupby, ngql, rowcodec, yieldpipe
from tests.support.rowsetenc import encode_rowset

pytestmark = pytest.mark.gpu

PARTS = 3
NOW = 1_600_000_000_000_000
E_SCHEMA = [("w", INT), ("x", DOUBLE), ("f", kvgen.FLOAT), ("s", STRING)]
G_SCHEMA = [("w", INT)]
T_SCHEMA = [("name", STRING)]
P_SCHEMA = [("i", INT), ("x", DOUBLE), ("b", BOOL), ("ts", TIMESTAMP), ("s", STRING)]
HUB, EDGE, LONG, MIX, NOWHERE = 1, 2, 3, 4, 999
N_HUB = 2100
I64_MIN = -(1 << 63)
INTS = [0, 127, 128, 16383, 16384, 1 << 31, 1 << 62, (1 << 63) - 1, -1, I64_MIN, 5, -7, 300]
DOUBLES = [float("nan"), -0.0, float("inf"), float("-inf"), 1.5, 0.0, -2.25e300]
STRS = ["", "a", "name-0", "name-1", "x" * 33]
LONG_S = ("0123456789abcdefghijklmnopqrstuvwxyz" * 1200)[:40000]
# EDGE's strings, by what `YIELD e.s, 16 x e.w` (w = 1) makes of them: the cord is varint(len) + len + 16
CORD_LENS = {255: 237, 256: 238, 65535: 65516, 65536: 65517}
# ... and `YIELD e.s' alone: the row is header + varint(len) + len
ROW_LENS = {127: 125, 128: 126}
EDGE_LENS = sorted(CORD_LENS.values()) + sorted(ROW_LENS.values()) + [0, 1]
RE_KERNELS = ("k_re_size", "k_re_scan", "k_re_emit")


def _hub_dst(i):
    return i + 10 if i % 2 == 0 else -(i + 10)


def _kv():
    kb = kvgen.KVBuilder(PARTS)
    for i in range(N_HUB):
        d = _hub_dst(i)
        kb.insert_edge(HUB, d, 1, 0, E_SCHEMA, [INTS[i % 13], DOUBLES[i % 7], 0.5, STRS[i % 5]], NOW)
        if i % 2 == 0:
            kb.insert_vertex(d, 7, T_SCHEMA, [f"n{i % 23}"], NOW)
        if i % 3 == 0:
            kb.insert_vertex(d, 9, P_SCHEMA, [INTS[i % 13], DOUBLES[(i + 1) % 7], i % 2 == 0, 1_500_000_000 + i, STRS[i % 5]], NOW)
    for i in range(5):
        kb.insert_edge(HUB, 5000 + i, 2, 0, G_SCHEMA, [i], NOW)
    for i, n in enumerate(EDGE_LENS):
        kb.insert_edge(EDGE, 6000 + i, 1, 0, E_SCHEMA, [1, 0.25, 0.5, ("q" * n)], NOW)
    for i in range(70):
        kb.insert_edge(LONG, 7000 + i, 1, 0, E_SCHEMA, [i, 0.0, 0.5, LONG_S], NOW)
    for i in range(2001):
        kb.insert_edge(MIX, 10000 + i, 1, 0, E_SCHEMA, [i, 0.0, 0.5, LONG_S if i == 1000 else "m"], NOW)
    for v in (HUB, EDGE, LONG, MIX):
        kb.insert_vertex(v, 7, T_SCHEMA, ["hub"], NOW)
    return kb


def _engine(kb, cls=Engine, *a):
    eng = cls(PARTS, *a)
    eng.register_edge(1, "e", E_SCHEMA)
    eng.register_edge(2, "g", G_SCHEMA)
    eng.register_tag(7, "t", T_SCHEMA)
    eng.register_tag(9, "p", P_SCHEMA)
    eng.load_builder(kb)
    return eng


@pytest.fixture(scope="module")
def eng():
    e = _engine(_kv())
    yield e
    e.close()


def _go(eng, yields, root=HUB, over="e", steps=1):
    """GO FROM root OVER ... YIELD yields on the device: (rows, column names)."""
    sent = ngql.Parser(f"GO FROM 1 OVER {over} YIELD {yields}").go()
    etypes = [{"e": 1, "g": 2}[n.strip()] for n in over.split(",")]
    rows = eng.go_device([root], etypes, steps, b"", [c.expr.encode() for c in sent.yields])
    return rows, [c.name() for c in sent.yields]


HUB_COLS = "e._dst AS d, e.w AS w, e.x AS x, e.s AS s, $$.t.name AS n, (bool)(e.w % 2 == 0) AS b, (timestamp)e.w AS ts"
HUB_TYPES = [VID, INT, DOUBLE, STRING, STRING, BOOL, TIMESTAMP]


@pytest.fixture(scope="module")
def hub(eng):
    rows, names = _go(eng, HUB_COLS)
    assert rows.count == N_HUB
    yield rows, names
    rows.free()


def _cell_bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def _bits(rows):
    return [[_cell_bits(v) for v in r] for r in rows]


def _check(rows, types):
    """encode() is the model's bytes of fetch(), its types are `types`, and the reader takes the
    fetched rows back out of it; returns (fetched rows, bytes)."""
    data, got_types = rows.encode()
    fetched = rows.fetch()
    assert got_types == types == rows.col_types()
    assert len(fetched) == rows.count
    want = encode_rowset(types, fetched)
    assert len(data) == len(want)
    assert data == want
    back = [rowcodec.decode_row(r, types) for r in rowcodec.split_rowset(data)]
    assert _bits(back) == _bits(fetched)
    return fetched, data


def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


# ------------------------------------------------------------------------------ framing
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049])
def test_one_segment_of_n_rows(eng, hub, n):
    rows, names = hub
    cut = eng.order_by(rows, names, [], (0, n))
    try:
        assert cut.count == n and eng.lib.nbg_rows_num_segments(cut.h) == 1
        _check(cut, HUB_TYPES)
    finally:
        cut.free()


def test_go_result_as_it_lies(eng, hub):
    fetched, data = _check(hub[0], HUB_TYPES)
    assert sorted(r[0] for r in fetched) == sorted(_hub_dst(i) for i in range(N_HUB))
    assert {r[1] for r in fetched} == set(INTS)


def test_several_short_segments(eng):
    """Two OVER types: each type's rows are segments of their own."""
    rows, _ = _go(eng, "e._dst AS d, g._dst AS gd, e.w AS w, g.w AS gw, e.s AS s", over="e, g")
    try:
        assert eng.lib.nbg_rows_num_segments(rows.h) >= 2 and rows.count == N_HUB + 5
        fetched, _ = _check(rows, [VID, VID, INT, INT, STRING])
        assert sum(r[1] != 0 for r in fetched) == 5
    finally:
        rows.free()


def test_zero_rows(eng, hub):
    """No rows: no bytes, and the columns' types all the same: a window without rows keeps its
    input's types.  (A GO without rows has no schema in the reference either: GoExecutor finishes
    with the column names alone; its columns report what nbg_rows_col_type does.)"""
    cut = eng.order_by(hub[0], hub[1], [], (0, 0))
    rows, _ = _go(eng, HUB_COLS, root=NOWHERE)
    try:
        assert cut.count == 0 and cut.encode() == (b"", HUB_TYPES) and cut.col_types() == HUB_TYPES
        assert rows.count == 0 and len(rows.col_types()) == len(HUB_TYPES)
        assert rows.encode() == (b"", rows.col_types())
        out = C.c_void_p()
        assert eng.lib.nbg_rows_encode(eng.h, cut.h, C.byref(out)) == L.OK
        assert eng.lib.nbg_rowset_len(out) == 0 and eng.lib.nbg_rowset_rows(out) == 0
        assert eng.lib.nbg_rowset_num_cols(out) == len(HUB_TYPES)
        assert [eng.lib.nbg_rowset_col_type(out, c) for c in range(len(HUB_TYPES))] == HUB_TYPES
        assert eng.lib.nbg_rowset_col_type(out, len(HUB_TYPES)) == -1 and eng.lib.nbg_rowset_col_type(out, -1) == -1
        eng.lib.nbg_rowset_free(out)
    finally:
        cut.free()
        rows.free()


def test_rowset_accessors(eng, hub):
    rows, _ = hub
    out = C.c_void_p()
    assert eng.lib.nbg_rows_encode(eng.h, rows.h, C.byref(out)) == L.OK
    try:
        assert eng.lib.nbg_rowset_rows(out) == N_HUB and eng.lib.nbg_rowset_num_cols(out) == len(HUB_TYPES)
        n = eng.lib.nbg_rowset_len(out)
        data = C.string_at(eng.lib.nbg_rowset_data(out), n)
        assert len(rowcodec.split_rowset(data)) == N_HUB
    finally:
        eng.lib.nbg_rowset_free(out)
    assert eng.lib.nbg_rows_col_type(rows.h, -1) == -1 and eng.lib.nbg_rows_col_type(rows.h, len(HUB_TYPES)) == -1


# ------------------------------------------------------------------------------ varint widths
def test_int_widths_and_vids_of_both_signs(eng):
    rows, _ = _go(eng, "e.w AS w, e._dst AS d, e._src AS s, e._rank AS r, (timestamp)e.w AS ts, e.w + 0 AS w0")
    try:
        fetched, data = _check(rows, [INT, VID, VID, INT, TIMESTAMP, INT])
        assert {r[0] for r in fetched} == set(INTS)
        assert any(r[1] < 0 for r in fetched) and any(r[1] > 0 for r in fetched)
        # the widths themselves, on the bytes: (w, ts) take 1, 1, 2, 2, 3, 5, 9, 9, 10, 10 bytes each
        width = {0: 1, 127: 1, 128: 2, 16383: 2, 16384: 3, 1 << 31: 5, 1 << 62: 9, (1 << 63) - 1: 9, -1: 10, I64_MIN: 10}
        for raw, r in zip(rowcodec.split_rowset(data), fetched):
            if r[0] in width:
                assert len(raw) == 1 + 3 * width[r[0]] + 8 + 8 + 1
    finally:
        rows.free()


# ------------------------------------------------------------------------------ doubles and booleans
def test_doubles_and_booleans(eng):
    rows, _ = _go(eng, "e.x AS x, (bool)(e.w % 2 == 0) AS b, e.x * 0.0 AS z, (bool)e.w AS nz")
    try:
        fetched, _ = _check(rows, [DOUBLE, BOOL, DOUBLE, BOOL])
        seen = {struct.pack("<d", r[0]) for r in fetched}
        assert {struct.pack("<d", v) for v in DOUBLES} == seen
        assert {r[1] for r in fetched} == {True, False} and {r[3] for r in fetched} == {True, False}
    finally:
        rows.free()


def test_bool_written_into_an_int_column(eng):
    """`e.w > 0' has no root cast, so its column takes the type of the last prop read, INT
    (Collector::getSchema), and RowWriter writes the BOOL value as the INT default: one zero byte.
    The stored cell is INT 0, and varint 0 is that byte."""
    rows, _ = _go(eng, "e.w > 0 AS p, e.w AS w")
    try:
        fetched, data = _check(rows, [INT, INT])
        assert {r[0] for r in fetched} == {0} and any(r[1] > 0 for r in fetched)
        assert all(raw[1] == 0 for raw in rowcodec.split_rowset(data))
    finally:
        rows.free()


# ------------------------------------------------------------------------------ block offsets and header
@pytest.mark.parametrize("ncols", [15, 16, 17, 31, 32])
def test_column_counts_around_the_block_offsets(eng, ncols):
    picks = ["e.w AS c%d", "e._dst AS c%d", "e.s AS c%d", "e.x AS c%d"]
    types = [[INT, VID, STRING, DOUBLE][c % 4] for c in range(ncols)]
    rows, _ = _go(eng, ", ".join(picks[c % 4] % c for c in range(ncols)))
    try:
        fetched, data = _check(rows, types)
        for raw in rowcodec.split_rowset(data)[:50]:
            _, offs, hlen = rowcodec.header(raw, ncols)
            assert len(offs) == ncols // 16 and hlen == 1 + len(offs) * ((raw[0] & 7) + 1)
    finally:
        rows.free()


def test_cord_sizes_around_the_offset_widths(eng):
    """17 columns, the dictionary string first: cords of 255, 256, 65,535 and 65,536 bytes have
    offsetBytes 1, 2, 2 and 3, and the offset after column 16 is the cord less the last cell."""
    rows, _ = _go(eng, "e.s AS s, " + ", ".join(f"e.w AS w{c}" for c in range(16)), root=EDGE)
    try:
        fetched, data = _check(rows, [STRING] + [INT] * 16)
        by_cord = {}
        for raw, r in zip(rowcodec.split_rowset(data), fetched):
            _, offs, hlen = rowcodec.header(raw, 17)
            by_cord[len(raw) - hlen] = ((raw[0] & 7) + 1, offs)
        for cord, ob in ((255, 1), (256, 2), (65535, 2), (65536, 3)):
            assert by_cord[cord] == (ob, [cord - 1])
    finally:
        rows.free()


def test_row_lengths_around_the_prefix_widths(eng):
    rows, _ = _go(eng, "e.s AS s", root=EDGE)
    try:
        fetched, data = _check(rows, [STRING])
        lens = {len(r) for r in rowcodec.split_rowset(data)}
        assert {127, 128} <= lens
        assert len(data) == sum(n + (1 if n < 128 else 2 if n < 16384 else 3) for n in (len(r) for r in rowcodec.split_rowset(data)))
    finally:
        rows.free()


# ------------------------------------------------------------------------------ strings
def test_strings_empty_one_byte_and_dictionary(eng):
    rows, _ = _go(eng, "e.s AS s, $$.t.name AS n, $^.t.name AS h")
    try:
        fetched, _ = _check(rows, [STRING, STRING, STRING])
        assert {r[0] for r in fetched} == set(STRS) and "" in {r[1] for r in fetched} and {r[2] for r in fetched} == {"hub"}
    finally:
        rows.free()


def test_constants_outside_the_dictionary_per_over_type(eng):
    """The alias prop `e._type' is the row's type on e's rows and the default 0 on g's
    (getAliasProp, GoExecutor.cpp:851-878), so its cast to string folds to "1" and to "0": neither
    is in the dictionary, and each segment writes its own OVER type's spelling.  Beside it a
    constant every type spells alike."""
    own_type = E.cast("string", E.Expr(E.K_ALIAS, alias="e", prop="_type"))
    ys = [own_type, E.const("no such name"), E.edge_prop("e", "w"), E.edge_prop("g", "w")]
    rows = eng.go_device([HUB], [1, 2], 1, b"", [y.encode() for y in ys])
    try:
        fetched, _ = _check(rows, [STRING, STRING, INT, INT])
        assert sorted({r[0] for r in fetched}) == ["0", "1"] and {r[1] for r in fetched} == {"no such name"}
        assert sum(r[0] == "0" for r in fetched) == 5 and len(fetched) == N_HUB + 5
    finally:
        rows.free()


def test_long_string_rows_take_the_direct_path(eng):
    rows, _ = _go(eng, "e.w AS w, e.s AS s, e._dst AS d", root=LONG)
    try:
        fetched, data = _check(rows, [INT, STRING, VID])
        assert len(fetched) == 70 and all(r[1] == LONG_S for r in fetched) and len(data) > 70 * 40000
    finally:
        rows.free()


def test_one_long_row_between_short_ones(eng):
    """One chunk (one segment of 2,001 rows) whose tiles take the staged path but for the tile
    holding the 40,000-byte row."""
    rows, names = _go(eng, "e.w AS w, e.s AS s, e._dst AS d", root=MIX)
    cut = eng.order_by(rows, names, [], (0, 2001))
    try:
        assert cut.count == 2001 and eng.lib.nbg_rows_num_segments(cut.h) == 1
        fetched, _ = _check(cut, [INT, STRING, VID])
        at = [i for i, r in enumerate(fetched) if r[1] == LONG_S]
        assert len(at) == 1 and sum(r[1] == "m" for r in fetched) == 2000
        _check(rows, [INT, STRING, VID])
    finally:
        cut.free()
        rows.free()


# ------------------------------------------------------------------------------ stage outputs
def test_group_by_output(eng, hub):
    rows, names = hub
    gs = groupby.parse_sentence("GROUP BY $-.s YIELD $-.s AS s, AVG($-.w) AS a, COUNT(*) AS n, MAX($-.d) AS m, SUM($-.x) AS sx")
    out = eng.group_by(rows, names, [c.expr.encode() for c in gs.groups], [(c.fun, c.expr.encode(), c.alias) for c in gs.yields])
    try:
        fetched, _ = _check(out, [STRING, DOUBLE, INT, VID, DOUBLE])
        assert sorted(r[0] for r in fetched) == sorted(STRS)
    finally:
        out.free()


def test_order_by_limit_output_is_in_result_order(eng, hub):
    rows, names = hub
    out = eng.order_by(rows, names, [("w", True), ("d", False)], (3, 500))
    try:
        fetched, data = _check(out, HUB_TYPES)
        keys = [(-r[1], r[0]) for r in fetched]
        assert len(fetched) == 500 and keys == sorted(keys)
        assert [rowcodec.decode_row(r, HUB_TYPES)[0] for r in rowcodec.split_rowset(data)] == [r[0] for r in fetched]
    finally:
        out.free()


def test_yield_and_yield_agg_outputs(eng, hub):
    rows, names = hub
    st = yieldpipe.parse_sentence("YIELD $-.d AS d, (timestamp)$-.w AS t, $-.x AS x, $-.s AS s, $-.b AS b, $-.w > 0 AS p WHERE $-.w != 5")
    out = eng.yield_rows(rows, names, [c.expr.encode() for c in st.yields], st.where.encode())
    try:
        fetched, _ = _check(out, [INT, TIMESTAMP, DOUBLE, STRING, BOOL, BOOL])     # (a passed-through VID column is an INT one)
        assert 0 < len(fetched) < N_HUB
    finally:
        out.free()
    w, x = E.input_prop("w").encode(), E.input_prop("x").encode()
    out = eng.yield_agg(rows, names, [w, x, E.const("*").encode(), w], ["SUM", "AVG", "COUNT", "MAX"])
    try:
        fetched, _ = _check(out, [INT, DOUBLE, INT, INT])
        assert len(fetched) == 1 and fetched[0][2] == N_HUB and fetched[0][3] == (1 << 63) - 1
    finally:
        out.free()


def test_fetch_vertices_output(eng, hub):
    rows, names = hub
    st = fetchpipe.parse_sentence("FETCH PROP ON p $-.d YIELD p.i, p.x, p.b, p.ts, p.s")
    out = eng.fetch_vertices(rows, names, "d", 9, [c.expr.encode() for c in st.yields])
    try:
        fetched, _ = _check(out, [INT, DOUBLE, BOOL, TIMESTAMP, STRING])
        assert len(fetched) == N_HUB // 3
    finally:
        out.free()


def _fetch_edges(eng, yields):
    """`GO FROM HUB OVER e YIELD e._src AS s, e._dst AS d | FETCH PROP ON e $-.s->$-.d YIELD yields`
    on the device: (the keys' rows, the fetched rows)."""
    keys, names = _go(eng, "e._src AS s, e._dst AS d")
    sent = ngql.Parser(f"GO FROM 1 OVER e YIELD {yields}").go()
    return keys, eng.fetch_edges(keys, names, "s", "d", None, 1, [c.expr.encode() for c in sent.yields])


def test_fetch_edges_output(eng):
    """FetchExecutor::prepareYield's types: a bare prop the edge schema's, a root cast the cast's,
    `_dst' and `_rank' (no alias expressions there) and arithmetic the value's natural type."""
    keys, out = _fetch_edges(eng, "e.w AS w, e.x AS x, e.s AS s, (timestamp)e.w AS ts, e._dst AS d, e._rank AS r, "
                                  "(bool)(e.w % 2 == 0) AS b, e.w % 7 AS m")
    try:
        fetched, _ = _check(out, [INT, DOUBLE, STRING, TIMESTAMP, INT, INT, BOOL, INT])
        assert len(fetched) == N_HUB and {r[0] for r in fetched} == set(INTS) and {r[2] for r in fetched} == set(STRS)
        assert sorted(r[4] for r in fetched) == sorted(_hub_dst(i) for i in range(N_HUB))
    finally:
        out.free()
        keys.free()


def test_set_op_output(eng, hub):
    rows, names = hub
    out = eng.set_op(rows, rows, "UNION")
    try:
        fetched, _ = _check(out, HUB_TYPES)
        assert len(fetched) == 2 * N_HUB
    finally:
        out.free()


# ------------------------------------------------------------------------------ repeatability, profile
def test_two_calls_give_identical_bytes(eng, hub):
    a, b = hub[0].encode(), hub[0].encode()
    assert a == b and len(a[0]) > N_HUB * 10


def test_profile_entries(eng, hub):
    eng.profile(True)
    try:
        data, _ = hub[0].encode()
        prof = eng.profile_read()
    finally:
        eng.profile(False)
    for k in RE_KERNELS:
        assert prof[k]["launches"] == 1 and prof[k]["ms"] > 0
    assert prof["k_re_emit"]["algo_bytes"] == N_HUB * (8 * len(HUB_TYPES) + 4) + len(data)


# ------------------------------------------------------------------------------ statuses and limits
def test_status_1_invalid_arguments(eng, hub):
    rows, _ = hub
    out = C.c_void_p()
    assert eng.lib.nbg_rows_encode(None, rows.h, C.byref(out)) == L.E_INVALID_ARGUMENT
    assert eng.lib.nbg_rows_encode(eng.h, None, C.byref(out)) == L.E_INVALID_ARGUMENT
    assert eng.lib.nbg_rows_encode(eng.h, rows.h, None) == L.E_INVALID_ARGUMENT
    assert eng.lib.nbg_rows_col_type(None, 0) == -1
    # host-only rows
    req, keep = eng._go_request([HUB], [1], 1, b"", [E.edge_prop("e", "_dst").encode()], False, False)
    h = C.c_void_p()
    assert eng.lib.nbg_go(eng.h, C.byref(req), C.byref(h)) == L.OK
    host = DeviceRows(eng, h)
    try:
        assert _code(host.encode) == L.E_INVALID_ARGUMENT
        assert host.col_types() == [VID]
    finally:
        host.free()
    # rows of another engine
    kb = kvgen.KVBuilder(PARTS)
    kb.insert_edge(1, 2, 1, 0, E_SCHEMA, [1, 0.0, 0.5, "s"], NOW)
    other = _engine(kb)
    try:
        theirs, _ = _go(other, "e._dst AS d")
        assert theirs.encode()[1] == [VID]
        out = C.c_void_p()
        assert eng.lib.nbg_rows_encode(eng.h, theirs.h, C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
        theirs.free()
    finally:
        other.close()


def test_status_2_partitioned_engine():
    """A LocalCluster of 2 in-process ranks: its rows live on several ranks."""
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.register_edge(2, "g", G_SCHEMA)
        c.register_tag(7, "t", T_SCHEMA)
        c.register_tag(9, "p", P_SCHEMA)
        c.load_builder(_kv())
        ys = [E.edge_prop("e", "_dst").encode()]
        rows = c.each(lambda e: e.go_device([HUB], [1], 1, b"", ys))
        assert sum(r.count for r in rows) > 0
        for r in rows:
            assert _code(r.encode) == L.E_UNSUPPORTED
            assert r.col_types() == [VID]
            r.free()
    finally:
        c.close()


def test_limit_misaligned_and_float_inputs(eng):
    for ys in ("e._dst AS d, e.f AS f", "e._dst AS d, e.x + e.w AS m, e.w AS w"):
        rows, _ = _go(eng, ys)
        try:
            assert _code(rows.encode) == L.E_UNSUPPORTED
        finally:
            rows.free()


def test_limit_derived_string_column(eng):
    rows, _ = _go(eng, '$$.t.name + "!" AS s, e.w AS w')
    try:
        assert rows.count == N_HUB and _code(rows.encode) == L.E_UNSUPPORTED
        assert rows.col_types() == [STRING, INT]
    finally:
        rows.free()


# ------------------------------------------------------------------------------ col_types on its own
def test_col_types_of_a_go_result_and_of_each_stage(eng, hub):
    rows, names = hub
    assert rows.col_types() == HUB_TYPES
    made = []
    try:
        more, _ = _go(eng, "e._src AS s, e._rank AS r, e.w % 7 AS w2, e.x + 1 AS x1, (int)e.w AS xi, (double)e.w AS wd, "
                           "(string)e.w AS ws, $^.t.name AS h, e.w > 0 AS p")
        made.append(more)
        # (`e.w > 0' takes its last getter's type: a BOOL written into an INT column)
        assert more.col_types() == [VID, INT, INT, DOUBLE, INT, DOUBLE, STRING, STRING, INT]
        gs = groupby.parse_sentence("GROUP BY $-.d YIELD $-.d AS d, COUNT(*) AS n, AVG($-.w) AS a, MIN($-.ts) AS t, MAX($-.s) AS s")
        made.append(eng.group_by(rows, names, [c.expr.encode() for c in gs.groups],
                                 [(c.fun, c.expr.encode(), c.alias) for c in gs.yields]))
        assert made[-1].col_types() == [VID, INT, DOUBLE, TIMESTAMP, STRING]
        made.append(eng.order_by(rows, names, [("x", False)], (0, 5)))
        assert made[-1].col_types() == HUB_TYPES
        made.append(eng.set_op(rows, rows, "INTERSECT"))
        assert made[-1].col_types() == HUB_TYPES
        st = yieldpipe.parse_sentence("YIELD $-.d AS d, $-.ts AS t, (timestamp)$-.w AS c, $-.w + 1 AS w1, $-.x AS x, $-.s AS s, $-.b AS b")
        made.append(eng.yield_rows(rows, names, [c.expr.encode() for c in st.yields]))
        assert made[-1].col_types() == [INT, INT, TIMESTAMP, INT, DOUBLE, STRING, BOOL]
        made.append(eng.yield_agg(rows, names, [E.input_prop("w").encode(), E.input_prop("x").encode(), E.const("*").encode()],
                                  ["MAX", "SUM", "COUNT"]))
        assert made[-1].col_types() == [INT, DOUBLE, INT]
        st = fetchpipe.parse_sentence("FETCH PROP ON p $-.d YIELD p.ts, p.s, (timestamp)p.i AS c")
        made.append(eng.fetch_vertices(rows, names, "d", 9, [c.expr.encode() for c in st.yields]))
        assert made[-1].col_types() == [TIMESTAMP, STRING, TIMESTAMP]
        keys, edges = _fetch_edges(eng, "e.w AS w, e.x AS x, e.s AS s, (timestamp)e.w AS ts, e._src AS f")
        made += [keys, edges]
        assert keys.col_types() == [VID, VID] and edges.col_types() == [INT, DOUBLE, STRING, TIMESTAMP, INT]
        piped = eng.go_piped(rows, names, "d", [1], 1, b"", [E.edge_prop("e", "_dst").encode(), E.input_prop("w").encode()])
        made.append(piped)
        assert piped.col_types() == [VID, INT]
    finally:
        for r in made:
            r.free()
