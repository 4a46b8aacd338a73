"""TEST HARNESS: device-resident results with chosen cells, and a numpy reference for
nbg_group_by / nbg_order_by over them.

Row tables.  A `Table` is a list of typed columns of chosen cells (bit patterns for doubles).
`load_value_table` / `load_numeric_table` turn it into a graph whose one-step GO yields exactly
those rows: row r is an out-edge of source vertex `table.src[r]` that carries the cells as edge
props; a VID cell is the edge's `_dst`, a STRING cell is the tag prop `t.name` of that destination
(so the string is a function of the vid).  Every table also carries the INT column `pos`, the
row's index, which makes every row unique: a result row is identified by its `pos`, and
`order_by(rows, [("pos", asc)])` is an input whose physical row i is table row i (nbg_order_by's
output is one segment in result order).
  * the value table goes through kvgen.KVBuilder, so the CPU Oracle loads the same records
    (INT, DOUBLE, BOOL, TIMESTAMP, VID and STRING columns; a Python loop per row);
  * the numeric table goes through Engine.load_edges from numpy arrays (int64, double bit patterns,
    bool; millions of rows, no per-row Python).
Both loaders assert that the GO's fetched rows (DeviceRows.fetch_bits) are the table, bit for bit,
and the value loader that the oracle's rows are too.

Reference.  `order_ref`, `window_ref` and `group_ref` are numpy over the table's bit columns,
written from include/nbg.h's text ("Order", "LIMIT", "Group identity", "Functions"), not from the
kernels; tests/test_rowtable_model.py pins them on the CPU to orderby.order_model and
groupby.group_model, which are pinned to the reference's golden vectors.  String cells are held as
the rank of their encoded bytes among the table's distinct strings (unsigned byte order), and a
device string column is mapped to those ranks through nbg_rows_string before anything is compared.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from typing import List, Optional, Sequence

import numpy as np

from nebula_amd import Engine, _lib as L, expr as E, kvgen
from tests.support import groupby, ngql
from tests.support.oracle import Oracle

INT, VID, DOUBLE, BOOL, STRING, TIMESTAMP = (groupby.INT, groupby.VID, groupby.DOUBLE, groupby.BOOL, groupby.STRING,
                                             groupby.TIMESTAMP)
INT_LIKE = (INT, VID, TIMESTAMP)
KV_TYPE = {INT: kvgen.INT, DOUBLE: kvgen.DOUBLE, BOOL: kvgen.BOOL, TIMESTAMP: kvgen.TIMESTAMP, VID: kvgen.VID}
KIND = {INT: L.V_INT, VID: L.V_INT, TIMESTAMP: L.V_INT, DOUBLE: L.V_DOUBLE, BOOL: L.V_BOOL, STRING: L.V_STRING}
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SIGN = np.uint64(1 << 63)
U = 2.0 ** -53                 # unit roundoff of a double
SRC0 = 3_000_000_000_000       # source vids: away from every cell a test uses as a VID
DST0 = 5_000_000_000_000       # destinations of a table without a VID column: DST0 + pos
E_TYPE, TAG = 1, 7


def dbits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def dval(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(bits) & ((1 << 64) - 1)))[0]


# ------------------------------------------------------------------------------------ tables
class Table:
    """columns: [(name, type, cells)].  Cells: ints for INT / VID / TIMESTAMP, uint64 bit patterns
    for DOUBLE, 0 / 1 for BOOL, str or bytes for STRING.  `src`: each row's source vertex as an
    index (default: `per_src` consecutive rows per source)."""

    def __init__(self, columns, src=None, per_src: int = 64):
        n = len(columns[0][2])
        self.n = n
        self.names = ["pos"]
        self.types = {"pos": INT}
        self.bits = {"pos": np.arange(n, dtype=np.int64)}
        self.strings: List[bytes] = []
        for name, t, cells in columns:
            assert len(cells) == n and name not in self.bits
            if t == STRING:
                raw = [c.encode() if isinstance(c, str) else bytes(c) for c in cells]
                assert not self.strings and all(b"\0" not in s for s in raw)
                self.strings = sorted(set(raw))          # bytes compare as unsigned bytes
                rank = {s: i for i, s in enumerate(self.strings)}
                b = np.array([rank[s] for s in raw], np.int64)
            elif t == DOUBLE:
                b = np.array(cells, dtype=np.uint64).view(np.int64)
            elif t == BOOL:
                b = np.array(cells).astype(np.int64)
                assert ((b == 0) | (b == 1)).all()
            else:
                assert t in INT_LIKE
                b = np.array(cells, dtype=np.int64)
            self.names.append(name)
            self.types[name] = t
            self.bits[name] = b
        self.src = (np.arange(n, dtype=np.int64) // per_src) if src is None else np.asarray(src, np.int64)
        assert len(self.src) == n
        self.vid_col = next((c for c in self.names if self.types[c] == VID), None)
        self.str_col = next((c for c in self.names if self.types[c] == STRING), None)
        assert sum(self.types[c] == VID for c in self.names) <= 1
        if self.str_col:                     # the string is the destination's tag prop
            assert self.vid_col
            pairs = set(zip(self.bits[self.vid_col].tolist(), self.bits[self.str_col].tolist()))
            assert len(pairs) == len(set(self.bits[self.vid_col].tolist())), "a vid with two strings"

    def dst(self):
        return self.bits[self.vid_col] if self.vid_col else DST0 + self.bits["pos"]

    def source_vids(self, rows=None):
        s = self.src if rows is None else self.src[rows]
        return (SRC0 + np.unique(s)).tolist()

    def rows_of_sources(self, lo: int, hi: int):
        """Indices of the rows whose source index lies in [lo, hi)."""
        return np.nonzero((self.src >= lo) & (self.src < hi))[0]

    def py_cell(self, name, r):
        b, t = int(self.bits[name][r]), self.types[name]
        if t == DOUBLE:
            return dval(b)
        if t == BOOL:
            return bool(b)
        if t == STRING:
            return self.strings[b].decode()
        return b

    def interim(self, names=None):
        """(Interim of Python values, the columns' types): the plain-Python models' input."""
        names = names or self.names
        rows = [[self.py_cell(c, r) for c in names] for r in range(self.n)]
        return ngql.Interim(list(names), rows), [self.types[c] for c in names]


# ------------------------------------------------------------------------------------ loading
class Loaded:
    """A table on the device: GO, GROUP BY and ORDER BY over it, results as bit columns."""

    def __init__(self, table: Table, eng: Engine, orc: Optional[Oracle]):
        self.table, self.eng, self.orc = table, eng, orc
        self.names = list(table.names)
        ys = []
        for c in self.names:
            if table.types[c] == VID:
                ys.append(E.edge_prop("e", "_dst"))
            elif table.types[c] == STRING:
                ys.append(E.dst_prop("t", "name"))
            else:
                ys.append(E.edge_prop("e", c))
        self.yields = [y.encode() for y in ys]

    def close(self):
        if self.eng:
            self.eng.close()
        if self.orc:
            self.orc.close()

    # -- results as {column: int64 bits}, string codes mapped to the table's ranks
    def _map_strings(self, rows, col_bits):
        rank = {s: i for i, s in enumerate(self.table.strings)}
        codes, inv = np.unique(col_bits, return_inverse=True)
        ranks = np.array([rank[self.eng.lib.nbg_rows_string(rows.h, int(c))] for c in codes], np.int64)
        return ranks[inv]

    def bits_of(self, rows, names=None, string_cols=None):
        """fetch_bits of `rows` as {name: bits}; `string_cols`: the names that hold the table's strings
        (default: the table's own string column)."""
        names = names or self.names
        cols = rows.fetch_bits()
        assert len(cols) == len(names)
        out = dict(zip(names, cols))
        if string_cols is None:
            string_cols = [c for c in names if self.table.types.get(c) == STRING]
        for c in string_cols:
            if len(out[c]):
                out[c] = self._map_strings(rows, out[c])
        return out

    def kinds_of(self, rows):
        return [self.eng.lib.nbg_rows_col_kind(rows.h, c) for c in range(self.eng.lib.nbg_rows_num_cols(rows.h))]

    def segments(self, rows):
        """The result's row ranges as (first fetched row, rows) in fetch order, empty ones left out."""
        lib, out, at = self.eng.lib, [], 0
        b, e = C.c_uint64(), C.c_uint64()
        for i in range(lib.nbg_rows_num_segments(rows.h)):
            assert lib.nbg_rows_segment(rows.h, i, C.byref(b), C.byref(e)) == 0
            if e.value > b.value:
                out.append((at, e.value - b.value))
                at += e.value - b.value
        assert at == rows.count
        return out

    # -- device calls
    def go(self, sources=None):
        return self.eng.go_device(self.table.source_vids() if sources is None else list(sources), [E_TYPE], 1, b"",
                                  self.yields)

    def by_pos(self, rows):
        """ORDER BY pos: one segment whose physical row i is the i-th smallest pos of `rows`."""
        out = self.eng.order_by(rows, self.names, [("pos", False)])
        assert self.eng.lib.nbg_rows_num_segments(out.h) == 1 and out.count == rows.count
        return out

    def order(self, rows, factors, limit=None):
        out = self.eng.order_by(rows, self.names, factors, limit)
        try:
            assert out.count == 0 or self.eng.lib.nbg_rows_num_segments(out.h) == 1
            return self.bits_of(out)
        finally:
            out.free()

    def group_rows(self, rows, keys, aggs):
        """nbg_group_by with the key columns yielded first, then `aggs` = [(fun, column or None)]
        (None: COUNT(*)); without keys the group list is the constant abs(5).  A DeviceRows."""
        groups = [E.input_prop(k).encode() for k in keys] or [E.Expr(E.K_FUNC, alias="abs", args=[E.const(5)]).encode()]
        ys = [("", E.input_prop(k).encode(), k) for k in keys]
        ys += [(f, (E.const("*") if c is None else E.input_prop(c)).encode(), None) for f, c in aggs]
        return self.eng.group_by(rows, self.names, groups, ys)

    def group(self, rows, keys, aggs):
        """(bit columns in yield order, their NBG_V_* kinds) of group_rows; string-valued columns
        (a STRING key, MAX / MIN of the STRING column) as the table's ranks."""
        out = self.group_rows(rows, keys, aggs)
        try:
            names = [f"c{i}" for i in range(len(keys) + len(aggs))]
            spec = [("", k) for k in keys] + list(aggs)
            strs = [n for n, (f, c) in zip(names, spec)
                    if c is not None and self.table.types[c] == STRING and f in ("", "MAX", "MIN")]
            cols = self.bits_of(out, names, strs)
            return [cols[n] for n in names], self.kinds_of(out)
        finally:
            out.free()


def _check_is_table(table: Table, cols: dict, rows=None):
    """The fetched columns are the table's rows (those of `rows`), as a multiset: `pos` is unique,
    so sorted by it the columns are equal bit for bit."""
    idx = np.arange(table.n) if rows is None else np.asarray(rows)
    o = np.argsort(cols["pos"], kind="stable")
    assert len(o) == len(idx) and np.array_equal(cols["pos"][o], np.sort(idx)), "the rows' pos differ from the table's"
    for c in table.names:
        want = table.bits[c][np.sort(idx)]
        bad = np.nonzero(cols[c][o] != want)[0]
        assert not len(bad), (f"column {c}: row pos {np.sort(idx)[bad[:5]]} holds {cols[c][o][bad[:5]]}, "
                              f"the table {want[bad[:5]]}")


T_SCHEMA = [("name", kvgen.STRING)]


def value_records(table: Table, parts: int = 3):
    """(KVBuilder, edge schema) of the table's records."""
    schema = [(c, KV_TYPE[table.types[c]]) for c in table.names if table.types[c] not in (VID, STRING)]
    kb = kvgen.KVBuilder(parts)
    now = 1_600_000_000_000_000
    dst = table.dst().tolist()
    if table.str_col:
        names = dict(zip(dst, table.bits[table.str_col].tolist()))
        for v, s in names.items():
            kb.insert_vertex(v, TAG, T_SCHEMA, [table.strings[s]], now)
    cells = []
    for c, _ in schema:
        if table.types[c] == DOUBLE:
            vals = [dval(b) for b in table.bits[c].tolist()]
            assert [dbits(v) for v in vals] == (table.bits[c].view(np.uint64)).tolist()   # NaN payloads survive
            cells.append(vals)
        else:
            cells.append(table.bits[c].tolist())
    for r, (s, d) in enumerate(zip(table.src.tolist(), dst)):
        kb.insert_edge(SRC0 + s, d, E_TYPE, r, schema, [col[r] for col in cells], now + 1)    # rank r: no duplicate keys
    return kb, schema


def load_oracle(table: Table, kb, schema, parts: int = 3) -> "Loaded":
    """The records in the CPU Oracle alone (no device): its GO's rows are asserted to be the table."""
    orc = Oracle(parts)
    orc.register(True, E_TYPE, "e", schema)
    if table.str_col:
        orc.register(False, TAG, "t", T_SCHEMA)
    orc.load_builder(kb)
    ld = Loaded(table, None, orc)
    _check_is_table(table, oracle_bits(ld))
    return ld


def load_value_table(table: Table, parts: int = 3) -> Loaded:
    """The table as KV records in an Engine and (the same records) in the CPU Oracle."""
    kb, schema = value_records(table, parts)
    ld = load_oracle(table, kb, schema, parts)
    eng = Engine(parts)
    eng.register_edge(E_TYPE, "e", schema)
    if table.str_col:
        eng.register_tag(TAG, "t", T_SCHEMA)
    eng.load_builder(kb)
    ld.eng = eng
    return ld


def oracle_bits(ld: Loaded, sources=None):
    """The CPU oracle's rows of the same GO as {column: bits} (strings as the table's ranks)."""
    t = ld.table
    got = ld.orc.go(t.source_vids() if sources is None else list(sources), [E_TYPE], 1, b"", ld.yields)
    rank = {s.decode(): i for i, s in enumerate(t.strings)}
    out = {}
    for k, c in enumerate(ld.names):
        vals = [r[k] for r in got]
        ty = t.types[c]
        if ty == DOUBLE:
            assert all(isinstance(v, float) for v in vals)
            out[c] = np.array([dbits(v) for v in vals], np.uint64).view(np.int64)
        elif ty == STRING:
            out[c] = np.array([rank[v] for v in vals], np.int64)
        elif ty == BOOL:
            assert all(isinstance(v, bool) for v in vals)
            out[c] = np.array(vals, np.int64)
        else:
            assert all(type(v) is int for v in vals)
            out[c] = np.array(vals, np.int64)
    return out


def load_numeric_table(table: Table, parts: int = 1) -> Loaded:
    """The table through Engine.load_edges: numpy arrays only."""
    assert not table.str_col
    cols = [c for c in table.names if table.types[c] != VID]
    schema = [(c, KV_TYPE[table.types[c]]) for c in cols]
    props = []
    for c in cols:
        b = table.bits[c]
        props.append(b.view(np.float64) if table.types[c] == DOUBLE else b.astype(np.uint8) if table.types[c] == BOOL else b)
    eng = Engine(parts)
    eng.register_edge(E_TYPE, "e", schema)
    rank = table.bits["pos"] if table.vid_col else None      # (a VID column repeats destinations)
    eng.load_edges(E_TYPE, SRC0 + table.src, table.dst(), props, rank)
    eng.finalize()
    return Loaded(table, eng, None)


def go_checked(ld: Loaded, rows_idx=None):
    """(DeviceRows, its bit columns) of the GO from the sources of `rows_idx` (default: every row),
    asserted to be exactly those table rows."""
    srcs = ld.table.source_vids(rows_idx)
    rows = ld.go(srcs)
    cols = ld.bits_of(rows)
    if rows_idx is None:
        _check_is_table(ld.table, cols)
    else:
        _check_is_table(ld.table, cols, np.nonzero(np.isin(ld.table.src, np.unique(ld.table.src[rows_idx])))[0])
    return rows, cols


# ------------------------------------------------------------------------------------ reference: order
def fold_zero(bits: np.ndarray, t: str) -> np.ndarray:
    """A DOUBLE cell with -0.0 as 0.0 (operator== makes them equal); everything else as it is."""
    if t != DOUBLE:
        return bits
    u = bits.view(np.uint64)
    return np.where(u == SIGN, np.uint64(0), u).view(np.int64)


def order_key(bits: np.ndarray, t: str, desc: bool = False) -> np.ndarray:
    """uint64 keys whose unsigned order is the column's order and whose equality is operator==:
    signed order for ints; IEEE order for doubles with the zeros equal and a NaN by the total-order
    image of its bits (a negative NaN below -inf, a positive one above +inf); false < true; strings
    by their rank under unsigned bytes."""
    u = np.ascontiguousarray(bits).view(np.uint64)
    if t == DOUBLE:
        u = fold_zero(bits, t).view(np.uint64)
        k = np.where((u & SIGN) != 0, ~u, u | SIGN)
    elif t in INT_LIKE:
        k = u ^ SIGN
    else:
        k = u.copy()
    return ~k if desc else k


def order_unkey(k: np.ndarray, t: str) -> np.ndarray:
    """The cell of an ascending order_key (a zero comes back as 0.0)."""
    if t == DOUBLE:
        return np.where((k & SIGN) != 0, k & ~SIGN, ~k).view(np.int64)
    if t in INT_LIKE:
        return (k ^ SIGN).view(np.int64)
    return k.view(np.int64)


def order_ref(table: Table, factors, rows=None) -> np.ndarray:
    """Table row indices in ORDER BY order (rows equal under every factor: in table order).  A
    stable sort by the first factor, then each later factor re-sorts only the rows that still
    tie — np.lexsort's result, without sorting millions of already distinct rows again."""
    idx = np.arange(table.n) if rows is None else np.asarray(rows)
    if not factors or not len(idx):
        return idx
    keys = [order_key(table.bits[c][idx], table.types[c], desc) for c, desc in factors]
    if len(keys) <= 2:
        return idx[np.lexsort(tuple(reversed(keys)))]
    perm = np.argsort(keys[0], kind="stable")
    new = np.ones(len(idx), bool)                      # a row that starts a run of equal keys so far
    new[1:] = keys[0][perm][1:] != keys[0][perm][:-1]
    for k in keys[1:]:
        starts = np.nonzero(new)[0]
        tied = np.repeat(np.diff(np.append(starts, len(idx))) > 1, np.diff(np.append(starts, len(idx))))
        sub = np.nonzero(tied)[0]
        if not len(sub):
            break
        run = np.cumsum(new)[sub]
        o = np.lexsort((k[perm[sub]], run))            # (stable: rows that still tie keep table order)
        perm[sub] = perm[sub][o]
        ks = k[perm[sub]]
        new[sub[1:]] |= (ks[1:] != ks[:-1]) & (run[1:] == run[:-1])
    return idx[perm]


def window_ref(rows: int, offset: int, count: int):
    """[lo, hi) of `LIMIT offset, count` over `rows` rows; offset + count saturates at INT64_MAX."""
    assert offset >= 0 and count >= 0
    if count == 0 or rows <= offset:
        return 0, 0
    return offset, min(rows, min(offset + count, INT64_MAX))


def check_order(dev: dict, table: Table, factors, limit=None, rows=None, exact=False):
    """orderby.check_window over bit columns.  The device's factor-key sequence is the window of
    order_ref's; every device row is a table row, bit for bit, and no row comes twice (`pos` is
    unique) — so the rows of a key wholly inside the window are the input's as a multiset and those
    of a key the window's edge cuts are a sub-multiset.  exact: the rows are order_ref's, in order."""
    perm = order_ref(table, factors, rows)
    lo, hi = window_ref(len(perm), *limit) if limit is not None else (0, len(perm))
    want = perm[lo:hi]
    assert len(dev["pos"]) == len(want), f"{len(dev['pos'])} rows, the window holds {len(want)}"
    for c, desc in factors:
        got_k, want_k = order_key(dev[c], table.types[c], desc), order_key(table.bits[c][want], table.types[c], desc)
        bad = np.nonzero(got_k != want_k)[0]
        assert not len(bad), (f"factor {c}: first difference at result row {bad[0]}: {dev[c][bad[0]]:#x} != "
                              f"{table.bits[c][want][bad[0]]:#x}")
    pos = dev["pos"]
    member, seen = np.zeros(table.n, bool), np.zeros(table.n, bool)
    member[np.arange(table.n) if rows is None else np.asarray(rows)] = True
    assert ((pos >= 0) & (pos < table.n)).all() and member[pos].all(), "a row that is not of the input"
    seen[pos] = True
    assert seen.sum() == len(pos), "a row twice"
    for c in table.names:
        assert np.array_equal(dev[c], table.bits[c][pos]), f"column {c} differs from the input row of the same pos"
    if exact:
        assert np.array_equal(pos, want)


# ------------------------------------------------------------------------------------ reference: groups
class RefCol:
    """One expected aggregate column: `bits` per group; kind; how to compare: 'exact', 'zero'
    (doubles, the zeros' sign folded), 'abs' (|dev - ref| <= tol, the class where ref is not finite)
    or 'rel' (|dev - ref| <= tol * |ref|)."""

    def __init__(self, bits, kind, how="exact", tol=None):
        self.bits, self.kind, self.how, self.tol = np.asarray(bits, np.int64), kind, how, tol


class GroupRef:
    def __init__(self, keys, cols, count):
        self.keys, self.cols, self.count = keys, cols, count     # keys: folded bits per key column
        self.n = len(count)


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def sum_ref(vals: Sequence[float]):
    """(the exactly rounded sum, a bound for any recursive summation's distance from it).  A group
    with a NaN, or with infinities of both signs, sums to NaN; with infinities of one sign, to that
    infinity (whatever the order, provided no finite partial sum overflows: the caller's groups).
    Finite: |s - fsum| <= gamma_{n-1} * sum|x_i|, gamma_k = k u / (1 - k u), u = 2^-53 (Higham,
    Accuracy and Stability of Numerical Algorithms, §4.2: any order of recursive summation)."""
    if any(math.isnan(v) for v in vals):
        return math.nan, 0.0
    pinf, ninf = any(v == math.inf for v in vals), any(v == -math.inf for v in vals)
    if pinf or ninf:
        return (math.nan if pinf and ninf else math.inf if pinf else -math.inf), 0.0
    if all(dbits(v) == 1 << 63 for v in vals):       # -0.0 + -0.0 is -0.0 (fsum answers 0.0)
        return -0.0, 0.0
    return math.fsum(vals), gamma(len(vals) - 1) * math.fsum(abs(v) for v in vals)


def group_ref(table: Table, keys, aggs, rows=None) -> GroupRef:
    """GROUP BY keys YIELD keys, aggs over the table rows `rows` (default: all).  aggs: [(fun,
    column or None)].  Group identity: the key cells' payloads, -0.0 folded into 0.0 in DOUBLE
    columns, NaNs by their bits."""
    idx = np.arange(table.n) if rows is None else np.asarray(rows)
    m = len(idx)
    kb = [fold_zero(table.bits[k][idx], table.types[k]) for k in keys]
    if keys:
        o = np.lexsort(tuple(reversed(kb)))
        new = np.zeros(m, bool)
        new[0] = True
        for b in kb:
            new[1:] |= b[o][1:] != b[o][:-1]
        starts = np.nonzero(new)[0]
    else:
        o, starts = np.arange(m), np.array([0])
    G = len(starts)
    count = np.diff(np.append(starts, m)).astype(np.int64)
    gid = np.repeat(np.arange(G), count)                   # of the sorted rows
    cols = []
    zeros = np.zeros(G, np.int64)
    for fun, c in aggs:
        fun = fun.upper()
        if fun == "COUNT":
            cols.append(RefCol(count, L.V_INT))
            continue
        t = table.types[c]
        v = table.bits[c][idx][o]
        if fun == "COUNT_DISTINCT":
            f = fold_zero(v, t)
            o2 = np.lexsort((f, gid))
            g2, f2 = gid[o2], f[o2]
            first = np.ones(m, bool)
            first[1:] = (g2[1:] != g2[:-1]) | (f2[1:] != f2[:-1])
            cols.append(RefCol(np.bincount(g2[first], minlength=G), L.V_INT))
        elif fun in ("SUM", "AVG") and t in INT_LIKE:
            s = np.add.reduceat(v.view(np.uint64), starts).view(np.int64)        # wraps
            if fun == "SUM":
                cols.append(RefCol(s, L.V_INT))
            else:
                assert t == INT, "AVG over a VID or TIMESTAMP column is NBG_E_UNSUPPORTED"
                cols.append(RefCol((s.astype(np.float64) / count).view(np.int64), L.V_DOUBLE))
        elif fun in ("SUM", "AVG") and t == DOUBLE:
            x = v.view(np.float64)
            out, tol = np.zeros(G), np.zeros(G)
            for g in range(G):
                out[g], tol[g] = sum_ref(x[starts[g]:starts[g] + count[g]].tolist())
            if fun == "AVG":
                # fl(a / n) and fl(b / n) with |a - b| <= tol: the quotients are tol / n apart and
                # each division rounds by at most u times its result (or half a subnormal step)
                with np.errstate(invalid="ignore"):
                    out = out / count
                    tol = tol / count
                    tol = tol + 2 * U * (np.abs(np.where(np.isfinite(out), out, 0.0)) + tol) + 5e-324
            cols.append(RefCol(out.view(np.int64), L.V_DOUBLE, "abs", tol))
        elif fun == "SUM":
            cols.append(RefCol(zeros, L.V_INT))
        elif fun == "AVG":
            cols.append(RefCol(np.zeros(G).view(np.int64), L.V_DOUBLE))
        elif fun in ("MAX", "MIN"):
            k = order_key(v, t)
            r = (np.maximum if fun == "MAX" else np.minimum).reduceat(k, starts)
            cols.append(RefCol(order_unkey(r, t), KIND[t], "zero" if t == DOUBLE else "exact"))
        elif fun == "STD":
            if t not in (INT, DOUBLE):
                cols.append(RefCol(zeros, L.V_INT))
                continue
            x = v.view(np.float64) if t == DOUBLE else v.astype(np.float64)
            if t == INT:
                avg = np.add.reduceat(v.view(np.uint64), starts).view(np.int64).astype(np.float64) / count
            else:
                avg = np.array([sum_ref(x[starts[g]:starts[g] + count[g]].tolist())[0] for g in range(G)]) / count
            d = x - avg[gid]
            std = np.sqrt(np.add.reduceat(d * d, starts) / count)
            cols.append(RefCol(std.view(np.int64), L.V_DOUBLE, "rel", count * 2.0 ** -52))
        elif fun in ("BIT_AND", "BIT_OR", "BIT_XOR"):
            if t != INT:
                cols.append(RefCol(zeros, L.V_INT))
                continue
            op = {"BIT_AND": np.bitwise_and, "BIT_OR": np.bitwise_or, "BIT_XOR": np.bitwise_xor}[fun]
            cols.append(RefCol(op.reduceat(v, starts), L.V_INT))
        else:
            raise ValueError(fun)
    return GroupRef([b[o][starts] for b in kb], cols, count)


def check_groups(dev_cols, dev_kinds, table: Table, keys, ref: GroupRef, what=""):
    """The device's groups are the reference's: the same keys (zeros folded), and per group every
    aggregate as its RefCol says.  Device rows come in any order."""
    nk = len(keys)
    assert len(dev_cols) == nk + len(ref.cols)
    assert len(dev_cols[0]) == ref.n, f"{what}: {len(dev_cols[0])} groups, the reference has {ref.n}"
    dk = [fold_zero(dev_cols[i], table.types[k]) for i, k in enumerate(keys)]
    for i, k in enumerate(keys):
        assert dev_kinds[i] == KIND[table.types[k]], (what, k, dev_kinds[i])
    if nk:
        od, orf = np.lexsort(tuple(reversed(dk))), np.lexsort(tuple(reversed(ref.keys)))
        for a, b, k in zip(dk, ref.keys, keys):
            assert np.array_equal(a[od], b[orf]), f"{what}: the groups' {k} keys differ"
    else:
        od = orf = np.arange(1)
    for j, rc in enumerate(ref.cols):
        got, want = dev_cols[nk + j][od], rc.bits[orf]
        assert dev_kinds[nk + j] == rc.kind, (what, j, dev_kinds[nk + j], rc.kind)
        if rc.how == "zero":
            got, want = fold_zero(got, DOUBLE), fold_zero(want, DOUBLE)
        if rc.how in ("exact", "zero"):
            bad = np.nonzero(got != want)[0]
            assert not len(bad), f"{what}: aggregate {j}: {len(bad)} groups differ, first {got[bad[0]]:#x} != {want[bad[0]]:#x}" \
                                 f" (keys {[int(b[orf][bad[0]]) for b in ref.keys]})"
            continue
        g, w = got.view(np.float64), want.view(np.float64)
        tol = np.broadcast_to(np.asarray(rc.tol, np.float64), w.shape)[orf] if np.ndim(rc.tol) else np.full(w.shape, rc.tol)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: aggregate {j}: NaN in other groups than the reference"
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), f"{what}: aggregate {j}: infinities differ"
        with np.errstate(invalid="ignore", over="ignore"):
            err = np.abs(g[fin] - w[fin])
            bound = tol[fin] * (np.abs(w[fin]) if rc.how == "rel" else 1.0)
        assert np.isfinite(g[fin]).all() and (err <= bound).all(), \
            (f"{what}: aggregate {j}: error {err.max() if len(err) else 0} over the bound "
             f"{bound[np.argmax(err - bound)] if len(err) else 0}")


# ------------------------------------------------------------------------------------ the value table
INT_SPECIALS = [INT64_MIN, INT64_MIN + 1, -(1 << 53) - 1, -(1 << 32), -(1 << 31) - 1, -1, 0, 1, (1 << 31) - 1, 1 << 31,
                1 << 32, (1 << 53) + 1, INT64_MAX - 1, INT64_MAX]
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF]
LOWEST_NAN, HIGHEST_NAN = 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000001      # by the total-order image
_POS = [0x0000000000000000, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x3FF0000000000000,
        0x3FF0000000000001, 0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000]
# (0, 5e-324, the largest subnormal, DBL_MIN, 1, 1 + 2^-52, DBL_MAX, inf; and their negatives)
DOUBLE_SPECIALS = _POS + [p | (1 << 63) for p in _POS]
VIDS = [INT64_MIN, -1, 1, INT64_MAX, -77, 1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009, 1010]
STRS = [b"", b"a", b"ab", b"abc", b"B", b"~", b"\x7f", "é".encode(), b"\xf0\x9f\x98\x80"]
LADDER_DIGITS = (0x00, 0x01, 0x7F, 0x80, 0xFF)
G_SPECIAL, G_FINITE, G_WRAP_MAX, G_WRAP_MIN, G_EXACT = 0, 300, 101, 102, 400
EXTRA_SRC0 = 1000


def ladder_images(j: int):
    """Family j of the byte ladder, as images (unsigned order; the INT cell is image ^ 2^63): equal
    in every byte above j, differing first — and only — at byte j, with members in bins 0x00 and
    0xFF of that byte.  The top byte (1 + j) keeps the families at the low end of the order and
    apart from each other; family 7 differs at the top byte itself."""
    if j == 7:
        return [(d << 56) | 0x0033333333333333 for d in (0x09, 0x0A, 0x0B)]
    hi = ((1 + j) << 56) | (0x0033333333333333 & ~((1 << (8 * (j + 1))) - 1))
    lo = 0xA5A5A5A5A5A5A5A5 & ((1 << (8 * j)) - 1)
    return [hi | (d << (8 * j)) | lo for d in LADDER_DIGITS]


def ladder_cells(high: bool):
    """The ladder's INT cells at the low end of the signed order, or mirrored (every image
    complemented) at its high end."""
    out = []
    for j in range(8):
        for img in ladder_images(j):
            img = (~img) & ((1 << 64) - 1) if high else img
            v = img ^ (1 << 63)
            out.append(v - (1 << 64) if v >= 1 << 63 else v)
    return out


def value_table(nan: bool = True, rows: int = 2400, seed: int = 5, per_src: Optional[int] = None) -> Table:
    """The value-domain table: i (INT: the extremes, a byte ladder at either end of the order, full-
    range filler between), x (DOUBLE bit patterns: every special of both signs and the NaNs, finite
    filler), d (VID, both signs and the extremes), s (STRING, a function of d), t (TIMESTAMP), b
    (BOOL), z (DOUBLE, zeros of both signs only), c (a constant INT) and g (INT group labels:
    G_SPECIAL for a row whose x is a special, G_FINITE + 0..2 for finite filler, and the small
    dedicated groups appended at the end).  Every special is present three times.  nan=False: the
    NaN cells are ordinary values (for the plain-Python models, whose max() / sort break on NaN).
    per_src: that many consecutive rows per source instead of the layout below (1: row `pos` is the
    only out-edge of source SRC0 + pos)."""
    rng = np.random.default_rng(seed)
    reps = 3
    u64 = (1 << 64) - 1
    i_fixed = (INT_SPECIALS + ladder_cells(False) + ladder_cells(True)) * reps
    # filler: images with a top byte in [0x10, 0xEF] — between the two ladder blocks
    img = (rng.integers(0x10, 0xF0, rows - len(i_fixed)).astype(np.uint64) << np.uint64(56)) | \
        (rng.integers(0, 1 << 56, rows - len(i_fixed)).astype(np.uint64))
    i_col = np.concatenate([np.array(i_fixed, np.int64), (img ^ SIGN).view(np.int64)])
    x_fixed = (DOUBLE_SPECIALS + (NANS if nan else [dbits(2.5 + k) for k in range(len(NANS))])) * reps
    nfill = rows - len(x_fixed)
    mant = rng.integers(-(1 << 40), 1 << 40, nfill).astype(np.float64)
    x_fill = mant * np.exp2(rng.integers(-60, 20, nfill).astype(np.float64))          # finite, both signs, inexact sums
    x_col = np.concatenate([np.array(x_fixed, np.uint64), x_fill.view(np.uint64)])
    g_col = np.concatenate([np.full(len(x_fixed), G_SPECIAL), G_FINITE + np.arange(nfill) % 3])
    px = rng.permutation(rows)
    i_col, x_col, g_col = i_col[rng.permutation(rows)], x_col[px], g_col[px]
    vid_ix = np.concatenate([np.arange(len(VIDS)).repeat(reps), rng.integers(0, len(VIDS), rows - reps * len(VIDS))])
    vid_ix = vid_ix[rng.permutation(rows)]
    t_col = rng.integers(0, 1 << 40, rows)
    t_col[::50] += 1 << 62                                                           # a SUM of these wraps
    b_col = rng.integers(0, 2, rows)
    z_col = np.where(rng.integers(0, 2, rows) == 1, np.uint64(1 << 63), np.uint64(0))
    # the dedicated groups: (g, i, x)
    one = dbits(1.0)
    extra = [(G_WRAP_MAX, INT64_MAX, one), (G_WRAP_MAX, INT64_MAX, one), (G_WRAP_MAX, 2, one),
             (G_WRAP_MIN, INT64_MIN, one), (G_WRAP_MIN, -1, one)]
    inf, ninf = dbits(math.inf), dbits(-math.inf)
    dbl_groups = {
        201: [inf, dbits(1.0), dbits(-3.5)],                      # +inf
        202: [inf, ninf, dbits(1.0)],                             # inf + -inf: NaN in any order
        203: [HIGHEST_NAN if nan else dbits(7.0), dbits(1.0)],    # a NaN
        204: [ninf, ninf, dbits(5.0)],                            # -inf
        205: [1, 1, 1, 1 | (1 << 63)],                            # subnormals: 3 * 5e-324 - 5e-324
        206: [0, 1 << 63, 1 << 63],                               # zeros of both signs
        207: [1 << 63, 1 << 63],                                  # only -0.0: the double SUM's identity
        208: [dbits(v) for v in (0.1, 0.2, 0.3, 1e16, -1e16, 1e-3, 7.0, -0.7)],
    }
    for g, xs in dbl_groups.items():
        extra += [(g, 10 + k, xb) for k, xb in enumerate(xs)]
    extra += [(G_EXACT, 3 * k - 40, dbits(k / 8.0)) for k in range(40)]                # exact double sums
    ne = len(extra)
    cols = [
        ("i", INT, np.concatenate([i_col, np.array([e[1] for e in extra], np.int64)])),
        ("x", DOUBLE, np.concatenate([x_col, np.array([e[2] & u64 for e in extra], np.uint64)])),
        ("d", VID, np.array([VIDS[k] for k in np.concatenate([vid_ix, np.arange(ne) % len(VIDS)])], np.int64)),
        ("s", STRING, [STRS[k % len(STRS)] for k in np.concatenate([vid_ix, np.arange(ne) % len(VIDS)])]),
        ("t", TIMESTAMP, np.concatenate([t_col, np.arange(ne)])),
        ("b", BOOL, np.concatenate([b_col, np.arange(ne) % 2])),
        ("z", DOUBLE, np.concatenate([z_col, np.zeros(ne, np.uint64)])),
        ("c", INT, np.full(rows + ne, 7)),
        ("g", INT, np.concatenate([g_col, np.array([e[0] for e in extra], np.int64)])),
    ]
    if per_src is not None:
        return Table(cols, per_src=per_src)
    # 61 rows per source; every dedicated group has a source of its own (EXTRA_SRC0 + g)
    return Table(cols, src=np.concatenate([np.arange(rows) // 61, EXTRA_SRC0 + np.array([e[0] for e in extra])]))


# ------------------------------------------------------------------------------------ Python rows as bit columns
def cells_to_bits(table: Table, vals: list):
    """(bits, NBG_V_* kind) of one column of Python cells (a model's output): the kind from the
    cells' Python type, strings as the table's ranks."""
    v0 = vals[0]
    if isinstance(v0, bool):
        assert all(isinstance(v, bool) for v in vals)
        return np.array(vals, np.int64), L.V_BOOL
    if isinstance(v0, float):
        assert all(isinstance(v, float) for v in vals)
        return np.array([dbits(v) for v in vals], np.uint64).view(np.int64), L.V_DOUBLE
    if isinstance(v0, str):
        rank = {s.decode(): i for i, s in enumerate(table.strings)}
        return np.array([rank[v] for v in vals], np.int64), L.V_STRING
    assert all(type(v) is int for v in vals)
    return np.array(vals, np.int64), L.V_INT


def rows_to_bits(table: Table, rows: list, ncols: int):
    """A model's rows as (bit columns, kinds)."""
    cols = [cells_to_bits(table, [r[c] for r in rows]) for c in range(ncols)]
    return [c[0] for c in cols], [c[1] for c in cols]
