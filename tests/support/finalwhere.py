"""The final step's `WHERE <int col> <cmp> <const>` at the ends of the column widths, on every
route a GO statement can take to its final step: the graph, the constants, a numpy model and the
table of routes shared by tests/test_final_where_model.py (model against the storage oracle, no
GPU) and tests/test_gpu_final_where.py (every route against the model).

Graph (one edge type `e`, four INT props a8 / a16 / a32 / a64; `Graph`): a root R with one edge to
each of 10 mid vertices of out-degree 0, 1, 2, 63, 64, 65, 255, 256, 257, 700 (wave, tile, 2-tile
edges, a hub), every final edge to a destination of its own, so `_dst` names the row.  a8, a16 and
a32 hold cells over the whole range of their width, among them min, min + 1, -1, 0, 1, 5, max - 1
and max; a64 spans int64 and also holds the cells around the int32 ends and 2^32 + 5, -2^32 + 5
(low 32 bits 5: a truncated compare takes them for 5).  The R -> mid edges carry 0.  Both loaders
choose a column's stored width from its min and max (1, 2, 4 bytes, none for a64); the width is
not observable through the ABI, so test_final_where_model.py pins the columns' min and max.  A
second root R2 with mids of degree 1, 2, 40 is small enough for the one-launch path.

Model: `col <op> k` in numpy over the edge arrays, the operator mirrored for `k <op> col`; it never
forms the lo / hi range detect_fast (kernels.hip) rewrites the comparison into.  The WHERE filters
the final step only: `GO 2 STEPS FROM R` and `GO FROM <mids>` both return the final edges whose
cell passes, and the per-step statistics (step_model) do not depend on it.

Routes.  ws_expand_final (kernels.hip) picks the final step's kernel from the statement's shape:
  * YIELDs all `_dst` / constants and a WHERE of the 3-instruction shape (or none) is FINALD-shaped:
      - a start list of <= 32 entries consumed by the final step itself (1 step) travels inline:
        k_expand<FINALD, INL>                                                     -> inline_dst
      - else k_final_dst<WB, ONE> (final.hip), WB the WHERE column's stored width, ONE for the
        single `_dst` YIELD                                          -> lean_dst, lean_dst_const
      - a prepared statement of this shape (>= 2 steps) builds its filtered adjacency (stmtidx.hip,
        Pass<T> evaluates the WHERE) and then runs with no WHERE left: k_final_copy for the single
        `_dst` YIELD, k_final_dst<0> under NBG_FINAL_COPY=0 or with more YIELDs
                                                                          -> index_copy, index_dst
  * YIELDs that are also plain columns: k_expand<FINALF>, or k_expand<FINALY> with >= 4 YIELDs over
    a small expansion (list and inline start list alike)                  -> fast_cols, wide_cols
  * any other WHERE: the interpreter over the 8-byte columns, k_expand<FINAL>        -> interp
  * host rows of a tiny walk: one launch, k_go_tiny (go.cpp tiny_type)                -> tiny
NBG_FINAL_LEAN=0 (k_expand<FINALD> from a device list instead of k_final_dst) is read once per
process through a static, so a test cannot switch it: that route is left out.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from nebula_amd import expr as E, kvgen
from tests.test_gpu_final_copy import final_copy_unset, nonempty_segments
from tests.test_gpu_stmt_index import env, prepare, step_model, where

E_TYPE = 1
COLUMNS = ("a8", "a16", "a32", "a64")
BITS = {"a8": 8, "a16": 16, "a32": 32, "a64": 64}
SCHEMA = [(c, kvgen.INT) for c in COLUMNS]
OPS = ("<", "<=", ">", ">=", "==", "!=")
MIRROR = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "==": "==", "!=": "!="}
_NP = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal, "==": np.equal,
       "!=": np.not_equal}

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
LOW5 = 2 ** 32 + 5     # low 32 bits equal the cell 5

R, R2 = 1, 2
MIDS = tuple(range(100, 110))
DEGS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 700)
MIDS2 = (200, 201, 202)
DEGS2 = (1, 2, 40)
LEAF = 5_000_000
SEED = 20240607


def width_range(col):
    b = BITS[col]
    return -2 ** (b - 1), 2 ** (b - 1) - 1


def base_cells(col):
    """The cells every column holds whatever the seed."""
    lo, hi = width_range(col)
    cells = [lo, lo + 1, -1, 0, 1, 5, hi - 1, hi]
    if col == "a64":
        cells += [I32_MIN - 1, I32_MIN, I32_MAX, I32_MAX + 1, LOW5, -2 ** 32 + 5]
    return cells


def _fits(k):
    return I64_MIN <= k <= I64_MAX


def width_edge_constants(col):
    """min_b - 1 ... max_b + 1 and the int32 and int64 extremes (what fits int64)."""
    lo, hi = width_range(col)
    ks = [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, I32_MIN - 1, I32_MIN, I32_MAX, I32_MAX + 1,
          I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX]
    return sorted({k for k in ks if _fits(k)})


def constants(col):
    """The WHERE constants of a column: 21, 21, 17 and 15 for a8, a16, a32, a64."""
    ks = width_edge_constants(col) + [-1, 0, 1, 5, 2 ** 32, -2 ** 32, LOW5]
    return sorted({k for k in ks if _fits(k)})


def cases(col, ks=None):
    """(op, constant, constant on the left) of every WHERE of a column."""
    return [(op, k, left) for k in (constants(col) if ks is None else ks) for op in OPS for left in (False, True)]


def where_bytes(col, op, k, left=False, interp=False):
    wb = where(op, k, const_left=left, col=col)
    if not interp:
        return wb
    # (col <op> k) && e.a8 >= -128: true for every a8 cell, and not the 3-instruction shape
    rel = E.binop(op, E.const(int(k)), E.edge_prop("e", col)) if left else E.binop(op, E.edge_prop("e", col),
                                                                                   E.const(int(k)))
    return E.binop("&&", rel, E.binop(">=", E.edge_prop("e", "a8"), E.const(-128))).encode()


def yield_bytes(yields):
    return [E.const(y).encode() if isinstance(y, int) else E.edge_prop("e", y).encode() for y in yields]


class Graph:
    """The edge arrays, the model and the per-step statistics (see the module's docstring)."""

    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        n1, n2 = sum(DEGS), sum(DEGS2)
        nf, hops = n1 + n2, len(MIDS) + len(MIDS2)
        self.src = np.concatenate([np.full(len(MIDS), R), np.full(len(MIDS2), R2), np.repeat(MIDS, DEGS),
                                   np.repeat(MIDS2, DEGS2)]).astype(np.int64)
        self.dst = np.concatenate([MIDS, MIDS2, LEAF + np.arange(nf)]).astype(np.int64)
        # final edges of R's mids / of R2's mids, as indices into the edge arrays
        self.final = {"R": hops + np.arange(n1), "mids": hops + np.arange(n1), "R2": hops + n1 + np.arange(n2)}
        self.starts = {"R": [R], "mids": list(MIDS), "R2": [R2]}
        self.cols = {}
        for c in COLUMNS:
            lo, hi = width_range(c)
            base = np.array(base_cells(c), np.int64)
            big = rng.integers(lo, hi, size=n1, dtype=np.int64, endpoint=True)
            big[rng.choice(n1, len(base), replace=False)] = base
            small = rng.permutation(np.resize(base, n2))   # R2's final edges: the base cells only
            self.cols[c] = np.concatenate([np.zeros(hops, np.int64), big, small])
        self._stats = {}

    def props(self):
        return [self.cols[c] for c in COLUMNS]

    def passes(self, col, op, k, left=False):
        """The model: col <op> k over every edge (k <op> col: the mirrored operator)."""
        return _NP[MIRROR[op] if left else op](self.cols[col], np.int64(k))

    def rows(self, starts, yields, col=None, op=None, k=None, left=False):
        """Expected rows as an int64 array (rows, yields) in `_dst` order: the final edges reached
        from `starts` ("R", "mids" or "R2") whose cell passes (col None: no WHERE)."""
        idx = self.final[starts]
        if col is not None:
            idx = idx[self.passes(col, op, k, left)[idx]]
        out = [np.full(len(idx), y, np.int64) if isinstance(y, int) else
               (self.dst[idx] if y == "_dst" else self.cols[y][idx]) for y in yields]
        return np.stack(out, 1).reshape(len(idx), len(yields))

    def step_stats(self, starts, steps):
        key = (starts, steps)
        if key not in self._stats:
            self._stats[key] = step_model(self.src, self.dst, self.starts[starts], steps)
        return self._stats[key]

    def engine(self, parts=100):
        from nebula_amd import Engine
        e = Engine(parts)
        e.register_edge(E_TYPE, "e", SCHEMA)
        e.load_edges(E_TYPE, self.src, self.dst, self.props())
        e.finalize()
        return e

    def oracle(self, parts=100):
        from tests.support.oracle import Oracle
        o = Oracle(parts)
        o.register(True, E_TYPE, "e", SCHEMA)
        o.load_edges(E_TYPE, self.src, self.dst, self.props())
        o.finalize()
        return o

    def kv_engine(self, parts=7):
        """The same edges as KV records (the in-edge mirrors with them)."""
        from nebula_amd import Engine
        kb = kvgen.KVBuilder(parts)
        vals = np.stack(self.props(), 1).tolist()
        for s, d, v in zip(self.src.tolist(), self.dst.tolist(), vals):
            kb.insert_edge(s, d, E_TYPE, 0, SCHEMA, v, 1_600_000_000_000_000)
        e = Engine(parts)
        e.register_edge(E_TYPE, "e", SCHEMA)
        e.load_builder(kb)
        return e


# ------------------------------------------------------------------------------------ routes
@dataclass(frozen=True)
class Variant:
    """One way to run a route's statement."""
    steps: int
    starts: str                       # "R", "mids" (inline start list, 1 step) or "R2"
    yields: Tuple                     # "_dst", a column's name or an int constant per YIELD
    prepare_env: dict = field(default_factory=dict)   # switches around nbg_go_prepare
    run_env: dict = field(default_factory=dict)       # switches around the execution
    index: Optional[bool] = None      # the statement holds an index after the run / holds none
    one_segment: bool = False         # k_final_copy: one non-empty segment when rows exist
    interp: bool = False              # the WHERE is wrapped out of the 3-instruction shape
    tiny: bool = False                # eng.go host rows; stats()["tiny_queries"] must rise


@dataclass(frozen=True)
class Route:
    name: str
    kernel: str
    variants: Tuple[Variant, ...]


_NO_INDEX = {"NBG_STMT_INDEX": 0}
_INDEX = {"NBG_STMT_INDEX_AFTER": 0}
_ALL = ("_dst",) + COLUMNS
ROUTES = {r.name: r for r in (
    Route("inline_dst", "k_expand<FINALD, INL>", (Variant(1, "mids", ("_dst",)),)),
    Route("lean_dst", "k_final_dst<WB, one>", (Variant(2, "R", ("_dst",), _NO_INDEX, index=False),)),
    Route("lean_dst_const", "k_final_dst<WB, !one>",
          (Variant(2, "R", ("_dst", 7, "_dst"), _NO_INDEX, index=False),)),
    Route("index_copy", "Pass<T> + k_final_copy", (Variant(2, "R", ("_dst",), _INDEX, index=True, one_segment=True),)),
    Route("index_dst", "Pass<T> + k_final_dst<0>",
          (Variant(2, "R", ("_dst",), _INDEX, {"NBG_FINAL_COPY": 0}, index=True),
           Variant(2, "R", ("_dst", 7), _INDEX, index=True))),
    Route("fast_cols", "k_expand<FINALF>",
          (Variant(2, "R", ("_dst", "a8", "a64")), Variant(1, "mids", ("_dst", "a8", "a64")))),
    Route("wide_cols", "k_expand<FINALY>", (Variant(2, "R", _ALL), Variant(1, "mids", _ALL))),
    Route("interp", "k_expand<FINAL>", (Variant(2, "R", ("_dst", "a16"), interp=True),)),
    Route("tiny", "k_go_tiny", (Variant(2, "R2", ("_dst", "a32"), tiny=True),)),
)}


def _sorted(cols, ncols):
    a = np.stack(cols, 1).reshape(-1, ncols)
    return a[np.argsort(a[:, 0], kind="stable")]


def run_variant(g, eng, v, col=None, op=None, k=None, left=False):
    """Run one statement on `eng` and compare it with the model.  Returns the mismatches as a list
    of strings (empty: all as expected); a device error is raised, not collected.  Every statement
    and result is freed."""
    wb = b"" if col is None else where_bytes(col, op, k, left, v.interp)
    ys = yield_bytes(v.yields)
    exp = g.rows(v.starts, v.yields, col, op, k, left)
    fr, ed = g.step_stats(v.starts, v.steps)
    starts, bad = g.starts[v.starts], []
    if v.tiny:
        before = eng.stats()["tiny_queries"]
        with final_copy_unset():
            rows = eng.go(starts, [E_TYPE], v.steps, wb, ys)
        if eng.stats()["tiny_queries"] != before + 1:
            bad.append("not the one-launch path")
        got = _sorted([np.array([r[c] for r in rows], np.int64) for c in range(len(ys))], len(ys))
        stats, scanned = tuple(eng.last_step_stats[:2]), eng.last_step_stats[2]
    else:
        stmt = prepare(eng, v.steps, wb, ys, **v.prepare_env)
        try:
            with final_copy_unset(), env(**v.run_env):
                res = stmt.run_device(starts)
            try:
                got = _sorted(res.fetch_bits(), len(ys))
                stats, scanned = res.step_stats(), res.edges_scanned
                if v.one_segment and nonempty_segments(eng, res) != (1 if len(exp) else 0):
                    bad.append("segments %d" % nonempty_segments(eng, res))
            finally:
                res.free()
            if v.index is not None and (stmt.index_bytes() > 0) != v.index:
                bad.append("index_bytes %d" % stmt.index_bytes())
        finally:
            stmt.free()
    if got.shape != exp.shape or not np.array_equal(got, exp):
        bad.append("rows %d, model %d" % (len(got), len(exp)))
    if stats != (fr, ed) or scanned != sum(ed):
        bad.append("step stats %r scanned %d, model %r" % (stats, scanned, (fr, ed)))
    return bad


def run_route(g, eng, route, col, ks=None):
    """Every WHERE of a column (or those of the constants `ks`) through every variant of a route.
    Returns (statements run, mismatches as strings)."""
    bad, n = [], 0
    for v in ROUTES[route].variants:
        for op, k, left in cases(col, ks):
            n += 1
            for b in run_variant(g, eng, v, col, op, k, left):
                bad.append("%s %s: e.%s %s %d%s: %s" % (route, "/".join(map(str, v.yields)), col, op, k,
                                                        " (constant on the left)" if left else "", b))
    return n, bad
