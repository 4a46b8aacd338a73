"""nbg_go_piped on the MI355X: `| GO FROM $-.col` over device-resident rows.

Who judges what.  The rows of a piped call are judged by the storage oracle (tests/support/
oracle.py, pinned by the golden vectors of tests/test_oracle_golden.py): the input is fetched, and
`Oracle.go(starts = the fetched FROM column, ..., inputs = the fetched table)` over the same KV
records gives the expected rows, which compare as sorted rows, cell kinds included.  The oracle
shares nothing with the engine: not the OP_INPUT lookup, not the interpreter's typing of $- cells,
not the hop and final kernels, DISTINCT or the statistics.  The engine's other route to the same
statement (nbg_rows_fetch, then nbg_go with the fetched table as its $- input) is kept as a third
witness of the rows, and it is the reference for what the oracle does not report: the step
statistics, the edges scanned and the numeric status of an error (the oracle must fail too; its
code space is its own).  For one-step calls over type `e` alone the statistics are also counted
from the fixture's adjacency.  Where the reference's own answer is one of several ($- props after
two or more steps: the backtracker's roots), the root column is checked against the admissible sets
of tests/test_gpu_backtracker.py and the other columns against the oracle.  The 4 M-row input of
test_more_chunks_than_the_grid is judged by numpy.

The graph is a seeded RMAT-11 over 5 parts with type `e` (w INT, x DOUBLE, f FLOAT; each (src, dst)
once), a second type `r` (i INT, s STRING) over every fourth edge, tag `t` (name STRING) on nine
vertices of ten and tag `c` (pop INT) on every fourth.  The KV builder adds:
  * vertices -5, INT64_MIN and INT64_MAX, reachable from the first root and with out-edges of their own;
  * INVIS, reachable from the first root, whose own out-edge lies in another part than its hash part:
    the vertex is in the snapshot and invisible, so as a start it contributes no row;
  * FAN with an edge to each of 2,048 leaves that have exactly one out-edge each: a GO from FAN,
    doubled eleven times by UNION ALL and one row more, is an input of 2,048 * 2,048 + 1 rows (more
    chunks than STAGE_GRID workgroups) whose start list has exactly that many edges.

Two NBG_E_UNSUPPORTED cases of include/nbg.h have no test because no GO result reaches them: a FROM
or referenced column whose kind differs between OVER types, and an input of 2^32 rows."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

from nebula_amd import Engine, LocalCluster, NbgError, _lib as L, expr as E, kvgen, rmat
from nebula_amd.engine import DeviceRows
from tests.support import setops
from tests.support.oracle import Oracle, OracleError

pytestmark = pytest.mark.gpu

SEED, PARTS = 11, 5
NOW = 1_600_000_000_000_000
OB_CHUNK = 2048                       # csrc/nbg_internal.h: rows a workgroup walks per chunk
STAGE_GRID = 2048                     # csrc/stage.h: workgroups of a stage's launch
INLINE_STARTS = 32                    # csrc/nbg_internal.h: start lists up to this size are read back
E_SCHEMA = [("w", kvgen.INT), ("x", kvgen.DOUBLE), ("f", kvgen.FLOAT)]
R_SCHEMA = [("i", kvgen.INT), ("s", kvgen.STRING)]
T_SCHEMA = [("name", kvgen.STRING)]
C_SCHEMA = [("pop", kvgen.INT)]
IMIN, IMAX, NEG = -(1 << 63), (1 << 63) - 1, -5
INVIS, FAN, LEAF0, END0, NOWHERE = 15, 900_001, 1_000_000, 2_000_000, 123
GP_KERNELS = ("k_gp_resolve", "k_gp_table", "k_gp_degrees", "k_gp_emit", "k_gp_compact")

ep, ip = E.edge_prop, E.input_prop
ID_S_W = [ep("e", "_dst").encode(), ep("e", "_src").encode(), ep("e", "w").encode()]   # columns id, s, w
NAMES = ["id", "s", "w"]


class Fixture:
    pass


def _kv():
    src, dst, _ = rmat.rmat_edges(11, seed=SEED)
    rng = np.random.default_rng(SEED)
    w = rng.integers(-50, 50, len(src)).tolist()
    kb = kvgen.KVBuilder(PARTS)
    out = defaultdict(list)             # type e adjacency, each (src, dst) once
    seen = set()

    def add_e(s, d, a):
        if (s, d) in seen:
            return False
        seen.add((s, d))
        out[s].append(d)
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, [a, a / 8.0, 0.5], NOW + 1)
        return True
    for n, (s, d) in enumerate(zip(src.tolist(), dst.tolist())):
        if add_e(s, d, w[n]) and n % 4 == 0:
            kb.insert_edge(s, d, 2, 0, R_SCHEMA, [w[n] + 1, f"r{n % 7}"], NOW + 1)
    verts = sorted(set(src.tolist()) | set(dst.tolist()))
    # two roots whose two-step GO has between 6,000 and 20,000 rows (three chunks or more)
    def two_step(r):
        return sum(len(out[d]) for d in set(out[r]))
    cand = [v for v in verts if v % 10 and 15 <= len(out[v]) <= 60]
    roots = next([a, b] for a in cand for b in cand if a < b and 7000 <= two_step(a) + two_step(b) <= 16000)
    r0 = roots[0]
    for n, v in enumerate((NEG, IMIN, IMAX)):
        add_e(r0, v, 40 + n)
    # (the edge to INVIS without its in-edge mirror, which would be a second home part of INVIS)
    p0 = kvgen.part_of(r0, PARTS)
    kb.put(p0, kvgen.edge_key(p0, r0, 1, 0, INVIS, kvgen.version_of(NOW + 1)), kvgen.encode_row(E_SCHEMA, [43, 43 / 8.0, 0.5]))
    out[r0].append(INVIS)
    for n, v in enumerate((NEG, IMIN, IMAX)):
        add_e(v, verts[3 + n], n + 1)
        add_e(v, verts[9 + n], n - 7)
    wrong = kvgen.part_of(INVIS, PARTS) % PARTS + 1
    kb.put(wrong, kvgen.edge_key(wrong, INVIS, 1, 0, verts[5], kvgen.version_of(NOW)), kvgen.encode_row(E_SCHEMA, [2, 0.5, 0.5]))
    for i in range(OB_CHUNK):
        add_e(FAN, LEAF0 + i, i % 100)
        add_e(LEAF0 + i, END0 + i, i % 100 - 50)
    for v in verts + [NEG, IMIN, IMAX]:
        if v % 10:
            kb.insert_vertex(v, 7, T_SCHEMA, [f"n{v % 23}"], NOW)
        if v % 4 == 0:
            kb.insert_vertex(v, 8, C_SCHEMA, [v % 1000], NOW)
    return kb, out, verts, roots


@pytest.fixture(scope="module")
def ff():
    """The engine, the oracle over the same records and three inputs, computed once and left unchanged: `two` (a two-step GO of many
    short segments with the same vid in many rows), `one` (a one-step GO with INT, DOUBLE and STRING
    payload columns) and `fan` (2,048 rows, one per leaf)."""
    kb, out, verts, roots = _kv()
    f = Fixture()
    f.out, f.verts, f.roots = out, verts, roots
    f.vertset = set(verts) | {NEG, IMIN, IMAX, INVIS, FAN} | set(range(LEAF0, LEAF0 + OB_CHUNK)) | set(range(END0, END0 + OB_CHUNK))
    f.eng = Engine(PARTS)
    f.orc = Oracle(PARTS)
    f.orc_calls = 0
    for be, reg_e, reg_t in ((f.eng, f.eng.register_edge, f.eng.register_tag),
                             (f.orc, lambda *a: f.orc.register(True, *a), lambda *a: f.orc.register(False, *a))):
        reg_e(1, "e", E_SCHEMA)
        reg_e(2, "r", R_SCHEMA)
        reg_t(7, "t", T_SCHEMA)
        reg_t(8, "c", C_SCHEMA)
        be.load_builder(kb)
    f.vert_arr = np.array(sorted(f.vertset), np.int64)
    f.two = f.eng.go_device(roots, [1], 2, b"", ID_S_W)
    f.two_rows = f.two.fetch()
    nseg = f.eng.lib.nbg_rows_num_segments(f.two.h)
    assert nseg >= 4 and 3 * OB_CHUNK <= f.two.count <= 20000
    # the same vid in rows of different chunks and of different segments, with different payloads
    first, last = {}, {}
    for n, r in enumerate(f.two_rows):
        first.setdefault(r[0], n)
        last[r[0]] = n
    bounds, at = [], 0
    for i in range(nseg):
        b, e = C.c_uint64(), C.c_uint64()
        assert f.eng.lib.nbg_rows_segment(f.two.h, i, C.byref(b), C.byref(e)) == 0
        at += e.value - b.value
        bounds.append(at)
    seg_of = lambda n: int(np.searchsorted(bounds, n, side="right"))
    far = [v for v in last if last[v] // OB_CHUNK != first[v] // OB_CHUNK and seg_of(last[v]) != seg_of(first[v])
           and f.two_rows[first[v]][1:] != f.two_rows[last[v]][1:]]
    assert len(far) >= 10
    f.one_yields = [ep("e", "_dst").encode(), ep("e", "w").encode(), ep("e", "x").encode(), E.src_prop("t", "name").encode()]
    f.one_names = ["id", "w", "x", "nm"]
    tagged = [v for v in verts if v % 10 and 4 <= len(out[v]) <= 40][:12] + [roots[0]]
    assert roots[0] % 10
    f.one = f.eng.go_device(tagged, [1], 1, b"", f.one_yields)
    f.one_rows = f.one.fetch()
    assert 100 <= f.one.count <= 600 and isinstance(f.one_rows[0][3], str) and isinstance(f.one_rows[0][2], float)
    assert {NEG, IMIN, IMAX, INVIS} <= {r[0] for r in f.one_rows}
    f.fan = f.eng.go_device([FAN], [1], 1, b"", [ep("e", "_dst").encode()])
    assert f.fan.count == OB_CHUNK
    f.digests = [r.digest() for r in (f.two, f.one, f.fan)]
    yield f
    assert [r.digest() for r in (f.two, f.one, f.fan)] == f.digests        # the inputs stayed unchanged
    for r in (f.two, f.one, f.fan):
        r.free()
    f.eng.close()
    f.orc.close()
    assert f.orc_calls > 0, "no call reached the oracle"


def _take(rows):
    try:
        return rows.fetch()
    finally:
        rows.free()


def _code(fn):
    with pytest.raises(NbgError) as ex:
        fn()
    return ex.value.code


def _sorted(rows):
    """Rows as sorted tuples of (kind, value) cells, doubles by their bits: True is not 1."""
    return sorted((tuple(setops.bits_cell(v) for v in r) for r in rows), key=repr)


def _oracle(f, fetched, names, col, etypes, steps=1, where=b"", yields=(), distinct=False, over_all=False):
    """The oracle's rows of the piped statement over the fetched table (an OracleError passes through)."""
    f.orc_calls += 1
    starts = [r[names.index(col)] for r in fetched]
    return f.orc.go(starts, etypes, steps, where, list(yields), distinct, over_all, inputs=(names, fetched, col))


def _counted(f, fetched, names, col, distinct):
    """([frontier], [edges]) of one step over type `e` from the fixture's adjacency: the starts that
    are vertices (INVIS is one, with no visible edge) and their out-degrees; DISTINCT starts once per vid."""
    starts = [r[names.index(col)] for r in fetched]
    if distinct:
        starts = sorted(set(starts))
    fr = int(np.isin(np.array(starts, np.int64), f.vert_arr).sum()) if starts else 0
    ed = sum(len(f.out[v]) for v in starts if v in f.out and v != INVIS)
    return [fr], [ed]


def _host_route(f, fetched, names, col, etypes, steps=1, where=b"", yields=(), distinct=False, over_all=False):
    """(rows, (frontiers, edges, scanned)) of nbg_go over the fetched table, or the error's code."""
    starts = [r[names.index(col)] for r in fetched]
    try:
        rows = f.eng.go(starts, etypes, steps, where, list(yields), distinct, over_all, inputs=(names, fetched, col))
    except NbgError as ex:
        return ex.code, None
    return rows, f.eng.last_step_stats


def _parity(f, rows, names, col, etypes, steps=1, where=b"", yields=(), distinct=False, over_all=False, fetched=None):
    """The piped call against the oracle (rows, or that it fails) and against the engine's host route
    (rows, statistics and status); one step over `e` alone: the statistics as counted.  Returns the rows."""
    fetched = rows.fetch() if fetched is None else fetched
    want, stats = _host_route(f, fetched, names, col, etypes, steps, where, yields, distinct, over_all)
    if stats is None:
        with pytest.raises(OracleError):
            _oracle(f, fetched, names, col, etypes, steps, where, yields, distinct, over_all)
        assert _code(lambda: f.eng.go_piped(rows, names, col, etypes, steps, where, list(yields), distinct, over_all)) == want
        return None
    judge = _oracle(f, fetched, names, col, etypes, steps, where, yields, distinct, over_all)
    got = f.eng.go_piped(rows, names, col, etypes, steps, where, list(yields), distinct, over_all)
    try:
        fr, ed = got.step_stats()
        assert (fr, ed, got.edges_scanned) == tuple(stats)
        if list(etypes) == [1] and steps == 1 and not over_all:
            counted = _counted(f, fetched, names, col, distinct)
            assert (fr, ed) == (counted if counted[0][0] else ([], [])) and got.edges_scanned == sum(ed)
        dev = got.fetch()
    finally:
        got.free()
    assert len(dev) == len(judge) and _sorted(dev) == _sorted(judge)
    assert len(dev) == len(want) and _sorted(dev) == _sorted(want)
    return dev


def _limit(f, rows, names, n, offset=0):
    return f.eng.order_by(rows, names, [], (offset, n))


# ------------------------------------------------------------------------------ 1. parity
W_LT = E.binop("<", ep("e", "w"), E.const(10)).encode()
CASES = {
    "default_yield": dict(),
    "two_steps": dict(steps=2),
    "three_steps": dict(steps=3),
    "two_types": dict(etypes=[1, 2]),
    "two_types_two_steps": dict(etypes=[2, 1], steps=2),
    "over_all": dict(etypes=[1, 2], over_all=True),
    "where_edge_prop": dict(where=W_LT, yields=[ep("e", "_dst").encode(), ep("e", "w").encode()]),
    "where_two_steps": dict(steps=2, where=W_LT, yields=[ep("e", "_src").encode(), ep("e", "x").encode()]),
    "input_columns": dict(yields=[ip("w").encode(), ip("x").encode(), ip("nm").encode(), ip("id").encode(), ep("e", "_dst").encode()]),
    "input_arithmetic": dict(yields=[E.binop("+", E.binop("*", ip("w"), E.const(2)), ep("e", "w")).encode(),
                                     E.binop("/", ip("x"), E.const(4.0)).encode()]),
    "input_in_where": dict(where=E.binop("&&", E.binop(">", ip("w"), E.const(0)), E.binop("<", ep("e", "w"), ip("w"))).encode(),
                           yields=[ip("w").encode(), ep("e", "w").encode()]),
    # (some sources of `one` carry no tag: the oracle and both routes answer these two with an error;
    # test_tag_props_over_tagged_sources has the rows)
    "tag_props_untagged_source": dict(yields=[E.src_prop("t", "name").encode(), E.dst_prop("c", "pop").encode(), ep("e", "_dst").encode()]),
    "tag_props_untagged_source_and_input": dict(yields=[E.dst_prop("t", "name").encode(), ip("nm").encode(), E.src_prop("c", "pop").encode()]),
    "input_prop_missing": dict(yields=[ip("nope").encode()]),               # an evaluation error everywhere
    "two_types_input": dict(etypes=[1, 2], yields=[ip("w").encode(), ep("e", "w").encode(), ep("r", "s").encode()]),
}


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_host_route(ff, name, distinct):
    """(The name is older than its judge: _parity compares with the oracle first, then with the host route.)"""
    kw = dict(etypes=[1], steps=1, where=b"", yields=(), over_all=False)
    kw.update(CASES[name])
    dev = _parity(ff, ff.one, ff.one_names, "id", kw["etypes"], kw["steps"], kw["where"], kw["yields"], distinct, kw["over_all"],
                  fetched=ff.one_rows)
    if name != "input_prop_missing" and not name.startswith("tag_props_untagged"):
        assert dev


@pytest.mark.parametrize("distinct", [False, True])
def test_tag_props_over_tagged_sources(ff, distinct):
    """The rows of `one` whose id carries tag `t` (id % 10 != 0; INVIS has none, and is invisible):
    `$^.t.name`, `$$.c.pop` and `$$.t.name` beside `$-` columns."""
    keep = E.binop("!=", E.binop("%", ip("id"), E.const(10)), E.const(0)).encode()
    rows = ff.eng.yield_rows(ff.one, ff.one_names, [ip("id").encode(), ip("nm").encode(), ip("w").encode()], keep)
    try:
        assert 50 <= rows.count < ff.one.count
        for ys in ([E.src_prop("t", "name"), E.dst_prop("c", "pop"), ep("e", "_dst")],
                   [E.dst_prop("t", "name"), ip("nm"), E.src_prop("t", "name"), E.binop("+", ip("w"), E.dst_prop("c", "pop"))]):
            assert _parity(ff, rows, ["id", "nm", "w"], "id", [1], 1, b"", [y.encode() for y in ys], distinct)
    finally:
        rows.free()


def _admissible(out, roots, steps):
    """tests/test_gpu_backtracker.py's helper over an adjacency map: per vertex reached at step
    steps - 1, the roots its backtracker may hold."""
    A = {r: {r} for r in roots}
    F = set(roots)
    for _ in range(1, steps):
        nxt = defaultdict(set)
        Fk = set()
        for u in F:
            for v in out.get(u, ()):
                nxt[v] |= A[u]
                Fk.add(v)
        changed = True
        while changed:
            changed = False
            for u in F & Fk:
                for v in out.get(u, ()):
                    before = len(nxt[v])
                    nxt[v] |= nxt[u]
                    changed = changed or len(nxt[v]) != before
        A, F = nxt, Fk
    return A


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("steps", [2, 3])
def test_input_props_after_several_steps_are_admissible(ff, steps, distinct):
    """`GO N STEPS FROM $-.id OVER e YIELD $-.id, e._src, e._dst`: the root each row names is one its
    source's backtracker may hold; the rows without the root column are exact, and the oracle's."""
    ys = [ip("id").encode(), ep("e", "_src").encode(), ep("e", "_dst").encode()]
    got = ff.eng.go_piped(ff.one, ff.one_names, "id", [1], steps, b"", ys, distinct)
    judge = _oracle(ff, ff.one_rows, ff.one_names, "id", [1], steps, b"", ys, distinct)
    host, stats = _host_route(ff, ff.one_rows, ff.one_names, "id", [1], steps, b"", ys, distinct)
    fr, ed = got.step_stats()
    assert (fr, ed, got.edges_scanned) == tuple(stats)
    dev = _take(got)
    roots = {r[0] for r in ff.one_rows} - {INVIS}
    A = _admissible(ff.out, roots, steps)
    assert dev and max(len(x) for x in A.values()) > 1
    assert all(r[0] in A.get(r[1], ()) for r in dev)
    for want in (judge, host):
        if not distinct:
            assert _sorted([r[1:] for r in dev]) == _sorted([r[1:] for r in want])
        else:
            assert {tuple(r[1:]) for r in dev} == {tuple(r[1:]) for r in want}


# ------------------------------------------------------------------------------ 2. the last row of a vid wins
LAST_YIELDS = [ip("id").encode(), ip("s").encode(), ip("w").encode()]
LAST_WHERE = E.binop("<", ep("e", "w"), E.const(-45)).encode()          # (keeps the result small)


def test_last_row_wins_across_chunks_and_segments(ff):
    dev = _parity(ff, ff.two, NAMES, "id", [1], 1, LAST_WHERE, LAST_YIELDS, fetched=ff.two_rows)
    last = {r[0]: tuple(r) for r in ff.two_rows}
    assert dev and all(tuple(r) == last[r[0]] for r in dev)


def test_last_row_wins_after_a_reversing_order_by(ff):
    """ORDER BY $-.w DESC, $-.s DESC puts other rows last: the winners change, and follow."""
    rev = ff.eng.order_by(ff.two, NAMES, [("w", True), ("s", True)])
    try:
        fetched = rev.fetch()
        before = {r[0]: tuple(r) for r in ff.two_rows}
        after = {r[0]: tuple(r) for r in fetched}
        assert sum(before[v] != after[v] for v in before) >= 10
        dev = _parity(ff, rev, NAMES, "id", [1], 1, LAST_WHERE, LAST_YIELDS, fetched=fetched)
        assert dev and all(tuple(r) == after[r[0]] for r in dev)
    finally:
        rev.free()


# ------------------------------------------------------------------------------ 3. vids
def _computed(ff, yields, names):
    bufs = [y.encode() for y in yields]
    return ff.eng.yield_rows(ff.one, ff.one_names, bufs), names


def test_absent_negative_and_extreme_vids(ff):
    """`id + 1' is mostly no vertex; -5, INT64_MIN and INT64_MAX are vertices with out-edges; INVIS
    is a vertex whose record lives in another part (invisible: no rows, but counted as a start)."""
    rows, names = _computed(ff, [E.binop("+", ip("id"), E.const(1)), ip("w")], ["id", "w"])
    try:
        fetched = rows.fetch()
        hits = sum(r[0] in ff.vertset for r in fetched)
        assert 0 <= hits < len(fetched) // 2
        _parity(ff, rows, names, "id", [1], 1, b"", [ip("w").encode(), ep("e", "_dst").encode()], fetched=fetched)
    finally:
        rows.free()
    ys = [ip("id").encode(), ep("e", "_src").encode(), ep("e", "_dst").encode()]
    dev = _parity(ff, ff.one, ff.one_names, "id", [1], 1, b"", ys, fetched=ff.one_rows)
    srcs = {r[1] for r in dev}
    assert {NEG, IMIN, IMAX} <= srcs and INVIS not in srcs
    assert all(r[0] == r[1] for r in dev)


def test_nothing_resolves(ff):
    rows, names = _computed(ff, [E.binop("+", E.binop("*", ip("w"), E.const(0)), E.const(NOWHERE)), ip("w")], ["id", "w"])
    try:
        assert rows.count == ff.one.count and NOWHERE not in ff.vertset
        for distinct in (False, True):
            got = ff.eng.go_piped(rows, names, "id", [1], 2, b"", [ip("w").encode()], distinct)
            assert got.count == 0 and ff.eng.lib.nbg_rows_num_cols(got.h) == 1 and got.step_stats() == ([], [])
            assert _take(got) == []
        _parity(ff, rows, names, "id", [1], 2, b"", [ip("w").encode()])
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 4. input shapes
@pytest.mark.parametrize("n", [1, INLINE_STARTS, INLINE_STARTS + 1, OB_CHUNK - 1, OB_CHUNK, OB_CHUNK + 1])
@pytest.mark.parametrize("distinct", [False, True])
def test_input_sizes(ff, n, distinct):
    """The first n rows of `two`: every id resolves, so n is the found count (32: the last list that
    is read back; 33: the first that stays on the device)."""
    part = _limit(ff, ff.two, NAMES, n)
    try:
        assert part.count == n and all(r[0] in ff.vertset for r in ff.two_rows[:n])
        ys = [ip("s").encode(), ep("e", "_dst").encode()]
        _parity(ff, part, NAMES, "id", [1], 1, LAST_WHERE if n > 100 else b"", ys, distinct, fetched=ff.two_rows[:n])
    finally:
        part.free()


def test_many_short_segments(ff):
    """The whole two-step result (its segments as they lie), without $-: the sorted rows against the
    oracle's, and by their digest against nbg_go_device from the fetched column."""
    starts = [r[0] for r in ff.two_rows]
    ys = [ep("e", "_dst").encode(), ep("e", "w").encode()]
    for distinct in (False, True):
        judge = _oracle(ff, ff.two_rows, NAMES, "id", [1], 1, W_LT, ys, distinct)
        want = ff.eng.go_device(starts, [1], 1, W_LT, ys, distinct)
        got = ff.eng.go_piped(ff.two, NAMES, "id", [1], 1, W_LT, ys, distinct)
        try:
            assert got.count == want.count > 0 and got.digest() == want.digest()
            assert got.step_stats() == want.step_stats() and got.edges_scanned == want.edges_scanned
            assert got.step_stats() == _counted(ff, ff.two_rows, NAMES, "id", distinct)
            assert got.count == len(judge) and _sorted(got.fetch()) == _sorted(judge)
        finally:
            got.free()
            want.free()


def test_more_chunks_than_the_grid(ff):
    """2,048 * 2,048 + 1 one-column rows: each cell a leaf with one out-edge, so the start list has
    as many edges as entries (far below 2^32), and DISTINCT folds it to the 2,048 leaves."""
    n = OB_CHUNK * STAGE_GRID + 1
    assert all(len(ff.out[LEAF0 + i]) == 1 for i in range(OB_CHUNK)) and 2 * n < 1 << 32
    cur = ff.fan
    for _ in range(11):
        nxt = ff.eng.set_op(cur, cur, "UNION")
        if cur is not ff.fan:
            cur.free()
        cur = nxt
    one = _limit(ff, ff.fan, ["id"], 1, 7)
    big = ff.eng.set_op(cur, one, "UNION")
    cur.free()
    one.free()
    try:
        assert big.count == n
        ys = [ip("id").encode(), ep("e", "_dst").encode(), ep("e", "w").encode()]
        got = ff.eng.go_piped(big, ["id"], "id", [1], 1, b"", ys)
        cells = big.fetch_bits(copy=False)[0]
        want = ff.eng.go_device(cells, [1], 1, b"", [ep("e", "_src").encode(), ep("e", "_dst").encode(), ep("e", "w").encode()])
        try:
            assert got.count == want.count == n and got.digest() == want.digest()
            assert got.step_stats() == want.step_stats() and got.edges_scanned == want.edges_scanned == n
            # by numpy: every input cell gives one row, the row of its leaf
            k = np.asarray(cells) - LEAF0
            gid, gdst, gw = got.fetch_bits(copy=False)
            assert k.min() == 0 and k.max() == OB_CHUNK - 1 and len(gid) == n
            assert gid.min() >= LEAF0 and gid.max() < LEAF0 + OB_CHUNK
            assert np.array_equal(np.bincount(gid - LEAF0, minlength=OB_CHUNK), np.bincount(k, minlength=OB_CHUNK))
            assert np.array_equal(gdst, END0 + (gid - LEAF0)) and np.array_equal(gw, (gid - LEAF0) % 100 - 50)
        finally:
            got.free()
            want.free()
        dev = _take(ff.eng.go_piped(big, ["id"], "id", [1], 1, b"", ys, True))
        assert _sorted(dev) == _sorted([LEAF0 + i, END0 + i, i % 100 - 50] for i in range(OB_CHUNK))
    finally:
        big.free()


# ------------------------------------------------------------------------------ 5. chaining
def test_inputs_from_every_stage(ff):
    grouped = ff.eng.group_by(ff.two, NAMES, [ip("id").encode()], [("", ip("id").encode(), "id"), ("COUNT", E.const("*").encode(), "n")])
    ordered = ff.eng.order_by(ff.two, NAMES, [("w", False)], (3, 700))
    united = ff.eng.set_op(ordered, ordered, "UNION")
    yielded = ff.eng.yield_rows(ff.two, NAMES, [ip("w").encode(), ip("s").encode()], E.binop(">", ip("w"), E.const(30)).encode())
    fetched_v = ff.eng.fetch_vertices(ordered, NAMES, "id", 7, [E.edge_prop("t", "name").encode()])
    fetched_e = ff.eng.fetch_edges(ordered, NAMES, "s", "id", None, 1, [ep("e", "_dst").encode(), ep("e", "w").encode()])
    piped = ff.eng.go_piped(ordered, NAMES, "id", [1], 1, LAST_WHERE, [ep("e", "_dst").encode(), ip("w").encode()])
    try:
        for rows, names, col, pay in ((grouped, ["id", "n"], "id", "n"), (ordered, NAMES, "id", "w"), (united, NAMES, "s", "w"),
                                      (yielded, ["w", "id"], "id", "w"), (fetched_e, ["id", "w"], "id", "w"),
                                      (piped, ["id", "w"], "id", "w")):
            assert rows.count
            dev = _parity(ff, rows, names, col, [1], 1, LAST_WHERE, [ip(pay).encode(), ep("e", "_dst").encode()])
            assert dev
        # a FETCH's result has no vid column: its string column is refused as the FROM column
        assert fetched_v.count and _code(lambda: ff.eng.go_piped(fetched_v, ["name"], "name", [1])) == L.E_EXECUTION_ERROR
    finally:
        for r in (grouped, ordered, united, yielded, fetched_v, fetched_e, piped):
            r.free()


def test_three_sentence_pipe(ff):
    """`GO FROM r OVER e YIELD e._dst AS id | GO FROM $-.id OVER e YIELD e._dst AS id | GO FROM $-.id
    OVER r YIELD $-.id, r.s`: go_piped into go_piped.  Each sentence against the oracle, fed the table
    the sentence before it left (fetched), and the last against three host calls."""
    ys = [ep("e", "_dst").encode()]
    first = ff.eng.go_device(ff.roots, [1], 1, b"", ys)
    second = ff.eng.go_piped(first, ["id"], "id", [1], 1, b"", ys)
    try:
        ff.orc_calls += 1
        t1, t2 = first.fetch(), second.fetch()
        assert t1 and _sorted(t1) == _sorted(ff.orc.go(ff.roots, [1], 1, b"", ys))
        assert _sorted(t2) == _sorted(_oracle(ff, t1, ["id"], "id", [1], 1, b"", ys))
        h1 = ff.eng.go(ff.roots, [1], 1, b"", ys)
        h2 = ff.eng.go([r[0] for r in h1], [1], 1, b"", ys)
        assert second.count == len(h2) > INLINE_STARTS
        last = [ip("id").encode(), ep("r", "s").encode()]
        third = _take(ff.eng.go_piped(second, ["id"], "id", [2], 1, b"", last))
        assert third and _sorted(third) == _sorted(_oracle(ff, t2, ["id"], "id", [2], 1, b"", last))
        h3 = ff.eng.go([r[0] for r in h2], [2], 1, b"", last, inputs=(["id"], h2, "id"))
        assert _sorted(third) == _sorted(h3)
    finally:
        first.free()
        second.free()


def test_output_feeds_every_stage(ff):
    ys = [ep("e", "_dst").encode(), ep("e", "_src").encode(), ep("e", "w").encode()]
    out = ff.eng.go_piped(ff.one, ff.one_names, "id", [1], 1, b"", ys)
    want = _oracle(ff, ff.one_rows, ff.one_names, "id", [1], 1, b"", ys)        # (every stage below is judged by these rows)
    try:
        assert out.count == len(want) > OB_CHUNK
        g = _take(ff.eng.group_by(out, NAMES, [ip("s").encode()], [("", ip("s").encode(), "s"), ("COUNT", E.const("*").encode(), "n")]))
        cnt = defaultdict(int)
        for r in want:
            cnt[r[1]] += 1
        assert _sorted(g) == _sorted(cnt.items())
        o = _take(ff.eng.order_by(out, NAMES, [("w", True), ("id", False), ("s", False)], (0, 50)))
        assert [tuple(r) for r in o] == sorted((tuple(r) for r in want), key=lambda r: (-r[2], r[0], r[1]))[:50]
        u = _take(ff.eng.set_op(out, out, "UNION", True))
        assert _sorted(u) == _sorted(set(tuple(r) for r in want))
        y = _take(ff.eng.yield_rows(out, NAMES, [E.binop("+", ip("w"), E.const(1)).encode()], E.binop("<", ip("w"), E.const(0)).encode()))
        assert _sorted(y) == _sorted([r[2] + 1] for r in want if r[2] < 0)
        a = _take(ff.eng.yield_agg(out, NAMES, [ip("w").encode(), E.const("*").encode()], ["SUM", "COUNT"]))
        assert [list(r) for r in a] == [[sum(r[2] for r in want), len(want)]]
        v = _take(ff.eng.fetch_vertices(out, NAMES, "id", 7, [E.edge_prop("t", "name").encode()]))
        assert _sorted(v) == _sorted([f"n{r[0] % 23}"] for r in want if r[0] % 10 and r[0] in set(ff.verts) | {NEG, IMIN, IMAX})
        e = _take(ff.eng.fetch_edges(out, NAMES, "s", "id", None, 1, [ep("e", "w").encode()]))
        assert _sorted(e) == _sorted([r[2]] for r in want)
        _parity(ff, out, NAMES, "id", [1], 1, LAST_WHERE, [ip("w").encode(), ep("e", "_dst").encode()], fetched=out.fetch())
    finally:
        out.free()


def test_host_rows_equal_device_rows_fetched(ff):
    ys = [ip("w").encode(), ip("nm").encode(), ep("e", "_dst").encode()]
    for distinct in (False, True):
        for rows, names, fetched in ((ff.one, ff.one_names, ff.one_rows), ):
            host = ff.eng.go_piped(rows, names, "id", [1], 2, b"", ys[2:], distinct, device=False)
            stats = ff.eng.last_step_stats
            dev = ff.eng.go_piped(rows, names, "id", [1], 2, b"", ys[2:], distinct)
            fr, ed = dev.step_stats()
            assert (fr, ed, dev.edges_scanned) == tuple(stats)
            assert host and _sorted(host) == _sorted(_take(dev))
            host = ff.eng.go_piped(rows, names, "id", [1], 1, b"", ys, distinct, device=False)
            assert host and _sorted(host) == _sorted(_take(ff.eng.go_piped(rows, names, "id", [1], 1, b"", ys, distinct)))
    # a short list (read back) may take the one-launch path of a host result
    few = _limit(ff, ff.two, NAMES, 3)
    try:
        host = ff.eng.go_piped(few, NAMES, "id", [1], 2, b"", [ep("e", "_dst").encode()], device=False)
        assert host and _sorted(host) == _sorted(_take(ff.eng.go_piped(few, NAMES, "id", [1], 2, b"", [ep("e", "_dst").encode()])))
    finally:
        few.free()


# ------------------------------------------------------------------------------ 6. statuses, in nbg.h's order
def _empty(ff):
    return ff.eng.go_device([NOWHERE], [1], 1, b"", ID_S_W)


def test_status_1_invalid_arguments(ff):
    good = ep("e", "w").encode()
    for bad in (b"\xff", good[:-1], good + b"\x00"):
        assert _code(lambda: ff.eng.go_piped(ff.two, NAMES, "id", [1], 1, b"", [bad])) == L.E_INVALID_ARGUMENT
        assert _code(lambda: ff.eng.go_piped(ff.two, NAMES, "id", [1], 1, bad, [good])) == L.E_INVALID_ARGUMENT
        assert _code(lambda: ff.eng.go_piped(ff.two, NAMES, "id", [999], 1, b"", [bad])) == L.E_INVALID_ARGUMENT   # before 3
    assert _code(lambda: ff.eng.go_piped(ff.two, NAMES[:2], "id", [1])) == L.E_INVALID_ARGUMENT       # two names, three columns
    assert _code(lambda: ff.eng.go_piped(ff.two, NAMES + ["z"], "id", [1])) == L.E_INVALID_ARGUMENT
    assert _code(lambda: ff.eng.go_piped(ff.two, NAMES, "zz", [1])) == L.E_INVALID_ARGUMENT           # input_vid_col = -1
    req, keep = ff.eng._go_request([], [1], 1, b"", [], False, False)
    out = C.c_void_p()
    req.num_input_cols, req.input_vid_col = 3, 0                                                       # input_names == NULL
    assert ff.eng.lib.nbg_go_piped(ff.eng.h, ff.two.h, C.byref(req), 1, C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    req.input_names = (C.c_char_p * 3)(b"id", None, b"w")
    assert ff.eng.lib.nbg_go_piped(ff.eng.h, ff.two.h, C.byref(req), 1, C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    req.input_names, req.input_vid_col = (C.c_char_p * 3)(b"id", b"s", b"w"), 3
    assert ff.eng.lib.nbg_go_piped(ff.eng.h, ff.two.h, C.byref(req), 1, C.byref(out)) == L.E_INVALID_ARGUMENT and not out.value
    # rows of another engine; host-only rows
    other = Engine(PARTS)
    try:
        other.register_edge(1, "e", E_SCHEMA)
        kb = kvgen.KVBuilder(PARTS)
        kb.insert_edge(1, 2, 1, 0, E_SCHEMA, [1, 0.5, 0.5], NOW)
        other.load_builder(kb)
        theirs = other.go_device([1], [1], 1, b"", ID_S_W)
        assert theirs.count == 1 and _code(lambda: ff.eng.go_piped(theirs, NAMES, "id", [1])) == L.E_INVALID_ARGUMENT
        theirs.free()
    finally:
        other.close()
    req, keep = ff.eng._go_request([ff.roots[0]], [1], 1, b"", ID_S_W, False, False)
    h = C.c_void_p()
    assert ff.eng.lib.nbg_go(ff.eng.h, C.byref(req), C.byref(h)) == L.OK
    host = DeviceRows(ff.eng, h)
    try:
        assert host.count and _code(lambda: ff.eng.go_piped(host, NAMES, "id", [1])) == L.E_INVALID_ARGUMENT
    finally:
        host.free()


def test_status_2_partitioned_engine():
    kb = kvgen.KVBuilder(PARTS)
    for s, d in ((10, 11), (11, 12), (12, 10), (13, 10)):
        kb.insert_edge(s, d, 1, 0, E_SCHEMA, [s, 0.5, 0.5], NOW)
    c = LocalCluster(PARTS, 2)
    try:
        c.register_edge(1, "e", E_SCHEMA)
        c.load_builder(kb)
        rows = c.each(lambda e: e.go_device([10, 11], [1], 1, b"", ID_S_W))
        assert sum(r.count for r in rows) > 0
        for e, r in zip(c.engines, rows):
            assert _code(lambda: e.go_piped(r, NAMES, "id", [1])) == L.E_UNSUPPORTED
            assert _code(lambda: e.go_piped(r, NAMES, "id", [999])) == L.E_UNSUPPORTED            # before 3
            r.free()
    finally:
        c.close()


def test_status_3_prepare_errors_and_their_order(ff):
    empty = _empty(ff)
    try:
        assert empty.count == 0
        for rows in (ff.two, empty):                                                  # 3 before 4: on an empty input too
            assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", [999])) == L.E_EXECUTION_ERROR           # unknown edge type
            assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", [-1])) == L.E_EXECUTION_ERROR            # REVERSELY
            assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", [])) == L.E_EXECUTION_ERROR              # empty OVER
            assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", [1], 0)) == L.E_INVALID_ARGUMENT         # steps
            assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", [1], 33)) == L.E_UNSUPPORTED             # over 32 steps
            # a status of nbg_go_prepare equals nbg_go's for the same statement
            for kw in (dict(etypes=[999]), dict(etypes=[1], steps=33)):
                want, _ = _host_route(ff, [], NAMES, "id", kw["etypes"], kw.get("steps", 1))
                assert _code(lambda: ff.eng.go_piped(rows, NAMES, "id", kw["etypes"], kw.get("steps", 1))) == want
    finally:
        empty.free()


def test_status_4_zero_input_rows(ff):
    empty = _empty(ff)
    filtered = ff.eng.yield_rows(ff.one, ff.one_names, [ip("x").encode(), ip("nm").encode()], E.binop(">", ip("w"), E.const(1000)).encode())
    try:
        assert empty.count == 0 and filtered.count == 0 and ff.eng.lib.nbg_rows_col_kind(filtered.h, 0) == L.V_DOUBLE
        for ys, ncols in (([], 1), ([ip("w").encode(), ep("e", "_dst").encode()], 2)):
            got = ff.eng.go_piped(empty, NAMES, "id", [1], 2, b"", ys)
            assert got.count == 0 and ff.eng.lib.nbg_rows_num_cols(got.h) == ncols and got.step_stats() == ([], [])
            assert _take(got) == []
            assert ff.eng.go_piped(empty, NAMES, "id", [1], 2, b"", ys, device=False) == []
        # 4 before 5 and 6: a DOUBLE or STRING FROM column of an empty input is no error
        for col in ("x", "nm"):
            got = ff.eng.go_piped(filtered, ["x", "nm"], col, [1], 1, b"", [ip("nm").encode()])
            assert got.count == 0 and _take(got) == []
    finally:
        empty.free()
        filtered.free()


def test_status_5_from_column_kinds(ff):
    for col in ("x", "nm"):                                           # DOUBLE, STRING
        with pytest.raises(NbgError, match=f"Column `{col}' not found") as ex:
            ff.eng.go_piped(ff.one, ff.one_names, col, [1])
        assert ex.value.code == L.E_EXECUTION_ERROR
    mixed = ff.eng.yield_rows(ff.one, ff.one_names, [ip("id").encode(), E.binop(">", ip("w"), E.const(0)).encode(),
                                                     E.cast("timestamp", ip("id")).encode()])
    try:
        for col in ("b", "t"):                                        # BOOL, TIMESTAMP
            assert _code(lambda: ff.eng.go_piped(mixed, ["id", "b", "t"], col, [1])) == L.E_EXECUTION_ERROR
        assert _parity(ff, mixed, ["id", "b", "t"], "id", [1], 1, b"", [ip("b").encode(), ip("t").encode(), ep("e", "_dst").encode()])
    finally:
        mixed.free()


def test_status_6_limits(ff):
    """A FLOAT column and a misaligned row schema; a referenced string column that can hold strings
    outside the dictionary (a derived table) — the same input is accepted while the column is not read."""
    for ys in ([ep("e", "_dst"), ep("e", "f")], [ep("e", "_dst"), E.binop("+", ep("e", "x"), ep("e", "w")), ep("e", "w")]):
        rows = ff.eng.go_device([ff.roots[0]], [1], 1, b"", [y.encode() for y in ys])
        try:
            names = ["id", "a", "b"][:len(ys)]
            assert rows.count > 0 and _code(lambda: ff.eng.go_piped(rows, names, "id", [1])) == L.E_UNSUPPORTED
            assert _code(lambda: ff.eng.go_piped(rows, names, "a", [1])) in (L.E_UNSUPPORTED, L.E_EXECUTION_ERROR)
        finally:
            rows.free()
    derived = ff.eng.go_device([ff.roots[0]], [1], 1, b"", [ep("e", "_dst").encode(), ep("e", "w").encode(),
                                                            E.binop("+", E.src_prop("t", "name"), E.const("!")).encode()])
    try:
        names = ["id", "w", "nm"]
        fetched = derived.fetch()
        assert derived.count > 0 and fetched[0][2].endswith("!")
        assert _code(lambda: ff.eng.go_piped(derived, names, "id", [1], 1, b"", [ip("nm").encode()])) == L.E_UNSUPPORTED
        assert _code(lambda: ff.eng.go_piped(derived, names, "id", [1], 1, E.binop("==", ip("nm"), E.const("a")).encode(), [])) == \
            L.E_UNSUPPORTED
        assert _parity(ff, derived, names, "id", [1], 1, b"", [ip("w").encode(), ep("e", "_dst").encode()], fetched=fetched)
    finally:
        derived.free()


def test_status_7_evaluation_errors_as_nbg_go(ff):
    ys = [E.binop("/", E.const(7), E.binop("-", ip("w"), ep("e", "w"))).encode()]      # fails where $-.w == e.w
    want, stats = _host_route(ff, ff.one_rows, ff.one_names, "id", [1], 1, b"", ys)
    assert want == L.E_EXECUTION_ERROR and stats is None
    for distinct in (False, True):
        with pytest.raises(OracleError):
            _oracle(ff, ff.one_rows, ff.one_names, "id", [1], 1, b"", ys, distinct)
    assert _code(lambda: ff.eng.go_piped(ff.one, ff.one_names, "id", [1], 1, b"", ys)) == L.E_EXECUTION_ERROR
    assert _code(lambda: ff.eng.go_piped(ff.one, ff.one_names, "id", [1], 1, b"", ys, True)) == L.E_EXECUTION_ERROR


# ------------------------------------------------------------------------------ 7. memory and the profile
def _free_device_memory():
    """hipMemGetInfo through the HIP runtime this process has loaded."""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_scratch_and_index_are_released(ff):
    ys = [ip("w").encode(), ep("e", "_dst").encode()]

    def calls():
        for distinct in (False, True):
            for rows, names in ((ff.two, NAMES), (ff.one, ff.one_names)):
                ff.eng.go_piped(rows, names, "id", [1], 1, LAST_WHERE, ys, distinct).free()
                ff.eng.go_piped(rows, names, "id", [1], 2, b"", [ep("e", "_dst").encode()], distinct).free()
                assert _code(lambda: ff.eng.go_piped(rows, names, "id", [1], 1, b"", [ip("nope").encode()], distinct)) == \
                    L.E_EXECUTION_ERROR
    calls()                                             # (grow-only buffers of the query workspace reach their size)
    # the free memory is the whole device's: another process may move it, a leak moves it every time
    seen = []
    for _ in range(3):
        before = (ff.eng.stats()["device_bytes"], _free_device_memory())
        calls()
        seen.append(((ff.eng.stats()["device_bytes"], _free_device_memory()), before))
        if seen[-1][0] == before:
            break
    assert seen[-1][0] == seen[-1][1], seen


def test_profile_entries(ff):
    ys = [ip("w").encode(), ep("e", "_dst").encode()]
    n = ff.two.count
    ff.eng.profile(True)
    ff.eng.go_piped(ff.two, NAMES, "id", [1], 1, LAST_WHERE, [ep("e", "_dst").encode()]).free()
    prof = ff.eng.profile_read()
    assert [prof[k]["launches"] for k in GP_KERNELS] == [1, 0, 1, 1, 0]
    assert prof["k_gp_resolve"]["algo_bytes"] == n * 12 and prof["k_gp_emit"]["algo_bytes"] == n * 8 and prof["k_gp_resolve"]["ms"] > 0
    ff.eng.profile(True)
    ff.eng.go_piped(ff.two, NAMES, "id", [1], 1, LAST_WHERE, ys, True).free()
    prof = ff.eng.profile_read()
    ff.eng.profile(False)
    assert [prof[k]["launches"] for k in GP_KERNELS] == [1, 1, 0, 0, 2]             # the DISTINCT list, the index
    assert all(prof[k]["ms"] > 0 for k in ("k_gp_resolve", "k_gp_table", "k_gp_compact"))
    assert prof["k_gp_resolve"]["algo_bytes"] == n * 16
