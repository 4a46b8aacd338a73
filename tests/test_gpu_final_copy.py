"""k_final_copy (finalcopy.hip): the final step of an indexed statement whose only YIELD is _dst,
written as one dense run.  Every case runs one statement three ways on one engine — over its
index with the copy kernel, over its index with NBG_FINAL_COPY=0 (k_final_dst), and without an
index (NBG_STMT_INDEX=0) — and compares each with the storage oracle (sorted rows, edges_scanned,
the per-step statistics against step_model); the two indexed runs are also compared by digest.

The hand-built graph holds one root per case.  A root's neighbours are the final frontier; the
passing / failing out-degree of each is chosen so that the final list's runs fall on the chunk
arithmetic the kernel can get wrong (a chunk is CH = 512 rows; a lane stores two rows at once).
The final list is in claim (arrival) order, not id order: a case fixes which runs the list holds,
not their order, except where the frontier fits one tile of the step before (the small cases).

The kernel finds a chunk's entry by a 64-ary search of the list: a list of up to 4,096 entries is
resolved by the round kept in registers, up to 262,144 by one gather more, beyond by two.  The
graphs of `wide_frontier` have 5,000 and 270,000 final entries, so both pipelined gathers run."""
import ctypes as C
import contextlib
import os

import numpy as np
import pytest

from nebula_amd import expr as E, kvgen
from tests.support import graphs
from tests.test_gpu_stmt_index import DST, check, env, prepare, step_model, where

pytestmark = pytest.mark.gpu

CH = 512
WB = where("<", 50)

# case -> [(passing out-degree, failing out-degree)] of the root's neighbours, in id order
CASES = {
    "all_fail": [(0, 3), (0, 1), (0, 40)],
    "one_row": [(1, 0)],
    "deg_1_2_3": [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1), (3, 1), (3, 0), (2, 0), (1, 0)],
    "zeros_around": [(0, 3), (5, 0), (0, 2), (0, 1), (7, 1), (1, 0), (0, 1)],
    "run_ends_at_chunk": [(CH, 0), (3, 0)],
    "run_ends_before_chunk": [(CH - 1, 0), (3, 0)],
    "run_ends_after_chunk": [(CH + 1, 0), (3, 0)],
    "total_ch": [(7, 0)] * 73 + [(1, 2)],
    "total_ch_minus_1": [(7, 0)] * 73,
    "total_ch_plus_1": [(7, 0)] * 73 + [(2, 0)],
    "total_3ch": [(3, 1)] * CH,
    "hub_after_odd_singles": [(1, 0)] * 3 + [(4 * CH + 300, 5)] + [(2, 0)],
    "hub_alone": [(5 * CH, 0)],
    "many_entries_per_chunk": [(1, 0), (0, 1)] * 400 + [(600, 0)],
}
TOTALS = {"all_fail": 0, "one_row": 1, "total_ch": CH, "total_ch_minus_1": CH - 1, "total_ch_plus_1": CH + 1,
          "total_3ch": 3 * CH, "run_ends_at_chunk": CH + 3, "hub_alone": 5 * CH}


def hand_graph():
    """Root c reaches its case's neighbours; each neighbour's edges go to leaves of its own (no
    out-edges), the passing ones with w = 10 and the failing ones with w = 90.  `lonely` has no
    out-edges: its final frontier is empty."""
    src, dst, w, roots = [], [], [], {}
    vid, leaf = 1000, 1_000_000
    for c, (name, degs) in enumerate(CASES.items()):
        roots[name] = 10 + c
        for dp, df in degs:
            src.append(roots[name]); dst.append(vid); w.append(10)
            for k in range(dp + df):
                src.append(vid); dst.append(leaf); w.append(10 if k < dp else 90)
                leaf += 1
            vid += 1
    roots["lonely"] = 5
    src.append(6); dst.append(5); w.append(10)   # (the vertex exists)
    return (np.array(src, np.int64), np.array(dst, np.int64), np.array(w, np.int64)), roots


@contextlib.contextmanager
def final_copy_unset():
    """NBG_FINAL_COPY (read per query) out of the environment, put back afterwards."""
    old = os.environ.pop("NBG_FINAL_COPY", None)
    try:
        yield
    finally:
        if old is not None:
            os.environ["NBG_FINAL_COPY"] = old


@pytest.fixture(autouse=True)
def default_kernel_choice():
    """Every test of this module starts with NBG_FINAL_COPY unset; the caller's value comes back."""
    with final_copy_unset():
        yield


def nonempty_segments(eng, res):
    n = 0
    for i in range(eng.lib.nbg_rows_num_segments(res.h)):
        b, e = C.c_uint64(), C.c_uint64()
        assert eng.lib.nbg_rows_segment(res.h, i, C.byref(b), C.byref(e)) == 0
        n += e.value > b.value
    return n


def three_ways(eng, orc, src, dst, roots, steps, indexed, plain):
    """The oracle comparison of `check` for the copy kernel, k_final_dst over the index and the
    WHERE path; the digests of the first two; one segment from the copy kernel.  Returns the rows."""
    with final_copy_unset():
        n = check(indexed, orc, src, dst, roots, steps, WB)
        assert indexed.index_bytes() > 0
        res = indexed.run_device(roots)
        try:
            d_copy = res.digest()
            assert res.count == n
            assert nonempty_segments(eng, res) == (1 if n else 0)
        finally:
            res.free()
    with env(NBG_FINAL_COPY=0):
        assert check(indexed, orc, src, dst, roots, steps, WB) == n
        res = indexed.run_device(roots)
        try:
            assert res.digest() == d_copy
        finally:
            res.free()
    assert check(plain, orc, src, dst, roots, steps, WB) == n
    assert plain.index_bytes() == 0
    return n


@pytest.fixture(scope="module")
def hand():
    (src, dst, w), roots = hand_graph()
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    indexed = prepare(eng, 2, WB)
    plain = prepare(eng, 2, WB, NBG_STMT_INDEX=0)
    yield src, dst, eng, orc, roots, indexed, plain
    indexed.free()
    plain.free()
    eng.close()
    orc.close()


@pytest.mark.parametrize("case", ["lonely"] + list(CASES))
def test_hand_built(hand, case):
    src, dst, eng, orc, roots, indexed, plain = hand
    n = three_ways(eng, orc, src, dst, [roots[case]], 2, indexed, plain)
    if case == "lonely":
        assert n == 0
    else:
        assert n == sum(dp for dp, _ in CASES[case])
    if case in TOTALS:
        assert n == TOTALS[case]


def test_several_roots_one_list(hand):
    """A start list of every case's root: one final list of all their runs, arrival order."""
    src, dst, eng, orc, roots, indexed, plain = hand
    n = three_ways(eng, orc, src, dst, [roots[c] for c in CASES], 2, indexed, plain)
    assert n == sum(dp for degs in CASES.values() for dp, _ in degs)


@pytest.fixture(scope="module")
def rmat10():
    src, dst, w = graphs.rmat_graph(10)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    yield src, dst, eng, orc
    eng.close()
    orc.close()


@pytest.mark.parametrize("steps", [2, 3])
def test_rmat10(rmat10, steps):
    src, dst, eng, orc = rmat10
    indexed = prepare(eng, steps, WB)
    plain = prepare(eng, steps, WB, NBG_STMT_INDEX=0)
    try:
        rows = 0
        for r in graphs.roots(src, 8):
            rows += three_ways(eng, orc, src, dst, [r], steps, indexed, plain)
        assert rows > 0
    finally:
        indexed.free()
        plain.free()


def test_rmat12_six_in_flight():
    """RMAT-12, 3 steps: six queries in flight through submit / wait, twice over; every result's
    digest equals its one-at-a-time run's, whose rows the oracle confirms."""
    src, dst, w = graphs.rmat_graph(12)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    indexed = prepare(eng, 3, WB)
    plain = prepare(eng, 3, WB, NBG_STMT_INDEX=0)
    try:
        roots = graphs.roots(src, 6, seed=9)
        solo = []
        for r in roots[:2]:
            three_ways(eng, orc, src, dst, [r], 3, indexed, plain)
        for r in roots:
            res = indexed.run_device([r])
            solo.append(res.digest())
            got = graphs.sorted_rows(res.fetch())
            res.free()
            assert got == graphs.sorted_rows(orc.go([r], [1], 3, WB)), r
        assert indexed.index_bytes() > 0
        for _ in range(2):
            tickets = [indexed.submit([r]) for r in roots]
            for i in (4, 1, 5, 0, 3, 2):
                res = indexed.wait(tickets[i])
                try:
                    assert res.digest() == solo[i], i
                    assert nonempty_segments(eng, res) == (1 if solo[i][0] else 0)
                finally:
                    res.free()
    finally:
        indexed.free()
        plain.free()
        eng.close()
        orc.close()


def test_multi_yield_keeps_its_kernel(rmat10):
    """YIELD _dst, 7 is not the single-_dst shape: the oracle's rows, over the index."""
    src, dst, eng, orc = rmat10
    ys = [DST, E.const(7).encode()]
    stmt = prepare(eng, 3, WB, ys)
    try:
        for r in graphs.roots(src, 3, seed=5):
            check(stmt, orc, src, dst, [r], 3, WB, ys)
        assert stmt.index_bytes() > 0
    finally:
        stmt.free()


def wide_graph(singles, hub):
    """A root with `singles` one-row neighbours (every third has a failing edge as well, every
    seventh only a failing one) and one hub of `hub` passing edges: a final list of more entries
    than the search's register round resolves, with chunk boundaries all along it."""
    R, V0, H, LEAF = 1, 10, 5, 10_000_000
    deg = np.ones(singles, np.int64) + (np.arange(singles) % 3 == 0)
    v = V0 + np.arange(singles, dtype=np.int64)
    es, ew = np.repeat(v, deg), np.full(int(deg.sum()), 10, np.int64)
    first = np.cumsum(deg) - deg
    ew[first[deg == 2] + 1] = 90
    ew[first[np.arange(singles) % 7 == 0]] = 90
    ed = LEAF + np.arange(len(es), dtype=np.int64)
    src = np.concatenate([np.full(singles + 1, R, np.int64), es, np.full(hub, H, np.int64)])
    dst = np.concatenate([v, [H], ed, LEAF + len(es) + np.arange(hub, dtype=np.int64)])
    w = np.concatenate([np.full(singles + 1, 10, np.int64), ew, np.full(hub, 10, np.int64)])
    rows = int(np.count_nonzero(ew == 10)) + hub
    return src, dst, w, R, rows


@pytest.mark.parametrize("singles", [5_000, 270_000])
def test_wide_frontier(singles):
    """More than 4,096 final entries (one search gather) and more than 262,144 (two): the copy
    kernel, k_final_dst over the index and the WHERE path against the storage oracle's rows and
    step_model's statistics, both computed once."""
    src, dst, w, R, rows = wide_graph(singles, 3 * CH + 77)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    indexed = prepare(eng, 2, WB)
    plain = prepare(eng, 2, WB, NBG_STMT_INDEX=0)
    try:
        exp = np.sort(np.array([r[0] for r in orc.go([R], [1], 2, WB)], np.int64))
        assert len(exp) == rows
        fr, ed = step_model(src, dst, [R], 2)
        seen = []
        for stmt, kv in ((indexed, {}), (indexed, {"NBG_FINAL_COPY": 0}), (plain, {})):
            with env(**kv):
                res = stmt.run_device([R])
            try:
                assert np.array_equal(np.sort(res.fetch_bits()[0]), exp), kv
                assert res.step_stats() == (fr, ed), kv
                assert res.edges_scanned == sum(ed), kv
                seen.append((res.digest(), nonempty_segments(eng, res)))
            finally:
                res.free()
        assert indexed.index_bytes() > 0 and plain.index_bytes() == 0
        assert seen[0][0] == seen[1][0] and seen[0][1] == 1
    finally:
        indexed.free()
        plain.free()
        eng.close()
        orc.close()


def test_invisible_vertex_in_the_final_frontier():
    """R -> A, X, B.  X's out-edges are stored in a part that is not X's home: X is in the snapshot,
    reached and listed, but invisible, so the final step scans none of its edges and E_N does not
    count them (the kernel's `visible` test).  A has 3 passing edges and 1 failing, B 2 passing:
    5 rows, step statistics ([1, 3], [3, 6]) by hand, 9 edges scanned."""
    from nebula_amd import Engine
    from tests.support.oracle import Oracle
    parts, now = 7, 1_600_000_000_000_000
    R, A, X, B = 101, 202, 303, 404
    kb = kvgen.KVBuilder(parts)
    put = lambda s, d, x: kb.insert_edge(s, d, graphs.E_TYPE, 0, graphs.E_SCHEMA, [x], now + 1)
    put(R, A, 10)
    put(R, B, 10)
    # (the edge to X without its in-edge mirror, which would be a second home part of X)
    p0 = kvgen.part_of(R, parts)
    kb.put(p0, kvgen.edge_key(p0, R, graphs.E_TYPE, 0, X, kvgen.version_of(now + 1)),
           kvgen.encode_row(graphs.E_SCHEMA, [10]))
    for k, x in enumerate((10, 20, 30, 90)):
        put(A, 5000 + k, x)
    for k in range(2):
        put(B, 6000 + k, 10)
    wrong = kvgen.part_of(X, parts) % parts + 1
    for k in range(5):
        kb.put(wrong, kvgen.edge_key(wrong, X, graphs.E_TYPE, 0, 7000 + k, kvgen.version_of(now)),
               kvgen.encode_row(graphs.E_SCHEMA, [10]))
    eng = Engine(parts)
    eng.register_edge(graphs.E_TYPE, "e", graphs.E_SCHEMA)
    eng.load_builder(kb)
    orc = Oracle(parts)
    orc.register(True, graphs.E_TYPE, "e", graphs.E_SCHEMA)
    orc.load_builder(kb)
    indexed = prepare(eng, 2, WB)
    plain = prepare(eng, 2, WB, NBG_STMT_INDEX=0)
    try:
        exp = graphs.sorted_rows(orc.go([R], [1], 2, WB))
        assert len(exp) == 5
        seen = []
        for stmt, kv in ((indexed, {}), (indexed, {"NBG_FINAL_COPY": 0}), (plain, {})):
            with env(**kv):
                res = stmt.run_device([R])
            try:
                assert graphs.sorted_rows(res.fetch()) == exp, kv
                print("step stats", res.step_stats(), "scanned", res.edges_scanned)
                assert res.step_stats() == ([1, 3], [3, 6]), kv
                assert res.edges_scanned == 9, kv
                seen.append(res.digest())
            finally:
                res.free()
        assert indexed.index_bytes() > 0 and plain.index_bytes() == 0
        assert seen[0] == seen[1]
    finally:
        indexed.free()
        plain.free()
        eng.close()
        orc.close()
