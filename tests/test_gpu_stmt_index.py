"""The statement index (nbg.h, nbg_go_prepare): a prepared statement whose final step is
`WHERE <col> <cmp> <const> YIELD _dst | <const>` builds the filtered adjacency once and its later
final steps run over it.  Rows, edges_scanned and the per-step statistics stay what the oracles
report: rows against the storage oracle, edges_scanned against the CSR oracle (RMAT graphs), the
per-step frontier / edge counts against GoExecutor's definition worked out here from the edge list
(step s scans the unfiltered out-degrees of the distinct destinations of step s - 1; the WHERE
only filters the final step's rows)."""
import contextlib
import os

import numpy as np
import pytest

from nebula_amd import expr as E
from tests.support import graphs

pytestmark = pytest.mark.gpu

DST = E.edge_prop("e", "_dst").encode()


def where(op, c, const_left=False, col="w"):
    col, k = E.edge_prop("e", col), E.const(int(c))
    return (E.binop(op, k, col) if const_left else E.binop(op, col, k)).encode()


@contextlib.contextmanager
def env(**kv):
    """The index switches are read by nbg_go_prepare: set them around prepare_go."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def prepare(eng, steps, wb, yields=(), **kv):
    kv.setdefault("NBG_STMT_INDEX_AFTER", 0)
    with env(**kv):
        return eng.prepare_go([1], steps, wb, yields)


def step_model(src, dst, roots, steps):
    """(frontier sizes, edges scanned) per step over the live edges (one per (src, dst))."""
    pairs = np.unique(np.stack([np.asarray(src, np.int64), np.asarray(dst, np.int64)], 1), axis=0)
    s, d = pairs[:, 0], pairs[:, 1]
    fr, ed = [], []
    cur = np.asarray(roots, np.int64)
    for k in range(steps):
        m = np.isin(s, cur)
        fr.append(len(cur))
        # (a start list keeps duplicates; later frontiers are sets)
        ed.append(int(sum(np.count_nonzero(s == v) for v in cur)) if k == 0 else int(m.sum()))
        cur = np.unique(d[m])
    return fr, ed


def check(stmt, orc, src, dst, roots, steps, wb, yields=(), csr_where=None, csr=None):
    """One device execution against the oracles: row multiset, edges_scanned, per-step stats."""
    res = stmt.run_device(roots)
    try:
        got = graphs.sorted_rows(res.fetch())
        exp = graphs.sorted_rows(orc.go(roots, [1], steps, wb, yields))
        assert got == exp, (roots, steps, len(got), len(exp))
        fr, ed = step_model(src, dst, roots, steps)
        print("step stats", res.step_stats(), "model", (fr, ed), "scanned", res.edges_scanned)
        assert res.step_stats() == (fr, ed)
        assert res.edges_scanned == sum(ed)
        if csr is not None:
            assert res.edges_scanned == csr.go(roots, steps, *csr_where)[1]
        return len(got)
    finally:
        res.free()


@pytest.fixture(scope="module")
def rmat10():
    from tests.support.oracle import CsrOracle
    src, dst, w = graphs.rmat_graph(10)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    csr = CsrOracle(src, dst, w, threads=1)
    yield src, dst, w, eng, orc, csr
    eng.close()
    orc.close()
    csr.close()


@pytest.fixture(scope="module")
def rmat12():
    src, dst, w = graphs.rmat_graph(12)
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    yield src, dst, w, eng, orc
    eng.close()
    orc.close()


@pytest.mark.parametrize("steps", [2, 3])
def test_before_and_after_build(rmat10, steps):
    """WHERE w < 50 YIELD _dst, 4 roots: a statement that never builds, one that builds at once, and
    one that builds after its first completed execution all report the oracles' figures."""
    src, dst, w, eng, orc, csr = rmat10
    wb = where("<", 50)
    roots = graphs.roots(src, 4)
    tiny = eng.stats()["tiny_queries"]
    never = prepare(eng, steps, wb, NBG_STMT_INDEX_AFTER=1e9)
    at_once = prepare(eng, steps, wb)
    later = prepare(eng, steps, wb, NBG_STMT_INDEX_AFTER=1e-9)
    try:
        rows = 0
        for r in roots:
            rows += check(never, orc, src, dst, [r], steps, wb, csr_where=("<", 50), csr=csr)
            assert never.index_bytes() == 0
            rows += check(at_once, orc, src, dst, [r], steps, wb, csr_where=("<", 50), csr=csr)
            assert at_once.index_bytes() > 0
        assert rows > 0
        assert later.index_bytes() == 0
        check(later, orc, src, dst, [roots[0]], steps, wb)   # launched before the threshold is crossed
        assert later.index_bytes() == 0
        for r in roots:
            check(later, orc, src, dst, [r], steps, wb, csr_where=("<", 50), csr=csr)
            assert later.index_bytes() > 0
        assert eng.stats()["tiny_queries"] == tiny   # (device results never take the one-launch path)
    finally:
        for s in (never, at_once, later):
            s.free()


def hand_graph():
    """About 600 edges.  R -> A, B, H, S.  A: 20 edges that all fail w < 50; B: 20 that all pass; H:
    a hub of 560 edges, 530 passing (its filtered row spans more than two 256-item tiles); S: no
    out-edges.  The leaves have no out-edges either."""
    R, A, B, H, S = 1001, 1002, 1003, 1004, 1005
    leaf = lambda k: 5000 + k
    src, dst, w = [R] * 4, [A, B, H, S], [10, 90, 10, 90]
    for k in range(20):
        src.append(A); dst.append(leaf(k)); w.append(90 + k % 5)
        src.append(B); dst.append(leaf(k + 7)); w.append(k % 40)
    for k in range(560):
        src.append(H); dst.append(leaf(k)); w.append(k % 49 if k < 530 else 50 + k % 30)
    return (np.array(src, np.int64), np.array(dst, np.int64), np.array(w, np.int64)), (R, A, B, H, S)


def test_hand_made_graph():
    """A frontier vertex whose edges all fail still counts in edges_scanned and the frontier stat; one
    whose edges all pass; a hub across tiles; a vertex without out-edges; a WHERE that passes
    nothing (empty filtered column) and one that passes everything."""
    (src, dst, w), (R, A, B, H, S) = hand_graph()
    eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    try:
        for c, rows2 in ((50, 20 + 530), (-5, 0), (1000, 600)):
            wb = where("<", c)
            for steps in (2, 3):
                stmt = prepare(eng, steps, wb)
                try:
                    n = check(stmt, orc, src, dst, [R], steps, wb)
                    assert stmt.index_bytes() > 0
                    assert n == (rows2 if steps == 2 else 0)
                    check(stmt, orc, src, dst, [R, A, B], steps, wb)   # a start list, on the built index
                finally:
                    stmt.free()
        # the model's figures, spelled out: 2 steps from R scan 4 + (20 + 20 + 560 + 0) edges over a
        # final frontier of 4, whatever the WHERE passes
        assert step_model(src, dst, [R], 2) == ([1, 4], [4, 600])
    finally:
        eng.close()
        orc.close()


@pytest.mark.parametrize("scale_w", [(-1, -50), (300, 0), (70000, 0), (10 ** 12, -7)])
def test_operators_and_widths(scale_w):
    """All six operators, the constant on either side, over WHERE columns stored in 1, 2, 4 and 8
    bytes (the affine maps of test_narrow_int_columns)."""
    mul, add = scale_w
    src, dst, w = graphs.rmat_graph(10)
    w2 = w * mul + add
    eng = graphs.rmat_engine(src, dst, w2)
    orc = graphs.rmat_oracle(src, dst, w2)
    try:
        mid = int(np.median(w2))
        roots = graphs.roots(src, 2, seed=13)
        ref = {}
        for op in ("<", "<=", ">", ">=", "==", "!="):
            for left in (False, True):
                wb = where(op, mid, const_left=left)
                stmt = prepare(eng, 2, wb)
                try:
                    for r in roots:
                        res = stmt.run_device([r])
                        got = graphs.sorted_rows(res.fetch())
                        res.free()
                        if (op, left, r) not in ref:
                            ref[(op, left, r)] = graphs.sorted_rows(orc.go([r], [1], 2, wb))
                        assert got == ref[(op, left, r)], (op, left, mul, add)
                    assert stmt.index_bytes() > 0, (op, left)
                finally:
                    stmt.free()
    finally:
        eng.close()
        orc.close()


def test_dst_const_dst_yields(rmat10):
    """YIELD _dst, <const>, _dst: the kernel instantiation that is not the single-_dst one."""
    src, dst, w, eng, orc, csr = rmat10
    wb = where("<", 50)
    ys = [DST, E.const(7).encode(), DST]
    stmt = prepare(eng, 3, wb, ys)
    try:
        for r in graphs.roots(src, 3, seed=5):
            check(stmt, orc, src, dst, [r], 3, wb, ys, csr_where=("<", 50), csr=csr)
        assert stmt.index_bytes() > 0
    finally:
        stmt.free()


def test_one_step_statement_beside_an_index(rmat10):
    """1-step queries consume the inline start list and keep the WHERE path: beside an indexed
    statement of the same WHERE they build nothing and return the oracle's rows."""
    src, dst, w, eng, orc, csr = rmat10
    wb = where("<", 50)
    two = prepare(eng, 2, wb)
    one = prepare(eng, 1, wb)
    try:
        roots = graphs.roots(src, 4, seed=3)
        check(two, orc, src, dst, roots[:1], 2, wb)
        assert two.index_bytes() > 0
        for r in roots:
            check(one, orc, src, dst, [r], 1, wb, csr_where=("<", 50), csr=csr)
        check(one, orc, src, dst, roots * 12, 1, wb)   # more starts than travel inline
        assert one.index_bytes() == 0
    finally:
        two.free()
        one.free()


def test_queries_in_flight_across_the_build(rmat12):
    """10 queries on the 6 slots, the threshold crossed when the first one completes (inside the
    7th submit): some were launched before the build and some after; waited for out of order."""
    src, dst, w, eng, orc = rmat12
    wb = where("<", 50)
    roots = graphs.roots(src, 10, seed=9)
    stmt = prepare(eng, 3, wb, NBG_STMT_INDEX_AFTER=1e-9)
    try:
        tickets = []
        for i, r in enumerate(roots):
            tickets.append(stmt.submit([r]))
            if i == 5:
                assert stmt.index_bytes() == 0
        assert stmt.index_bytes() > 0
        for i in (9, 2, 7, 0, 4, 8, 1, 3, 6, 5):
            res = stmt.wait(tickets[i])
            got = graphs.sorted_rows(res.fetch())
            fr, ed = step_model(src, dst, [roots[i]], 3)
            assert res.step_stats() == (fr, ed), i
            res.free()
            assert got == graphs.sorted_rows(orc.go([roots[i]], [1], 3, wb)), i
    finally:
        stmt.free()


def test_binding_cap_builds_nothing():
    """max_edge_returned_per_vertex below the largest degree clips rows before the WHERE runs: no
    index, the oracle's rows."""
    src, dst, w = graphs.rmat_graph(10)
    eng = graphs.rmat_engine(src, dst, w, max_edge=8)
    orc = graphs.rmat_oracle(src, dst, w, max_edge=8)
    wb = where("<", 50)
    stmt = prepare(eng, 2, wb)
    try:
        for r in graphs.roots(src, 3, seed=4):
            res = stmt.run_device([r])
            got = graphs.sorted_rows(res.fetch())
            res.free()
            assert got == graphs.sorted_rows(orc.go([r], [1], 2, wb)), r
            assert stmt.index_bytes() == 0
    finally:
        stmt.free()
        eng.close()
        orc.close()


def test_switches(rmat10, capfd):
    """NBG_STMT_INDEX=0 and NBG_STMT_INDEX_MB=0: no index, the same results.  nbg_go one-shots
    never build (no build is logged for them; one is for the prepared statement)."""
    src, dst, w, eng, orc, csr = rmat10
    wb = where("<", 50)
    roots = graphs.roots(src, 2, seed=6)
    for kv in ({"NBG_STMT_INDEX": 0}, {"NBG_STMT_INDEX_MB": 0}):
        stmt = prepare(eng, 3, wb, **kv)
        try:
            for r in roots:
                check(stmt, orc, src, dst, [r], 3, wb, csr_where=("<", 50), csr=csr)
                assert stmt.index_bytes() == 0, kv
        finally:
            stmt.free()
    capfd.readouterr()
    with env(NBG_STMT_INDEX_AFTER=0, NBG_STMT_INDEX_TRACE=1):
        for r in roots:
            assert graphs.sorted_rows(eng.go([r], [1], 3, wb)) == graphs.sorted_rows(orc.go([r], [1], 3, wb))
            eng.go_device([r], [1], 3, wb).free()
        assert "[stmt index]" not in capfd.readouterr().err
        stmt = eng.prepare_go([1], 3, wb)
        try:
            check(stmt, orc, src, dst, roots[:1], 3, wb)
            assert stmt.index_bytes() > 0
        finally:
            stmt.free()
        assert "[stmt index]" in capfd.readouterr().err


def test_two_statements_one_engine(rmat10):
    """Different constants: each statement has its own index and its own oracle result."""
    src, dst, w, eng, orc, csr = rmat10
    a, b = prepare(eng, 3, where("<", 50)), prepare(eng, 3, where(">=", 90))
    try:
        for r in graphs.roots(src, 3, seed=8):
            for _ in range(2):
                check(a, orc, src, dst, [r], 3, where("<", 50), csr_where=("<", 50), csr=csr)
                check(b, orc, src, dst, [r], 3, where(">=", 90), csr_where=(">=", 90), csr=csr)
        assert a.index_bytes() > b.index_bytes() > 0   # (half of the edges pass against a tenth)
    finally:
        a.free()
        b.free()


def test_flag_mode_list_builder():
    """NBG_MARK_FLAGS=1 (read when the engine's workspaces are made): the final list comes from the
    byte flags' compaction instead of the claims, built over the filtered rows all the same."""
    from tests.support.oracle import CsrOracle
    src, dst, w = graphs.rmat_graph(10)
    with env(NBG_MARK_FLAGS=1):
        eng = graphs.rmat_engine(src, dst, w)
    orc = graphs.rmat_oracle(src, dst, w)
    csr = CsrOracle(src, dst, w, threads=1)
    wb = where("<", 50)
    stmt = prepare(eng, 3, wb)
    try:
        for r in graphs.roots(src, 3, seed=12):
            check(stmt, orc, src, dst, [r], 3, wb, csr_where=("<", 50), csr=csr)
        assert stmt.index_bytes() > 0
    finally:
        stmt.free()
        eng.close()
        orc.close()
        csr.close()


def test_snapshot_round_trip(rmat10, tmp_path):
    """An engine restored from a snapshot file builds and uses the index like the one that wrote it."""
    from nebula_amd import Engine
    src, dst, w, eng, orc, csr = rmat10
    path = str(tmp_path / "snap.nbg")
    eng.snapshot_save(path)
    re = Engine(100)
    try:
        re.snapshot_load(path)
        wb = where("<", 50)
        stmt = prepare(re, 3, wb)
        try:
            for r in graphs.roots(src, 3, seed=11):
                check(stmt, orc, src, dst, [r], 3, wb, csr_where=("<", 50), csr=csr)
            assert stmt.index_bytes() > 0
        finally:
            stmt.free()
    finally:
        re.close()
