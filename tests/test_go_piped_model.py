"""tests/support/gopipe.py's model of `| GO FROM $-.col OVER e YIELD <$- columns>, e._src, e._dst, e.w`
against the storage oracle's `Oracle.go(..., inputs=...)` on the CPU: a graph of a few hundred edges
whose vertices include negative vids and both int64 extremes, and an input table with vids that come
several times with differing payloads (in chosen positions: the last row is not the one with the
largest payload), vids that are no vertex, and vertices without out-edges."""
import numpy as np
import pytest

from nebula_amd import expr as E
from tests.support import gopipe, graphs, setops

IMIN, IMAX = -(1 << 63), (1 << 63) - 1
ep, ip = E.edge_prop, E.input_prop


def _graph():
    rng = np.random.default_rng(23)
    verts = np.concatenate([rng.choice(1 << 20, 60, replace=False), -rng.choice(1 << 20, 20, replace=False) - 1,
                            np.array([IMIN, IMAX, -5, 0])]).astype(np.int64)
    pairs = set()
    while len(pairs) < 400:
        s, d = rng.choice(len(verts) - 10, 1)[0], rng.choice(len(verts), 1)[0]     # the last ten vertices: in-edges only
        pairs.add((int(verts[10 + s]), int(verts[d])))
    pairs = sorted(pairs)
    src, dst = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
    w = rng.integers(-1000, 1000, len(src)).astype(np.int64)
    return verts, src, dst, w


def _input(verts, src):
    """[id, p, x, s] rows: every third vertex three times, the middle copy with the largest p; vids
    next to a vertex that are none; the extremes; a sink."""
    rng = np.random.default_rng(29)
    vs = set(verts.tolist())
    sinks = sorted(vs - set(src.tolist()))
    assert sinks and {IMIN, IMAX, -5} <= set(src.tolist())
    ids = verts[::3].tolist() * 3 + [IMIN, IMAX, -5, sinks[0], IMAX, IMIN]
    ids += [v + 1 for v in verts[:12].tolist() if v + 1 not in vs and v != IMAX] + [IMIN + 1, IMAX - 1, 1 << 40]
    ids = [ids[k] for k in rng.permutation(len(ids))]
    n, third = len(ids), len(ids) // 3
    rows = []
    for r, v in enumerate(ids):
        p = 1_000_000 - r if third <= r < 2 * third else r
        rows.append([v, p, p / 8.0 - 3.0, f"s{p % 11}é"])
    assert len({r[1] for r in rows}) == n
    return rows


@pytest.fixture(scope="module")
def pinned():
    verts, src, dst, w = _graph()
    orc = graphs.rmat_oracle(src, dst, w, parts=7)
    yield verts, src, dst, w, orc
    orc.close()


def _cells(rows):
    return sorted((tuple(setops.bits_cell(v) for v in r) for r in rows), key=repr)


@pytest.mark.parametrize("distinct", [False, True])
def test_model_equals_the_oracle(pinned, distinct):
    verts, src, dst, w, orc = pinned
    table = _input(verts, src)
    names = ["id", "p", "x", "s"]
    cols = [[r[c] for r in table] for c in range(4)]
    ys = [ip(n).encode() for n in names] + [ep("e", "_src").encode(), ep("e", "_dst").encode(), ep("e", "w").encode()]
    want = orc.go(cols[0], [graphs.E_TYPE], 1, b"", ys, distinct, inputs=(names, table, "id"))
    got = gopipe.rows(gopipe.Adjacency(src, dst, w), cols, 0, distinct)
    assert len(want) > (100 if distinct else 300) and _cells(got) == _cells(want)
    # what the input was built to show
    ids = np.array(cols[0])
    dup = [v for v in set(cols[0]) if cols[0].count(v) >= 3 and v in set(src.tolist())]
    assert len(dup) >= 10 and sum(max(r[1] for r in table if r[0] == v) != [r[1] for r in table if r[0] == v][-1] for v in dup) >= 5
    assert all(r[0] == r[4] for r in got) and {IMIN, IMAX, -5} <= {r[0] for r in got}
    last = {r[0]: r for r in table}
    assert all(list(r[:4]) == last[r[0]] for r in got)
    assert (~np.isin(ids, verts)).sum() >= 8
    if distinct:
        assert len(got) < len(gopipe.rows(gopipe.Adjacency(src, dst, w), cols, 0, False))


@pytest.mark.parametrize("distinct", [False, True])
def test_projected_rows_and_statistics(pinned, distinct):
    """Fewer result columns: DISTINCT folds the rows that become equal.  The frontier counts the
    starts that are vertices, the edges their out-degrees."""
    verts, src, dst, w, orc = pinned
    table = _input(verts, src)
    names = ["id", "p", "x", "s"]
    cols = [[r[c] for r in table] for c in range(4)]
    adj = gopipe.Adjacency(src, dst, w)
    want = orc.go(cols[0], [graphs.E_TYPE], 1, b"", [ep("e", "_dst").encode(), ip("s").encode()], distinct, inputs=(names, table, "id"))
    got = gopipe.rows(adj, cols, 0, distinct, take=[5, 3])
    assert _cells(got) == _cells(want)
    if distinct:
        assert len(got) < len(gopipe.piped_go(adj, cols[0], True)[0])             # some rows did fold
    fr, ed = gopipe.frontier_and_edges(adj, cols[0], verts, distinct)
    ids = sorted(set(cols[0])) if distinct else cols[0]
    out = {}
    for s in src.tolist():
        out[s] = out.get(s, 0) + 1
    assert fr == sum(v in set(verts.tolist()) for v in ids) and ed == sum(out.get(v, 0) for v in ids)
    assert ed == len(gopipe.piped_go(adj, cols[0], distinct)[0])


def test_empty_and_unresolved_inputs(pinned):
    verts, src, dst, w, orc = pinned
    adj = gopipe.Adjacency(src, dst, w)
    for distinct in (False, True):
        assert gopipe.rows(adj, [[], []], 0, distinct) == []
        assert gopipe.rows(adj, [[1 << 50, (1 << 50) + 1], [1, 2]], 0, distinct) == []
        assert orc.go([1 << 50, (1 << 50) + 1], [graphs.E_TYPE], 1, b"", [ip("p").encode()], distinct,
                      inputs=(["id", "p"], [[1 << 50, 1], [(1 << 50) + 1, 2]], "id")) == []
