"""nbg_go_piped at the edges of its per-vertex table, at a vertex count where the table kernels'
grid stride runs, and over $- cells of every kind.  Expected rows never come from the device: they
come from tests/support/gopipe.py's numpy model (pinned to the storage oracle by
tests/test_go_piped_model.py) over the input as fetched, or from the value table's own cells.

csrc/gopipe.hip keeps a table last_row[nv] of one entry per dense vertex id whenever the statement
is DISTINCT or reads $-: k_gp_table counts it and k_gp_compact folds it, both in blocks of 2,048
entries strided over at most STAGE_GRID workgroups.  The graphs here put starts on chosen dense
ids: vids ascend with dense ids, so R roots with negative vids hold dense ids 0 .. R-1 and target
v >= 0 holds dense id R + v; there are no other vertices.

  1. table edges: nv around 256, 2,048 and 4,096; starts on every id, on the ids next to a wave,
     a stride and a block boundary, and on nv - 1 alone; each with and without DISTINCT and $-.p
     (k_gp_table / k_gp_compact run exactly when the table is needed, by the profile's launches);
  2. the winner's chunk: an input whose winning rows are row 0, a chunk's last row, the next
     chunk's first and a ragged last chunk's last;
  3. nv = STAGE_GRID * 2048 + 2048 + 1: 2,050 table blocks, of which two are a workgroup's second
     trip and the last holds one entry;
  4. every bit of a $- cell: NaN payloads, -0.0, the int64 extremes, 2^53 + 1, bytes >= 0x80."""
import math

import numpy as np
import pytest

from nebula_amd import _lib as L, expr as E
from tests.support import gopipe, graphs, rowtable as rt, setops

pytestmark = pytest.mark.gpu

BLOCK = 256                           # csrc/ws.h
OB_CHUNK = 2048                       # csrc/nbg_internal.h: rows per chunk, and table entries per block
STAGE_GRID = 2048                     # csrc/stage.h
INLINE_STARTS = 32                    # csrc/nbg_internal.h
GP_KERNELS = ("k_gp_resolve", "k_gp_table", "k_gp_degrees", "k_gp_emit", "k_gp_compact")
ep, ip = E.edge_prop, E.input_prop
INPUT_YIELDS = [ep("e", "_dst").encode(), ep("e", "w").encode()]          # id, p
NAMES = ["id", "p"]
EDGE_YIELDS = [ep("e", "_src").encode(), ep("e", "_dst").encode(), ep("e", "w").encode()]


class Fixture:
    pass


def cdiv(a, b):
    return -(-a // b)


def _hand_graph(nroots, nt, root_edges):
    """(src, dst, w): targets 0 .. nt-1 in a ring v -> (v + 1) % nt with w = v % 97 - 48, and per
    entry of `root_edges` = (root, targets, payloads) the edges of root vid root - nroots."""
    t = np.arange(nt, dtype=np.int64)
    src, dst, w = [t], [(t + 1) % nt], [t % 97 - 48]
    for k, targets, pay in root_edges:
        assert 0 <= k < nroots and len(targets) == len(pay) and len(np.unique(targets)) == len(targets)
        src.append(np.full(len(targets), k - nroots, np.int64))
        dst.append(np.asarray(targets, np.int64))
        w.append(np.asarray(pay, np.int64))
    src, dst, w = np.concatenate(src), np.concatenate(dst), np.concatenate(w)
    pay = w[nt:]
    assert len(np.unique(pay)) == len(pay), "a payload twice"
    return src, dst, w


def _sorted_cols(cols):
    cols = [np.asarray(c, np.int64) for c in cols]
    o = np.lexsort(tuple(reversed(cols)))
    return [c[o] for c in cols]


def _expected(adj, idc, pc, distinct, with_p):
    """The model's result columns ([$-.p,] e._src, e._dst, e.w) over the fetched input columns."""
    win, edge = gopipe.piped_go(adj, idc, distinct)
    if distinct:
        assert len(np.unique(edge)) == len(edge)      # one start per vid: no two rows are equal, nothing folds
    return ([pc[win]] if with_p else []) + [adj.src[edge], adj.dst[edge], adj.w[edge]]


def _launches(with_table, distinct, with_index):
    """The profile's launches per GP_KERNELS entry for a call whose list is not empty."""
    if not with_table:
        return [1, 0, 1, 1, 0]
    return [1, 1, 0 if distinct else 1, 0 if distinct else 1, int(distinct) + int(with_index)]


def _check_piped(eng, adj, rows, idc, pc, what):
    """go_piped over `rows` = (id, p), with and without DISTINCT and $-.p, against the model; the
    table kernels launch exactly when a table is needed."""
    for distinct in (False, True):
        for with_p in (False, True):
            ys = ([ip("p").encode()] if with_p else []) + EDGE_YIELDS
            eng.profile(True)
            try:
                out = eng.go_piped(rows, NAMES, "id", [1], 1, b"", ys, distinct)
                try:
                    got = out.fetch_bits()
                    stats, scanned = out.step_stats(), out.edges_scanned
                finally:
                    out.free()
                prof = eng.profile_read()
            finally:
                eng.profile(False)
            want = _expected(adj, idc, pc, distinct, with_p)
            tag = (what, "DISTINCT" if distinct else "", "$-.p" if with_p else "")
            print(tag, "rows", len(got[0]), "launches", [prof[k]["launches"] for k in GP_KERNELS])
            assert len(got[0]) == len(want[0]) > 0, tag
            for g, w_ in zip(_sorted_cols(got), _sorted_cols(want)):
                assert np.array_equal(g, w_), tag
            starts = len(np.unique(idc)) if distinct else len(idc)          # (every cell is a vertex here)
            assert stats == ([starts], [len(want[0])]) and scanned == len(want[0]), tag
            assert [prof[k]["launches"] for k in GP_KERNELS] == _launches(distinct or with_p, distinct, with_p), tag


# ------------------------------------------------------------------------------ 1. table edges
P_ALL, P_EDGE, P_LAST = 10_000, 50_000, 90_000         # root 0's payloads: p = base + target; root 1's: 5,000 more
NVS = [2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("nv", NVS)
def test_table_edges(nv):
    """Starts on chosen dense ids.  The last root reaches every target, with a payload that tells
    the targets on the boundary ids (>= P_EDGE) and the one on nv - 1 (>= P_LAST) from the rest; a
    root before it (when nv leaves room for one) reaches the boundary targets and every fifth
    other again, with other payloads: those vids come twice in the input."""
    R = 1 if nv == 2 else 2
    NT = nv - R
    t = np.arange(NT, dtype=np.int64)
    on_edge = sorted({d - R for d in (R, 63, 64, 255, 256, 2047, 2048, 2049, nv - 1) if R <= d < nv})
    assert on_edge[-1] == NT - 1
    base = np.full(NT, P_ALL)
    base[on_edge] = P_EDGE
    base[NT - 1] = P_LAST
    roots = [(R - 1, t, base + t)]
    again = t
    if R == 2:
        again = np.unique(np.concatenate([t[::5], np.array(on_edge)]))
        roots.append((0, again, base[again] + again + 5_000))
    src, dst, w = _hand_graph(R, NT, roots)
    eng = graphs.rmat_engine(src, dst, w)
    try:
        assert eng.stats()["num_vertices"] == nv
        adj = gopipe.Adjacency(src, dst, w)
        lists = set()
        for what, floor in (("every target", P_ALL), ("boundary ids", P_EDGE), ("nv - 1 alone", P_LAST)):
            where = E.binop(">=", ep("e", "w"), E.const(floor)).encode()
            rows = eng.go_device(list(range(-R, 0)), [1], 1, where, INPUT_YIELDS)
            try:
                idc, pc = rows.fetch_bits()
                mine = (src < 0) & (w >= floor)                    # the roots' edges the WHERE keeps
                assert sorted(zip(pc.tolist(), idc.tolist())) == sorted(zip(w[mine].tolist(), dst[mine].tolist()))
                want_ids = {"every target": t.tolist(), "boundary ids": on_edge, "nv - 1 alone": [NT - 1]}[what]
                assert sorted(set(idc.tolist())) == sorted(want_ids) and len(idc) == R * len(want_ids) - (NT - len(again) if floor == P_ALL else 0)
                lists.add(len(idc) > INLINE_STARTS)
                _check_piped(eng, adj, rows, idc, pc, (nv, what))
            finally:
                rows.free()
        assert lists == ({False} if nv == 2 else {False, True})           # a list that is read back and one that is not
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 2. the winner's chunk
@pytest.mark.parametrize("n", [OB_CHUNK + 1, 2 * OB_CHUNK + 1])
def test_winning_rows_at_chunk_edges(n):
    """Input row r holds p = r and id = r, but: rows 3 and 2047 hold one vid (the winner is a chunk's
    last row), rows 5 and 2048 one (the next chunk's first row), rows 1 and n - 1 one (the ragged last
    chunk's last row; at n = 2049 that row is 2048 itself, which rows 5 and 2048 cover), and row 0
    wins its own vid.  (Row 0 cannot both win alone and lose to row 2047: the pair starts on row 3.)
    Ordered by p the input is one segment in that order; the raw GO result holds the same rows in
    several segments, in whatever order fetch() shows."""
    ids = np.arange(n, dtype=np.int64)
    ids[OB_CHUNK - 1], ids[OB_CHUNK] = 3, 5
    if n - 1 != OB_CHUNK:
        ids[n - 1] = 1
    rows_of = np.arange(n, dtype=np.int64)
    nroots = 8                                     # row r is an edge of root r % 8: no root reaches a vid twice
    src, dst, w = _hand_graph(nroots, n, [(k, ids[rows_of % nroots == k], rows_of[rows_of % nroots == k]) for k in range(nroots)])
    eng = graphs.rmat_engine(src, dst, w)
    raw = one = None
    try:
        assert eng.stats()["num_vertices"] == n + nroots
        adj = gopipe.Adjacency(src, dst, w)
        raw = eng.go_device(list(range(-nroots, 0)), [1], 1, b"", INPUT_YIELDS)
        one = eng.order_by(raw, NAMES, [("p", False)])
        assert raw.count == one.count == n and eng.lib.nbg_rows_num_segments(one.h) == 1
        assert eng.lib.nbg_rows_num_segments(raw.h) >= 2
        idc, pc = one.fetch_bits()
        assert np.array_equal(pc, rows_of) and np.array_equal(idc, ids)
        # the expected $-.p by hand: the largest row that holds the id
        last = {}
        for r, v in enumerate(ids.tolist()):
            last[v] = r
        assert last[3] == OB_CHUNK - 1 and last[5] == OB_CHUNK and last[0] == 0 and last[1] == (n - 1 if n - 1 != OB_CHUNK else 1)
        for distinct in (False, True):
            out = eng.go_piped(one, NAMES, "id", [1], 1, b"", [ip("p").encode(), ep("e", "_src").encode()], distinct)
            try:
                gp, gs = out.fetch_bits()
            finally:
                out.free()
            starts = sorted(last) if distinct else ids.tolist()
            assert sorted(zip(gs.tolist(), gp.tolist())) == sorted((v, last[v]) for v in starts)
        _check_piped(eng, adj, one, idc, pc, (n, "one segment"))
        ridc, rpc = raw.fetch_bits()
        assert sorted(zip(rpc.tolist(), ridc.tolist())) == list(zip(rows_of.tolist(), ids.tolist()))
        _check_piped(eng, adj, raw, ridc, rpc, (n, "raw"))
    finally:
        for r in (raw, one):
            if r is not None:
                r.free()
        eng.close()


# ------------------------------------------------------------------------------ 3. more table blocks than workgroups
BIG_NV = STAGE_GRID * OB_CHUNK + OB_CHUNK + 1


@pytest.fixture(scope="module")
def big():
    """nv = BIG_NV: two roots and a ring of targets.  About 3,000 starts: in table blocks 0 and 1,
    in block 2047 (the last of the first trip), in block 2048 (workgroup 0's second trip), the one
    vertex of block 2049, and a few hundred spread; every seventh comes twice, from the other root."""
    R = 2
    NT = BIG_NV - R
    rng = np.random.default_rng(61)

    def block(b, k):
        lo, hi = max(b * OB_CHUNK, R), min((b + 1) * OB_CHUNK, BIG_NV)
        edge = [d for d in (lo, lo + 63, lo + 64, lo + 255, lo + 256, hi - 1) if lo <= d < hi]
        return np.concatenate([np.array(edge), rng.choice(np.arange(lo, hi), k, replace=False)])
    dense = np.unique(np.concatenate([block(0, 500), block(1, 500), block(STAGE_GRID - 1, 600), block(STAGE_GRID, 700),
                                      np.array([BIG_NV - 1]), rng.integers(R, BIG_NV, 400)]))
    rng.shuffle(dense)
    targets = dense - R
    f = Fixture()
    f.dense = dense
    src, dst, w = _hand_graph(R, NT, [(1, targets, 10_000 + np.arange(len(targets))),
                                      (0, targets[::7], 1_000_000 + np.arange(len(targets[::7])))])
    f.eng = graphs.rmat_engine(src, dst, w)
    f.adj = gopipe.Adjacency(src, dst, w)
    yield f
    f.eng.close()


def test_more_table_blocks_than_the_grid(big):
    eng = big.eng
    assert eng.stats()["num_vertices"] == BIG_NV
    nblocks = cdiv(BIG_NV, OB_CHUNK)
    assert nblocks > STAGE_GRID and nblocks == STAGE_GRID + 2, "more table blocks than workgroups: the grid stride runs"
    assert BIG_NV - (nblocks - 1) * OB_CHUNK == 1, "the last block holds one entry"
    blk = big.dense // OB_CHUNK
    assert all((blk == b).sum() >= (1 if b == nblocks - 1 else 300) for b in (0, 1, STAGE_GRID - 1, STAGE_GRID, nblocks - 1))
    assert 2500 <= len(big.dense) <= 3500 and len(np.unique(blk)) > 300
    rows = eng.go_device([-2, -1], [1], 1, b"", INPUT_YIELDS)
    try:
        idc, pc = rows.fetch_bits()
        assert len(idc) == len(big.dense) + len(big.dense[::7]) and set(idc.tolist()) == set((big.dense - 2).tolist())
        _check_piped(eng, big.adj, rows, idc, pc, "big")
    finally:
        rows.free()


# ------------------------------------------------------------------------------ 4. every bit of a $- cell
@pytest.fixture(scope="module")
def vt():
    """rowtable's value table with one row per source: source SRC0 + pos has the one out-edge that
    is table row pos.  `raw` is the GO's rows with `e._src AS id` beside them (several segments);
    `piped` passes every column of the plain GO through a YIELD that computes id; `one` is the same
    over the rows as one segment in table order."""
    f = Fixture()
    f.t = rt.value_table(per_src=1)
    f.ld = rt.load_value_table(f.t)
    assert np.array_equal(f.t.src, np.arange(f.t.n))
    eng = f.ld.eng
    f.names = f.ld.names + ["id"]
    f.plain, _ = rt.go_checked(f.ld)               # the GO's rows are the table's, bit for bit
    f.raw = eng.go_device(f.t.source_vids(), [rt.E_TYPE], 1, b"", f.ld.yields + [ep("e", "_src").encode()])
    through = [ip(c).encode() for c in f.ld.names] + [E.binop("+", ip("pos"), E.const(rt.SRC0)).encode()]
    f.piped = eng.yield_rows(f.plain, f.ld.names, through)
    by_pos = f.ld.by_pos(f.plain)
    f.one = eng.yield_rows(by_pos, f.ld.names, through)
    by_pos.free()
    assert eng.lib.nbg_rows_num_segments(f.raw.h) >= 2 and eng.lib.nbg_rows_num_segments(f.one.h) == 1
    f.inputs = {"raw": f.raw, "yielded": f.piped, "one segment": f.one}
    yield f
    for r in (f.plain, f.raw, f.piped, f.one):
        r.free()
    f.ld.close()


def _table_cells(t, names, rows):
    return [tuple(setops.bits_cell(t.py_cell(c, r)) for c in names) + (("int", r),) for r in rows]


def test_value_table_shows_what_it_should(vt):
    """The input of the tests below, as fetched: the NaNs of rt.NANS, -0.0, both int64 extremes,
    2^53 + 1 and a string with a byte >= 0x80; id is the row's own source."""
    cols = vt.names
    for rows in vt.inputs.values():
        got = rows.fetch()
        assert len(got) == vt.t.n
        x, i, s = cols.index("x"), cols.index("i"), cols.index("s")
        assert {rt.dbits(r[x]) for r in got if math.isnan(r[x])} == set(rt.NANS)
        assert any(rt.dbits(r[x]) == 1 << 63 for r in got)
        assert {rt.INT64_MIN, rt.INT64_MAX, (1 << 53) + 1} <= {r[i] for r in got}
        assert any(any(ch >= 0x80 for ch in r[s].encode()) for r in got) and any(r[s] == "" for r in got)
        assert all(r[-1] == rt.SRC0 + r[0] for r in got)
        assert sorted(tuple(setops.bits_cell(v) for v in r[:-1]) + (("int", r[0]),) for r in got) == \
            sorted(_table_cells(vt.t, vt.ld.names, range(vt.t.n)))


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("which", ["raw", "yielded", "one segment"])
def test_input_cells_keep_every_bit(vt, which, distinct):
    """`GO FROM $-.id OVER e YIELD $-.<every column>, e.pos`: every row wins its own vid, so the
    cells beside e.pos = r are table row r's, bit for bit and kind for kind."""
    rows, cols = vt.inputs[which], vt.ld.names
    ys = [ip(c).encode() for c in cols] + [ep("e", "pos").encode()]
    out = vt.ld.eng.go_piped(rows, vt.names, "id", [rt.E_TYPE], 1, b"", ys, distinct)
    try:
        assert vt.ld.kinds_of(out) == vt.ld.kinds_of(vt.plain) + [L.V_INT]
        dev = out.fetch()
    finally:
        out.free()
    assert len(dev) == vt.t.n and all(r[0] == r[-1] for r in dev)
    assert sorted(tuple(setops.bits_cell(v) for v in r) for r in dev) == sorted(_table_cells(vt.t, cols, range(vt.t.n)))


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("which", ["raw", "yielded", "one segment"])
def test_where_reads_the_index(vt, which, distinct):
    """WHERE $-.x < 0.0 || $-.b: the kept rows by numpy over the table's cells, a NaN comparing as
    false (and -0.0 as not below 0.0)."""
    rows, cols = vt.inputs[which], vt.ld.names
    with np.errstate(invalid="ignore"):
        keep = (vt.t.bits["x"].view(np.float64) < 0.0) | (vt.t.bits["b"] != 0)
    nan = np.isnan(vt.t.bits["x"].view(np.float64))
    assert 0.5 * vt.t.n < keep.sum() < vt.t.n and (nan & ~keep).any() and (nan & keep).any()
    where = E.binop("||", E.binop("<", ip("x"), E.const(0.0)), ip("b")).encode()
    ys = [ip(c).encode() for c in cols] + [ep("e", "pos").encode()]
    out = vt.ld.eng.go_piped(rows, vt.names, "id", [rt.E_TYPE], 1, where, ys, distinct)
    try:
        dev = out.fetch()
    finally:
        out.free()
    assert sorted(tuple(setops.bits_cell(v) for v in r) for r in dev) == sorted(_table_cells(vt.t, cols, np.nonzero(keep)[0].tolist()))
