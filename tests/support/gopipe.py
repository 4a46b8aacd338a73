"""TEST HARNESS: a plain numpy model of the one-step piped GO

    <input> | GO FROM $-.col OVER e YIELD [DISTINCT] <$- columns>, e._src, e._dst, e.w

written from include/nbg.h's text on nbg_go_piped ("the start list and the input index"), not from
the kernels: no table of dense ids, no chunks, no bisection.  tests/test_go_piped_model.py pins it
on the CPU to the storage oracle.

The rules:
  * the start list is every cell of the FROM column that is a vertex with out-edges of `e`, in the
    input's order; a vid that comes twice starts twice, unless DISTINCT, which keeps each vid once;
  * every start yields one row per out-edge;
  * the $- columns of a row are those of the LAST input row whose FROM cell is the row's start vid;
  * DISTINCT also folds equal result rows (cells compared by their bits).
A vertex that the snapshot holds and storage does not show (its records lie in a foreign part) is
out of the model's scope: the adjacency the caller passes is the visible one.

The model works on indices, so that no cell is ever converted: `piped_go` returns, per result row,
the winning input row and the edge.  `rows` turns the two into tuples of the caller's own cells, and
`frontier_and_edges` gives the step statistics of the same call."""
from __future__ import annotations

import struct

import numpy as np


class Adjacency:
    """One edge type as (src, dst, w) numpy arrays, each (src, dst) once."""

    def __init__(self, src, dst, w):
        src, dst, w = (np.ascontiguousarray(a, np.int64) for a in (src, dst, w))
        assert len(src) == len(dst) == len(w)
        self.order = np.argsort(src, kind="stable")
        self.src, self.dst, self.w = src[self.order], dst[self.order], w[self.order]
        if len(src):
            both = np.lexsort((self.dst, self.src))
            same = (self.src[both][1:] == self.src[both][:-1]) & (self.dst[both][1:] == self.dst[both][:-1])
            assert not same.any(), "an edge (src, dst) twice: which record is live is not the model's business"

    def span(self, vids):
        """[lo, hi) of each vid's out-edges in the sorted arrays (empty: no out-edge, or no vertex)."""
        vids = np.asarray(vids, np.int64)
        return np.searchsorted(self.src, vids, "left"), np.searchsorted(self.src, vids, "right")


def last_rows(vids):
    """Per input row, the index of the last row that holds the same vid."""
    vids = np.asarray(vids, np.int64)
    n = len(vids)
    if not n:
        return np.zeros(0, np.int64)
    uniq, first_of_reversed = np.unique(vids[::-1], return_index=True)
    last = n - 1 - first_of_reversed
    return last[np.searchsorted(uniq, vids)]


def piped_go(adj: Adjacency, from_cells, distinct: bool = False):
    """(win, edge): per result row, the input row whose cells are the row's $- columns and the
    index of its edge in adj.src / adj.dst / adj.w.  Rows come start by start, in the input's order
    (DISTINCT: in the order of each vid's last row), a start's edges in adj's order."""
    vids = np.asarray(from_cells, np.int64)
    win = last_rows(vids)
    start_rows = np.arange(len(vids), dtype=np.int64)
    if distinct:
        start_rows = np.unique(win)                  # one row per vid: its last
    lo, hi = adj.span(vids[start_rows])
    deg = hi - lo
    keep = deg > 0
    start_rows, lo, deg = start_rows[keep], lo[keep], deg[keep]
    total = int(deg.sum())
    first = np.cumsum(deg) - deg                     # a start's first result row
    edge = np.arange(total, dtype=np.int64) - np.repeat(first, deg) + np.repeat(lo, deg)
    return np.repeat(win[start_rows], deg), edge


def _key(v):
    return ("double", struct.pack("<d", v)) if isinstance(v, float) else (type(v).__name__, v)


def rows(adj: Adjacency, cols, from_col: int, distinct: bool = False, take=None):
    """The model's rows as tuples (<cols' cells of the winner>, e._src, e._dst, e.w); `take` picks
    and orders result columns by their index in that tuple (default: all).  The cells are the
    caller's own objects.  DISTINCT folds rows that are equal cell by cell, a double by its bits."""
    win, edge = piped_go(adj, cols[from_col], distinct)
    full = [[c[r] for r in win.tolist()] for c in cols] + [adj.src[edge].tolist(), adj.dst[edge].tolist(), adj.w[edge].tolist()]
    take = range(len(full)) if take is None else take
    out = list(zip(*[full[k] for k in take])) if len(win) else []
    if distinct:
        seen, folded = set(), []
        for r in out:
            k = tuple(_key(v) for v in r)
            if k not in seen:
                seen.add(k)
                folded.append(r)
        out = folded
    return out


def frontier_and_edges(adj: Adjacency, from_cells, vertices, distinct: bool = False):
    """(frontier, edges) of the one step: the starts that are vertices (`vertices`: every vid of the
    snapshot, sorted or not) and the sum of their out-degrees."""
    vids = np.asarray(from_cells, np.int64)
    if distinct:
        vids = np.unique(vids)
    lo, hi = adj.span(vids)
    return int(np.isin(vids, np.asarray(vertices, np.int64)).sum()), int((hi - lo).sum())
