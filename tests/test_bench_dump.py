"""bench.py --dump-outputs on the CPU: run_queries_kept makes the calls run_queries makes and keeps
the step's tail results; dump_outputs writes float64 files that do not depend on the order the
device happened to append the rows in."""
import os

import numpy as np

import bench


class FakeRows:
    def __init__(self, stmt, dst, scanned):
        self.stmt, self.dst, self.edges_scanned, self.freed = stmt, dst, scanned, False

    @property
    def count(self):
        return len(self.dst)

    def digest(self):
        u = self.dst.view(np.uint64)
        return len(u), int(np.bitwise_xor.reduce(u)) if len(u) else 0, int(u.sum(dtype=np.uint64)) if len(u) else 0

    def fetch_bits(self, copy=True):
        return [self.dst]

    def free(self):
        assert not self.freed
        self.freed = True
        self.stmt.calls.append("free")


class FakeStmt:
    """Root r returns r % 7 * 1000 rows of seeded int64 payloads, shuffled by `order_seed`."""

    def __init__(self, order_seed):
        self.calls, self.order = [], np.random.default_rng(order_seed)

    def _rows(self, r):
        dst = np.random.default_rng(r).integers(-2**63, 2**63 - 1, size=r % 7 * 1000, dtype=np.int64)
        return FakeRows(self, self.order.permutation(dst), 3 * len(dst) + r)

    def submit(self, starts):
        self.calls.append(("submit", starts[0]))
        return starts[0]

    def wait(self, ticket):
        self.calls.append(("wait", ticket))
        return self._rows(ticket)

    def run_device(self, starts):
        self.calls.append(("run", starts[0]))
        return self._rows(starts[0])


ROOTS = list(range(3, 19))


def _dump(tmp, inflight, order_seed):
    stmt = FakeStmt(order_seed)
    keep = {"stats": [], "tail": []}
    totals = bench.run_queries_kept(stmt, ROOTS, inflight, keep)
    held = [res for _, res in keep["tail"]]
    assert [q for q, _ in keep["tail"]] == list(range(len(ROOTS) - min(len(ROOTS), max(1, inflight)), len(ROOTS)))
    assert not any(res.freed for res in held)
    bench.dump_outputs(str(tmp), keep, 0, 1)
    assert all(res.freed for res in held) and not keep["tail"]
    files = {n[:-4]: np.load(os.path.join(tmp, n)) for n in sorted(os.listdir(tmp))}
    return stmt, totals, files


def test_kept_step_makes_the_same_calls(tmp_path):
    for inflight in (0, 1, 6, 32):
        plain = FakeStmt(1)
        want = bench.run_queries(plain, ROOTS, inflight)
        stmt, got, _ = _dump(tmp_path / f"i{inflight}", inflight, 1)
        assert got == want
        # the same submits / waits / runs in the same order; only the tail's frees come later
        ops = lambda calls: [c for c in calls if c != "free"]
        assert ops(stmt.calls) == ops(plain.calls)
        assert stmt.calls.count("free") == plain.calls.count("free") == len(ROOTS)


def test_dump_is_float_exact_and_order_free(tmp_path):
    _, (scanned, rows), a = _dump(tmp_path / "a", 6, 1)
    _, _, b = _dump(tmp_path / "b", 6, 2)   # the same rows, appended in another order
    assert sorted(a) == ["go_edges_scanned", "go_rows", "go_tail_digest", "go_tail_rows_sample"]
    for name in a:
        assert a[name].dtype == np.float64
        assert np.array_equal(a[name], b[name]), name
    assert a["go_rows"].tolist() == [r % 7 * 1000 for r in ROOTS] and a["go_rows"].sum() == rows
    assert a["go_edges_scanned"].sum() == scanned
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # the sample: the 1-in-256 subset of each tail query's rows, rebuilt exactly from its halves
    smp = a["go_tail_rows_sample"]
    for q in range(len(ROOTS) - 6, len(ROOTS)):
        dst = np.random.default_rng(ROOTS[q]).integers(-2**63, 2**63 - 1, size=ROOTS[q] % 7 * 1000, dtype=np.int64)
        u = dst.view(np.uint64)
        want = np.sort(dst[(u * np.uint64(bench.DUMP_SAMPLE_MUL)) >> np.uint64(56) == 0])
        mine = smp[smp[:, 0] == q]
        got = (mine[:, 1].astype(np.uint64) << np.uint64(32) | mine[:, 2].astype(np.uint64)).view(np.int64)
        assert np.array_equal(got, want)
        d = a["go_tail_digest"][a["go_tail_digest"][:, 0] == q][0]
        assert d[1] == len(dst)
        assert int(d[2]) << 32 | int(d[3]) == (int(np.bitwise_xor.reduce(u)) if len(u) else 0)
