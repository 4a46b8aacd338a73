"""nbg_set_op over chosen cells and at scale.  Inputs are rowtable tables (tests/support/rowtable.py):
one-step GOs from chosen sources of a table yield exactly its rows, and the yields leave `pos` out
(except where said), so rows repeat.  Expected rows come from the plain-Python model of
tests/support/setops.py over the table's own cells — or, at scale, from numpy over them — never
from the device.

The value table V has 1,024 rows in sources of 63, 64, 65, 255, 256, 257, 1 and 63 rows.  Every
column is a function of a pattern index p(r): r % 37 for the first 600 rows, 20 + (7 r) % 40 after,
so the sources {0..3} hold patterns 0..36 and {5, 7} hold 20..59: an intersection, a difference and
differing counts.  Columns: i (INT: the int64 extremes, -2, 2^53, 2^53 + 1), d (VID, both signs and
the extremes), s (STRING, bytes >= 0x80 among them; a function of d), t (TIMESTAMP), x (DOUBLE: every
special of both signs, both zeros, NaNs of both signs and several payloads), xs (DOUBLE cells whose
cast to an integer is defined: -2.75, 0.5, both zeros, 2^53 ...) and b (BOOL).

Doubles are compared by their bits, -0.0 folded into 0.0 (which zero a surviving row reports is
unspecified); NaN payloads and signs must survive.

The probe-chain test mirrors so_mix64 / so_row_hash of csrc/setops.hip for one INT column the way
tests/test_gpu_rowtable_scale.py mirrors gb_key_hash: if the kernel's hash changes, parity still
holds but the case stops being adversarial — the mirror must follow the kernel."""
import math

import numpy as np
import pytest

from nebula_amd import expr as E
from tests.support import ngql, rowtable as rt, setops

pytestmark = pytest.mark.gpu

BLOCK = 256                    # csrc/ws.h
OB_CHUNK, OB_GRID = 2048, 2048 # csrc/nbg_internal.h, csrc/stage.h (STAGE_GRID)
SO_MIN_SLOTS = 1024            # csrc/nbg_internal.h
OPS = [("UNION", False), ("UNION", True), ("INTERSECT", False), ("MINUS", False)]
SIGN = 1 << 63


class Fixture:
    pass


# ------------------------------------------------------------------------------ the value table
COUNTS = [63, 64, 65, 255, 256, 257, 1, 63]
LEFT, RIGHT = (0, 1, 2, 3), (5, 7)
PI = rt.INT_SPECIALS + [-2, 1 << 53, 3, -7, 2]
PX = rt.DOUBLE_SPECIALS + rt.NANS
PXS = [rt.dbits(v) for v in (-2.75, 0.5, -0.0, 0.0, 2.0 ** 53, 3.0, -7.9, 1.0, -2.0, 2.0 ** 31)]
PT = [0, 1, 1 << 40, (1 << 62) + 5]


def _value_table():
    n = sum(COUNTS)
    r = np.arange(n)
    p = np.where(r < 600, r % 37, 20 + (7 * r) % 40)
    cols = [
        ("i", rt.INT, [PI[k % len(PI)] for k in p]),
        ("d", rt.VID, [rt.VIDS[k % len(rt.VIDS)] for k in p]),
        ("s", rt.STRING, [rt.STRS[(k % len(rt.VIDS)) % len(rt.STRS)] for k in p]),
        ("t", rt.TIMESTAMP, [PT[k % len(PT)] for k in p]),
        ("x", rt.DOUBLE, [PX[k % len(PX)] for k in p]),
        ("xs", rt.DOUBLE, [PXS[k % len(PXS)] for k in p]),
        ("b", rt.BOOL, [(k // 3) % 2 for k in p]),
    ]
    return rt.Table(cols, src=np.repeat(np.arange(len(COUNTS)), COUNTS))


@pytest.fixture(scope="module")
def vt():
    f = Fixture()
    f.t = _value_table()
    f.ld = rt.load_value_table(f.t)
    f.all, f.types = f.t.interim()
    rows, _ = rt.go_checked(f.ld)             # the GO's rows are the table's, bit for bit
    rows.free()
    yield f
    f.ld.close()


def _yields(t, names):
    out = []
    for c in names:
        e = E.edge_prop("e", "_dst") if t.types[c] == rt.VID else E.dst_prop("t", "name") if t.types[c] == rt.STRING \
            else E.edge_prop("e", c)
        out.append(e.encode())
    return out


def _operand(f, names, sources):
    """(device rows, the model's Interim, its types) of the one-step GO from `sources` yielding `names`."""
    rows = f.ld.eng.go_device([rt.SRC0 + s for s in sources], [rt.E_TYPE], 1, b"", _yields(f.t, names))
    idx = np.nonzero(np.isin(f.t.src, list(sources)))[0]
    cols = [f.all.columns.index(c) for c in names]
    inp = ngql.Interim([f"c{k}" for k in range(len(names))], [[f.all.rows[r][c] for c in cols] for r in idx])
    assert rows.count == len(inp.rows)
    return rows, inp, [f.t.types[c] for c in names]


def _norm(rows):
    def cell(v):
        if isinstance(v, float):
            b = rt.dbits(v)
            return ("double", 0 if b == SIGN else b)
        return (type(v).__name__, v)
    return sorted((tuple(cell(v) for v in r) for r in rows), key=repr)


def _run(f, names, lsrc, rsrc, ops=OPS, rnames=None):
    """Every operator of `ops` over the two operands against the model; {(op, distinct): device rows}."""
    lrows, li, lt = _operand(f, names, lsrc)
    rrows, ri, rtypes = _operand(f, rnames or names, rsrc)
    out = {}
    try:
        digests = lrows.digest(), rrows.digest()
        for op, d in ops:
            res = f.ld.eng.set_op(lrows, rrows, op, d)
            assert res.count == 0 or f.ld.eng.lib.nbg_rows_num_segments(res.h) == 1
            dev = res.fetch()
            res.free()
            want = setops.set_model(li, ri, op, d, lt, rtypes)[0].rows
            assert _norm(dev) == _norm(want), (names, lsrc, rsrc, op, d)
            if op == "UNION" and not d and not rnames:         # exact: the left's fetch order, then the right's
                assert [tuple(setops.bits_cell(v) for v in r) for r in dev] == \
                    [tuple(setops.bits_cell(v) for v in r) for r in lrows.fetch() + rrows.fetch()]
            out[(op, d)] = dev
        assert (lrows.digest(), rrows.digest()) == digests
    finally:
        lrows.free()
        rrows.free()
    return out, li, ri


def test_value_rows(vt):
    names = ["i", "d", "s", "t", "x", "b"]
    out, li, ri = _run(vt, names, LEFT, RIGHT)
    nan_l = {rt.dbits(r[4]) for r in li.rows if math.isnan(r[4])}
    nan_r = {rt.dbits(r[4]) for r in ri.rows if math.isnan(r[4])}
    assert nan_l & nan_r and any(b >> 63 for b in nan_l) and any(not b >> 63 for b in nan_l)    # NaNs of both signs, on both sides
    assert any(r[1] < 0 for r in li.rows) and any(r[0] == rt.INT64_MIN for r in li.rows) and any(r[0] == rt.INT64_MAX for r in li.rows)
    assert any(any(ch >= 0x80 for ch in r[2].encode()) for r in li.rows)
    assert out[("INTERSECT", False)] and out[("MINUS", False)]
    assert len(out[("UNION", True)]) < len(out[("UNION", False)])


@pytest.mark.parametrize("col", ["i", "d", "s", "t", "x", "xs", "b"])
def test_one_column_rows(vt, col):
    _run(vt, [col], LEFT, RIGHT)
    _run(vt, [col], RIGHT, LEFT)


def test_nans_never_equal_but_distinct_by_bits(vt):
    out, li, ri = _run(vt, ["x"], LEFT, RIGHT)
    nl = [rt.dbits(r[0]) for r in li.rows if math.isnan(r[0])]
    nr = [rt.dbits(r[0]) for r in ri.rows if math.isnan(r[0])]
    assert set(nl) == set(nr) == set(rt.NANS)

    def nans(rows):
        return sorted(rt.dbits(r[0]) for r in rows if math.isnan(r[0]))
    assert nans(out[("INTERSECT", False)]) == []                    # a NaN cell equals nothing
    assert nans(out[("MINUS", False)]) == sorted(nl)                # ... so every left NaN row survives
    assert nans(out[("UNION", True)]) == sorted(rt.NANS)            # by bits: one row per payload and sign
    assert nans(out[("UNION", False)]) == sorted(nl + nr)
    zeros = [r for r in out[("UNION", True)] if r[0] == 0.0]
    assert len(zeros) == 1                                          # -0.0 == 0.0


def test_32_column_rows(vt):
    names = [("i", "x", "b", "t", "xs")[k % 5] for k in range(32)]
    out, _, _ = _run(vt, names, LEFT, RIGHT)
    assert out[("INTERSECT", False)] and out[("MINUS", False)]


@pytest.mark.parametrize("k", range(7), ids=[f"rows{c}" for c in COUNTS[:7]])
def test_row_counts(vt, k):
    """Inputs of 63, 64, 65 (a wave's edges), 255, 256, 257 (a workgroup step's) rows and of one."""
    _run(vt, ["i", "b"], (k,), RIGHT)
    _run(vt, ["i", "b"], RIGHT, (k,))
    _run(vt, ["i", "b"], (k,), (k,), OPS[1:])


def test_cast_edges(vt):
    every = tuple(range(len(COUNTS)))
    # DOUBLE -> INT truncates toward zero: -2.75 and -2.0 both meet the left's -2
    out, li, ri = _run(vt, ["i"], every, every, rnames=["xs"])
    assert [-2] in li.rows and [-2.75] in ri.rows
    assert [-2] in out[("INTERSECT", False)] and [-2] not in out[("MINUS", False)]
    assert [0] in out[("INTERSECT", False)]                          # 0.5, -0.0 and 0.0 are 0
    # INT -> DOUBLE rounds to nearest even: 2^53 and 2^53 + 1 are one double
    out, li, ri = _run(vt, ["xs"], every, every, rnames=["i"])
    big = 2.0 ** 53
    cl = sum(r == [big] for r in li.rows)
    cr = sum(r[0] in (1 << 53, (1 << 53) + 1) for r in ri.rows)
    assert cl >= 1 and sum(r == [1 << 53] for r in ri.rows) >= 1 and sum(r == [(1 << 53) + 1] for r in ri.rows) >= 1
    assert sum(r == [big] for r in out[("UNION", True)]) == 1
    assert sum(r == [big] for r in out[("INTERSECT", False)]) == min(cl, cr)
    assert sum(r == [big] for r in out[("UNION", False)]) == cl + cr
    # DOUBLE -> BOOL: 0.5 is true, -0.0 is false
    out, li, ri = _run(vt, ["b"], every, every, rnames=["xs"])
    assert out[("MINUS", False)] == [] and _norm(out[("UNION", True)]) == _norm([[False], [True]])
    only_zeros, _, _ = _run(vt, ["b"], every, (6,), rnames=["xs"])  # the one-row source
    cell = vt.all.rows[int(np.nonzero(vt.t.src == 6)[0][0])][vt.all.columns.index("xs")]
    want_true = cell != 0.0
    assert all(r[0] is not want_true for r in only_zeros[("MINUS", False)]) and only_zeros[("MINUS", False)]
    # BOOL -> DOUBLE and BOOL -> INT
    _run(vt, ["xs"], every, every, rnames=["b"])
    _run(vt, ["i"], every, every, rnames=["b"])
    _run(vt, ["d"], every, every, rnames=["i"])                     # VID against INT


# ------------------------------------------------------------------------------ the probe chain
SO_SEED = np.uint64(0x7365746F70)


def _mix(x):
    """so_mix64 of csrc/setops.hip over uint64 arrays."""
    x = np.asarray(x, np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def _home(v, mask=SO_MIN_SLOTS - 1):
    """so_row_hash for a row of one INT column (c = 0), masked as k_so_insert / k_so_probe mask it."""
    with np.errstate(over="ignore"):
        return _mix(SO_SEED ^ np.asarray(v, np.int64).view(np.uint64) ^ np.uint64(0)) & np.uint64(mask)


def test_probe_chain_wraps_past_the_last_slot():
    rng = np.random.default_rng(77)
    cand = np.unique(rng.integers(rt.INT64_MIN, rt.INT64_MAX, 200_000, endpoint=True))
    home = _home(cand)
    tail = rng.permutation(cand[home >= SO_MIN_SLOTS - 8])          # homes in the last eight slots
    head = rng.permutation(cand[home < 32])                         # homes where the wrapped chain lands
    assert len(tail) >= 56 and len(head) >= 24
    a, absent, b = tail[:40], tail[40:56], head[:24]
    assert (_home(a) >= SO_MIN_SLOTS - 8).all() and (_home(absent) >= SO_MIN_SLOTS - 8).all() and (_home(b) < 32).all()
    assert len(a) > 8                                               # 40 rows from 8 home slots: the chain runs into slot 0
    right = np.concatenate([a, a, b[:12]])
    left = np.concatenate([a, b, absent, a[:7]])
    assert 2 * (len(left) + len(right)) <= SO_MIN_SLOTS             # the 1,024-slot table, UNION DISTINCT included
    t = rt.Table([("h", rt.INT, np.concatenate([right, left]))],
                 src=np.concatenate([np.zeros(len(right), np.int64), np.ones(len(left), np.int64)]))
    f = Fixture()
    f.t, f.ld = t, rt.load_value_table(t)
    f.all, f.types = t.interim()
    try:
        out, _, _ = _run(f, ["h"], (1,), (0,))
        assert sorted(r[0] for r in out[("MINUS", False)]) == sorted(np.concatenate([b[12:], absent]).tolist())
        assert sorted(r[0] for r in out[("INTERSECT", False)]) == sorted(np.concatenate([a, b[:12], a[:7]]).tolist())
        _run(f, ["h"], (0,), (1,))
    finally:
        f.ld.close()


# ------------------------------------------------------------------------------ scale
PER_SRC = 512
BIG_ROWS = 4_600_000 // PER_SRC * PER_SRC
G_VALUES = 1_000_000


def _chunks(segs):
    return sum(-(-n // OB_CHUNK) for _, n in segs)


@pytest.fixture(scope="module")
def big():
    """The numeric table sized as tests/test_gpu_rowtable_scale.py's: i (INT, unique with overwhelming
    probability), x (DOUBLE: random bit patterns, specials and NaNs), g and b (G_VALUES x 3
    combinations: every row value repeats).  The operands are overlapping source ranges."""
    rng = np.random.default_rng(43)
    n = BIG_ROWS
    x = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    special = np.array(rt.DOUBLE_SPECIALS + rt.NANS, np.uint64)
    at = rng.choice(n, n // 50, replace=False)
    x[at] = special[rng.integers(0, len(special), len(at))]
    f = Fixture()
    f.t = rt.Table([("i", rt.INT, rng.integers(rt.INT64_MIN, rt.INT64_MAX, n, endpoint=True)), ("x", rt.DOUBLE, x),
                    ("g", rt.INT, rng.integers(0, G_VALUES, n)), ("b", rt.INT, rng.integers(0, 3, n))], per_src=PER_SRC)
    f.ld = rt.load_numeric_table(f.t)
    nsrc = n // PER_SRC
    f.lsrc, f.rsrc = (0, nsrc * 19 // 20), (nsrc // 20, nsrc)
    yield f
    f.ld.close()


def _big_operand(f, names, rng_src):
    srcs = [rt.SRC0 + s for s in range(*rng_src)]
    rows = f.ld.eng.go_device(srcs, [rt.E_TYPE], 1, b"", _yields(f.t, names))
    idx = f.t.rows_of_sources(*rng_src)
    assert rows.count == len(idx)
    return rows, idx


def _structure(f, rows):
    segs = f.ld.segments(rows)
    assert _chunks(segs) > OB_GRID, "more chunks than workgroups: the grid stride runs"
    assert any(n > OB_CHUNK and n % BLOCK for _, n in segs), "a segment of several chunks, the last one ragged"


def test_scale_unique_rows(big):
    """With `pos` every row is unique: the result is a set of table rows, identified by pos.  A row
    whose x is a NaN equals nothing in INTERSECT / MINUS."""
    names = ["pos", "i", "x"]
    lrows, lidx = _big_operand(big, names, big.lsrc)
    rrows, ridx = _big_operand(big, names, big.rsrc)
    try:
        _structure(big, lrows)
        _structure(big, rrows)
        nan = np.isnan(big.t.bits["x"].view(np.float64))
        both = np.intersect1d(lidx, ridx)
        assert len(both) > OB_CHUNK * OB_GRID // 2 and nan[both].any() and len(np.setdiff1d(lidx, ridx))
        want = {("UNION", True): np.union1d(lidx, ridx), ("INTERSECT", False): both[~nan[both]],
                ("MINUS", False): np.union1d(np.setdiff1d(lidx, ridx), both[nan[both]])}
        lfetch, rfetch = lrows.fetch_bits(), rrows.fetch_bits()
        for (op, d), pos in want.items():
            res = big.ld.eng.set_op(lrows, rrows, op, d)
            assert big.ld.eng.lib.nbg_rows_num_segments(res.h) == 1
            cols = res.fetch_bits()
            res.free()
            o = np.argsort(cols[0], kind="stable")
            assert np.array_equal(cols[0][o], pos), (op, d)
            assert np.array_equal(cols[1][o], big.t.bits["i"][pos]) and np.array_equal(cols[2][o], big.t.bits["x"][pos])
        res = big.ld.eng.set_op(lrows, rrows, "UNION")               # UNION ALL: the two fetches, in order
        cols = res.fetch_bits()
        res.free()
        for c in range(3):
            assert np.array_equal(cols[c], np.concatenate([lfetch[c], rfetch[c]]))
    finally:
        lrows.free()
        rrows.free()


def test_scale_repeating_rows(big):
    """Without `pos` the (g, b) rows repeat: multiplicities against numpy's bincount."""
    names = ["g", "b"]
    lrows, lidx = _big_operand(big, names, big.lsrc)
    rrows, ridx = _big_operand(big, names, big.rsrc)
    try:
        _structure(big, lrows)
        key = big.t.bits["g"] * 3 + big.t.bits["b"]
        cl = np.bincount(key[lidx], minlength=3 * G_VALUES)
        cr = np.bincount(key[ridx], minlength=3 * G_VALUES)
        assert ((cl > cr) & (cr >= 1)).any() and ((cr > cl) & (cl >= 1)).any() and ((cl > 0) & (cr == 0)).any()
        want = {("UNION", False): cl + cr, ("UNION", True): ((cl + cr) > 0).astype(np.int64),
                ("INTERSECT", False): np.minimum(cl, cr), ("MINUS", False): np.where(cr == 0, cl, 0)}
        for (op, d), counts in want.items():
            res = big.ld.eng.set_op(lrows, rrows, op, d)
            cols = res.fetch_bits()
            res.free()
            assert ((cols[1] >= 0) & (cols[1] < 3) & (cols[0] >= 0) & (cols[0] < G_VALUES)).all()
            assert np.array_equal(np.bincount(cols[0] * 3 + cols[1], minlength=3 * G_VALUES), counts), (op, d)
    finally:
        lrows.free()
        rrows.free()
